/* fc_hip.h -- C ABI of libfc_hip.so: the MI355X (gfx950) ensemble-geometry
 * hot path of FIRECODE behind plain pointers and sizes.
 *
 * The reference (ntampellini/FIRECODE v2.0.4, paths relative to
 * /root/reference) has no FFI: its hot path is NumPy/SciPy calls made from
 * Python.  Each entry point below names the reference call it replaces; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and lives
 * in firecode_amd/_lib.py.
 *
 * Conventions
 *   - every pointer is a HOST pointer to a caller-owned buffer unless the
 *     parameter name ends in _dev; coordinates are float64, C-order
 *     (N, A, 3) -- firecode/typing_.py:6-8; masks are 1 byte per element
 *     (np.bool_, typing_.py:12); index arrays are int64.
 *   - return value: 0 = OK, < 0 = error (FC_E_*); the message is kept per
 *     thread and read with fc_last_error().  No exceptions, no callbacks and
 *     no stdout writes cross this boundary.  Calls block until results are in
 *     the output buffers.
 *   - the HIP context is created lazily, per process, on the first call
 *     (the reference may call from spawn()ed pool workers, embedder.py:116).
 *   - threads: the library keeps ONE context (device, streams, staging buffers) per
 *     process.  Entry points may be called from several host threads; each holds the
 *     library's lock for its whole duration, so calls run one after the other (the
 *     reference's hot path is single-threaded per process).  fc_last_error() is per thread.
 *     fc_shutdown / fc_init(other device) end the context: ensembles created before are
 *     refused afterwards (FC_E_INVALID) and may only be destroyed.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry point returns FC_E_NODEVICE.
 */
#ifndef FC_HIP_H
#define FC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_OK 0
#define FC_E_INVALID (-1)   /* bad argument (shape, NULL, range)              */
#define FC_E_NODEVICE (-2)  /* no HIP device / HIP runtime error at init      */
#define FC_E_HIP (-3)       /* HIP runtime error (message has the hipError)   */
#define FC_E_NOMEM (-4)     /* device allocation failed                       */
#define FC_E_LIMIT (-5)     /* size outside what a kernel supports            */
#define FC_E_INTERNAL (-6)  /* a device-side bound of the library's own was hit: a bug, reported instead of a hang */
/* FC_E_LIMIT as CONTRACT -- where the reference has no size regime and this library refuses (everything else is served at
 * any size, more slowly beyond the tiled kernels: complete alignments above 104 atoms and prune screens above 192 atoms
 * leave the matrix pipes, tests/test_gpu_parity.py checks them at 105 ... 320 atoms):
 *   - per-structure clash / rotation / fitness kernels, torsion scan, embed pose grids (fc_clash_*, fc_rototranslate,
 *     fc_fitness, fc_torsion_scan*, fc_embed_*): one structure (or pose table) lives in a workgroup's 160 KB of LDS --
 *     A <= 1706 atoms per structure (4 x A x 24 B), for the pose grids the per-group bytes the message states;
 *   - TFD (fc_tfd_simbits, fc_tfd_first_match, fc_torsion_scan_tfd*): Q <= 128 fingerprint entries -- np.sum switches to
 *     pairwise summation above 128 addends (firecode/torsion_module.py:1064) and the kernels reproduce the plain order;
 *   - cyclical embed: at most 85 distinct step angles per molecule and 2^31 poses per call (split the jobs);
 *   - A <= 32767 atoms per conformer, bit matrices below 2^32 words, and the queue capacities stated with the entry
 *     points that have one (they name the entry point to use instead).
 * The TFD ladder has no size limit of its own: what exceeds a device capacity (components above 4096 nodes, last chunks
 * that hold edges) is finished on the host from the device's flags (fc_tfd_ladder_from_first_match). */

/* ---- lifecycle --------------------------------------------------------- */
int fc_abi_version(void);
int fc_device_count(void);
int fc_init(int device);
int fc_shutdown(void);
const char *fc_last_error(void);
/* Optional: pays the one-time costs of a process now instead of inside its first calls -- the HIP runtime loads a
 * translation unit's device code at that unit's first launch (a few ms each, ~0.1 s over the library) and the first
 * large call takes its device buffers from the runtime one by one.  For long-running callers and for timing runs;
 * fc_init stays lazy and cheap (FIRECODE calls from short-lived pool workers, embedder.py:116-120). */
int fc_warmup(void);
/* Enqueue everything on the caller's HIP stream (a hipStream_t, e.g. the stream a
 * collective library orders itself against) instead of the library's own non-blocking
 * stream; NULL switches back.  The previous stream is drained first.  The legacy null
 * stream cannot be named this way (NULL means "own stream"). */
int fc_stream_set(void *hip_stream);
/* The same switch WITHOUT draining the previous stream: for a caller that orders its streams
 * with events itself (the overlapped multi-GPU steps of firecode_amd/dist.py). */
int fc_stream_use(void *hip_stream);
/* Device temporaries of the entry points come from a caching pool (released blocks are kept
 * and reused; FC_POOL_MB caps what is kept, default 8192, 0 disables).  fc_memory_trim returns
 * the kept blocks to the HIP runtime; fc_shutdown does the same. */
int fc_memory_trim(void);
/* Page-locked host memory for a caller that can choose where its coordinate arrays live (FIRECODE's Ensemble holds one
 * (N, A, 3) float64 array per ensemble: firecode/ensemble.py:58-98).  An upload from such memory is a direct DMA -- the
 * library's staging copy for pageable arrays (0.24 ms per 12 MB) is skipped, nothing else changes:
 * every entry point takes either kind of pointer.  fc_host_free_pinned releases a block; blocks still alive at
 * fc_shutdown stay valid host memory and must still be freed by their owner. */
int fc_host_alloc_pinned(int64_t bytes, void **out);
int fc_host_free_pinned(void *p);
/* name, CU count and bytes of HBM of the active device (diagnostics) */
int fc_device_info(char *name, int64_t name_len, int64_t *n_cu, int64_t *hbm_bytes);

/* ---- resident ensemble -------------------------------------------------
 * Uploads (N, A, 3) coordinates once and keeps the prepared layout in HBM:
 * the atoms selected by atom_mask (NULL = all; the "heavy atoms" of
 * prism_pruner's RMSD pruner), optionally centred on their centroid, stored
 * conformer-minor  Xs[(a*3+c)*Npad + n]  so that a wavefront reads 64
 * conformers of one coordinate with one coalesced 512-byte load, plus
 * G[n] = sum |x|^2.  Everything below that takes an fc_ensemble works on
 * HBM-resident data only. */
typedef struct fc_ensemble fc_ensemble;
int fc_ensemble_create(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask,
                       int center, fc_ensemble **out);
int fc_ensemble_destroy(fc_ensemble *ens);
int fc_ensemble_shape(const fc_ensemble *ens, int64_t *N, int64_t *A_selected);

/* ---- a4: rmsd_and_max(p, q, center) -- prism_pruner.rmsd; call sites
 * firecode/utils.py:499, embedder.py:1784, ase_manipulations.py:1384.
 * P pairs (pair_i[k], pair_j[k]) of one coordinate block. */
int fc_kabsch_rmsd_pairs(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask,
                         const int64_t *pair_i, const int64_t *pair_j, int64_t P, int center,
                         double *rmsd_out, double *maxdev_out);
/* same over a resident ensemble */
int fc_ensemble_rmsd_pairs(fc_ensemble *ens, const int64_t *pair_i, const int64_t *pair_j,
                           int64_t P, double *rmsd_out, double *maxdev_out);
/* all pairs: rmsd_out / maxdev_out are (N, N) row-major, symmetric, 0 diagonal */
int fc_ensemble_rmsd_matrix(fc_ensemble *ens, double *rmsd_out, double *maxdev_out);
/* The complete alignment of ALL pairs, timed on the device: rmsd_and_max's two outputs (RMSD and
 * max per-atom deviation; firecode/utils.py:499) for every i < j -- covariance tiles on the fp64
 * matrix pipe, rotation (Newton eigenvalue + adjugate column; Jacobi sweeps where the eigenvalue is
 * not clearly simple) and one atom pass in the epilogue.  The max deviation is taken from the explicit
 * rotated difference p - R q; the rmsd from the largest eigenvalue of the pair's quaternion matrix,
 * sqrt(((Gp + Gq) - 2 lambda) / A) -- the sum of squares of that same difference under the optimal
 * rotation, equal to it within 1e-11 on everything tested (tests/test_complete_eig_bound.py pins the
 * bound) -- except for pairs closer than ~1e-3 A, where that difference of large numbers no longer
 * holds 1e-10: those, like pairs with a declined rotation, are recomputed by a fix-up kernel from the
 * explicit sum.  FC_COMPLETE_EIG=0: the explicit running sum for every pair (the form of rounds 2-4).
 * rmsd_out / maxdev_out (N, N) symmetric with 0 diagonal, either may be NULL (timing only);
 * ms_kernel (may be NULL) = HIP-event time of the kernels.  fc_ensemble_rmsd_matrix is this
 * call with both outputs required. */
int fc_ensemble_rmsd_and_max_all(fc_ensemble *ens, double *rmsd_out, double *maxdev_out, double *ms_kernel);
/* all-pairs RMSD VALUES on the fp64 matrix pipe: covariance by MFMA, largest
 * quaternion eigenvalue by Newton (QCP), rmsd = sqrt((Gp+Gq-2*lambda)/A); pairs
 * below 0.02 A, and pairs whose largest eigenvalue is (nearly) double -- one atom, two atoms about their
 * centroid, atoms on a line: the iteration stalls short of such a root -- are re-evaluated with the explicit
 * rotated difference (FC_E_LIMIT when they outnumber the fix-up queue).  No max
 * deviation (that needs the rotation: fc_ensemble_rmsd_matrix).  rmsd_out (N, N)
 * symmetric, may be NULL (timing only); ms_kernel (may be NULL) = HIP-event time
 * of the two kernels. */
int fc_ensemble_rmsd_values(fc_ensemble *ens, double *rmsd_out, double *ms_kernel);
/* RMSD-diverse selection: greedy max-min (farthest point, Gonzalez k-center) under the ensemble's Kabsch RMSD --
 * FIRECODE's csearch mode 1, "keep the n most diverse conformers" (firecode/torsion_module.py:608-611), whose
 * most_diverse_conformers (:574-586) returns a random draw.  d(i, j) is the value fc_ensemble_rmsd_pairs returns for
 * (i, j) within a few ulp (the ensemble's atom selection and centring; the rotation by Newton eigenvalue + adjugate
 * eigenvector where the eigenvalue is clearly simple, the Jacobi sweeps otherwise).  The contract:
 *
 *   s[0] = start;  D[j] = d(s0, j);  D[s0] = 0;  L[j] = 0;  radius[0] = +inf
 *   for k = 1 .. n_max-1, while fewer than N are selected:
 *       m   = max D[j] over the conformers not yet selected;  s_k = the smallest such j with D[j] == m
 *       if stop_rmsd >= 0 and m <= stop_rmsd: stop
 *       radius[k] = m;  D[s_k] = 0;  L[s_k] = k
 *       for all j: t = d(s_k, j); if t < D[j]: D[j] = t; L[j] = k      (strict: ties keep the earlier representative)
 *
 * Outputs: indices_out (n_max; the first *n_selected = K written) in selection order; radii_out (n_max or NULL) the
 * covering radius just before each pick, nonincreasing, radii[0] = +inf; labels_out (N or NULL) the position in
 * indices of each conformer's representative; dist_out (N or NULL) the distance to it (0 for a representative).
 * No N x N matrix: a step aligns one conformer against all N (one kernel launch per step).  stop_rmsd < 0: no radius
 * stop.  FC_E_INVALID before any device use: n_max < 1, start outside [0, N), NULL indices_out or n_selected, NaN
 * stop_rmsd.  N = 0: *n_selected = 0.  Limits: N < 2^31 - 256; no atom limit (the representative is staged in LDS up
 * to 2 048 selected atoms and read from HBM beyond). */
int fc_ensemble_select_diverse(fc_ensemble *ens, int64_t n_max, int64_t start, double stop_rmsd,
                               int64_t *indices_out, double *radii_out, int32_t *labels_out, double *dist_out,
                               int64_t *n_selected);
/* The symmetry- and mirror-aware form: the same selection under
 *
 *   d_sym(i, j) = min over k < K, h in H of rmsd_and_max(X[i], h * X[j][perms[k]])[0]
 *   H = {+1}, or {+1, -1} when mirror != 0      (-1: the partner inverted through the origin, as in the
 *                                                enantiomer-aware forms below)
 *
 * X = the prepared ensemble (atom selection applied, centred); perms = a (K, A_sel) table exactly as in the
 * symmetry-aware forms below: row 0 the identity, closed under inverse (which makes d_sym symmetric), K <= FC_PERM_MAX.
 * The greedy loop, its tie rules, start, stop_rmsd, every output and the argument checks are those of
 * fc_ensemble_select_diverse with d replaced by d_sym; the value is the explicit rotated-difference rmsd of the winning
 * (k, h).  K = 1 with mirror = 0 is fc_ensemble_select_diverse itself, bit for bit.  Refused before the device is
 * touched, the table first (it is checked before the handle is looked at) -- FC_E_LIMIT: K > FC_PERM_MAX; the
 * representative (24 A_sel bytes) + the table as 16-bit indices (2 K A_sel bytes, rounded up to 8) + 64 bytes of the
 * kernel's own exceed the 160 KiB of LDS (A_sel <= 5 849 at K = 2, <= 1 077 at K = 64; no HBM fallback).  FC_E_INVALID:
 * the table checks of fc_prune_rmsd_perm, A_sel that is not the ensemble's, mirror outside {0, 1}; then the sibling's
 * own checks.  Not offered: sharded, multi-GPU and twin-workspace forms. */
int fc_ensemble_select_diverse_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                    int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out,
                                    double *radii_out, int32_t *labels_out, double *dist_out, int64_t *n_selected);
/* k nearest neighbours of every conformer under the ensemble's Kabsch RMSD: what shows a sensible
 * max_rmsd for fc_rmsd_dbscan (the sorted distance to the (min_samples - 1)-th neighbour, the "k-distance" curve) and
 * feeds local density estimates, outlier scores and mutual-k-NN graphs (fc_clusters_from_pairs takes a caller's graph).
 * No N x N matrix: the top-k selection happens in the kernel that computes the distances.  The contract:
 *
 *   d(i, j) = rmsd_and_max(X[i][sel], X[j][sel], center=True)[0] over the ensemble's atom selection -- the d of
 *   fc_ensemble_select_diverse.  For every conformer i the list holds the k conformers j != i with the smallest d(i, j),
 *   in ascending order of (d(i, j), j): on equal distances the lower index comes first, inside the list and at its cut.
 *
 * Outputs: indices_out (N, k) int32 and dist_out (N, k) float64, row-major.  1 <= k <= FC_KNN_MAX.  When k > N - 1 the
 * trailing k - (N - 1) entries of every row are index -1 and distance +inf (N = 1: one row of them); N = 0: nothing is
 * written.  The self-pair is left out by index, not by value: exact duplicates of i appear in its list.
 * Determinism: d(i, j) is produced by one fixed instruction sequence over the atoms in order, whatever tile, strip,
 * wavefront or launch the pair falls into, so two columns with bitwise-identical coordinates give bitwise-identical
 * distances in a row, and the outputs are bit-identical for every strip count (FC_KNN_STRIPS=<n>, a speed-only knob);
 * no floating-point atomics.  Bit symmetry d(i, j) == d(j, i) is NOT promised (the two are computed separately).
 * Every value is the explicit rotated-difference rmsd (pair_exact_aos's sums; the rotation by Newton eigenvalue +
 * adjugate eigenvector where the eigenvalue is clearly simple, the Jacobi sweeps otherwise, as the diverse selection):
 * within a few ulp of fc_ensemble_rmsd_pairs, ~1e-15 for a duplicate pair where the eigenvalue form gives ~1e-8.  The
 * eigenvalue serves only as a conservative filter -- the explicit pass is skipped for columns that provably cannot enter
 * a row's current list (margin: DESIGN.md section 18) -- and decides no value and no order: FC_KNN_FILTER=0 (speed only)
 * takes every pair through the explicit pass and gives the same bits.
 * FC_E_INVALID before any device use: NULL ens or outputs, k < 1; FC_E_LIMIT before any device use: k > FC_KNN_MAX.
 * Limits: N < 2^31 - 256; no atom limit (a workgroup's 16 row conformers are staged in LDS up to 256 selected atoms and
 * read from HBM beyond).  Not offered: sharded, multi-GPU and twin-workspace forms (queries of one ensemble against
 * another: fc_ensemble_knn_cross; symmetry- and mirror-aware forms: fc_ensemble_knn_perm, both below). */
#define FC_KNN_MAX 64
int fc_ensemble_knn(fc_ensemble *ens, int64_t k, int32_t *indices_out, double *dist_out);
/* The same lists across two ensembles: for every conformer of `queries` its k nearest conformers
 * of `refs` -- what answers "which of these conformers are not in the ensemble I hold" (novelty: k = 1 with max_rmsd at
 * the duplicate threshold), "does my ensemble contain every conformer of a reference set to within max_rmsd" (coverage:
 * the roles swapped) and "which conformer of B is closest to each conformer of A".  The kernels, the arithmetic and the
 * determinism promises are those of fc_ensemble_knn: the rows come from `queries`, the columns from `refs`.  The contract:
 *
 *   d(i, j) = rmsd_and_max(Q[i][sel], R[j][sel], center=True)[0], Q = queries, R = refs.  For every i < Nq the list holds
 *   the k conformers j < Nr with the smallest d(i, j) among those with d(i, j) < max_rmsd (strict, like the prune's
 *   rmsd < max_rmsd; max_rmsd = +inf: no cap), in ascending order of (d(i, j), j): on equal distances the lower index
 *   comes first, inside the list and at its cut.  NO pair is left out: a query that is a bitwise copy of a reference
 *   lists that reference first, at ~1e-15.
 *
 * Outputs: indices_out (Nq, k) int32, indices into `refs`, and dist_out (Nq, k) float64, row-major.  1 <= k <= FC_KNN_MAX.
 * Where fewer than k references qualify -- k > Nr, or the cap -- the trailing entries of the row are index -1 and
 * distance +inf.  Nq = 0: nothing is written.  Nr = 0: every slot is -1 / +inf, written without any device use.
 * queries == refs (the same handle) is allowed: a row then lists itself first.
 * Both ensembles must belong to the current context epoch and have the same number of selected atoms A; like
 * fc_ensemble_knn the distances mean what the contract says only when both hold CENTRED coordinates (center != 0 at
 * fc_ensemble_create) of the SAME atom selection: the library checks A, the selection and the centring are the caller's
 * (firecode_amd.pruner.knn_by_rmsd_against guarantees both).  Nq and Nr are independent.
 * Determinism: as fc_ensemble_knn -- one fixed instruction sequence per d(i, j), bit-identical outputs for every strip
 * count (strips are chosen from the row tiles of Nq and the 64-column chunks of Nr; FC_KNN_STRIPS=<n>) and with
 * FC_KNN_FILTER=0.  An ensemble against a bitwise copy of itself gives, for every i != j, the distance bits of
 * fc_ensemble_knn.  With a cap the eigenvalue filter starts from tau = max_rmsd instead of an empty list's +inf -- a
 * smaller tau under the same margins, never a different value or order -- which is what makes a novelty query cheap.
 * Refused before any device use -- FC_E_INVALID: k < 1, max_rmsd NaN or <= 0, NULL queries, refs or outputs, an ensemble
 * of an earlier context epoch, different A; FC_E_LIMIT: k > FC_KNN_MAX, Nq or Nr >= 2^31 - 256.  k and max_rmsd are
 * judged first, then the pointers.  No atom limit (LDS stage as fc_ensemble_knn).  Not offered: max-deviation or
 * energy criteria, sharded, multi-GPU and twin-workspace forms (symmetry- and mirror-aware: fc_ensemble_knn_cross_perm). */
int fc_ensemble_knn_cross(fc_ensemble *queries, fc_ensemble *refs, int64_t k, double max_rmsd, int32_t *indices_out,
                          double *dist_out);
/* The symmetry- and mirror-aware forms of the two: the same lists under
 *
 *   d_sym(i, j) = min over p < K, h in H of rmsd_and_max(Q[i], h * R[j][perms[p]])[0]       (Q = R = X in the self form)
 *   H = {+1}, or {+1, -1} when mirror != 0      (-1: the partner inverted through the origin, as in
 *                                                fc_ensemble_select_diverse_perm and the enantiomer-aware forms below)
 *
 * X, Q, R = prepared ensembles (atom selection applied, centred); perms = a (K, A_sel) table exactly as in
 * fc_ensemble_select_diverse_perm: row 0 the identity, closed under inverse, K <= FC_PERM_MAX; the cross form applies
 * the one table to both ensembles (the same molecule, the same atom selection: the caller's, as in fc_ensemble_knn_cross).
 * The table and the flag combine: a minimum over both.  Everything else of fc_ensemble_knn / fc_ensemble_knn_cross
 * holds with d replaced by d_sym: ascending order of (d_sym, j), the lower index first on ties; the self form leaves
 * j == i out by index (a relabelled or mirrored copy of i is its first neighbour, at ~1e-15); the cross form leaves
 * nothing out and keeps the strict cap d_sym < max_rmsd; -1 / +inf padding; N = 0, Nr = 0 and 1 <= k <= FC_KNN_MAX as
 * there.  The value written out is the explicit rotated-difference rmsd of the winning (p, h) (h = -1: -B, p + R q),
 * never the eigenvalue form.
 * Determinism: one fixed instruction sequence per (pair, p, h); the value of a pair is the minimum over the explicit
 * sums that were formed, and the winning (p, h) of a pair that belongs in a list is always among them (fc_knn.hip says
 * why), so the outputs are the same bits for every strip count (FC_KNN_STRIPS) and with FC_KNN_FILTER=0, and an
 * ensemble against a bitwise copy of itself gives, for every i != j, the distance bits of the self form.  K = 1 with
 * mirror = 0 is fc_ensemble_knn / fc_ensemble_knn_cross itself, bit for bit.
 * Refused before any device use, in this order: the table (FC_E_INVALID: the table checks of fc_prune_rmsd_perm;
 * FC_E_LIMIT: K > FC_PERM_MAX, or the LDS limit: a workgroup keeps its 16 row conformers (16 x 24 A_sel bytes) and the
 * table as 16-bit indices (2 K A_sel bytes, rounded up to 8) in the 160 KiB of LDS -- A_sel <= 422 at K = 2,
 * <= 413 at K = 6, <= 320 at K = 64; no HBM fallback); mirror outside {0, 1} (FC_E_INVALID); an A_sel that is not the
 * ensemble's -- either ensemble's -- or a NULL handle (FC_E_INVALID); then the sibling's own checks in its own order.
 * Not offered: max-deviation or energy criteria, sharded, multi-GPU and twin-workspace forms. */
int fc_ensemble_knn_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, int64_t k,
                         int32_t *indices_out, double *dist_out);
int fc_ensemble_knn_cross_perm(fc_ensemble *queries, fc_ensemble *refs, const int32_t *perms, int64_t K, int64_t A_sel,
                               int mirror, int64_t k, double max_rmsd, int32_t *indices_out, double *dist_out);
/* ---- medoids and k-medoids under the RMSD: which conformer stands for a group ----
 * The distance.  d(i, j) for i < j is the d of fc_ensemble_knn, computed as k_knn_tile computes the value it writes out:
 * the covariance, the rotation from the Newton eigenvalue and the adjugate (the Jacobi sweeps where the eigenvalue is not
 * clearly simple), the explicit rotated difference with conformer i as the row (p) and j as the column (q); never the
 * eigenvalue form.  d is evaluated ONCE per unordered pair and used for both partners.
 *   q(d) = (uint64) rint(d * 2^32)          the distance in units of 2^-32 A
 * Per-conformer sums and the k-medoids cost are sums of q values in 64-bit integers: they do not depend on the order, the
 * launch shape (FC_MEDOID_STRIPS=<n>) or the arrival of atomics -- the same bits every time -- and the two members of a
 * two-member group tie exactly.
 *
 * fc_ensemble_medoids.  labels: (N) int32, a negative label = in no group, labels[i] < n_groups; NULL = one group (0) of
 * all conformers (the other n_groups - 1 groups are empty).  The labels of fc_rmsd_clusters, fc_rmsd_dbscan (-1 = noise)
 * and fc_rmsd_butina are taken as they come.
 *   S[i] = sum of q(d(i, j)) over j != i with labels[j] == labels[i] >= 0
 *   E[i] = max of d(i, j) over the same j (a double; a max is exact); both 0 for a singleton and an unlabelled conformer
 *   for each group c < n_groups:  medoid[c] = the member with the smallest S, the lowest index on ties;
 *     size[c] = the member count;  mean[c] = S[medoid] 2^-32 / (size - 1), 0 for a singleton;  radius[c] = E[medoid];
 *     an empty group: medoid -1, size 0, mean and radius NaN.
 * Outputs: medoids_out, sizes_out, mean_out, radius_out (n_groups each, required); sums_q32_out (N, the S) and ecc_out
 * (N, the E), each or NULL; ms_kernel (or NULL): HIP-event time of the sums kernel with the zeroing of its outputs (0 when
 * no group has two members: then no device is used).
 *
 * fc_ensemble_kmedoids.  n representatives by the alternating form (Park & Jun 2009); init: n distinct conformers, or NULL:
 * the picks of fc_ensemble_select_diverse(n_max = n, start = 0).
 *   M_0 = init
 *   for t = 0, 1, ...:
 *     assign: (lab_t[j], dist_t[j]) = the nearest member of M_t to j, ties to the earlier position in M_t -- the k = 1
 *             list of fc_ensemble_knn_cross(ens, fc_ensemble_subset(ens, M_t)), bit for bit; a medoid gets its own
 *             position and distance 0, set by index
 *     cost_t = sum over j of q(dist_t[j])
 *     if t > 0 and cost_t >= cost_{t-1}: return iteration t-1's (M, lab, dist, cost)
 *     if t == max_iter:                  return iteration t's
 *     M_{t+1}[c] = the medoid of {j : lab_t[j] == c}   (the rule of fc_ensemble_medoids)
 *     if M_{t+1} == M_t:                 return iteration t's
 * The integer costs fall strictly until the loop ends, so it ends (the assignment and the sums round d differently in the
 * last bits: row and column change places); the cost returned is the smallest seen.  Outputs, all required: medoids_out
 * (n), labels_out (N) int32 = position in medoids_out, dist_out (N), *cost_q32_out, *n_iter_out = assignments made.
 *
 * fc_ensemble_subset.  *out = a new ensemble (fc_ensemble_destroy) of the conformers indices[0 .. n), in that order,
 * repeats allowed, n >= 0: the prepared coordinates and G are COPIED, not recomputed -- every distance within the subset
 * has the bits it has in `ens`.  The atom selection is that of `ens`.
 *
 * Refused with FC_E_INVALID before any device use, the message naming the argument: a NULL ens or required output;
 * n_groups < 1; labels[i] >= n_groups; n < 1 (subset: n < 0) or n > N; max_iter < 0; init or indices outside [0, N), or
 * repeated within init; an ensemble of an earlier context epoch.  The scalar arguments (n_groups, n, max_iter) are judged
 * first, then the pointers, then what needs N.  N = 0 is an empty success (medoids: every group empty;
 * k-medoids: cost 0, 0 iterations, nothing else written).  FC_E_LIMIT: N >= 2^31 - 256; and, once the ensemble's largest
 * G is known, a group too large for the 64-bit sum: (largest size) (ceil(sqrt(4 g_max / A)) + 1) 2^32 >= 2^63 (k-medoids
 * judges N, which no group exceeds) -- tens of millions of members at molecular coordinates.
 * Symmetry- and mirror-aware forms: fc_ensemble_medoids_perm / fc_ensemble_kmedoids_perm, below.  Not offered: a
 * multi-GPU form, PAM's swap phase (between-group sums: the silhouettes below).
 *
 * fc_ensemble_silhouette.  How good is a labelling: labels and n_groups as for fc_ensemble_medoids.
 * A conformer with a negative label is in no group: it is neither a row nor a column, and gets a = b = s = NaN and
 * nearest = -1.  For the labelled conformers d(i, j) is the d of fc_ensemble_knn as above (i the row, j the column),
 * evaluated for EVERY ORDERED pair i != j -- the full square, not once per unordered pair -- and, with size_g the member
 * count of group g:
 *   T[i, g] = sum of q(d(i, j)) over the members j != i of g       64-bit integers: the same bits for every launch shape
 *                                                                  (FC_SILHOUETTE_STRIPS=<n>) and on every run
 *   a[i]    = (double) T[i, own] 2^-32 / (size_own - 1), 0 for a singleton
 *   m[i, g] = (double) T[i, g] 2^-32 / size_g                      for every non-empty g != own
 *   b[i]    = min over g of m[i, g];  nearest[i] = the g that attains it, the lowest label on ties
 *   s[i]    = (b - a) / max(a, b);  0 for a singleton;  0 when max(a, b) == 0
 * Fewer than two non-empty groups: b = s = NaN and nearest = -1 for everyone (a singleton included), a is still given,
 * and the device is used only for a (not at all with fewer than two labelled conformers).
 *   for each group c < n_groups:  size[c];  cluster_mean[c] = the mean of s over its members, summed in ascending
 *     conformer index, NaN for an empty group;  score = the mean of s over all labelled conformers, summed in the same
 *     order, NaN when there is none.  s, cluster_mean and score are formed on the host from a, b and the labels.
 * a comes from this call's own full-square values, the S of fc_ensemble_medoids from one evaluation per unordered pair:
 * a (size - 1) 2^32 and S may differ by the last unit of q per distance.
 * Outputs, all required but ms_kernel: s_out, a_out, b_out (N doubles each), nearest_out (N int32), cluster_mean_out
 * (n_groups), sizes_out (n_groups int64), *score_out; ms_kernel (or NULL): HIP-event time of the kernel pair (0 when no
 * device is used).  Refusals and limits as for fc_ensemble_medoids, in the same order (N = 0: every group empty, score
 * NaN); the 64-bit check is made on the number of LABELLED conformers -- a prefix runs over a whole row.
 * Symmetry- and mirror-aware form: fc_ensemble_silhouette_perm, below.  Not offered: a multi-GPU form, the "simplified"
 * silhouette against medoids, other indices (Davies-Bouldin, Calinski-Harabasz). */
int fc_ensemble_silhouette(fc_ensemble *ens, const int32_t *labels /* N or NULL = one group */, int64_t n_groups,
                           double *s_out, double *a_out, double *b_out, int32_t *nearest_out, double *cluster_mean_out,
                           int64_t *sizes_out, double *score_out, double *ms_kernel /* or NULL */);
int fc_ensemble_subset(fc_ensemble *ens, const int64_t *indices, int64_t n, fc_ensemble **out);
int fc_ensemble_medoids(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, int64_t *medoids_out, int64_t *sizes_out,
                        double *mean_out, double *radius_out, uint64_t *sums_q32_out /* N or NULL */,
                        double *ecc_out /* N or NULL */, double *ms_kernel /* or NULL */);
int fc_ensemble_kmedoids(fc_ensemble *ens, const int64_t *init /* n or NULL */, int64_t n, int64_t max_iter,
                         int64_t *medoids_out, int32_t *labels_out, double *dist_out, uint64_t *cost_q32_out,
                         int64_t *n_iter_out);
/* ---- the symmetry- and mirror-aware forms of the three ----
 * perms (K, A_sel), mirror: the table and the flag of fc_ensemble_knn_perm, with its checks.  The distance:
 *
 *   d_sym(i, j) = sqrt(min over p < K, h in H of ssq(p, h) / A_sel),   H = {+1}, or {+1, -1} when mirror != 0
 *
 * the value k_knn_tile_sym writes for row i and column j: ssq(p, h) the explicit rotated sum of squares of
 * (X[i][perms[p]], h X[j]) under the rotation of its own covariance -- the permutation applied to the row side, h = -1 as
 * -B, p + R q -- never the eigenvalue form.  Everything else is the contract of the plain twin with d replaced by d_sym:
 *   fc_ensemble_medoids_perm: d_sym(i, j) is evaluated once per unordered pair, as (row i, column j) with i < j -- in the
 *     order of the label-sorted conformers, which within a group is the ascending conformer index -- and serves both
 *     partners; q, S, E, the medoid (the lowest index on ties), mean and radius as in fc_ensemble_medoids.
 *   fc_ensemble_silhouette_perm: every ordered pair i != j; T, a, m, b, nearest (the lowest label on ties), s, negative
 *     labels, singletons, fewer than two groups, cluster_mean and score as in fc_ensemble_silhouette.
 *   fc_ensemble_kmedoids_perm: the loop of fc_ensemble_kmedoids where init = NULL stands for the picks of
 *     fc_ensemble_select_diverse_perm(n_max = n, start = 0) under the same table and flag, the assignment is the k = 1
 *     list of fc_ensemble_knn_cross_perm(ens, fc_ensemble_subset(ens, M_t)) (a representative: its own position and
 *     distance 0, by index) and the move uses the S of fc_ensemble_medoids_perm; the same stopping rule on integer costs.
 *     The table is uploaded once per call.
 * The same bits: the sums are 64-bit integers and d_sym(i, j) is one value per (row, column) -- the minimum over the
 * explicit sums that were formed; a (p, h) is skipped only where its eigenvalue form of A msd exceeds the pair's smallest
 * explicit sum so far by more than A * 1e-6 for every counting lane of the wavefront, and a pair's first (p, h) is always
 * explicit -- so every output is the same bits on every run, for every strip count (FC_MEDOID_STRIPS / FC_SILHOUETTE_STRIPS,
 * the plain forms' knobs), with FC_MEDOID_SYM_FILTER=0 (every (p, h) explicit) and for any number of rows a wavefront
 * puts through one atom loop; and d_sym here is bit for bit the d_sym fc_ensemble_knn_perm lists for the same (row,
 * column).  K = 1 with mirror = 0 runs the plain twin's kernels, bit for bit.
 * stats (2 values, or NULL; medoids and silhouette): (pair, p, h) whose eigenvalue was formed, and those taken through the
 * explicit pass; 0 where no device is used and for K = 1 without the flag.
 * Refused before any device use, in this order: the table (FC_E_INVALID / FC_E_LIMIT: K > FC_PERM_MAX), the LDS limit
 * (FC_E_LIMIT: 16 x 24 A_sel bytes of rows and 2 K A_sel bytes of table, rounded up to 8, within 160 KiB -- A_sel <= 422 at
 * K = 2, <= 413 at K = 6, <= 320 at K = 64; these kernels are staged only, there is no global-memory fallback), mirror
 * outside {0, 1}, a NULL handle, an earlier epoch or an A_sel that is not the ensemble's (FC_E_INVALID); then the plain
 * twin's own checks in its own order.  Not offered: sharded, multi-GPU and twin-workspace forms, a max-deviation or energy
 * criterion. */
int fc_ensemble_medoids_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                             const int32_t *labels, int64_t n_groups, int64_t *medoids_out, int64_t *sizes_out,
                             double *mean_out, double *radius_out, uint64_t *sums_q32_out /* N or NULL */,
                             double *ecc_out /* N or NULL */, double *ms_kernel /* or NULL */, int64_t *stats /* 2 or NULL */);
int fc_ensemble_kmedoids_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                              const int64_t *init /* n or NULL */, int64_t n, int64_t max_iter, int64_t *medoids_out,
                              int32_t *labels_out, double *dist_out, uint64_t *cost_q32_out, int64_t *n_iter_out);
int fc_ensemble_silhouette_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                const int32_t *labels /* N or NULL = one group */, int64_t n_groups, double *s_out,
                                double *a_out, double *b_out, int32_t *nearest_out, double *cluster_mean_out,
                                int64_t *sizes_out, double *score_out, double *ms_kernel /* or NULL */,
                                int64_t *stats /* 2 or NULL */);
/* ---- mean structures and per-atom fluctuations of groups: what a cluster looks like ----
 * fc_ensemble_group_means.  X is the prepared ensemble: the atom selection applied, every conformer centred on its
 * selected atoms -- create the handle with center = 1; an uncentred ensemble is taken as it is and its means are not
 * centroids of anything.  labels and n_groups as for fc_ensemble_medoids (int32 per conformer, negative = in no group,
 * NULL = one group, the same checks).  refs: (n_groups) one conformer per group, the member the iteration starts from (the
 * medoid, say); the entry of an empty group is not read; NULL = the smallest-index member of each group.
 * For every non-empty group g, members n in ascending conformer index:
 *   M_g(0) = X[ref_g]
 *   turn t = 0, 1, ... while t < max_iter and g is not frozen:
 *       R_n = the Kabsch rotation that takes X[n] onto M_g(t): the rotation fc_ensemble_rmsd_pairs uses for the pair
 *             (p = M_g, q = X[n]) -- covariance sum_a p_a q_a^T, Newton eigenvalue and adjugate, the Jacobi sweeps where the
 *             eigenvalue is not clearly simple
 *       M'  = (sum over n in g of R_n X[n]) / |g|          (no re-centring: rotations keep the centroid at 0)
 *       c   = sqrt(sum_a |M'_a - M_g(t)_a|^2 / A_sel)
 *       M_g(t+1) = M';  n_iter_g = t + 1;  if c <= tol: g is frozen
 *   final pass, against M_g = M_g(n_iter_g):
 *       R_n;  Y_n = R_n X[n];  d_n = sqrt(sum_a |Y_na - M_ga|^2 / A_sel)
 *       rmsf_g[a] = sqrt(sum over n in g of |Y_na - M_ga|^2 / |g|)
 *       closest_g = the member with the smallest d_n, the lowest index on ties
 * A frozen group's mean is never touched again: a group's outputs are a function of its own members, ref_g, max_iter and
 * tol alone -- not of what other groups of the call are still doing, and not of how often the host reads the device's "a
 * group is still moving" word (it is read every few turns; FC_GROUP_MEAN_BATCH=<turns>).
 * max_iter = 0: the mean is the reference member and d_n the plain RMSD to it.  A singleton: mean = itself, rmsf = 0,
 * d = 0, R = identity, n_iter = 0, by definition.  An empty group id: NaN mean and rmsf, size 0, closest -1, n_iter 0.  A
 * conformer in no group: d = NaN, R = identity.
 * The order of the sums (part of the contract; double precision, no atomics, no integer quantisation -- a mean rounded to
 * 2^-33 A would cost the 1e-10 the coordinates are held to).  A group's members in ascending conformer index are cut into
 * chunks of 64, counted from the group's first member; the last chunk is filled up with +0.0.  A chunk's 64 values v[0..64)
 * are added as a tree of neighbouring pairs: v[l] += v[l ^ 1], then ^ 2, ^ 4, ^ 8, ^ 16, ^ 32.  The chunk sums are added in
 * ascending chunk order, starting from the first chunk's, and the total is DIVIDED by |g| (M') or divided by |g| and
 * rooted (rmsf, whose values are (dx dx + dy dy) + dz dz per member and atom).  c: the squares of M' - M over the 3 A_sel
 * coordinates r, 256 partial sums (r = k, k + 256, ... ascending), each 64 consecutive partials by the tree above, the
 * four results added in order.  d_n: the atoms a = s, s + 8, ... per partial s < 8, dx dx + dy dy + dz dz added left to
 * right, the eight partials by the tree; the covariance likewise, by fused multiply-adds.
 * Hence the same bits on every run and for every launch shape: the mean staged in LDS or read from global memory
 * (FC_GROUP_MEAN_STAGE=0; staged up to 2048 selected atoms, and only where a workgroup's 32 conformers share a group), any
 * grid of the reduction kernels (FC_GROUP_MEAN_GRID=<workgroups>), any FC_GROUP_MEAN_BATCH.
 * Outputs: means_out (n_groups, A_sel, 3), rmsf_out (n_groups, A_sel), dist_out (N), closest_out, sizes_out, n_iter_out
 * (n_groups each), all required; rot_out (N, 9) row-major, applied as R x, or NULL; ms_kernel (or NULL): HIP-event time
 * from the first launch to the last, the host's reads of the word included (0 when no device is used: nobody in a group).
 * Refused with FC_E_INVALID before any device use, the message naming the argument: n_groups < 1; max_iter < 0; tol
 * negative or NaN; a NULL ens or required output; labels[i] >= n_groups; for a non-empty group g a refs[g] outside [0, N)
 * or not a member of g; an ensemble of an earlier context epoch.  N = 0 writes nothing.  FC_E_LIMIT: N >= 2^31 - 256.
 * Not offered: symmetry- and mirror-aware forms, sharded, multi-GPU and twin-workspace forms, weights. */
int fc_ensemble_group_means(fc_ensemble *ens, const int32_t *labels /* N or NULL = one group */, int64_t n_groups,
                            const int64_t *refs /* n_groups or NULL */, int64_t max_iter, double tol, double *means_out,
                            double *rmsf_out, double *dist_out, double *rot_out /* (N, 9) or NULL */, int64_t *closest_out,
                            int64_t *sizes_out, int64_t *n_iter_out, double *ms_kernel /* or NULL */);
/* a9: get_alignment_matrix(p, q) -- prism_pruner.rmsd; call site
 * hypermolecule_class.py:77.  M (3,3) row-major, applied as (M @ q.T).T */
int fc_alignment_matrices(const double *p, const double *q, int64_t n_pairs, int64_t A,
                          double *M_out);

/* ---- a5: prune_by_rmsd(structures, atoms, max_rmsd, energies=, max_dE=)
 * -- prism_pruner.pruner; call sites firecode/ensemble.py:230-235,
 * embedder.py:1472-1474, operators.py:619-624.
 *
 * fc_rmsd_simbits: similarity bits of rows [row_begin,row_end) against all
 * later conformers: bit j of row i (j > i) = rmsd(i,j) < max_rmsd &&
 * maxdev(i,j) < max_dev [&& |E_i-E_j| < max_dE when energies != NULL].
 * bits_out: (row_end-row_begin) rows of W = ceil(N/64) uint64 words.
 * n_grey (may be NULL): pairs within 1e-9 of either threshold.
 *
 * fc_prune_rmsd: the whole stage on the GPU -- similarity bits, then the
 * k-ladder greedy replay -- conformers taken in the order given (the host
 * pre-sorts by energy as the reference does).  mask_out: N bytes.
 * stats (may be NULL): [0]=pairs evaluated, [1]=candidate pairs refined,
 * [2]=similar pairs, [3]=grey pairs, [4]=ladder levels run, [5]=survivors. */
int fc_rmsd_simbits(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies,
                    double max_dE, int64_t row_begin, int64_t row_end, uint64_t *bits_out,
                    int64_t *n_grey);
int fc_prune_rmsd(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies,
                  double max_dE, int64_t min_per_group, uint8_t *mask_out, int64_t *stats);
/* prism_pruner.pruner.prune_by_rmsd as FIRECODE calls it (firecode/ensemble.py:230-235, firecode/embedder.py:1472-1474:
 * host arrays in, mask out) in ONE call: coords (N, A, 3), atom_mask (A bytes or NULL = all atoms), center as in
 * fc_ensemble_create; the other arguments, mask_out (N bytes) and stats (6 values or NULL) as in fc_prune_rmsd.  Same
 * mask as fc_ensemble_create + fc_prune_rmsd + fc_ensemble_destroy; nothing stays resident. */
int fc_prune_rmsd_host(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask, int center, double max_rmsd,
                       double max_dev, const double *energies, double max_dE, int64_t min_per_group, uint8_t *mask_out,
                       int64_t *stats);
/* ---- enantiomer-aware forms: mirror images count as duplicates ----
 * The contract, once.  X = the prepared ensemble (atom selection applied, each conformer centred on the centroid of its
 * selected atoms when created with center = 1).  For a pair (i, j):
 *
 *   (r+, m+) = rmsd_and_max(X[i],  X[j])      the values of fc_ensemble_rmsd_pairs: best PROPER rotation
 *   (r-, m-) = rmsd_and_max(X[i], -X[j])      partner inverted through the origin = its mirror image, any mirror plane
 *   similar_enant(i, j) = (r+ < max_rmsd && m+ < max_dev) || (r- < max_rmsd && m- < max_dev)
 *                         [&& |E_i - E_j| < max_dE when energies != NULL: applies to both handednesses]
 *
 * -- the OR of two complete tests, not "the smaller rmsd, then its max deviation".  Comparison operators, max_dev,
 * conformer order, fc_prune_conventions and the k-ladder exactly as in fc_rmsd_simbits / fc_prune_rmsd: only the
 * predicate changes.  A pair is grey when EITHER handedness is within 1e-9 of a threshold by the rule of
 * fc_rmsd_simbits; it is counted once (n_grey, stats[3]).  Explicit entry points, no mode on the handle: every other
 * entry point does what it did.  Same argument checks, error codes and limits as the sibling named in each line; the
 * screen that runs is the one the default prune of the same ensemble runs (fc_screen_last_kind).
 *
 * fc_ensemble_rmsd_pairs_inv / fc_kabsch_rmsd_pairs_inv: (r-, m-) of fc_ensemble_rmsd_pairs / fc_kabsch_rmsd_pairs'
 * pairs, literally rmsd_and_max(p, -q, center): with center = 1 the centroids are removed first, then q is negated;
 * with center = 0 the caller's coordinates are negated as they are.
 * fc_rmsd_simbits_enant: fc_rmsd_simbits with similar_enant.   fc_prune_rmsd_enant: fc_prune_rmsd with it (stats alike). */
int fc_ensemble_rmsd_pairs_inv(fc_ensemble *ens, const int64_t *pair_i, const int64_t *pair_j, int64_t P,
                               double *rmsd_out, double *maxdev_out);
int fc_kabsch_rmsd_pairs_inv(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask, const int64_t *pair_i,
                             const int64_t *pair_j, int64_t P, int center, double *rmsd_out, double *maxdev_out);
int fc_rmsd_simbits_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                          int64_t row_begin, int64_t row_end, uint64_t *bits_out, int64_t *n_grey);
int fc_prune_rmsd_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                        int64_t min_per_group, uint8_t *mask_out, int64_t *stats);
/* One of the conventions of prism_pruner's pruner that the reference tree does not show (SURVEY.md
 * Appendix A) as a switch: 0 (default) = inside a chunk a structure is removed at the first LATER
 * similar one; 1 = the mirror rule (a structure falls to any earlier similar one of its chunk).
 * The other conventions need no kernel support: "<" against "<=" is one ulp on the threshold
 * (firecode_amd.pruner.CONVENTIONS).  Process-wide; 1 is served by the pair ladder only
 * (FC_E_INVALID from a prune that needs the bit-matrix levels). */
int fc_prune_conventions(int drop_later);
/* greedy k-ladder replay over caller-supplied bits (N rows x ceil(N/64) words) */
int fc_greedy_prune_from_bits(const uint64_t *bits, int64_t N, int64_t min_per_group,
                              uint8_t *mask_out);

/* ---- similarity clusters: the connected components of the prune's graph ----
 * The contract, once.  X = the prepared ensemble in processing order.  G = the undirected graph on its N conformers with
 * an edge (i, j) exactly when bit j of row i of fc_rmsd_simbits would be set (fc_rmsd_clusters_enant: of
 * fc_rmsd_simbits_enant): the same thresholds, the same "<", max_dev, energy window and grey counting.
 * fc_prune_conventions and min_per_group play no part.  Outputs:
 *
 *   labels_out (N, int32)                 the cluster of each conformer; clusters are numbered 0 .. K-1 by ascending
 *                                         smallest member index
 *   reps_out   (N entries, K written)     the smallest member index of each cluster
 *   sizes_out  (N entries, K written)     member counts
 *   *n_clusters = K
 *
 * The result is a function of G alone: not of launch order, nor of which internal path ran (the exact similar-pair list
 * in the usual case; the bit matrix when similarity is dense or the candidate queue overflowed).  The host pre-sorts by
 * energy with the stable argsort of prune_by_rmsd, so "smallest index" is "lowest energy, earliest on ties" whenever
 * energies are given.  stats (6 values, may be NULL): [0] pairs evaluated, [1] pairs refined, [2] edges, [3] grey pairs,
 * [4] 1 if the bit-matrix path produced the result, else 0, [5] K.  N = 0: K = 0.  Limit: N < 2^31 - 256.
 * Argument checks as in fc_prune_rmsd (FC_E_INVALID: NULL ens / outputs, thresholds <= 0).  FC_E_INTERNAL: a union
 * exceeded its retry bound on the device (cannot happen by the termination argument of fc_clusters.hip; an error code
 * instead of a hang if that argument is ever broken).
 *
 * fc_clusters_from_pairs / fc_clusters_from_bits: the same labelling of a caller's graph, host arrays in (e.g. the output
 * of fc_prune_similar_pairs, fc_tfd_simbits, fc_moi_simbits).  pairs: n_pairs entries (i << 32) | j, in either order,
 * duplicates allowed; i == j or an index >= N is FC_E_INVALID, checked on the host before any device use.  bits: N rows
 * of ceil(N/64) words, the layout of fc_greedy_prune_from_bits; only bits j > i are read. */
int fc_rmsd_clusters(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                     int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int64_t *n_clusters, int64_t *stats);
int fc_rmsd_clusters_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                           int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int64_t *n_clusters,
                           int64_t *stats);
int fc_clusters_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int32_t *labels_out, int64_t *reps_out,
                           int64_t *sizes_out, int64_t *n_clusters);
int fc_clusters_from_bits(const uint64_t *bits, int64_t N, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out,
                          int64_t *n_clusters);

/* ---- density-based clusters: core, border and noise on the prune's graph (DBSCAN) ----
 * The contract, once.  G = exactly the graph of fc_rmsd_clusters on the N conformers in processing order (fc_rmsd_dbscan_enant:
 * of fc_rmsd_clusters_enant; fc_rmsd_dbscan_perm: of fc_rmsd_clusters_perm): the same thresholds, "<", max_dev, energy
 * window and grey handling.  fc_prune_conventions and min_per_group play no part.  With m = min_samples >= 1:
 *
 *   degree  d(i) = the number of neighbours of i in G: i itself excluded, every unordered pair counted once
 *   core    i is a core point when d(i) + 1 >= m (the point counts itself: the usual DBSCAN convention)
 *   cluster a connected component of the subgraph induced on the core points.  Its representative is its smallest core
 *           member; clusters are numbered 0 .. K-1 by ascending representative
 *   border  a point that is not core and has at least one core neighbour joins the cluster of its SMALLEST-INDEX core
 *           neighbour (textbook DBSCAN leaves that choice to the visiting order; here the result is a function of G and
 *           the processing order alone, never of launch order or of which internal path ran)
 *   noise   a point that is not core and has no core neighbour: label -1
 *
 *   labels_out  (N, int32)              the cluster of each conformer, -1 for noise
 *   reps_out    (N entries, K written)  the smallest core member of each cluster
 *   sizes_out   (N entries, K written)  core and border members of each cluster
 *   core_out    (N, uint8)              1 for a core point
 *   degrees_out (N, int32)              d(i): the local density of a conformer at the prune's threshold
 *   *n_clusters = K
 *
 * The host pre-sorts by energy as for fc_rmsd_clusters, so with usable energies the representative is the lowest-energy
 * core member.  m = 1: labels, reps and sizes are those of fc_rmsd_clusters, exactly.  m = 2: the same, except that
 * clusters of one become noise.  stats (8 values, may be NULL): [0 .. 5] as fc_rmsd_clusters, [6] core points, [7] noise
 * points.  N = 0: K = 0.  Limit: N < 2^31 - 256.  FC_E_INVALID before any device use: min_samples < 1, NULL ens / outputs,
 * thresholds <= 0 (fc_rmsd_dbscan_perm: first the table's checks, as fc_rmsd_clusters_perm).  FC_E_INTERNAL: as fc_rmsd_clusters.
 *
 * fc_dbscan_from_pairs / fc_dbscan_from_bits: the same labelling of a caller's graph, host arrays in the formats of
 * fc_clusters_from_pairs / fc_clusters_from_bits with the same host-side index checks.  ONE DIFFERENCE from the components:
 * degrees count list entries, so fc_dbscan_from_pairs requires every unordered pair AT MOST ONCE (in either order), as
 * fc_prune_similar_pairs delivers it; a pair listed twice counts twice in both degrees.  The bit form cannot hold a pair
 * twice: only bits j > i are read. */
int fc_rmsd_dbscan(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_samples, const double *energies,
                   double max_dE, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, uint8_t *core_out,
                   int32_t *degrees_out, int64_t *n_clusters, int64_t *stats);
int fc_rmsd_dbscan_enant(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_samples, const double *energies,
                         double max_dE, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, uint8_t *core_out,
                         int32_t *degrees_out, int64_t *n_clusters, int64_t *stats);
int fc_dbscan_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int64_t min_samples, int32_t *labels_out,
                         int64_t *reps_out, int64_t *sizes_out, uint8_t *core_out, int32_t *degrees_out,
                         int64_t *n_clusters);
int fc_dbscan_from_bits(const uint64_t *bits, int64_t N, int64_t min_samples, int32_t *labels_out, int64_t *reps_out,
                        int64_t *sizes_out, uint8_t *core_out, int32_t *degrees_out, int64_t *n_clusters);

/* ---- sphere-exclusion clusters: centroids and their members on the prune's graph (Butina 1999) ----
 * The contract, once.  G = exactly the graph of fc_rmsd_clusters on the N conformers in processing order (fc_rmsd_butina_enant:
 * of fc_rmsd_clusters_enant; fc_rmsd_butina_perm: of fc_rmsd_clusters_perm): the same thresholds, "<", max_dev, energy
 * window and grey handling.  fc_prune_conventions and min_per_group play no part.
 *
 *   degree    d(i) = the number of neighbours of i in G, as fc_rmsd_dbscan counts them
 *   priority  i comes before j when d(i) > d(j), or d(i) == d(j) and i < j
 *   walk      the conformers are visited in priority order.  One that is unassigned when the walk reaches it becomes a
 *             CENTROID and takes itself and every neighbour that is still unassigned.  Degrees are never recomputed:
 *             Butina's fixed order (RDKit: reordering=False)
 *
 * The walk is these two statements, which are what the device computes:
 *   - v is a centroid exactly when none of its neighbours that come before it is a centroid;
 *   - the centroid of any other conformer u is the first centroid, in priority order, among u's neighbours.
 * So every member is a neighbour of its centroid (within max_rmsd and max_dev of it), and no two centroids are neighbours.
 *
 *   labels_out  (N, int32)              the cluster of each conformer; clusters numbered 0 .. K-1 by ascending centroid index
 *   reps_out    (N entries, K written)  the centroids
 *   sizes_out   (N entries, K written)  members of each cluster, the centroid included
 *   degrees_out (N, int32)              d(i)
 *   *n_clusters = K
 *
 * The host pre-sorts by energy as for fc_rmsd_clusters, so among conformers of one degree the lower energy comes first.
 * The result is a function of G and the processing order alone: never of launch order, grid size, FC_BUTINA_ROUNDS, or
 * of which source (pair list or bit matrix) produced it.  stats (8 values, may be NULL): [0 .. 5] as fc_rmsd_clusters,
 * [6] the synchronous rounds of the rule the device needed (the dependency depth of the walk on this graph; the same for
 * every setting of the knob), [7] the conformers still undecided when the grid-wide rounds ended (FC_BUTINA_ROUNDS of them
 * and the one that writes down what is left), which one workgroup then finished.  N = 0: K = 0.  Limit: N < 2^31 - 256.
 * FC_E_INVALID before any device use: NULL ens / outputs, thresholds <= 0 (fc_rmsd_butina_perm: first the table's checks,
 * as fc_rmsd_clusters_perm).  FC_E_INTERNAL: as fc_rmsd_clusters, and when the finish ran out of its round bound (one
 * round per conformer it was given; every round decides at least one).
 *
 * fc_butina_from_pairs / fc_butina_from_bits: the same labelling of a caller's graph, in the formats and with the host-side
 * checks of fc_dbscan_from_pairs / fc_dbscan_from_bits; as there, every unordered pair AT MOST ONCE in the list.
 *
 * Against RDKit's Butina.ClusterData, two differences in the definition: RDKit takes "<=" at the threshold and breaks
 * degree ties by the HIGHEST index; here it is the prune's "<" and the lowest index (the lowest energy).  Parity with
 * RDKit is not pinned by any test (it is not part of the build).  reordering=True (degrees updated
 * after every cluster) is not offered. */
int fc_rmsd_butina(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                   int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int32_t *degrees_out, int64_t *n_clusters,
                   int64_t *stats);
int fc_rmsd_butina_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                         int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int32_t *degrees_out,
                         int64_t *n_clusters, int64_t *stats);
int fc_butina_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int32_t *labels_out, int64_t *reps_out,
                         int64_t *sizes_out, int32_t *degrees_out, int64_t *n_clusters);
int fc_butina_from_bits(const uint64_t *bits, int64_t N, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out,
                        int32_t *degrees_out, int64_t *n_clusters);

/* ---- symmetry-aware forms: atom permutations of equivalent atoms ----
 * The contract, once.  X = the prepared ensemble of the RMSD stage (atom selection applied, each conformer centred on the
 * centroid of its selected atoms).  perms = a (K, A_sel) row-major table of permutations of the selected atoms, in
 * selected-atom indices 0 .. A_sel-1: row 0 is the identity and the set is closed under inverse (the automorphisms of a
 * bond graph are).  For i < j:
 *
 *   (r_k, m_k) = rmsd_and_max(X[i], X[j][perms[k]])            k = 0 .. K-1
 *   similar_sym(i, j) = any_k (r_k < max_rmsd && m_k < max_dev)     [&& |E_i - E_j| < max_dE when energies != NULL]
 *
 * -- the OR of K complete tests, not "the smallest rmsd, then its max deviation".  Comparison operators, max_dev,
 * conformer order, fc_prune_conventions and the k-ladder exactly as in fc_rmsd_simbits / fc_prune_rmsd; the clusters are
 * the components of that graph, numbered as fc_rmsd_clusters numbers them.  Only the predicate changes.  A pair is grey
 * when any of its r_k, or an m_k whose r_k passes, lies within 1e-9 of its threshold; it is counted once (n_grey,
 * stats[3]).  (Values of k behind a pass that is itself clear of both thresholds are not looked at: they cannot turn
 * the verdict.)  K = 1 gives the bits and the mask of the default forms, bit for bit.  Explicit entry points, no mode on
 * the handle: every other entry point does what it did.
 *
 * One exact-fp64 all-pairs kernel (no screen: fc_screen_last_kind is not touched).  stats as the sibling's, with
 * [1] = pairs whose polynomial test passed for at least one k; fc_rmsd_clusters_perm's [4] = 1 when the bit matrix
 * produced the labels.  Refused before the device is touched -- FC_E_LIMIT: K > FC_PERM_MAX; an A_sel whose tile
 * -- 2 x 16 conformers at ((3 A_sel) | 1) doubles each, the table of 2 K A_sel bytes rounded up to 8, and 8200 bytes of
 * candidate queue -- exceeds the 160 KiB of LDS (A_sel <= 201 at K = 2); N beyond the 32-bit
 * word index of the bit matrix (fc_rmsd_clusters_perm: N >= 2^31 - 256).  FC_E_INVALID: NULL perms, K < 1, A_sel
 * that is not the ensemble's, a row that is not a permutation of 0 .. A_sel-1, row 0 not the identity, a row whose
 * inverse is not in the table; then the sibling's own checks.  The table is checked before the handle is looked at.
 * Not offered: sharded and multi-GPU forms, fc_prune_rmsd_many, the one-call host form, twin workspaces,
 * fc_prune_rmsd_rot_corr, the MOI stage; no combination with the enantiomer-aware forms on the prune and the clusters
 * (the diverse selection has a form that takes both: fc_ensemble_select_diverse_perm).
 *
 * fc_ensemble_rmsd_pairs_perm: all K values of each requested pair (any i, j), rmsd_out and maxdev_out (P, K)
 * row-major: element (p, k) = rmsd_and_max(X[pair_i[p]], X[pair_j[p]][perms[k]]).  Choosing among them is the caller's. */
#define FC_PERM_MAX 64
int fc_ensemble_rmsd_pairs_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, const int64_t *pair_i,
                                const int64_t *pair_j, int64_t P, double *rmsd_out, double *maxdev_out);
int fc_rmsd_simbits_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                         const double *energies, double max_dE, int64_t row_begin, int64_t row_end, uint64_t *bits_out,
                         int64_t *n_grey);
int fc_prune_rmsd_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                       const double *energies, double max_dE, int64_t min_per_group, uint8_t *mask_out, int64_t *stats);
int fc_rmsd_clusters_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd,
                          double max_dev, const double *energies, double max_dE, int32_t *labels_out, int64_t *reps_out,
                          int64_t *sizes_out, int64_t *n_clusters, int64_t *stats);
/* the density-based clusters (above) of the graph of fc_rmsd_clusters_perm */
int fc_rmsd_dbscan_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                        int64_t min_samples, const double *energies, double max_dE, int32_t *labels_out, int64_t *reps_out,
                        int64_t *sizes_out, uint8_t *core_out, int32_t *degrees_out, int64_t *n_clusters, int64_t *stats);
/* the sphere-exclusion clusters (above) of the graph of fc_rmsd_clusters_perm */
int fc_rmsd_butina_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                        const double *energies, double max_dE, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out,
                        int32_t *degrees_out, int64_t *n_clusters, int64_t *stats);

/* sharded form (conformer rows dealt block-cyclically to ranks):
 * fc_prune_rmsd_begin computes this rank's rows of the bit matrix;
 * fc_prune_level applies one ladder level to this rank's rows given the
 * GLOBAL mask of the previous level (mask_in, N bytes) and returns the rows'
 * new flags in mask_out (N bytes, only owned rows written, others copied
 * from mask_in) -- the caller all-gathers between levels. */
/* stats of fc_prune_rmsd_begin: [0] pairs owned by this rank, [1] refined, [2] similar,
 * [3] grey, [4] duration of this rank's screen kernel in ns (HIP events), [5] 0 */
int fc_prune_rmsd_begin(fc_ensemble *ens, double max_rmsd, double max_dev,
                        const double *energies, double max_dE, int64_t rank, int64_t world,
                        int64_t row_block, int64_t *stats);
int fc_prune_level(fc_ensemble *ens, int64_t k, const uint8_t *mask_in, uint8_t *mask_out);
/* Preferred exchange when similar pairs are sparse (the usual case): after
 * fc_prune_rmsd_begin, fc_prune_similar_pairs returns this rank's exactly-
 * similar pairs as (i << 32) | j in processing order indices (n_out = count;
 * FC_E_LIMIT when the candidate queue overflowed -- use fc_prune_level then).
 * The ranks all-gather the lists ONCE and every rank replays the whole ladder
 * locally with fc_prune_from_pairs (pairs from all ranks, any order).
 * fc_prune_from_pairs leaves the rank's own list and its length alone:
 * fc_prune_similar_pairs returns the same list before and after it. */
int fc_prune_similar_pairs(fc_ensemble *ens, uint64_t *pairs_out, int64_t capacity, int64_t *n_out);
int fc_prune_from_pairs(fc_ensemble *ens, const uint64_t *pairs, int64_t n_pairs,
                        int64_t min_per_group, uint8_t *mask_out);
/* The same exchange without leaving the device (multi-GPU path of bench.py):
 *   fc_prune_rmsd_begin_async   enqueue screen + refine of this rank's row blocks, no sync;
 *   fc_prune_export_pairs_dev   write this rank's message into a CALLER-OWNED DEVICE buffer of
 *                               cap+1 words: [count | pairs ... | padding]; count is
 *                               0xFFFFFFFFFFFFFFFE when the candidate queue overflowed;
 *   (caller: one all-gather of the cap+1 words -- RCCL on the stream given to fc_stream_set)
 *   fc_prune_from_gathered_dev  compact the world*(cap+1) gathered words (device pointer), replay
 *                               the whole ladder, ONE sync, mask to the host.  FC_E_LIMIT when a
 *                               rank's list was missing or longer than cap: every rank sees the same
 *                               words, so every rank falls back to the host exchange above together.
 * stats (6): [0] pairs owned, [1] refined, [2] similar (this rank), [3] grey, [4] screen ns,
 * [5] survivors. */
int fc_prune_rmsd_begin_async(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t rank,
                              int64_t world, int64_t row_block);
int fc_prune_export_pairs_dev(fc_ensemble *ens, uint64_t *dev_out, int64_t cap);
int fc_prune_from_gathered_dev(fc_ensemble *ens, const uint64_t *dev_gathered, int64_t world,
                               int64_t cap, int64_t min_per_group, uint8_t *mask_out, int64_t *stats);
/* Stream-ordered form for a batch of n_slots prunes: ..._enqueue(slot) returns without waiting
 * (begin_async, export, all-gather and this call of prune k+1 may be issued while prune k still
 * runs); fc_prune_collect(slot) waits for the stream and delivers that prune's mask and stats
 * (FC_E_LIMIT: its ladder declined -- redo that prune through fc_prune_from_gathered_dev or the
 * host exchange).  Slot 0 must be enqueued first: it sizes the pinned result area of the batch. */
int fc_prune_from_gathered_dev_enqueue(fc_ensemble *ens, const uint64_t *dev_gathered, int64_t world,
                                       int64_t cap, int64_t min_per_group, int64_t slot, int64_t n_slots);
int fc_prune_collect(fc_ensemble *ens, int64_t slot, int64_t n_slots, uint8_t *mask_out, int64_t *stats);
/* Overlap of consecutive sharded prunes of ONE resident ensemble:
 *   fc_ensemble_twin                  a second prune workspace (bit rows, queues, counters, ladder
 *                                     words) over the same coordinates; owned by `ens`, destroyed
 *                                     with it; takes every prune call an ensemble takes;
 *   fc_prune_rmsd_begin_split_async   begin_async with the screen on `screen_stream` (all screens of a
 *                                     batch go there, in order) and counters reset + refine on the
 *                                     current stream (fc_stream_use), tied together with events;
 *                                     timed != 0: HIP events around the screen kernel (what stats[4]
 *                                     of fc_prune_collect reports; ~14 us of stream time).
 * Prune k on workspace k&1 and stream k&1 of two: export, all-gather and ladder of prune k run
 * beside the screen of prune k+1. */
int fc_ensemble_twin(fc_ensemble *ens, fc_ensemble **twin_out);
int fc_prune_rmsd_begin_split_async(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t rank,
                                    int64_t world, int64_t row_block, void *screen_stream, int timed);

/* ---- the exchange of the sharded path: RCCL over xGMI behind the C ABI (no PyTorch) ---------
 * "ensembles shard by conformer across the GPUs of one node with a single RCCL
 * all-gather to reassemble the surviving-conformer mask".  One process per GPU, started by any
 * launcher; librccl.so is bound at run time (dlopen) by the first of these calls, so single-GPU
 * users never load it.  Rank 0 calls fc_comm_unique_id and passes the 128 bytes to the other
 * ranks out of band (firecode_amd/dist.py: a file next to MASTER_PORT, or FC_COMM_ID);
 * every rank then calls fc_comm_init (collective; after fc_init(device of this rank)).
 * Without a communicator the calls below behave as a group of one rank.
 *   fc_allgather_mask     host buffers, blocking: mask_global = world x n_local bytes, rank-major
 *                         (the per-level mask exchange and the pass masks of the pose grid / scan);
 *   fc_allgather_u8_dev   device buffers, enqueued behind the library's current stream;
 *   fc_comm_barrier       all ranks have arrived (a 1-byte all-gather + wait). */
#define FC_COMM_ID_BYTES 128
int fc_comm_unique_id(uint8_t *id_out);
int fc_comm_init(int64_t rank, int64_t world, const uint8_t *id);
int fc_comm_destroy(void);
int fc_comm_info(int64_t *rank, int64_t *world);
int fc_allgather_mask(const uint8_t *mask_local, int64_t n_local, uint8_t *mask_global);
int fc_allgather_u8_dev(const uint8_t *send_dev, uint8_t *recv_dev, int64_t bytes_per_rank);
int fc_comm_barrier(void);
/* test hook: act as `rank` of `world` without a communicator -- the all-gather writes only this
 * rank's slot and leaves the others as earlier calls left them, so the logical ranks of one GPU can
 * be run one after the other (tests/test_gpu_parity.py); world = 0 switches it off */
int fc_debug_comm_loopback(int64_t rank, int64_t world);
/* prune_by_rmsd over the ranks of the communicator: every rank holds the whole ensemble and
 * calls this with the same arguments; rows of the similarity matrix are dealt in snake order
 * (row_block rows at a time, <= 0: default), each rank screens + refines its own, ONE all-gather of
 * the ranks' exactly-similar pair lists (cap = 1024 + 4N/world pairs each), the whole k-ladder
 * replayed on every rank: identical mask_out (N bytes) everywhere.  Dense similarity (a list that
 * does not fit): one fc_allgather_mask per ladder level instead, decided alike on every rank.
 * stats (6, may be NULL): [0] pairs owned, [1] refined, [2] similar (this rank), [3] grey,
 * [4] screen kernel ns, [5] survivors. */
int fc_prune_rmsd_sharded(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_per_group,
                          int64_t row_block, uint8_t *mask_out, int64_t *stats);

/* ---- a7: prune_by_rmsd_rot_corr(structures, atoms, graph, max_rmsd=, energies=, max_dE=) --
 * prism_pruner.pruner (NOT in the reference tree); call sites firecode/ensemble.py:253-260,
 * embedder.py:1489-1496, operators.py:626-632.  PARITY UNPINNED: restated after the predecessor's
 * published routine (see the kernel's header).  The caller does the graph perception and passes
 * the locally symmetric torsions (T,4), the rotation mask of each (T,A: atoms that move with i4,
 * firecode/torsion_module.py:354-382), and per torsion its n-fold trial angles in degrees
 * (angles (T,max_angles), n_angles (T); 0 first, as Torsion.get_angles gives them).
 * Structures are centred on their plain mean; similarity = rmsd_and_max over heavy_mask atoms
 * after the torsional correction; then the same k-ladder as fc_prune_rmsd.  coords in processing
 * order (energy-sorted by the caller when energies are given).  bits_out: optional (N, W).
 * Limits, both refused with FC_E_LIMIT before the device is touched: 4*A*24 bytes <= 160 KiB of LDS
 * (A <= 1706), and N <= FC_ROTCORR_MAX_ROWS: the kernel takes one grid row per structure, and 65 535
 * is the y extent every HIP device guarantees.  The stage is meant for ensembles the MOI and RMSD
 * stages have already thinned (one wavefront per pair: 2e9 of them at the limit). */
#define FC_ROTCORR_MAX_ROWS 65535
int fc_prune_rmsd_rot_corr(const double *coords, int64_t N, int64_t A, const uint8_t *heavy_mask,
                           const int64_t *torsions, int64_t T, const uint8_t *rotation_masks,
                           const double *angles, const int32_t *n_angles, int64_t max_angles,
                           double max_rmsd, double max_dev, const double *energies, double max_dE,
                           int64_t min_per_group, uint8_t *mask_out, uint64_t *bits_out);

/* ---- a9: align_by_moi(atoms, structures) -- firecode/hypermolecule_class.py:45-86.
 * Every structure centred on its plain mean; M = get_alignment_matrix(diag(I_ref), diag(I_n))
 * applied as (M @ X.T).T; structure 0 is copied unrotated.  masses (A,), out (N, A, 3). */
int fc_align_by_moi(const double *coords, int64_t N, int64_t A, const double *masses, double *out);

/* ---- a6: prune_by_moment_of_inertia -- prism_pruner.pruner; call sites
 * firecode/ensemble.py:211-216, embedder.py:1452-1454.
 * fc_inertia_moments: get_inertia_moments(coords, masses) for N conformers,
 * moments_out (N,3) ascending. */
int fc_inertia_moments(const double *coords, int64_t N, int64_t A, const double *masses,
                       double *moments_out);
int fc_prune_moi(const double *coords, int64_t N, int64_t A, const double *masses,
                 double max_deviation, const double *energies, double max_dE,
                 int64_t min_per_group, uint8_t *mask_out);
/* The similarity bits fc_prune_moi replays: bit j of row i (j > i only) is set when
 *   not (|I_i[k] - I_j[k]| / I_i[k] >= max_deviation)   for k = 0, 1, 2
 * [and |E_i - E_j| < max_dE when energies are given].  The negated form is the reference's early exit:
 * a zero moment against a zero moment (0/0, not a number) does not tell two structures apart, a zero
 * moment against a non-zero one (infinite) does.  bits_out (N, ceil(N/64)) words. */
int fc_moi_simbits(const double *coords, int64_t N, int64_t A, const double *masses, double max_deviation,
                   const double *energies, double max_dE, uint64_t *bits_out);

/* ---- a2/a3: the similarity stages of the drivers on ONE upload -- Ensemble.similarity_pruning
 * (firecode/ensemble.py:205-235) and Embedder.similarity_refining (embedder.py:1445-1474) run
 * prune_by_moment_of_inertia, apply its mask, then prune_by_rmsd on the survivors.  coords (N, A, 3) in
 * processing order (energy-sorted by the caller when energies are given) are uploaded once; the MOI
 * stage (do_moi; all atoms, `masses`, relative tolerance moi_tol) works on them in HBM, its survivors
 * are gathered on the device into the RMSD stage's layout (do_rmsd; atoms of heavy_mask, NULL = all),
 * the masks are composed on the way out.  Each stage's result is the stand-alone entry point's.
 * mask_moi_out (N bytes, may be NULL): after the MOI stage; mask_out (N bytes): after both;
 * counts (3, may be NULL): structures in, after MOI, after RMSD. */
int fc_prune_similarity(const double *coords, int64_t N, int64_t A, const uint8_t *heavy_mask, const double *masses,
                        int do_moi, double moi_tol, int do_rmsd, double max_rmsd, double max_dev,
                        const double *energies, double max_dE, int64_t min_per_group, uint8_t *mask_moi_out,
                        uint8_t *mask_out, int64_t *counts);

/* ---- a8: align_structures(structures, indices) -- prism_pruner.utils;
 * call sites embedder.py:1704,1910,2218,2300; operators.py:262.
 * out (N,A,3): every conformer superposed on conformer 0 using the n_idx
 * atoms in idx (NULL = all). */
int fc_align_to_first(const double *coords, int64_t N, int64_t A, const int64_t *idx,
                      int64_t n_idx, double *out);

/* ---- a13: get_embed -- firecode/embeds.py:808-817: out[k] = (R_k @ X_k.T).T + t_k
 * for n blocks of A atoms (R (n,3,3), t (n,3)). */
int fc_rototranslate(const double *coords, int64_t n, int64_t A, const double *R,
                     const double *t, double *out);

/* ---- a11/a12: count_clashes (firecode/algebra.py:52-54) and
 * compenetration_check (firecode/utils.py:507-575), batched over N structures.
 * fc_clash_self: ordered pairs with lo < d < hi (reference: 0 < d < 0.5).
 * fc_clash_fragments: ids = fragment lengths (2 or 3 entries); bimolecular
 * counts d < thresh, trimolecular counts d <= thresh cumulatively over
 * (m2,m1),(m3,m2),(m1,m3); pass_out[n] = 1 when within max_clashes. */
int fc_clash_self(const double *coords, int64_t N, int64_t A, double lo, double hi,
                  int64_t *counts_out);
int fc_clash_fragments(const double *coords, int64_t N, int64_t A, const int64_t *ids,
                       int64_t n_ids, double thresh, int64_t max_clashes,
                       int64_t *counts_out, uint8_t *pass_out);

/* graph mode of compenetration_check (utils.py:528-542): ordered, off-diagonal,
 * NON-BONDED pairs with d < thresh; adj is an (A, A) byte adjacency matrix. */
int fc_clash_graph(const double *coords, int64_t N, int64_t A, const uint8_t *adj, double thresh,
                   int64_t *counts_out);
/* ---- bond-topology check: molecule_check / scramble_check (firecode/utils.py:341-400), batched over N structures
 * (DESIGN.md section 11).  The bond rule is graphize's: i < j are bonded in a structure iff
 *   fl(sqrt(((dx*dx) + dy*dy) + dz*dz)) < class_thresh[atom_class[i] * n_class + atom_class[j]]     (strict <)
 * -- the caller fills class_thresh (n_class x n_class, symmetric, 1 <= n_class <= 64) with graphize's own
 * fl(1.2 * fl(r_p + r_q)); the library turns each entry into a squared threshold once (no square roots on the device).
 * For structure n (coords (N, A, 3)):
 *   delta(n) = { i < j : bonded(coords[n], i, j) != (i, j) in B_ref(n) }  minus every pair with i or j in excluded(n)
 *   counts_out[n] = |delta(n)|,  ok_out[n] = counts_out[n] <= max_newbonds   (negative max_newbonds: never ok)
 * Exactly one reference:
 *   molecule mode  ref_coords: B_ref(n) = the bonds of ref_coords + n * ref_stride (ref_stride 0: one (A, 3) reference
 *                  shared by all structures; 3A: (N, A, 3), one per structure), ref_bits = NULL;
 *   scramble mode  ref_bits: (A, ceil(A/64)) uint64 words, bit j of row i (word j/64, bit j%64) set when i-j is a
 *                  reference bond (only i < j is read), shared by all structures; ref_coords = NULL.
 * excluded(n): CSR over atom indices -- excl_offsets (excl_sets + 1, [0] = 0, non-decreasing), excl_atoms; excl_sets
 * = 1 (one set for all structures) or N; values outside [0, A) and duplicates are ignored.  excl_offsets = NULL: none.
 * counts_out / ok_out (N, either may be NULL).
 * fc_bond_changes_list: the changed bonds themselves.  offsets (N + 1) = 0 followed by the running sum of the
 * counts of fc_bond_changes on the same inputs; bonds_out (offsets[N], 3) int64: rows offsets[n] .. offsets[n+1]-1
 * are structure n's (i, j, +1 formed / -1 broken) in row-major (i, j) order.  FC_E_INVALID when the offsets do not
 * match the counts (nothing is written).
 * FC_E_INVALID before any device use: bad shape, NULL pointers, class or stride out of range, both or neither
 * reference, malformed offsets.  N = 0: nothing to do.  FC_E_LIMIT: A >= 2^31, or more device memory than the device
 * has.  Any A and N otherwise: structures are read from HBM in row tiles, not staged in LDS. */
int fc_bond_changes(const double *coords, int64_t N, int64_t A, const int32_t *atom_class, int64_t n_class,
                    const double *class_thresh, const double *ref_coords, int64_t ref_stride, const uint64_t *ref_bits,
                    const int64_t *excl_offsets, const int64_t *excl_atoms, int64_t excl_sets, int64_t max_newbonds,
                    int64_t *counts_out, uint8_t *ok_out);
int fc_bond_changes_list(const double *coords, int64_t N, int64_t A, const int32_t *atom_class, int64_t n_class,
                         const double *class_thresh, const double *ref_coords, int64_t ref_stride,
                         const uint64_t *ref_bits, const int64_t *excl_offsets, const int64_t *excl_atoms,
                         int64_t excl_sets, const int64_t *offsets, int64_t *bonds_out);
/* a21: fitness_check (optimization_methods.py:163-180) for N structures with C
 * constraints each: pairs (N, C, 2), targets (N, C) (NaN = no target);
 * pass_out[n] = sum(|x_a - x_b| - target) < threshold; error_out may be NULL. */
int fc_fitness_check(const double *coords, int64_t N, int64_t A, const int64_t *pairs,
                     const double *targets, int64_t C, double threshold, double *error_out,
                     uint8_t *pass_out);

/* ---- a14: bimolecular rigid embed poses -- firecode/embeds.py:713-722:
 * pose k uses conformer c1[k] of m1 (n1,A1,3) moved by (R1[k], t1[k]) and
 * conformer c2[k] of m2 (n2,A2,3) moved by (R2[k], t2[k]); counts atom pairs
 * closer than thresh (strict <) without materialising the pose;
 * pass_out[k] = count <= max_clashes.  poses_out (may be NULL): (P, A1+A2, 3). */
int fc_embed_poses_clash(const double *m1, int64_t n1, int64_t A1, const double *m2,
                         int64_t n2, int64_t A2, const int64_t *c1, const int64_t *c2,
                         const double *R1, const double *t1, const double *R2,
                         const double *t2, int64_t P, double thresh, int64_t max_clashes,
                         int64_t *counts_out, uint8_t *pass_out, double *poses_out);

/* Whole bimolecular rigid-embed grid (embeds.py:597-722 for one pivot per
 * conformer): molecule i has n_i conformers of A_i atoms, nr_i (1 or 2)
 * reactive atom indices, one pivot (start, end 3-vectors) per conformer and
 * na_i step angles (degrees).  fc_embed_mol_transforms returns the per-
 * molecule tables R (n,2,na,3,3), t (n,2,na,3) over (conformer, orientation,
 * angle); fc_embed_grid_clash tests every pose
 *   p = ((c2*n1 + c1)*2 + o)*(na1*na2) + (a2*na1 + a1)
 * (the reference's loop order) and writes pass_out[p] = count(d < thresh) <=
 * max_clashes; counts_out (may be NULL) saturates just above max_clashes:
 * molecule-2 atoms b are taken in order, the whole row b (all molecule-1 atoms)
 * is added while the running count is <= max_clashes, then counting stops.
 * Exact for any coordinates: NaN and +-inf distances never count (`<` is
 * false), far-away coordinates only make the fp32 screen pass more pairs on to
 * the fp64 recount.  Limit: A1 <= 1636 (A1*40 + 64 bytes of LDS <= 64 KiB),
 * FC_E_LIMIT beyond. */
int fc_embed_mol_transforms(const double *coords, int64_t n, int64_t A, const int64_t *reactive,
                            int64_t nr, const double *pivot_start, const double *pivot_end,
                            int64_t mol, const double *angles, int64_t na, double *R_out,
                            double *t_out);
int fc_embed_grid_clash(const double *m1, int64_t n1, int64_t A1, const int64_t *reactive1,
                        int64_t nr1, const double *ps1, const double *pe1, const double *m2,
                        int64_t n2, int64_t A2, const int64_t *reactive2, int64_t nr2,
                        const double *ps2, const double *pe2, const double *angles1, int64_t na1,
                        const double *angles2, int64_t na2, double thresh, int64_t max_clashes,
                        uint8_t *pass_out, int32_t *counts_out, double *ms_kernel);
/* same grid followed by the in-group de-duplication of embeds.py:723
 * (rmsd_similarity(pose, poses kept so far in this (conformer pair, orientation)
 * group, rmsd_thr)): accept_out[p] = pass[p] && the pose is new.
 * Limits: A1 as above; na1*na2 <= 4096 angle pairs per group (the LDS list of
 * kept poses), FC_E_LIMIT beyond; rmsd_thr > 0 (FC_E_INVALID). */
int fc_embed_grid_dedupe(const double *m1, int64_t n1, int64_t A1, const int64_t *reactive1,
                         int64_t nr1, const double *ps1, const double *pe1, const double *m2,
                         int64_t n2, int64_t A2, const int64_t *reactive2, int64_t nr2,
                         const double *ps2, const double *pe2, const double *angles1, int64_t na1,
                         const double *angles2, int64_t na2, double thresh, int64_t max_clashes,
                         double rmsd_thr, uint8_t *pass_out, uint8_t *accept_out);

/* ---- a14, three molecules: the body of cyclical_embed, firecode/embeds.py:409-585.
 * A "job" is one (conformer triple, pivot triple); the host enumerates jobs in the reference's
 * loop order and supplies, per job: conf (J,3); the three pivots' start / end points
 * (J,3,3 each; Pivot.pivot = start - end); polygonize(norms) as vecs (J,8,3,2,3);
 * _get_directions(norms) as dirs0 (J,3,3); run (J,8) = the orientation passes the pairings filter
 * (:471-475); rtab (J,8,3,3): atom index of molecule m's reactive atom facing molecule k
 * (the r table of :338-352); norms (J,3).  ua (3,U): distinct step angles (degrees) per molecule,
 * aidx (S,3) int32: pose s of embedder.systematic_angles -> indices into ua.
 * Per job the 8 orientations run in order: _adjust_directions (:262-407, 343 candidates, first
 * minimum) whose result also seeds the next orientation; then the S poses: R, t per molecule
 * (:488-546), trimolecular compenetration_check (utils.py:556-575, d <= thresh, sum over the three
 * fragment pairs <= max_clashes) and the rmsd_similarity(rmsd_thr) filter against the poses
 * already accepted in the group (:553-566).
 * Out: dirs_out (J,8,3,3) directions used by each orientation; Rt_out (J,8,3,U,12): R (9, row
 * major) and t (3) of molecule i at step angle u; pass_out / accept_out (J,8,S) uint8.
 * Limits (FC_E_LIMIT beyond): U <= 85; J*8*S < 2^31; the LDS of one group,
 *   U*Atot*24 + 3*U*96 + 3*U*U*4 + S*5 bytes rounded up to 16, <= 160 KiB. */
int fc_embed_trimolecular(const double *const coords[3], const int64_t n_conf[3], const int64_t n_atoms[3],
                          const int64_t *const reactive[3], const int64_t n_reactive[3], int64_t J,
                          const int64_t *conf, const double *piv_start, const double *piv_end,
                          const double *vecs, const double *dirs0, const uint8_t *run, const int64_t *rtab,
                          const double *norms, const double *ua, int64_t U, const int32_t *aidx, int64_t S,
                          double thresh, int64_t max_clashes, double rmsd_thr, double *dirs_out,
                          double *Rt_out, uint8_t *pass_out, uint8_t *accept_out);

/* String embed (firecode/embeds.py:51-158) for two molecules with one reactive atom
 * each: molecule i has n_i conformers, K_i orbital centres per conformer
 * (centers_i, orbvecs_i: (n_i, K_i, 3) -- RAtom.center / .orb_vecs) and the run
 * has nA rotation angles.  Pose p = ((c2*n1 + c1)*(K1*K2) + (k2*K1 + k1))*nA + ia
 * (the reference's loop order).  pass_out[p]: compenetration_check of the pose;
 * accept_out[p]: passed AND its torsion fingerprint over quads (Q,4; atom indices
 * in the concatenated pose) is not TFD-similar (tfd_thresh) to any pose accepted
 * before it.  R2_out (P,3,3) / t2_out (P,3) (may be NULL): molecule 2's transform
 * (molecule 1 is not moved).  Limits (FC_E_LIMIT beyond): Q <= 128;
 * A1 <= 1706 (four structures of A1*24 bytes in 160 KiB of LDS). */
int fc_string_embed(const double *m1, int64_t n1, int64_t A1, const double *centers1,
                    const double *orbvecs1, int64_t K1, const double *m2, int64_t n2, int64_t A2,
                    const double *centers2, const double *orbvecs2, int64_t K2,
                    const double *angles, int64_t nA, const int64_t *quads, int64_t Q,
                    double thresh, int64_t max_clashes, double tfd_thresh, uint8_t *pass_out,
                    uint8_t *accept_out, double *R2_out, double *t2_out);

/* ---- a17-a19: torsion scan -- firecode/torsion_module.py:812-856
 * (clustered_csearch inner loops) with rotate_dihedral (prism_pruner.utils)
 * and torsion_comp_check (torsion_module.py:894-918).
 * base (A,3); torsions (T,4) int64; rotmasks (T,A) bytes; angles (S,T) int64
 * degrees.  coords_out (S,A,3); rotated_bonds_out (S) int64. */
int fc_torsion_scan(const double *base, int64_t A, const int64_t *torsions, int64_t T,
                    const uint8_t *rotmasks, const int64_t *angles, int64_t S, double thresh,
                    int64_t backoff_deg, double *coords_out, int64_t *rotated_bonds_out);
/* The same scan with the torsion fingerprint of every generated conformer taken while it is
 * still in LDS (get_torsion_fingerprint, torsion_module.py:1070-1077): tf_out (S, Q) degrees for
 * quads (Q,4).  coords_out may be NULL -- for 1.7 M angle-sets the conformers are 2 GB of which
 * prune_conformers_tfd keeps a few thousand: fingerprint all, prune, re-scan only the survivors. */
int fc_torsion_scan_fingerprints(const double *base, int64_t A, const int64_t *torsions, int64_t T,
                                 const uint8_t *rotmasks, const int64_t *angles, int64_t S, double thresh,
                                 int64_t backoff_deg, const int64_t *quads, int64_t Q, double *tf_out,
                                 int64_t *rotated_bonds_out, double *coords_out);
/* fc_torsion_scan_fingerprints followed by the TFD prune of `[starting structure] + [scanned conformers
 * with at least one rotated bond]`, the list clustered_csearch hands to prune_conformers_tfd
 * (firecode/torsion_module.py:858-870, 957-1043) -- with the fingerprints never leaving the device
 * (at 1.7 M angle-sets they are 107 MB each way).  keep_out: S + 1 bytes, [0] = the starting structure,
 * [1 + s] = 1 when conformer s rotated a bond AND survived the prune.  Same mask as fc_tfd_prune on the
 * same rows. */
int fc_torsion_scan_tfd(const double *base, int64_t A, const int64_t *torsions, int64_t T, const uint8_t *rotmasks,
                        const int64_t *angles, int64_t S, double thresh, int64_t backoff_deg, const int64_t *quads,
                        int64_t Q, double tfd_thresh, int64_t *rotated_bonds_out, uint8_t *keep_out);
/* fc_torsion_scan_tfd over the whole n-fold grid of clustered_csearch (firecode/torsion_module.py:822: `for angles in
 * cartesian_product(*rotations)`): values = the T value lists one after the other (counts[t] entries each, degrees), the
 * S = prod counts angle-sets are the rows of the reference's cartesian_product (firecode/utils.py:219-221, array #2
 * slowest, then #1, #3 ... #T) and are generated on the device -- at 8 x 6-fold the grid is 107 MB that otherwise is built
 * on the host and sent.  rotated_bonds_out: S, keep_out: S + 1, row numbers = row numbers of that product. */
int fc_torsion_scan_tfd_grid(const double *base, int64_t A, const int64_t *torsions, int64_t T, const uint8_t *rotmasks,
                             const int64_t *values, const int64_t *counts, double thresh, int64_t backoff_deg,
                             const int64_t *quads, int64_t Q, double tfd_thresh, int64_t *rotated_bonds_out, uint8_t *keep_out);

/* ---- a20: torsion fingerprints and TFD similarity bits --
 * firecode/torsion_module.py:1046-1076.
 * tf_out (N,Q) degrees in (-180,180].  fc_tfd_simbits: bit j of row i (all
 * j != i) = sum |wrap(tf_i - tf_j)| < thresh; rows [row_begin,row_end). */
int fc_torsion_fingerprint(const double *coords, int64_t N, int64_t A, const int64_t *quads,
                           int64_t Q, double *tf_out);
int fc_tfd_simbits(const double *tf, int64_t N, int64_t Q, double thresh, int64_t row_begin,
                   int64_t row_end, uint64_t *bits_out);

/* prune_conformers_tfd at any N (firecode/torsion_module.py:957-1043):
 * fc_tfd_first_match: first_out[i] = min{ j > i : TFD-similar(i, j) } or -1 (GPU).  From 65 536 structures on
 * (and angles within +-270 degrees, all finite: the reference's delta is the circular distance exactly there) the
 * pair tests run on 16-bit angles with the fp64 sum in NumPy's order for every pair within 0.055 degrees of the
 * threshold -- same array as the fp32-filtered kernels, which serve every other input (FC_TFD_U16=0: always);
 * fc_tfd_ladder_from_first_match: the reference's k-ladder / match-graph /
 * "keep group[0]" bookkeeping replayed from that array -- bit-identical to the
 * reference under CPython >= 3.8 + networkx 3.x because it reproduces their set
 * iteration order.  With an initialised device and N >= 20000 the ladder runs
 * there (fc_tfd_ladder.hip; FC_TFD_GPU=0: on the host anyway), otherwise it is
 * pure host code (no device needed);
 * fc_tfd_prune = both. */
int fc_tfd_first_match(const double *tf, int64_t N, int64_t Q, double thresh, int64_t *first_out);
/* The device form the last first-match took (fc_tfd_first_match, fc_tfd_prune, fc_torsion_scan_tfd*), as bits:
 * 1 = one-phase fp32 kernel, 2 = fp32 look-ahead + column chunks, 4 = 16-bit dense phase, 8 = 16-bit walk launched
 * (rows were left open), 16 = the 16-bit path refused the angles and the fp32 kernels redid the array; 0 = none yet
 * (or N = 0, or Q = 0, which launches nothing).  n_open_out (may be NULL): the rows still open after the first phase.  Results do not depend on it. */
int fc_tfd_last_form(int64_t *n_open_out);
int fc_tfd_ladder_from_first_match(const int64_t *first_match, int64_t N, uint8_t *mask_out);
int fc_tfd_prune(const double *tf, int64_t N, int64_t Q, double thresh, uint8_t *mask_out);
/* test hooks for the CPython set-order emulation used by the ladder: iteration
 * order of set(keys) (non-negative ints inserted in the given order) and of a
 * set of 2-tuples (returned as indices into the input) */
int fc_debug_pyset_order_ints(const int64_t *keys, int64_t n, int64_t *order_out, int64_t *n_out);
int fc_debug_pyset_order_pairs(const int64_t *pairs, int64_t n, int64_t *order_out, int64_t *n_out);
/* the same order for n DISTINCT pairs computed on the device (fc_tfd_ladder.hip: staged priority first-fit, what the
 * coarse levels of the TFD ladder use); order_out: n indices.  Test hook. */
int fc_debug_pyset_order_pairs_device(const int64_t *pairs, int64_t n, int64_t *order_out);
/* the device ladder's per-chunk and per-component routines (fc_tfd_core.h) run on the CPU by one host thread standing
 * for a wavefront: same mask as fc_tfd_ladder_from_first_match.  Pure host code.  Test hook. */
int fc_debug_tfd_ladder_emulate(const int64_t *first_match, int64_t N, uint8_t *mask_out);
/* The greedy k-ladder of the RMSD prunes over a caller's list of similar pairs ((i << 32) | j; entries with j <= i or
 * j >= N never act, duplicates are harmless), in ONE chosen device form -- the prunes pick a form from the list's
 * length and the ensemble's history, so a test cannot otherwise drive a given form from a given graph:
 *   form 0  the list scattered into an N x ceil(N/64) bit matrix, then one launch per level over it (what a prune
 *           runs on dense similarity or a list the pair ladder declines);
 *   form 1  the one-workgroup pair ladder: the whole ladder in one launch (what every ordinary prune runs);
 *   form 2  the launch-per-level pair ladder with `grid` workgroups per level, 1 .. 4096 (what a prune runs, with
 *           FC_LADDER_MANY_GRID = 16 workgroups by default, once more than 2^17 similar pairs were seen).
 * Exactly the requested form runs, or the call returns FC_E_LIMIT: forms 1 and 2 when N > 245 760 (two masks of
 * ceil(N/64) words in 60 KB of LDS) or n_pairs > min(2^20, max(1024, N (N - 1) / 2)).  fc_prune_conventions is
 * honoured as by the prunes: forms 1 and 2 implement drop_later, form 0 returns FC_E_INVALID under it.
 * mask_out: N bytes; levels_out (may be NULL): the number of ladder levels that ran (counters[8] of the prunes).
 * `grid` is read by form 2 only.  Test hook. */
int fc_debug_ladder_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int64_t min_per_group, int form,
                               int64_t grid, uint8_t *mask_out, int64_t *levels_out);

/* ---- a1: the .xyz wire format (host code; firecode/ensemble.py:58-98, 284-297;
 * firecode/utils.py:105-116).  atoms: A C strings.  mode 0 = Ensemble.to_xyz text
 * (label = basename), mode 1 = utils.write_xyz text repeated per conformer
 * (label = title).  Byte-identical to the Python writers.
 * fc_xyz_scan: conformer count and atoms per conformer of a file;
 * fc_xyz_read: atoms_out A x 8 bytes (NUL padded symbols of the first conformer),
 * coords_out (N, A, 3) parsed exactly like Python's float(). */
int fc_xyz_write(const char *path, const char *const *atoms, int64_t A, const double *coords,
                 int64_t N, const char *label, int mode);
int fc_xyz_scan(const char *path, int64_t *N_out, int64_t *A_out);
/* ---- cartesian_product (firecode/utils.py:219-221; callers torsion_module.py:484, 822) -------------------
 * Rows of np.stack(np.meshgrid(*arrays), -1).reshape(-1, T): `values` = the T arrays one after the other
 * (counts[t] entries each), out = (prod counts) x T, array #2 varying slowest, then #1, then #3 ... #T.
 * Host code (threads), no device needed: the angle grid of a conformational search (1 679 616 x 8 at cfg3)
 * is an INPUT of the scan kernels and costs NumPy 1 s.  FC_E_INVALID: T < 1, negative length. */
int fc_cartesian_product_i64(const int64_t *values, const int64_t *counts, int64_t T, int64_t *out);
int fc_cartesian_product_f64(const double *values, const int64_t *counts, int64_t T, double *out);
int fc_xyz_read(const char *path, int64_t N, int64_t A, char *atoms_out, double *coords_out);

/* ---- many ensembles in flight -------------------------------------------
 * fc_prune_rmsd_many: fc_prune_rmsd (no energy window) for `n` distinct resident ensembles,
 * enqueued together and waited for once.  What a caller with a queue of ensembles gains:
 * no host round trip between two prunes, and the small kernels of one prune (refine, level
 * buckets, ladder, result copy) run beside the all-pairs screen of the next one on other
 * streams (FC_PRUNE_LANES=1: strictly one after another).  Results are those of n calls of
 * fc_prune_rmsd: the reference has no batched form, a maintainer's loop over
 * prune_by_rmsd (firecode/ensemble.py:230-235 in a loop over ensembles) maps to one call.
 * mask_out[r]: N_r bytes; survivors_out (may be NULL): n counts.
 * FC_E_INVALID: NULL or repeated ensemble, n outside 0..4096, thresholds <= 0. */
int fc_prune_rmsd_many(fc_ensemble *const *ens, int64_t n, double max_rmsd, double max_dev,
                       int64_t min_per_group, uint8_t *const *mask_out, int64_t *survivors_out);

/* ---- bench / profiling hooks (resident data, device-side timing) --------
 * Runs the all-pairs similarity stage + greedy replay `reps` times on the
 * resident ensemble and returns HIP-event times (ms, per rep) of the
 * dominant kernel and of the whole step measured on the library's stream.  The kernel time is
 * the mean over every 8th prune (FC_BENCH_EVENT_STRIDE): the event pair costs the stream ~14 us. */
/* Arithmetic of the all-pairs screen the last prune launched: 16 = single-precision covariance on the
 * half-precision matrix pipe (coordinates split into two halfs, three f16 products) + bounded fp32
 * polynomial (default where its undecidable band is narrow and the structure has at most 128 atoms),
 * 32 = the same on the fp32 matrix pipe (FC_SCREEN_H2=0, more than 128 atoms), 64 = fp64 matrix pipe
 * (FC_SCREEN_F32=0, large structures with tight thresholds), 1 = VALU kernel, 0 = none yet.  Results do
 * not depend on it: every pair a screen lets through is decided by the exact fp64 refine. */
int fc_screen_last_kind(void);
/* Choice of the all-pairs screen for the prunes that follow: 0 = automatic (default), 16 / 32 = that
 * single-precision screen whatever its band (16: FC_E_INVALID from the prune when it does not apply),
 * 64 = the fp64 screen (the reference's arithmetic in every kernel of the step).  Process-wide;
 * results never depend on it. */
int fc_screen_select(int kind);
/* Which screen a prune of this shape would launch, without a device: the rule of launch_simbits_screen (fc_kabsch.hip,
 * plan_screen) on N conformers of A selected atoms, one rank, the given row block, lean (1: the pair lists only) or not,
 * largest G g_max (sum of squares of a centred conformer; NaN: the single-precision screens decline) and threshold
 * max_rmsd, with the f16 matrix-pipe model check taken as h2_model_ok (0 / 1), and FC_SCREEN_* and fc_screen_select read
 * as a prune reads them.  plan_out[0..4] = kind (as fc_screen_last_kind; 0: no screen), column tile, stages (2: the
 * two-stage fp32 launch), speculative (1: verdict and gated fp64 screen behind it), fp64 waves (4 / 8 where the fp64
 * screen runs, 0 otherwise).  Returns the error the prune would return (FC_E_INVALID / FC_E_LIMIT) or FC_OK. */
int fc_debug_screen_plan(int64_t N, int64_t A, int64_t row_block, int64_t lean, double g_max, double max_rmsd,
                         int64_t h2_model_ok, int64_t plan_out[5]);
/* Checks of what the split-half screen (kind 16) assumes, for the tests -- no FIRECODE call maps to them.
 * fc_debug_mfma_f16_model: runs the model check of v_mfma_f32_16x16x32_f16 the library runs itself before it
 * uses that screen: flags_out[0..7] = 1 where the pattern behaves as assumed (subnormal inputs honoured, one
 * rounding to nearest per instruction, the largest addend's last place kept for the others, exact large
 * products); worst_out = largest |D - exact| / (2^-24 (|C| + sum |a b|)) over `trials` random and adversarial
 * 16 x 16 x 32 products -- the error bounds charge 66 per instruction (an order-independent bound of a 33-addend
 * fp32 sum); the library refuses the screen on a device where this probe exceeds 18.
 * fc_debug_h2_covariance: the 16 x 16 tile of covariances (rows ib.., columns jb.., multiples of 16) exactly
 * as that screen accumulates them: B_out[(row*16 + col)*9 + 3x + y] = scale^2 sum_a p_ax q_ay; entry_bound_out
 * = the bound on |B_out / scale^2 - B| / s the screen's polynomial bounds start from (s = (Gp + Gq)/2).
 * scale_out = 0 (B_out untouched): the screen does not apply to this ensemble. */
int fc_debug_mfma_f16_model(int64_t trials, int64_t *flags_out, double *worst_out);
int fc_debug_h2_covariance(fc_ensemble *ens, int64_t ib, int64_t jb, float *B_out, double *scale_out,
                           double *entry_bound_out);
/* The per-lane routines of csrc/fc_kabsch_math.h on the device, one lane per record, for the tests that hold them to
 * an arbitrary-precision reference (tests/test_gpu_kabsch_math.py) -- no FIRECODE call maps to it.  `in` holds n records,
 * `out` receives n records (float64 throughout); launches are whole wavefronts, padded with copies of the last record.
 *   routine 0  the probe of csrc/fc_kabsch_math_probe.h: in 12 per record (B[9] row-major, Gp + Gq, A, A thr^2), out 94
 *              (enum KabschProbeSlot): the Newton eigenvalues and their certificates, the fp64 screen and its three
 *              values, the Jacobi rotation, the QCP rotations and quaternions in every form, flags included
 *   routine 1  the fp32 screens: in 16 per record (B[9], s, A thr^2 / 2 -- values of fp32 --, a count, a kind, tiny_floor,
 *              two unused), bounds = kabsch_f32_bounds(count) for kind 0, kabsch_h2_bounds(count) for kind 1; out 16:
 *              for plain then ENANT the three-test verdict, the two-test verdict and its redo, the wave form's verdict
 *              and redo bit of the lane (5 + 5), then the bounds p0, p1, p2 and three zeros
 *   routine 2  in 1, out 2: fc_sqrt_nonneg(x), fc_rsqrt(x)
 * FC_E_INVALID before any device use: NULL pointers, n outside 0..2^20, an unknown routine, a count outside 0..2^20 or a
 * kind other than 0 / 1.  n = 0 needs no device. */
int fc_debug_kabsch_math(int routine, const double *in, int64_t n, double *out);
int fc_bench_prune_rmsd(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t reps,
                        double *ms_simbits_kernel, double *ms_step, uint8_t *mask_out,
                        int64_t *stats);
/* The exact refine of the prune alone: one all-pairs screen fills the candidate-pair queue of the resident
 * ensemble, then `reps` launches of the refine over that queue (k_refine_pairs: one exact fp64 alignment --
 * covariance, rotation, rmsd, max deviation, decision -- per queued pair), HIP events around each.
 * ms_refine: mean; n_candidates: pairs per launch.  FC_E_LIMIT when the pair queue overflowed. */
int fc_bench_refine(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t reps, double *ms_refine,
                    int64_t *n_candidates);
/* `reps` complete all-pairs alignment passes (fc_ensemble_rmsd_and_max_all: the a4 contract of
 * firecode/utils.py:499 for every pair, fp64) over the resident ensemble, enqueued back to back, the two
 * dense (N, N) outputs staying in HBM; one host wait.  ms_kernel_mean: HIP events on the kernel's stream
 * around the tiled kernel of every pass; ms_total: first launch to the end of the last pass (fix-up
 * kernels included).  stats[4]: pairs this rank computed per pass, pairs the last pass sent to the Jacobi
 * fix-up, 1 when the tiled kernel ran (0: the one-wave-per-row kernel for structures beyond its LDS tile),
 * 16 x 16 sub-tiles of the last pass whose rotations took the general adjugate form (0 where every sub-tile of
 * the shared frame certified column 0; every sub-tile with FC_COMPLETE_FRAME=0 or FC_COMPLETE_COL0=0).
 * Under a communicator (fc_comm_init) a rank computes the rows of the row blocks (of 128) dealt to it in
 * snake order -- the units shard by row with no exchange -- and keeps its rows of the matrices.
 * FC_E_LIMIT: more degenerate pairs than the fix-up queue holds. */
int fc_bench_rmsd_and_max_all(fc_ensemble *ens, int64_t reps, double *ms_kernel_mean, double *ms_total,
                              int64_t *stats);
/* The same passes, and behind them (inside the call's wall-clock time -- about 0.1 ms -- but outside the HIP-event kernel
 * times it reports) the elements (pair_i[p], pair_j[p]),
 * p < P, of the two output matrices as the LAST pass left them: what bench.py's `value_check` and the
 * full-size parity tests compare with the oracle's rmsd_and_max (firecode/utils.py:494-504: `(rmsd,
 * maxdev)` per pair).  Under a communicator only rows this rank owns hold values.  (i > j reads (j, i).) */
int fc_bench_rmsd_and_max_all_sampled(fc_ensemble *ens, int64_t reps, const int64_t *pair_i, const int64_t *pair_j,
                                      int64_t P, double *rmsd_out, double *maxdev_out, double *ms_kernel_mean,
                                      double *ms_total, int64_t *stats);
/* `reps` selections (fc_ensemble_select_diverse, the same arguments; only the indices are copied back) one after the
 * other: ms_device_mean = HIP events on the library's stream from the first step's launch to the last one's end (with a
 * radius stop: the host's reads of the stop word every 64 steps included), ms_host_mean = wall-clock time per call;
 * lanes_out (may be NULL) = lanes per conformer the step kernel used (1 or 8). */
int fc_bench_select_diverse(fc_ensemble *ens, int64_t n_max, int64_t start, double stop_rmsd, int64_t reps,
                            double *ms_device_mean, double *ms_host_mean, int64_t *indices_out, int64_t *n_selected,
                            int64_t *lanes_out);
/* the same for fc_ensemble_select_diverse_perm.  stats (2 values, may be NULL), summed over the steps of the last
 * selection: [0] = (k, h) of a (representative, conformer) pair whose eigenvalue was formed, [1] = those of them that
 * reached the rotation and the explicit deviation pass. */
int fc_bench_select_diverse_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                 int64_t n_max, int64_t start, double stop_rmsd, int64_t reps, double *ms_device_mean,
                                 double *ms_host_mean, int64_t *indices_out, int64_t *n_selected, int64_t *stats);
/* `reps` calls of fc_ensemble_knn (the same arguments; the lists are copied back each time) one after the other:
 * ms_device_mean = HIP events on the library's stream from the first launch to the end of the merge, ms_host_mean =
 * wall-clock time per call; strips_out (may be NULL) = the column strips of the launch. */
int fc_bench_knn(fc_ensemble *ens, int64_t k, int64_t reps, double *ms_device_mean, double *ms_host_mean,
                 int64_t *strips_out);
/* the same for fc_ensemble_knn_cross (its arguments and refusals) */
int fc_bench_knn_cross(fc_ensemble *queries, fc_ensemble *refs, int64_t k, double max_rmsd, int64_t reps,
                       double *ms_device_mean, double *ms_host_mean, int64_t *strips_out);
/* the same for fc_ensemble_knn_perm and fc_ensemble_knn_cross_perm (their arguments and refusals).  stats (2 values, may be
 * NULL), over one further call made without the clock: [0] = (pair, p, h) whose eigenvalue was formed, [1] = those that
 * were taken through the rotation and the explicit pass (a pair rides along when another column of its 64-column chunk
 * needs the pass: the figure is the work done). */
int fc_bench_knn_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, int64_t k, int64_t reps,
                      double *ms_device_mean, double *ms_host_mean, int64_t *strips_out, int64_t *stats);
int fc_bench_knn_cross_perm(fc_ensemble *queries, fc_ensemble *refs, const int32_t *perms, int64_t K, int64_t A_sel,
                            int mirror, int64_t k, double max_rmsd, int64_t reps, double *ms_device_mean,
                            double *ms_host_mean, int64_t *strips_out, int64_t *stats);
/* (fc_bench_prune_rmsd writes EIGHT stats: [6] = 16 x 32-pair units the subset stage of the lean fp32
 * screen queued for the full test in the last prune, [7] = 1 when its sample found similarity dense
 * and the single-stage kernel did the launch) */
/* the same for fc_prune_rmsd_sharded: `reps` sharded prunes enqueued back to back, one host wait;
 * overlap != 0: prune k on workspace / lane k&1, its refine + export + all-gather + ladder beside
 * the screen of prune k+1 */
int fc_bench_prune_rmsd_sharded(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t reps, int overlap,
                                double *ms_screen_kernel, double *ms_step, uint8_t *mask_out, int64_t *stats);

#ifdef __cplusplus
}
#endif
#endif /* FC_HIP_H */
