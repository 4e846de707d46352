// fc_api_geom.cpp -- the extern "C" surface (include/fc_hip.h) of alignment, moments, clash, bond, fitness and embed:
// argument checks, host<->HBM staging, kernel sequencing.  No compute here.
#include "fc_internal.h"

using namespace fc;

extern "C" {

int fc_alignment_matrices(const double *p, const double *q, int64_t n_pairs, int64_t A,
                          double *M_out) {
  FC_API_LOCK;
  FC_REQUIRE(n_pairs >= 0 && A >= 1, "bad shape");
  if (n_pairs == 0) return FC_OK;
  FC_REQUIRE(p && q && M_out, "NULL pointer argument");
  FC_TRY(ensure_init());
  DevBuf dp, dq, dM;
  FC_TRY(upload(dp, p, (size_t)n_pairs * A * 3));
  FC_TRY(upload(dq, q, (size_t)n_pairs * A * 3));
  FC_TRY(dM.reserve((size_t)n_pairs * 9 * sizeof(double)));
  FC_TRY(launch_alignment_matrices(dp.as<double>(), dq.as<double>(), n_pairs, A, dM.as<double>()));
  FC_TRY(d2h(M_out, dM.p, (size_t)n_pairs * 9 * sizeof(double)));
  return sync();
}

// ---- a9: align_by_moi (firecode/hypermolecule_class.py:45-86) ------------------------------
int fc_align_by_moi(const double *coords, int64_t N, int64_t A, const double *masses, double *out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && masses && out, "NULL pointer argument");
  FC_TRY(ensure_init());
  DevBuf dc, dm, dcen, dmom, dP, dQ, dM, dt, dout;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(upload(dm, masses, (size_t)A));
  FC_TRY(dcen.reserve((size_t)N * A * 3 * sizeof(double)));
  FC_TRY(dmom.reserve((size_t)N * 3 * sizeof(double)));
  FC_TRY(dP.reserve((size_t)N * 9 * sizeof(double)));
  FC_TRY(dQ.reserve((size_t)N * 9 * sizeof(double)));
  FC_TRY(dM.reserve((size_t)N * 9 * sizeof(double)));
  FC_TRY(dt.reserve((size_t)N * 3 * sizeof(double)));
  FC_TRY(dout.reserve((size_t)N * A * 3 * sizeof(double)));
  FC_TRY(launch_center_structures(dc.as<double>(), N, A, dcen.as<double>()));
  FC_TRY(launch_inertia_moments(dcen.as<double>(), N, A, dm.as<double>(), dmom.as<double>()));
  FC_TRY(launch_moi_diag_pairs(dmom.as<double>(), N, dP.as<double>(), dQ.as<double>()));
  FC_TRY(launch_alignment_matrices(dP.as<double>(), dQ.as<double>(), N, 3, dM.as<double>()));
  FC_TRY(launch_set_identity(dM.as<double>()));
  FC_HIP_TRY(hipMemsetAsync(dt.p, 0, (size_t)N * 3 * sizeof(double), ctx().stream));
  FC_TRY(launch_rototranslate(dcen.as<double>(), N, A, dM.as<double>(), dt.as<double>(), dout.as<double>()));
  FC_TRY(d2h(out, dout.p, (size_t)N * A * 3 * sizeof(double)));
  return sync();
}

// ---- a6 ------------------------------------------------------------------------
int fc_inertia_moments(const double *coords, int64_t N, int64_t A, const double *masses,
                       double *moments_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && masses && moments_out, "NULL pointer argument");
  FC_TRY(ensure_init());
  DevBuf dc, dm, dout;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(upload(dm, masses, (size_t)A));
  FC_TRY(dout.reserve((size_t)N * 3 * sizeof(double)));
  FC_TRY(launch_inertia_moments(dc.as<double>(), N, A, dm.as<double>(), dout.as<double>()));
  FC_TRY(d2h(moments_out, dout.p, (size_t)N * 3 * sizeof(double)));
  return sync();
}

// ---- a8 / a13 --------------------------------------------------------------------
int fc_align_to_first(const double *coords, int64_t N, int64_t A, const int64_t *idx,
                      int64_t n_idx, double *out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && out, "NULL pointer argument");
  if (idx == nullptr) n_idx = A;
  FC_REQUIRE(n_idx >= 1, "n_idx must be >= 1");
  if (idx)
    for (int64_t k = 0; k < n_idx; ++k)
      FC_REQUIRE(idx[k] >= 0 && idx[k] < A, "idx[%lld] out of range", (long long)k);
  FC_TRY(ensure_init());
  DevBuf dc, di, dout;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  if (idx) FC_TRY(upload(di, idx, (size_t)n_idx));
  FC_TRY(dout.reserve((size_t)N * A * 3 * sizeof(double)));
  FC_TRY(launch_align_to_first(dc.as<double>(), N, A, idx ? di.as<int64_t>() : nullptr, n_idx,
                               dout.as<double>()));
  FC_TRY(d2h(out, dout.p, (size_t)N * A * 3 * sizeof(double)));
  return sync();
}

int fc_rototranslate(const double *coords, int64_t n, int64_t A, const double *R, const double *t,
                     double *out) {
  FC_API_LOCK;
  FC_REQUIRE(n >= 0 && A >= 1, "bad shape");
  if (n == 0) return FC_OK;
  FC_REQUIRE(coords && R && t && out, "NULL pointer argument");
  FC_TRY(ensure_init());
  DevBuf dc, dR, dt, dout;
  FC_TRY(upload(dc, coords, (size_t)n * A * 3));
  FC_TRY(upload(dR, R, (size_t)n * 9));
  FC_TRY(upload(dt, t, (size_t)n * 3));
  FC_TRY(dout.reserve((size_t)n * A * 3 * sizeof(double)));
  FC_TRY(launch_rototranslate(dc.as<double>(), n, A, dR.as<double>(), dt.as<double>(),
                              dout.as<double>()));
  FC_TRY(d2h(out, dout.p, (size_t)n * A * 3 * sizeof(double)));
  return sync();
}

// ---- a11 / a12 ---------------------------------------------------------------------
static const int64_t kMaxLdsAtoms = (int64_t)kLdsLimit / 24;  // one structure per wavefront in LDS

int fc_clash_self(const double *coords, int64_t N, int64_t A, double lo, double hi,
                  int64_t *counts_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && counts_out, "NULL pointer argument");
  if (A > kMaxLdsAtoms) return set_error(FC_E_LIMIT, "A=%lld exceeds %lld atoms", (long long)A, (long long)kMaxLdsAtoms);
  FC_TRY(ensure_init());
  DevBuf dc, dn;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(dn.reserve((size_t)N * sizeof(int64_t)));
  FC_TRY(launch_clash_self(dc.as<double>(), N, A, lo, hi, dn.as<int64_t>()));
  FC_TRY(d2h(counts_out, dn.p, (size_t)N * sizeof(int64_t)));
  return sync();
}

int fc_clash_fragments(const double *coords, int64_t N, int64_t A, const int64_t *ids,
                       int64_t n_ids, double thresh, int64_t max_clashes, int64_t *counts_out,
                       uint8_t *pass_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  FC_REQUIRE(ids != nullptr && (n_ids == 2 || n_ids == 3), "ids must hold 2 or 3 fragment lengths");
  int64_t tot = 0;
  for (int64_t k = 0; k < n_ids; ++k) {
    FC_REQUIRE(ids[k] >= 0, "negative fragment length");
    tot += ids[k];
  }
  // reference slices m_last = coords[sum(ids[:-1]):] -- the last fragment takes the rest
  FC_REQUIRE(tot - ids[n_ids - 1] <= A, "fragment lengths exceed A");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && (counts_out || pass_out), "NULL pointer argument");
  if (A > kMaxLdsAtoms) return set_error(FC_E_LIMIT, "A=%lld exceeds %lld atoms", (long long)A, (long long)kMaxLdsAtoms);
  FC_TRY(ensure_init());
  DevBuf dc, dn, dp;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(dn.reserve((size_t)N * sizeof(int64_t)));
  FC_TRY(dp.reserve((size_t)N));
  FC_TRY(launch_clash_fragments(dc.as<double>(), N, A, ids, n_ids, thresh, max_clashes,
                                dn.as<int64_t>(), dp.as<uint8_t>()));
  if (counts_out) FC_TRY(d2h(counts_out, dn.p, (size_t)N * sizeof(int64_t)));
  if (pass_out) FC_TRY(d2h(pass_out, dp.p, (size_t)N));
  return sync();
}

int fc_clash_graph(const double *coords, int64_t N, int64_t A, const uint8_t *adj, double thresh,
                   int64_t *counts_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && adj && counts_out, "NULL pointer argument");
  FC_REQUIRE(thresh > 0.0, "thresh must be positive");
  if (A > kMaxLdsAtoms) return set_error(FC_E_LIMIT, "A=%lld exceeds %lld atoms", (long long)A, (long long)kMaxLdsAtoms);
  FC_TRY(ensure_init());
  DevBuf dc, da, dn;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(upload(da, adj, (size_t)A * A));
  FC_TRY(dn.reserve((size_t)N * sizeof(int64_t)));
  FC_TRY(launch_clash_graph(dc.as<double>(), N, A, da.as<uint8_t>(), thresh, dn.as<int64_t>()));
  FC_TRY(d2h(counts_out, dn.p, (size_t)N * sizeof(int64_t)));
  return sync();
}

// ---- bond-topology check (molecule_check / scramble_check, firecode/utils.py:341-400) ---------------------------
// every argument is checked here, before the device is touched; then the job runs
static int bond_check_and_run(BondJob &j) {
  FC_REQUIRE(j.N >= 0 && j.A >= 1, "bad shape");
  if (j.A > INT32_MAX - 1) return set_error(FC_E_LIMIT, "A=%lld: atom indices are 32-bit", (long long)j.A);
  FC_REQUIRE(j.n_class >= 1 && j.n_class <= 64, "n_class=%lld outside 1..64", (long long)j.n_class);
  FC_REQUIRE((j.ref_coords != nullptr) != (j.ref_bits != nullptr),
             "exactly one reference: ref_coords (molecule mode) or ref_bits (scramble mode)");
  FC_REQUIRE(!j.ref_coords || j.ref_stride == 0 || j.ref_stride == 3 * j.A, "ref_stride must be 0 or 3*A");
  if (j.N == 0) return FC_OK;
  FC_REQUIRE(j.coords && j.atom_class && j.class_thresh, "NULL pointer argument");
  for (int64_t a = 0; a < j.A; ++a)
    FC_REQUIRE(j.atom_class[a] >= 0 && j.atom_class[a] < j.n_class, "atom_class[%lld] out of range", (long long)a);
  for (int64_t p = 0; p < j.n_class; ++p)
    for (int64_t q = 0; q < j.n_class; ++q) {
      const double u = j.class_thresh[p * j.n_class + q], v = j.class_thresh[q * j.n_class + p];
      FC_REQUIRE(u == v || (u != u && v != v), "class_thresh must be symmetric");
    }
  if (j.excl_offsets) {
    FC_REQUIRE(j.excl_sets == 1 || j.excl_sets == j.N, "excl_sets must be 1 or N");
    FC_REQUIRE(j.excl_offsets[0] == 0, "excl_offsets[0] must be 0");
    for (int64_t s = 0; s < j.excl_sets; ++s)
      FC_REQUIRE(j.excl_offsets[s + 1] >= j.excl_offsets[s], "excl_offsets must be non-decreasing");
    FC_REQUIRE(j.excl_offsets[j.excl_sets] == 0 || j.excl_atoms, "NULL excl_atoms");
  }
  if (j.offsets) {
    FC_REQUIRE(j.offsets[0] == 0, "offsets[0] must be 0");
    for (int64_t n = 0; n < j.N; ++n) FC_REQUIRE(j.offsets[n + 1] >= j.offsets[n], "offsets must be non-decreasing");
    FC_REQUIRE(j.offsets[j.N] == 0 || j.bonds_out, "NULL bonds_out");
  } else {
    FC_REQUIRE(j.counts_out || j.ok_out, "no output requested");
  }
  FC_TRY(ensure_init());
  return bond_changes(j);
}

// the part of a BondJob the two entry points share
static BondJob bond_job(const double *coords, int64_t N, int64_t A, const int32_t *atom_class, int64_t n_class,
                        const double *class_thresh, const double *ref_coords, int64_t ref_stride, const uint64_t *ref_bits,
                        const int64_t *excl_offsets, const int64_t *excl_atoms, int64_t excl_sets) {
  BondJob j;
  j.coords = coords, j.N = N, j.A = A, j.atom_class = atom_class, j.n_class = n_class, j.class_thresh = class_thresh;
  j.ref_coords = ref_coords, j.ref_stride = ref_stride, j.ref_bits = ref_bits;
  j.excl_offsets = excl_offsets, j.excl_atoms = excl_atoms, j.excl_sets = excl_sets;
  return j;
}

int fc_bond_changes(const double *coords, int64_t N, int64_t A, const int32_t *atom_class, int64_t n_class,
                    const double *class_thresh, const double *ref_coords, int64_t ref_stride, const uint64_t *ref_bits,
                    const int64_t *excl_offsets, const int64_t *excl_atoms, int64_t excl_sets, int64_t max_newbonds,
                    int64_t *counts_out, uint8_t *ok_out) {
  FC_API_LOCK;
  BondJob j = bond_job(coords, N, A, atom_class, n_class, class_thresh, ref_coords, ref_stride, ref_bits, excl_offsets,
                       excl_atoms, excl_sets);
  j.max_newbonds = max_newbonds, j.counts_out = counts_out, j.ok_out = ok_out;
  return bond_check_and_run(j);
}

int fc_bond_changes_list(const double *coords, int64_t N, int64_t A, const int32_t *atom_class, int64_t n_class,
                         const double *class_thresh, const double *ref_coords, int64_t ref_stride,
                         const uint64_t *ref_bits, const int64_t *excl_offsets, const int64_t *excl_atoms,
                         int64_t excl_sets, const int64_t *offsets, int64_t *bonds_out) {
  FC_API_LOCK;
  BondJob j = bond_job(coords, N, A, atom_class, n_class, class_thresh, ref_coords, ref_stride, ref_bits, excl_offsets,
                       excl_atoms, excl_sets);
  FC_REQUIRE(offsets != nullptr, "NULL offsets");
  j.offsets = offsets, j.bonds_out = bonds_out;
  return bond_check_and_run(j);
}

int fc_fitness_check(const double *coords, int64_t N, int64_t A, const int64_t *pairs,
                     const double *targets, int64_t C, double threshold, double *error_out,
                     uint8_t *pass_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1 && C >= 0, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && pass_out && (C == 0 || (pairs && targets)), "NULL pointer argument");
  for (int64_t k = 0; k < N * C * 2; ++k) FC_REQUIRE(pairs[k] >= 0 && pairs[k] < A, "constraint index out of range");
  FC_TRY(ensure_init());
  DevBuf dc, dp, dt, de, dm;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(upload(dp, pairs, (size_t)N * C * 2));
  FC_TRY(upload(dt, targets, (size_t)N * C));
  FC_TRY(de.reserve((size_t)N * sizeof(double)));
  FC_TRY(dm.reserve((size_t)N));
  FC_TRY(launch_fitness(dc.as<double>(), N, A, dp.as<int64_t>(), dt.as<double>(), C, threshold,
                        de.as<double>(), dm.as<uint8_t>()));
  if (error_out) FC_TRY(d2h(error_out, de.p, (size_t)N * sizeof(double)));
  FC_TRY(d2h(pass_out, dm.p, (size_t)N));
  return sync();
}

// ---- a14 -------------------------------------------------------------------------
int fc_embed_poses_clash(const double *m1, int64_t n1, int64_t A1, const double *m2, int64_t n2,
                         int64_t A2, const int64_t *c1, const int64_t *c2, const double *R1,
                         const double *t1, const double *R2, const double *t2, int64_t P,
                         double thresh, int64_t max_clashes, int64_t *counts_out,
                         uint8_t *pass_out, double *poses_out) {
  FC_API_LOCK;
  FC_REQUIRE(n1 >= 1 && n2 >= 1 && A1 >= 1 && A2 >= 1 && P >= 0, "bad shape");
  if (P == 0) return FC_OK;
  FC_REQUIRE(m1 && m2 && c1 && c2 && R1 && t1 && R2 && t2, "NULL pointer argument");
  FC_REQUIRE(counts_out || pass_out || poses_out, "no output requested");
  if (4 * A1 * 24 > (int64_t)kLdsLimit) return set_error(FC_E_LIMIT, "A1=%lld too large for the LDS slice", (long long)A1);
  for (int64_t k = 0; k < P; ++k)
    FC_REQUIRE(c1[k] >= 0 && c1[k] < n1 && c2[k] >= 0 && c2[k] < n2, "conformer id out of range at pose %lld", (long long)k);
  FC_TRY(ensure_init());
  DevBuf dm1, dm2, dc1, dc2, dR1, dt1, dR2, dt2, dn, dp, dposes;
  FC_TRY(upload(dm1, m1, (size_t)n1 * A1 * 3));
  FC_TRY(upload(dm2, m2, (size_t)n2 * A2 * 3));
  FC_TRY(upload(dc1, c1, (size_t)P));
  FC_TRY(upload(dc2, c2, (size_t)P));
  FC_TRY(upload(dR1, R1, (size_t)P * 9));
  FC_TRY(upload(dt1, t1, (size_t)P * 3));
  FC_TRY(upload(dR2, R2, (size_t)P * 9));
  FC_TRY(upload(dt2, t2, (size_t)P * 3));
  FC_TRY(dn.reserve((size_t)P * sizeof(int64_t)));
  FC_TRY(dp.reserve((size_t)P));
  if (poses_out) FC_TRY(dposes.reserve((size_t)P * (A1 + A2) * 3 * sizeof(double)));
  FC_TRY(launch_embed_poses_clash(dm1.as<double>(), A1, dm2.as<double>(), A2, dc1.as<int64_t>(),
                                  dc2.as<int64_t>(), dR1.as<double>(), dt1.as<double>(),
                                  dR2.as<double>(), dt2.as<double>(), P, thresh, max_clashes,
                                  dn.as<int64_t>(), dp.as<uint8_t>(),
                                  poses_out ? dposes.as<double>() : nullptr));
  if (counts_out) FC_TRY(d2h(counts_out, dn.p, (size_t)P * sizeof(int64_t)));
  if (pass_out) FC_TRY(d2h(pass_out, dp.p, (size_t)P));
  if (poses_out) FC_TRY(d2h(poses_out, dposes.p, (size_t)P * (A1 + A2) * 3 * sizeof(double)));
  return sync();
}

static int check_embed_mol(const double *m, int64_t n, int64_t A, const int64_t *reactive, int64_t nr,
                           const double *ps, const double *pe, const double *angles, int64_t na) {
  FC_REQUIRE(m && reactive && ps && pe && angles, "NULL pointer argument");
  FC_REQUIRE(n >= 1 && A >= 1 && na >= 1, "bad shape");
  FC_REQUIRE(nr == 1 || nr == 2, "a molecule has 1 or 2 reactive atoms");
  for (int64_t k = 0; k < nr; ++k) FC_REQUIRE(reactive[k] >= 0 && reactive[k] < A, "reactive index out of range");
  return FC_OK;
}

int fc_embed_mol_transforms(const double *coords, int64_t n, int64_t A, const int64_t *reactive,
                            int64_t nr, const double *pivot_start, const double *pivot_end,
                            int64_t mol, const double *angles, int64_t na, double *R_out,
                            double *t_out) {
  FC_API_LOCK;
  FC_TRY(check_embed_mol(coords, n, A, reactive, nr, pivot_start, pivot_end, angles, na));
  FC_REQUIRE((mol == 0 || mol == 1) && R_out && t_out, "bad arguments");
  FC_TRY(ensure_init());
  DevBuf dc, dr, dps, dpe, da, dR, dt;
  FC_TRY(upload(dc, coords, (size_t)n * A * 3));
  FC_TRY(upload(dr, reactive, (size_t)nr));
  FC_TRY(upload(dps, pivot_start, (size_t)n * 3));
  FC_TRY(upload(dpe, pivot_end, (size_t)n * 3));
  FC_TRY(upload(da, angles, (size_t)na));
  const size_t G = (size_t)n * 2 * na;
  FC_TRY(dR.reserve(G * 9 * sizeof(double)));
  FC_TRY(dt.reserve(G * 3 * sizeof(double)));
  FC_TRY(launch_embed_mol_transforms(dc.as<double>(), n, A, dr.as<int64_t>(), (int)nr, dps.as<double>(),
                                     dpe.as<double>(), (int)mol, da.as<double>(), na, dR.as<double>(),
                                     dt.as<double>()));
  FC_TRY(d2h(R_out, dR.p, G * 9 * sizeof(double)));
  FC_TRY(d2h(t_out, dt.p, G * 3 * sizeof(double)));
  return sync();
}

static int embed_grid(const double *m1, int64_t n1, int64_t A1, const int64_t *reactive1,
                      int64_t nr1, const double *ps1, const double *pe1, const double *m2,
                      int64_t n2, int64_t A2, const int64_t *reactive2, int64_t nr2,
                      const double *ps2, const double *pe2, const double *angles1, int64_t na1,
                      const double *angles2, int64_t na2, double thresh, int64_t max_clashes,
                      uint8_t *pass_out, int32_t *counts_out, double *ms_kernel, double rmsd_thr,
                      uint8_t *accept_out) {
  FC_TRY(check_embed_mol(m1, n1, A1, reactive1, nr1, ps1, pe1, angles1, na1));
  FC_TRY(check_embed_mol(m2, n2, A2, reactive2, nr2, ps2, pe2, angles2, na2));
  FC_REQUIRE(pass_out != nullptr && max_clashes >= 0, "bad arguments");
  if (A1 * 40 + 64 > 64 * 1024) return set_error(FC_E_LIMIT, "A1=%lld too large for the LDS stage", (long long)A1);
  if (accept_out != nullptr) {  // refused before anything is launched
    FC_REQUIRE(rmsd_thr > 0.0, "rmsd_thr must be positive");
    if (na1 * na2 * 4 * (int64_t)sizeof(int) > 64 * 1024)
      return set_error(FC_E_LIMIT, "na1*na2=%lld angle pairs per group exceed the 4096 of the LDS list",
                       (long long)(na1 * na2));
  }
  FC_TRY(ensure_init());
  Context &c = ctx();
  const int64_t P = n1 * n2 * 2 * na1 * na2;
  const int64_t S2 = ceil_div(n2 * na2, 64) * 64;
  DevBuf d1, d2, r1, r2, s1, e1, s2, e2, a1, a2, R1, t1, R2, t2, X1, X2s, dpass, dcnt, dmax;
  FC_TRY(upload(d1, m1, (size_t)n1 * A1 * 3));
  FC_TRY(upload(d2, m2, (size_t)n2 * A2 * 3));
  FC_TRY(upload(r1, reactive1, (size_t)nr1));
  FC_TRY(upload(r2, reactive2, (size_t)nr2));
  FC_TRY(upload(s1, ps1, (size_t)n1 * 3));
  FC_TRY(upload(e1, pe1, (size_t)n1 * 3));
  FC_TRY(upload(s2, ps2, (size_t)n2 * 3));
  FC_TRY(upload(e2, pe2, (size_t)n2 * 3));
  FC_TRY(upload(a1, angles1, (size_t)na1));
  FC_TRY(upload(a2, angles2, (size_t)na2));
  const size_t G1 = (size_t)n1 * 2 * na1, G2 = (size_t)n2 * 2 * na2;
  FC_TRY(R1.reserve(G1 * 9 * sizeof(double)));
  FC_TRY(t1.reserve(G1 * 3 * sizeof(double)));
  FC_TRY(R2.reserve(G2 * 9 * sizeof(double)));
  FC_TRY(t2.reserve(G2 * 3 * sizeof(double)));
  FC_TRY(X1.reserve(G1 * A1 * 3 * sizeof(double)));
  FC_TRY(X2s.reserve((size_t)2 * A2 * 3 * S2 * sizeof(double)));
  FC_TRY(dmax.reserve(256 + (size_t)2 * A2 * 3 * S2 * sizeof(float)));  // scratch of the clash kernel
  FC_TRY(dpass.reserve((size_t)P));
  if (counts_out) FC_TRY(dcnt.reserve((size_t)P * sizeof(int32_t)));
  FC_HIP_TRY(hipMemsetAsync(X2s.p, 0, (size_t)2 * A2 * 3 * S2 * sizeof(double), c.stream));
  FC_TRY(launch_embed_mol_transforms(d1.as<double>(), n1, A1, r1.as<int64_t>(), (int)nr1, s1.as<double>(),
                                     e1.as<double>(), 0, a1.as<double>(), na1, R1.as<double>(), t1.as<double>()));
  FC_TRY(launch_embed_mol_transforms(d2.as<double>(), n2, A2, r2.as<int64_t>(), (int)nr2, s2.as<double>(),
                                     e2.as<double>(), 1, a2.as<double>(), na2, R2.as<double>(), t2.as<double>()));
  FC_TRY(launch_embed_pretransform(d1.as<double>(), n1, A1, na1, R1.as<double>(), t1.as<double>(), 1, 0,
                                   X1.as<double>()));
  FC_TRY(launch_embed_pretransform(d2.as<double>(), n2, A2, na2, R2.as<double>(), t2.as<double>(), 0, S2,
                                   X2s.as<double>()));
  FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  FC_TRY(launch_embed_grid_clash(X1.as<double>(), n1, A1, na1, X2s.as<double>(), n2, A2, na2, S2, thresh,
                                 max_clashes, dmax.p, dmax.bytes, dpass.as<uint8_t>(),
                                 counts_out ? dcnt.as<int32_t>() : nullptr));
  FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  DevBuf X2a, dacc;
  if (accept_out != nullptr) {
    FC_REQUIRE(rmsd_thr > 0.0, "rmsd_thr must be positive");
    if (na1 * na2 * 4 * (int64_t)sizeof(int) > 64 * 1024)
      return set_error(FC_E_LIMIT, "na1*na2=%lld angle pairs per group exceed the 4096 of the LDS list",
                       (long long)(na1 * na2));
    FC_TRY(X2a.reserve(G2 * A2 * 3 * sizeof(double)));
    FC_TRY(dacc.reserve((size_t)P));
    FC_TRY(launch_embed_pretransform(d2.as<double>(), n2, A2, na2, R2.as<double>(), t2.as<double>(), 1, 0,
                                     X2a.as<double>()));
    FC_TRY(launch_embed_group_dedupe(X1.as<double>(), n1, A1, na1, X2a.as<double>(), n2, A2, na2, rmsd_thr,
                                     dpass.as<uint8_t>(), dacc.as<uint8_t>()));
    FC_TRY(d2h(accept_out, dacc.p, (size_t)P));
  }
  FC_TRY(d2h(pass_out, dpass.p, (size_t)P));
  if (counts_out) FC_TRY(d2h(counts_out, dcnt.p, (size_t)P * sizeof(int32_t)));
  FC_TRY(sync());
  if (ms_kernel) {
    float ms = 0.f;
    FC_HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    *ms_kernel = ms;
  }
  return FC_OK;
}

int fc_embed_grid_clash(const double *m1, int64_t n1, int64_t A1, const int64_t *reactive1,
                        int64_t nr1, const double *ps1, const double *pe1, const double *m2,
                        int64_t n2, int64_t A2, const int64_t *reactive2, int64_t nr2,
                        const double *ps2, const double *pe2, const double *angles1, int64_t na1,
                        const double *angles2, int64_t na2, double thresh, int64_t max_clashes,
                        uint8_t *pass_out, int32_t *counts_out, double *ms_kernel) {
  FC_API_LOCK;
  return embed_grid(m1, n1, A1, reactive1, nr1, ps1, pe1, m2, n2, A2, reactive2, nr2, ps2, pe2, angles1,
                    na1, angles2, na2, thresh, max_clashes, pass_out, counts_out, ms_kernel, 0.0, nullptr);
}

int fc_embed_grid_dedupe(const double *m1, int64_t n1, int64_t A1, const int64_t *reactive1,
                         int64_t nr1, const double *ps1, const double *pe1, const double *m2,
                         int64_t n2, int64_t A2, const int64_t *reactive2, int64_t nr2,
                         const double *ps2, const double *pe2, const double *angles1, int64_t na1,
                         const double *angles2, int64_t na2, double thresh, int64_t max_clashes,
                         double rmsd_thr, uint8_t *pass_out, uint8_t *accept_out) {
  FC_API_LOCK;
  FC_REQUIRE(accept_out != nullptr, "accept_out is NULL");
  return embed_grid(m1, n1, A1, reactive1, nr1, ps1, pe1, m2, n2, A2, reactive2, nr2, ps2, pe2, angles1,
                    na1, angles2, na2, thresh, max_clashes, pass_out, nullptr, nullptr, rmsd_thr, accept_out);
}

// ---- a14, three molecules: cyclical_embed (firecode/embeds.py:409-585) -----------------------
int fc_embed_trimolecular(const double *const coords[3], const int64_t n_conf[3], const int64_t n_atoms[3],
                          const int64_t *const reactive[3], const int64_t n_reactive[3], int64_t J,
                          const int64_t *conf, const double *piv_start, const double *piv_end,
                          const double *vecs, const double *dirs0, const uint8_t *run, const int64_t *rtab,
                          const double *norms, const double *ua, int64_t U, const int32_t *aidx, int64_t S,
                          double thresh, int64_t max_clashes, double rmsd_thr, double *dirs_out,
                          double *Rt_out, uint8_t *pass_out, uint8_t *accept_out) {
  FC_API_LOCK;
  FC_REQUIRE(coords && n_conf && n_atoms && reactive && n_reactive, "NULL pointer argument");
  FC_REQUIRE(J >= 0 && U >= 1 && S >= 1, "bad shape");
  if (J == 0) return FC_OK;
  FC_REQUIRE(conf && piv_start && piv_end && vecs && dirs0 && run && rtab && norms && ua && aidx && dirs_out &&
                 Rt_out && pass_out && accept_out,
             "NULL pointer argument");
  FC_REQUIRE(thresh > 0.0 && rmsd_thr > 0.0 && max_clashes >= 0, "thresholds must be positive");
  int64_t Atot = 0;
  for (int i = 0; i < 3; ++i) {
    FC_REQUIRE(coords[i] && reactive[i] && n_conf[i] >= 1 && n_atoms[i] >= 1, "bad molecule %d", i);
    FC_REQUIRE(n_reactive[i] >= 1 && n_reactive[i] <= 2, "molecule %d: 1 or 2 reactive atoms expected", i);
    for (int64_t r = 0; r < n_reactive[i]; ++r)
      FC_REQUIRE(reactive[i][r] >= 0 && reactive[i][r] < n_atoms[i], "reactive index out of range");
    Atot += n_atoms[i];
  }
  // every index a kernel dereferences is checked here
  for (int64_t j = 0; j < J; ++j)
    for (int i = 0; i < 3; ++i) {
      FC_REQUIRE(conf[j * 3 + i] >= 0 && conf[j * 3 + i] < n_conf[i], "conformer index out of range (job %lld)",
                 (long long)j);
      for (int v = 0; v < 8; ++v)
        for (int k = 0; k < 3; ++k) {
          const int64_t r = rtab[((j * 8 + v) * 3 + i) * 3 + k];
          FC_REQUIRE(r >= 0 && r < n_atoms[i], "reactive-pair table entry out of range (job %lld)", (long long)j);
        }
    }
  for (int64_t s = 0; s < S * 3; ++s) FC_REQUIRE(aidx[s] >= 0 && aidx[s] < U, "angle index out of range");
  if (3 * U > 256) return set_error(FC_E_LIMIT, "U=%lld distinct step angles per molecule exceed 85", (long long)U);
  if (J * 8 * S >= (1ll << 31)) return set_error(FC_E_LIMIT, "too many poses in one call: split the jobs");
  const size_t lds = tri_group_lds_bytes(Atot, (int)U, (int)S);
  if (lds > kLdsLimit)
    return set_error(FC_E_LIMIT, "%zu bytes of LDS per group (atoms %lld x angles %lld, %lld poses) exceed 160 KB",
                     lds, (long long)Atot, (long long)U, (long long)S);
  FC_TRY(ensure_init());
  DevBuf dc[3], dr[3], dconf, dps, dpe, dvecs, dd0, drun, drt, dn, dua, daidx, ddirs, dRt, dpass, dacc;
  const double *cdev[3];
  const int64_t *rdev[3];
  for (int i = 0; i < 3; ++i) {
    FC_TRY(upload(dc[i], coords[i], (size_t)n_conf[i] * n_atoms[i] * 3));
    FC_TRY(upload(dr[i], reactive[i], (size_t)n_reactive[i]));
    cdev[i] = dc[i].as<double>();
    rdev[i] = dr[i].as<int64_t>();
  }
  FC_TRY(upload(dconf, conf, (size_t)J * 3));
  FC_TRY(upload(dps, piv_start, (size_t)J * 9));
  FC_TRY(upload(dpe, piv_end, (size_t)J * 9));
  FC_TRY(upload(dvecs, vecs, (size_t)J * 8 * 18));
  FC_TRY(upload(dd0, dirs0, (size_t)J * 9));
  FC_TRY(upload(drun, run, (size_t)J * 8));
  FC_TRY(upload(drt, rtab, (size_t)J * 8 * 9));
  FC_TRY(upload(dn, norms, (size_t)J * 3));
  FC_TRY(upload(dua, ua, (size_t)3 * U));
  FC_TRY(upload(daidx, aidx, (size_t)S * 3));
  FC_TRY(ddirs.reserve((size_t)J * 8 * 9 * sizeof(double)));
  FC_TRY(dRt.reserve((size_t)J * 8 * 3 * U * 12 * sizeof(double)));
  FC_TRY(dpass.reserve((size_t)J * 8 * S));
  FC_TRY(dacc.reserve((size_t)J * 8 * S));
  FC_HIP_TRY(hipMemsetAsync(dRt.p, 0, (size_t)J * 8 * 3 * U * 12 * sizeof(double), ctx().stream));
  FC_TRY(launch_tri_embed(cdev, rdev, n_atoms, n_reactive, J, dconf.as<int64_t>(), dps.as<double>(),
                          dpe.as<double>(), dvecs.as<double>(), dd0.as<double>(), drun.as<uint8_t>(),
                          drt.as<int64_t>(), dn.as<double>(), dua.as<double>(), (int)U, daidx.as<int32_t>(),
                          (int)S, thresh, (int)max_clashes, rmsd_thr, ddirs.as<double>(), dRt.as<double>(),
                          dpass.as<uint8_t>(), dacc.as<uint8_t>()));
  FC_TRY(d2h(dirs_out, ddirs.p, (size_t)J * 8 * 9 * sizeof(double)));
  FC_TRY(d2h(Rt_out, dRt.p, (size_t)J * 8 * 3 * U * 12 * sizeof(double)));
  FC_TRY(d2h(pass_out, dpass.p, (size_t)J * 8 * S));
  FC_TRY(d2h(accept_out, dacc.p, (size_t)J * 8 * S));
  return sync();
}

int fc_string_embed(const double *m1, int64_t n1, int64_t A1, const double *centers1,
                    const double *orbvecs1, int64_t K1, const double *m2, int64_t n2, int64_t A2,
                    const double *centers2, const double *orbvecs2, int64_t K2,
                    const double *angles, int64_t nA, const int64_t *quads, int64_t Q,
                    double thresh, int64_t max_clashes, double tfd_thresh, uint8_t *pass_out,
                    uint8_t *accept_out, double *R2_out, double *t2_out) {
  FC_API_LOCK;
  FC_REQUIRE(m1 && m2 && centers1 && orbvecs1 && centers2 && orbvecs2 && angles && pass_out && accept_out,
             "NULL pointer argument");
  FC_REQUIRE(n1 >= 1 && n2 >= 1 && A1 >= 1 && A2 >= 1 && K1 >= 1 && K2 >= 1 && nA >= 1 && Q >= 0, "bad shape");
  FC_REQUIRE(quads || Q == 0, "quads is NULL");
  if (Q > 128) return set_error(FC_E_LIMIT, "Q=%lld fingerprints exceed 128", (long long)Q);
  for (int64_t k = 0; k < Q * 4; ++k) FC_REQUIRE(quads[k] >= 0 && quads[k] < A1 + A2, "quadruplet index out of range");
  if (4 * A1 * 24 > (int64_t)kLdsLimit) return set_error(FC_E_LIMIT, "A1=%lld too large for the LDS slice", (long long)A1);
  FC_TRY(ensure_init());
  const int64_t P = n1 * n2 * K1 * K2 * nA;
  DevBuf d1, d2, dc1, dv1, dc2, dv2, da, dq, dR, dt, di1, di2, dpass, dacc, drej, dtf, daccT, dn;
  FC_TRY(upload(d1, m1, (size_t)n1 * A1 * 3));
  FC_TRY(upload(d2, m2, (size_t)n2 * A2 * 3));
  FC_TRY(upload(dc1, centers1, (size_t)n1 * K1 * 3));
  FC_TRY(upload(dv1, orbvecs1, (size_t)n1 * K1 * 3));
  FC_TRY(upload(dc2, centers2, (size_t)n2 * K2 * 3));
  FC_TRY(upload(dv2, orbvecs2, (size_t)n2 * K2 * 3));
  FC_TRY(upload(da, angles, (size_t)nA));
  FC_TRY(upload(dq, quads, (size_t)Q * 4));
  FC_TRY(dR.reserve((size_t)P * 9 * sizeof(double)));
  FC_TRY(dt.reserve((size_t)P * 3 * sizeof(double)));
  FC_TRY(di1.reserve((size_t)P * sizeof(int64_t)));
  FC_TRY(di2.reserve((size_t)P * sizeof(int64_t)));
  FC_TRY(dpass.reserve((size_t)P));
  FC_TRY(dacc.reserve((size_t)P));
  FC_TRY(drej.reserve(256));
  FC_TRY(dtf.reserve((size_t)P * std::max<int64_t>(Q, 1) * sizeof(double)));
  FC_TRY(daccT.reserve((size_t)P * std::max<int64_t>(Q, 1) * sizeof(double)));
  FC_TRY(dn.reserve(sizeof(uint64_t)));
  FC_HIP_TRY(hipMemsetAsync(dn.p, 0, sizeof(uint64_t), ctx().stream));
  FC_HIP_TRY(hipMemsetAsync(drej.p, 0, 256, ctx().stream));
  FC_TRY(launch_string_transforms(dc1.as<double>(), dv1.as<double>(), n1, K1, dc2.as<double>(), dv2.as<double>(),
                                  n2, K2, da.as<double>(), nA, dR.as<double>(), dt.as<double>(),
                                  di1.as<int64_t>(), di2.as<int64_t>()));
  FC_TRY(launch_embed_poses_clash(d1.as<double>(), A1, d2.as<double>(), A2, di1.as<int64_t>(), di2.as<int64_t>(),
                                  nullptr, nullptr, dR.as<double>(), dt.as<double>(), P, thresh, max_clashes,
                                  nullptr, dpass.as<uint8_t>(), nullptr));
  FC_TRY(launch_pose_fingerprints(d1.as<double>(), A1, d2.as<double>(), A2, di1.as<int64_t>(), di2.as<int64_t>(),
                                  dR.as<double>(), dt.as<double>(), P, dq.as<int64_t>(), Q, dpass.as<uint8_t>(),
                                  dtf.as<double>()));
  for (int64_t c0 = 0; c0 < P; c0 += 256)
    FC_TRY(launch_leader_chunk(dtf.as<double>(), Q, c0, P, dpass.as<uint8_t>(), daccT.as<double>(), P,
                               reinterpret_cast<unsigned long long *>(dn.p), tfd_thresh, drej.as<uint8_t>(),
                               dacc.as<uint8_t>()));
  FC_TRY(d2h(pass_out, dpass.p, (size_t)P));
  FC_TRY(d2h(accept_out, dacc.p, (size_t)P));
  if (R2_out) FC_TRY(d2h(R2_out, dR.p, (size_t)P * 9 * sizeof(double)));
  if (t2_out) FC_TRY(d2h(t2_out, dt.p, (size_t)P * 3 * sizeof(double)));
  return sync();
}

}  // extern "C"
