// fc_internal.h -- every function that one translation unit of libfc_hip.so defines and another one uses is declared
// here and nowhere else, grouped by the file that defines it (what fc_common.h already declares stays there).  The
// defining file includes this header too: a signature that drifts fails to compile instead of failing to link, or
// linking and misbehaving.  Default arguments appear here only.  It brings fc_common.h with it.
#pragma once

#include "fc_common.h"

namespace fc {

// ---- fc_kabsch.hip ---------------------------------------------------------------------------------------
int prebuild_screen_items(fc_ensemble *e);
int launch_rmsd_values(fc_ensemble *e, double small_rmsd, double *rmsd_dev, double *maxdev_dev, int64_t rank = 0,
                       int64_t world = 1, bool explicit_sum = false);
int launch_gather_matrix_pairs(const double *rmsd_m, const double *maxdev_m, int64_t N, const int64_t *pi_dev,
                               const int64_t *pj_dev, int64_t P, double *rmsd_out, double *maxdev_out);
int launch_mirror_upper(double *m_dev, int64_t N);
int launch_scatter_pairs(const uint64_t *pairs_dev, int64_t n_pairs, int64_t N, int64_t W, uint64_t *bits_dev);
int launch_prep_begin(fc_ensemble *e);
int launch_prep_body(const double *coords_dev, int64_t N, int64_t A_all, const int32_t *sel_dev, int64_t A, int center,
                     fc_ensemble *e, const int32_t *conf_idx_dev);
int launch_pairs_exact(const fc_ensemble *e, const int64_t *pi_dev, const int64_t *pj_dev, int64_t P, double *rmsd_dev,
                       double *maxdev_dev, double *R_dev, bool inverted = false);  // inverted: the values of (X_i, -X_j)
int launch_matrix_exact(const fc_ensemble *e, double *rmsd_dev, double *maxdev_dev);
int last_screen_kind();
void screen_select(int kind);
int ensure_h2_operands(fc_ensemble *e, double *scale_out);
int launch_simbits_screen(fc_ensemble *e, double thr2_margin);
int debug_screen_plan(int64_t N, int64_t A, int64_t row_block, bool lean, double g_max, double max_rmsd, int h2_model,
                      int64_t plan_out[5]);
int launch_simbits_refine(fc_ensemble *e, double max_rmsd, double max_dev, const double *energies_dev, double max_dE);
int launch_align_to_first(const double *coords_dev, int64_t N, int64_t A, const int64_t *idx_dev, int64_t n_idx,
                          double *out_dev);
int launch_alignment_matrices(const double *p_dev, const double *q_dev, int64_t n, int64_t A, double *M_dev);
int warm_kabsch();
// ---- fc_h2_check.hip -------------------------------------------------------------------------------------
int h2_model_ok(bool *ok);
int h2_model_report(int64_t trials, int64_t *flags_out, double *worst_out);
int launch_h2_cov_tile(const fc_ensemble *e, int64_t ib, int64_t jb, float *out_dev);
int warm_h2_check();
// ---- fc_prune.hip ----------------------------------------------------------------------------------------
int launch_leader_chunk(const double *tf_dev, int64_t Q, int64_t chunk0, int64_t P, const uint8_t *pass_dev,
                        double *accT_dev, int64_t cap, unsigned long long *n_acc_dev, double thresh,
                        uint8_t *rejected_dev, uint8_t *accept_dev);
int launch_pack_mask(const uint8_t *mask_dev, int64_t N, uint64_t *mbits_dev, int64_t W,
                     unsigned long long *counters_dev);
int launch_level(const uint64_t *bits_dev, int64_t W, const uint64_t *mbits_dev, const uint8_t *mask_in,
                 uint8_t *mask_out, int64_t N, int64_t k, int64_t IB, int64_t rank, int64_t world, int64_t rows_local);
int launch_mask_init(uint64_t *mb_dev, int64_t N, int64_t W, int64_t total_words);
int launch_level_fused(const uint64_t *bits_dev, int64_t W, const uint64_t *mb_in, uint64_t *mb_out, int64_t N,
                       int64_t k, int64_t min_per_group, unsigned long long *counters);
void prune_conventions_set(int drop_later);
int prune_drop_later();
int launch_ladder_pairs_many(const uint64_t *pairs_dev, uint64_t *buckets_dev, const unsigned long long *n_pairs_dev,
                             const unsigned long long *n_cand_dev, unsigned long long cand_cap, unsigned long long cap,
                             int64_t N, int64_t W, int64_t min_per_group, const int64_t *ladder_dev,
                             const int64_t *ladder_host, int n_ladder, uint64_t *mask_bufs_dev, uint64_t *mask_out_dev,
                             unsigned long long *counters_dev, unsigned grid);
constexpr long kLadderManyGridMax = 4096;
unsigned ladder_many_grid();
int launch_ladder_pairs(const uint64_t *pairs_dev, uint64_t *buckets_dev, const unsigned long long *n_pairs_dev,
                        const unsigned long long *n_cand_dev, unsigned long long cand_cap, unsigned long long cap,
                        int64_t N, int64_t W, int64_t min_per_group, const int64_t *ladder_dev, int n_ladder,
                        uint64_t *mask_out_dev, unsigned long long *counters_dev);
int launch_export_pairs(const uint64_t *simq_dev, const unsigned long long *counters_dev, unsigned long long cand_cap,
                        int64_t cap, uint64_t *out_dev);
int launch_compact_gathered(const uint64_t *gathered_dev, int world, int64_t cap, uint64_t *list_dev,
                            unsigned long long *counters_dev);
int launch_copy_bytes(const uint8_t *src, uint8_t *dst, int64_t n);
int launch_inertia_moments(const double *coords_dev, int64_t N, int64_t A, const double *masses_dev,
                           double *moments_dev);
int launch_moi_simbits(const double *moments_dev, int64_t N, double tol, const double *energies_dev, double max_dE,
                       uint64_t *bits_dev, int64_t W);
int launch_transpose_pad(const double *in_dev, int64_t N, int64_t Q, int64_t Npad, double *out_dev);
int launch_gather_transpose_pad(const double *in_dev, const double *first_dev, const int64_t *idx_dev, int64_t M,
                                int64_t Q, int64_t Npad, double *out_dev);
int launch_tfd_first_match(const double *tfT_dev, int64_t N, int64_t Npad, int64_t Q, double thresh, int64_t *fm_dev,
                           float *tfF_scratch);
int tfd_last_form(int64_t *n_open_out);
int launch_tfd_simbits(const double *tf_dev, int64_t N, int64_t Q, double thresh, int64_t row_begin, int64_t row_end,
                       uint64_t *bits_dev, int64_t W);
int warm_prune();
// ---- fc_clash.hip ----------------------------------------------------------------------------------------
double sq_threshold_lt(double t);
double sq_threshold_le(double t);
int launch_clash_self(const double *coords_dev, int64_t N, int64_t A, double lo, double hi, int64_t *counts_dev);
int launch_clash_fragments(const double *coords_dev, int64_t N, int64_t A, const int64_t *ids, int64_t n_ids,
                           double thresh, int64_t max_clashes, int64_t *counts_dev, uint8_t *pass_dev);
int launch_clash_graph(const double *coords_dev, int64_t N, int64_t A, const uint8_t *adj_dev, double thresh,
                       int64_t *counts_dev);
int launch_fitness(const double *coords_dev, int64_t N, int64_t A, const int64_t *pairs_dev, const double *targets_dev,
                   int64_t C, double threshold, double *err_dev, uint8_t *pass_dev);
int launch_rototranslate(const double *coords_dev, int64_t n, int64_t A, const double *R_dev, const double *t_dev,
                         double *out_dev);
int launch_center_structures(const double *coords_dev, int64_t N, int64_t A, double *out_dev);
int launch_moi_diag_pairs(const double *moments_dev, int64_t N, double *P_dev, double *Q_dev);
int launch_set_identity(double *M_dev);
int launch_embed_poses_clash(const double *m1_dev, int64_t A1, const double *m2_dev, int64_t A2, const int64_t *c1_dev,
                             const int64_t *c2_dev, const double *R1_dev, const double *t1_dev, const double *R2_dev,
                             const double *t2_dev, int64_t P, double thresh, int64_t max_clashes, int64_t *counts_dev,
                             uint8_t *pass_dev, double *poses_dev);
int warm_clash();
// ---- fc_torsion.hip --------------------------------------------------------------------------------------
int launch_torsion_scan(const double *base_dev, int64_t A, const int64_t *torsions_dev, int64_t T,
                        const uint8_t *rotmasks_dev, const int16_t *mv_dev, const int16_t *rs_dev,
                        const int32_t *nmv_dev, const int32_t *nrs_dev, const int64_t *angles_dev, int64_t S,
                        double thresh, int64_t backoff, double *out_dev, int64_t *rot_dev, const int64_t *quads_dev,
                        int64_t Q, double *tf_dev);
int launch_rotcorr_simbits(const double *X_dev, int64_t N, int64_t A, const uint8_t *heavy_dev, const int64_t *tors_dev,
                           int64_t T, const uint8_t *rotmasks_dev, const double *angles_dev,
                           const int32_t *n_angles_dev, int max_angles, double max_rmsd, double max_dev,
                           const double *energies_dev, double max_dE, uint64_t *bits_dev, int64_t W);
int launch_torsion_fingerprint(const double *coords_dev, int64_t N, int64_t A, const int64_t *quads_dev, int64_t Q,
                               double *tf_dev);
int launch_angle_grid(const int64_t *values_dev, const int64_t *first_dev, const int64_t *counts_dev, int64_t T,
                      int64_t S, int64_t *out_dev);
int launch_rows_to_sets(const int64_t *idx_dev, const int64_t *rows_dev, int64_t n, int64_t *out_dev);
int launch_select_rotated(const int64_t *rot_dev, int64_t S, int64_t *idx_dev, int64_t *count_dev, DevBuf &tmp);
int warm_torsion();
// ---- fc_embed.hip ----------------------------------------------------------------------------------------
int launch_string_transforms(const double *cen1, const double *vec1, int64_t n1, int64_t K1, const double *cen2,
                             const double *vec2, int64_t n2, int64_t K2, const double *angles, int64_t nA,
                             double *R_dev, double *t_dev, int64_t *c1_dev, int64_t *c2_dev);
int launch_pose_fingerprints(const double *m1, int64_t A1, const double *m2, int64_t A2, const int64_t *c1,
                             const int64_t *c2, const double *R2, const double *t2, int64_t P, const int64_t *quads,
                             int64_t Q, const uint8_t *pass, double *tf);
int launch_embed_group_dedupe(const double *X1a, int64_t n1, int64_t A1, int64_t na1, const double *X2a, int64_t n2,
                              int64_t A2, int64_t na2, double thr, const uint8_t *pass_dev, uint8_t *accept_dev);
int launch_embed_mol_transforms(const double *coords_dev, int64_t n, int64_t A, const int64_t *reactive_dev, int nr,
                                const double *ps_dev, const double *pe_dev, int mol, const double *angles_dev,
                                int64_t na, double *R_dev, double *t_dev);
int launch_embed_pretransform(const double *coords_dev, int64_t n, int64_t A, int64_t na, const double *R_dev,
                              const double *t_dev, int aos, int64_t S, double *out_dev);
int launch_embed_grid_clash(const double *X1_dev, int64_t n1, int64_t A1, int64_t na1, const double *X2s_dev,
                            int64_t n2, int64_t A2, int64_t na2, int64_t S2, double thresh, int64_t max_clashes,
                            void *scratch, size_t scratch_bytes, uint8_t *pass_dev, int32_t *counts_dev);
int warm_embed();
// ---- fc_embed3.hip ---------------------------------------------------------------------------------------
size_t tri_group_lds_bytes(int64_t Atot, int U, int S);
int launch_tri_embed(const double *const coords_dev[3], const int64_t *const reactive_dev[3], const int64_t A[3],
                     const int64_t nr[3], int64_t J, const int64_t *conf_dev, const double *piv_start_dev,
                     const double *piv_end_dev, const double *vecs_dev, const double *dirs0_dev, const uint8_t *run_dev,
                     const int64_t *rtab_dev, const double *norms_dev, const double *ua_dev, int U,
                     const int32_t *aidx_dev, int S, double thresh, int max_clashes, double rmsd_thr, double *dirs_dev,
                     double *Rt_dev, uint8_t *pass_dev, uint8_t *accept_dev);
int warm_embed3();
// ---- fc_diverse.hip and fc_knn.hip: the table of a launch under d_sym -----------------------------------------
// on the device as 16-bit indices, K rows of the ensembles' A selected atoms (k_diverse_step_sym, k_knn_tile_sym)
struct SymTable {
  const uint16_t *perms_dev = nullptr;
  int K = 1;
  bool mirror = false;
  // two counters, or nullptr: the (k, h) of a step / the (pair, p, h) of a tile whose eigenvalue was formed, and those
  // of them that went on to the explicit pass
  unsigned long long *stats_dev = nullptr;
};
// ---- fc_diverse.hip --------------------------------------------------------------------------------------
int diverse_lanes(int64_t N);
size_t diverse_sym_lds_bytes(int64_t A, int64_t K);  // representative + table + the kernel's static LDS
int select_diverse(fc_ensemble *e, int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out,
                   double *radii_out, int32_t *labels_out, double *dist_out, int64_t *n_selected, double *ms_device,
                   const SymTable *sym = nullptr);
int warm_diverse();
// ---- fc_clusters.hip -------------------------------------------------------------------------------------
// the graph whose components are labelled: a device pair list OR a bit matrix
struct ClusterGraph {
  const uint64_t *pairs_dev = nullptr;               // (i << 32) | j, either order, duplicates allowed
  const unsigned long long *n_pairs_dev = nullptr;   // the list's length on the device (counters + 2); nullptr: n_pairs_host
  unsigned long long n_pairs_host = 0;
  bool known_short = false;                          // speed only: the list is known to be short, hook it in one launch
  const unsigned long long *n_cand_dev = nullptr;    // counters + 6: the list is declined when it exceeds cand_cap
  unsigned long long cand_cap = 0;
  const unsigned long long *redo_dev = nullptr;      // counters + 12: ... or when the screen's verdict asked for a redo
  const uint64_t *bits_dev = nullptr;                // rows of W words, only bits j > i are read
  int64_t W = 0;
};
// words of the status block behind the results
constexpr int kClStatusErr = 0;    // 1: a union ran into its retry cap (FC_E_INTERNAL)
constexpr int kClStatusList = 1;   // 1: the pair list produced the result, 0: the hook kernel declined it
constexpr int kClStatusK = 2;      // number of clusters
constexpr int kClStatusPairs = 3;  // length of a list uploaded by the caller
constexpr int64_t kClShortList = 1 << 16;  // pair lists below this are hooked in one launch (fc_clusters.hip)
// words of the status block that only the sphere-exclusion form has
constexpr int kBuStatusRounds = 4;  // rounds of the rule until nothing was undecided
constexpr int kBuStatusLeft = 5;    // vertices that went to the finish
// which labelling a block serves
enum ClKind { kClComponents = 0, kClDensity = 1, kClButina = 2 };
// one block: labels | reps | sizes [| core | degrees] | status (the part that travels to the host, result_bytes from
// offset 0) | scratch [+ attach | the sphere-exclusion scratch].  kClDensity adds core, degrees and attach, kClButina
// degrees (no core), four more status words and its own scratch behind everything else; the fields a kind does not have
// stay 0, and the offsets of the other two kinds do not depend on it.  live_cap: entries of kClButina's live-edge list
struct ClusterLayout {
  size_t labels, reps, sizes, status, result_bytes, parent, root, flags, prefix, total, core, degrees, attach;
  size_t bu_key, bu_owner, bu_state, bu_claim, bu_stamp, bu_live_v, bu_words, bu_live_e;
};
constexpr int kBuRoundsMax = 64;             // parallel rounds at most (FC_BUTINA_ROUNDS is cut to it)
constexpr int kBuWords = kBuRoundsMax + 8;   // und[0 .. kBuRoundsMax + 1] and the live-edge count
inline ClusterLayout cluster_layout(int64_t N, ClKind kind, size_t live_cap = 0) {
  const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t n = (size_t)(N > 0 ? N : 1), w = (n + 63) / 64;
  const bool density = kind == kClDensity, butina = kind == kClButina;
  ClusterLayout L{};
  L.labels = 0;
  L.reps = up(n * sizeof(int32_t));
  L.sizes = L.reps + up(n * sizeof(int64_t));
  L.status = L.sizes + up(n * sizeof(int64_t));
  if (density) {
    L.core = L.status;
    L.degrees = L.core + up(n * sizeof(uint8_t));
    L.status = L.degrees + up(n * sizeof(int32_t));
  }
  if (butina) {
    L.degrees = L.status;
    L.status = L.degrees + up(n * sizeof(int32_t));
  }
  L.result_bytes = L.status + (butina ? 8 : 4) * sizeof(uint64_t);
  L.parent = up(L.result_bytes);
  L.root = L.parent + up(n * sizeof(int32_t));
  L.flags = L.root + up(n * sizeof(int32_t));
  L.prefix = L.flags + up(w * sizeof(uint64_t));
  L.total = L.prefix + up(w * sizeof(int32_t));
  if (density) {
    L.attach = L.total;
    L.total = L.attach + up(n * sizeof(uint32_t));
  }
  if (butina) {
    L.bu_key = L.total;
    L.bu_owner = L.bu_key + up(n * sizeof(uint64_t));
    L.bu_state = L.bu_owner + up(n * sizeof(uint64_t));
    L.bu_claim = L.bu_state + up(n * sizeof(int32_t));
    L.bu_stamp = L.bu_claim + up(n * sizeof(int32_t));
    L.bu_live_v = L.bu_stamp + up(n * sizeof(int32_t));
    L.bu_words = L.bu_live_v + up(n * sizeof(int32_t));
    L.bu_live_e = L.bu_words + up(kBuWords * sizeof(uint64_t));
    L.total = L.bu_live_e + up((live_cap > 0 ? live_cap : 1) * sizeof(uint64_t));
  }
  return L;
}
// `work` holds cluster_layout(N, kClComponents).total bytes
int launch_clusters(const ClusterGraph &g, int64_t N, DevBuf &work);
// the graph of launch_clusters under the core rule (degree + 1 >= min_samples); pair lists: each unordered pair once;
// `work` holds cluster_layout(N, kClDensity).total bytes
int launch_dbscan(const ClusterGraph &g, int64_t N, int64_t min_samples, DevBuf &work);
// the sphere-exclusion clusters of the same graph (include/fc_hip.h, "sphere-exclusion clusters"); pair lists: each
// unordered pair once; `work` holds cluster_layout(N, kClButina, butina_live_cap(g, N)).total bytes
size_t butina_live_cap(const ClusterGraph &g, int64_t N);
int launch_butina(const ClusterGraph &g, int64_t N, DevBuf &work);
int warm_clusters();
// ---- fc_symm.hip -----------------------------------------------------------------------------------------
constexpr int64_t kPermMax = FC_PERM_MAX;
size_t symm_lds_bytes(int64_t A, int64_t K);  // dynamic LDS of a tile of k_symm_simbits: both coordinate tiles + the table
int launch_symm_simbits(fc_ensemble *e, const uint16_t *perms_dev, int64_t K, double max_rmsd, double max_dev,
                        const double *energies_dev, double max_dE);
int launch_symm_pairs(const fc_ensemble *e, const uint16_t *perms_dev, int64_t K, const int64_t *pi_dev,
                      const int64_t *pj_dev, int64_t P, double *rmsd_dev, double *maxdev_dev);  // (P, K) outputs
int warm_symm();
// ---- fc_knn.hip ------------------------------------------------------------------------------------------
int knn_strips(int64_t Nq, int64_t Nr);  // column strips of the launch of Nq rows against Nr columns (FC_KNN_STRIPS forces it)
size_t knn_sym_lds_bytes(int64_t A, int64_t K);  // the workgroup's 16 row conformers + the table
int knn(fc_ensemble *q, fc_ensemble *r, bool cross, int64_t k, double max_rmsd, int32_t *indices_out, double *dist_out,
        double *ms_device, int64_t *strips_out, const SymTable *sym = nullptr);
int warm_knn();
// ---- fc_medoid.hip ---------------------------------------------------------------------------------------
int medoid_strips(int64_t N);  // strips a row tile's chunk range is cut into (FC_MEDOID_STRIPS forces it)
// S | E; sym (may be NULL): under d_sym (k_group_sums_sym), the rows and the table within the LDS (knn_sym_lds_bytes)
int launch_group_sums(const fc_ensemble *e, const int32_t *seg_end_dev, unsigned long long *out_dev, bool timed,
                      const SymTable *sym = nullptr);
int sums_sym_filter();  // FC_MEDOID_SYM_FILTER=0: every (p, h) explicit in k_group_sums_sym and k_silhouette_tile_sym
int ensemble_gather(const fc_ensemble *src, const int32_t *idx_dev, int64_t n, fc_ensemble *out, bool exact_gmax);
int warm_medoid();
// ---- fc_silhouette.hip -----------------------------------------------------------------------------------
int silhouette_strips(int64_t M);  // the same rule (FC_SILHOUETTE_STRIPS forces it)
size_t silhouette_result_bytes(int64_t M);  // a (M doubles) | b (M doubles) | nearest (M int32) at the front of the work block
size_t silhouette_work_bytes(int64_t M, int S);
int launch_silhouette(const fc_ensemble *e, const int32_t *seg_begin_dev, const int32_t *seg_end_dev, int S, uint8_t *work_dev,
                      bool timed, const SymTable *sym = nullptr);  // sym (may be NULL): under d_sym (k_silhouette_tile_sym)
int warm_silhouette();
// ---- fc_group_mean.hip -----------------------------------------------------------------------------------
// the tables of a call, on the device, over the label-sorted ensemble (fc_api_group_mean.cpp builds them)
struct GroupMeanPlan {
  int64_t M = 0, n_groups = 0;          // positions of the sorted copy; group ids
  const int32_t *grp_dev = nullptr;     // (M) the group of a position
  const int32_t *init_dev = nullptr;    // (n_init, 2) group, position of its reference member: every non-empty group
  int64_t n_init = 0;
  const int32_t *chunks_dev = nullptr;  // (n_chunks, 3) begin, end, group: group_mean_chunk() positions of a segment each
  int64_t n_chunks = 0;
  const int32_t *active_dev = nullptr;  // (n_active, 4) group, first chunk, chunks, members: groups of two or more
  int64_t n_active = 0;
};
// mean (n_groups, A, 3), rmsf (n_groups, A), frozen and n_iter (n_groups) are the caller's to size; the rest is sized
// by group_means_run
struct GroupMeanWork {
  DevBuf mean, Gm, rmsf, frozen, n_iter, Y, part, d, R, words;
};
int64_t group_mean_stage_atoms();  // the mean is staged in LDS up to this many selected atoms
int group_mean_chunk();
bool group_mean_stage(int64_t A);
int group_means_run(const fc_ensemble *e, const GroupMeanPlan &pl, GroupMeanWork &w, int64_t max_iter, double tol, bool timed);
int warm_group_mean();
// ---- fc_api_medoids.cpp ----------------------------------------------------------------------------------
// the conformers by group: order = a stable sort of the labelled conformers by label, group c = order[offs[c] .. offs[c + 1])
struct Grouping {
  std::vector<int32_t> order;
  std::vector<int64_t> offs;
  int64_t largest = 0;
};
void group_by_label(const int32_t *labels, int64_t N, int64_t n_groups, Grouping &g);
int labels_check(const int32_t *labels, int64_t N, int64_t n_groups);
// ---- fc_tfd_ladder.hip -----------------------------------------------------------------------------------
int tfd_ladder_device(const int64_t *fm_dev, const int64_t *fm_host, int64_t N, uint8_t *mask_out);
int pyset_order_pairs_device(const int64_t *pairs_host, int64_t n, int64_t *order_out);
int warm_tfd_ladder();
// ---- fc_tfd_host.cpp -------------------------------------------------------------------------------------
void pyset_order_ints(const int64_t *keys, int64_t n, std::vector<int64_t> &out);
void pyset_order_pairs(const int64_t *pairs, int64_t n, std::vector<int64_t> &out);
int tfd_apply_levels_host(const int64_t *fm, int64_t N, const std::vector<const uint8_t *> &level_flags,
                          int first_level, const uint8_t *first_last_flags, uint8_t *mask_out, int64_t active_known);
int tfd_ladder_host_only(const int64_t *fm, int64_t N, uint8_t *mask_out);
int tfd_ladder_from_first_match(const int64_t *fm, int64_t N, uint8_t *mask_out, const int64_t *fm_dev = nullptr);
int tfd_ladder_from_device(const int64_t *fm_dev, int64_t N, uint8_t *mask_out);
uint32_t host_component_first_big(const uint32_t *mx, const uint32_t *mp, const uint32_t *ms, int64_t n,
                                  uint32_t n_graph);
int tfd_ladder_emulate_device(const int64_t *fm, int64_t N, uint8_t *mask_out);
// ---- fc_comm.cpp -----------------------------------------------------------------------------------------
int comm_rank();
int comm_world();
int comm_allgather_dev(const void *send_dev, void *recv_dev, size_t bytes, int lane);
void comm_teardown();
// ---- fc_xyz.cpp ------------------------------------------------------------------------------------------
int xyz_write(const char *path, const char *const *atoms, int64_t A, const double *coords, int64_t N, const char *label,
              int mode);
int xyz_read(const char *path, int64_t *N_io, int64_t *A_io, char *atoms_out, double *coords_out);
// ---- fc_api_ensemble.cpp ---------------------------------------------------------------------------------
constexpr int64_t kHostGmaxDoubles = 36000;  // N * A * 3 up to which host_largest_g beats the wait for the device's
double host_largest_g(const double *coords, int64_t N, int64_t A_all, const std::vector<int32_t> &sel, int center);
int ensemble_build(const double *coords, int64_t N, int64_t A_all, const uint8_t *atom_mask, int center, fc_ensemble *e,
                   bool defer_wait = false, bool host_gmax = false);
int ensemble_build_dev(const double *raw_dev, int64_t N, int64_t A_all, const uint8_t *atom_mask, int center,
                       const int32_t *conf_idx_dev, fc_ensemble *e, bool defer_wait = false);
int ensemble_build_finish(fc_ensemble *e);
int ensemble_shard(fc_ensemble *e, int64_t rank, int64_t world, int64_t row_block);
int ensemble_twin(fc_ensemble *ens, fc_ensemble **out);
int64_t owned_pairs(int64_t N, int64_t row_block, int64_t rank, int64_t world);
int timing_events(int64_t n);
int elapsed_ms(hipEvent_t a, hipEvent_t b, double *out);
int mean_elapsed_ms(const std::vector<hipEvent_t> &ev, int64_t n, int64_t per, int64_t step, double *out);
int perm_table_check(const int32_t *perms, int64_t K, int64_t A_sel, std::vector<uint16_t> &table);
int perm_lds_check(size_t lds, int64_t A_sel, int64_t K, const char *per = "");
int perm_ensemble_check(const fc_ensemble *ens, int64_t K, int64_t A_sel, bool bit_matrix);
// ---- fc_api_prune.cpp ------------------------------------------------------------------------------------
int64_t default_row_block();
int simbits_local(fc_ensemble *e, double max_rmsd, double max_dev, const double *energies, double max_dE,
                  bool zero_counters, bool lean = false);
int symm_local(fc_ensemble *e, const std::vector<uint16_t> &table, int64_t K, DevBuf &dperm, double max_rmsd,
               double max_dev, const double *energies, double max_dE);
void note_candidates(fc_ensemble *e, unsigned long long refined, unsigned long long similar);
void fill_stats(int64_t *stats, int64_t pairs, const unsigned long long *cnt, int64_t s4, int64_t s5);

// ---- shared by the fc_api_*.cpp files ----------------------------------------------------------------------------
// host array -> device buffer (grown to fit)
template <class T>
inline int upload(DevBuf &b, const T *host, size_t count) {
  FC_TRY(b.reserve(count * sizeof(T)));
  return h2d(b.p, host, count * sizeof(T));
}

// On an error nothing of a DevBuf may be in flight when it goes out of scope: `return drained(rc);` in front of it waits
// for the stream first (rc passes through; FC_OK costs nothing).
inline int drained(int rc) {
  if (rc != FC_OK && ctx().ready) (void)hipStreamSynchronize(cur_stream());
  return rc;
}

// ---- the forms under d_sym (fc_api_neighbours.cpp, fc_api_medoids.cpp) -------------------------------------------
// a checked table, as the entry point was given it
struct SymArgs {
  std::vector<uint16_t> table;  // (K, A_sel), as perm_table_check leaves it
  int K = 1;
  bool mirror = false;
  int64_t *stats = nullptr;  // (may be NULL) the two counters of SymTable::stats_dev after the call
};

// what every form under d_sym refuses first: the table, the LDS its kernel needs for it, the flag
inline int sym_args_check(const int32_t *perms, int64_t K, int64_t A_sel, int mirror, size_t (*lds_bytes)(int64_t, int64_t),
                          SymArgs &a) {
  FC_TRY(perm_table_check(perms, K, A_sel, a.table));
  FC_TRY(perm_lds_check(lds_bytes(A_sel, K), A_sel, K));
  FC_REQUIRE(mirror == 0 || mirror == 1, "mirror=%d: 0 or 1", mirror);
  a.K = (int)K, a.mirror = mirror != 0;
  return FC_OK;
}

// the table on the device and, when they are asked for, the two counters behind it
struct SymUpload {
  DevBuf perm, stats;
  int put(const SymArgs &a, SymTable &sym) {
    FC_TRY(upload(perm, a.table.data(), a.table.size()));
    sym.perms_dev = perm.as<uint16_t>(), sym.K = a.K, sym.mirror = a.mirror;
    if (!a.stats) return FC_OK;
    FC_TRY(stats.reserve(2 * sizeof(unsigned long long)));
    FC_HIP_TRY(hipMemsetAsync(stats.p, 0, 2 * sizeof(unsigned long long), ctx().stream));
    sym.stats_dev = reinterpret_cast<unsigned long long *>(stats.p);
    return FC_OK;
  }
  int read(int64_t out[2]) {
    unsigned long long cnt[2] = {0, 0};
    FC_TRY(d2h(cnt, stats.p, sizeof cnt));
    FC_TRY(sync());
    out[0] = (int64_t)cnt[0], out[1] = (int64_t)cnt[1];
    return FC_OK;
  }
};

// call(sym) behind the checks and ensure_init; a (may be NULL): under d_sym -- the table goes up first and lives, like the
// counters, until the call's last wait
template <class Call>
inline int with_sym_table(const SymArgs *a, const Call &call) {
  if (!a) return call(nullptr);
  SymUpload up;
  SymTable sym;
  int rc = up.put(*a, sym);
  if (rc == FC_OK) rc = call(&sym);
  if (rc == FC_OK && a->stats) rc = up.read(a->stats);
  return drained(rc);
}

// The enantiomer-aware forms (include/fc_hip.h) are the plain entry points with fc_ensemble::enant set for the call: the
// flag selects the ENANT instantiations of the screen and refine kernels (launch_simbits_screen / _refine); it is cleared
// when the call returns, whatever it returns, so no other entry point ever sees it.
struct EnantScope {
  fc_ensemble *e;
  explicit EnantScope(fc_ensemble *ens) : e(ens) { e->enant = true; }
  ~EnantScope() { e->enant = false; }
  EnantScope(const EnantScope &) = delete;
  EnantScope &operator=(const EnantScope &) = delete;
};

}  // namespace fc
