// fc_api_clusters.cpp -- the extern "C" surface (include/fc_hip.h) of the cluster labellings: components, density-based
// and sphere-exclusion clusters of the prune's graph (plain, enantiomer- and symmetry-aware) or of a caller's graph.
#include <algorithm>

#include "fc_internal.h"

// ---- similarity clusters and density-based clusters (the contract: include/fc_hip.h; the kernels: fc_clusters.hip) ----
// Two axes, each said once: WHICH labelling runs on the graph (Labelling) and WHO makes the graph (a graph source, below).
using namespace fc;

namespace {
// the components of the graph, its density-based clusters with min_samples bound, or its sphere-exclusion clusters
struct Labelling {
  bool density;
  int64_t min_samples;
  const char *what;  // (in the error text)
  bool butina = false;
  ClKind kind() const { return density ? kClDensity : butina ? kClButina : kClComponents; }
  ClusterLayout layout(const ClusterGraph &g, int64_t N) const {
    return cluster_layout(N, kind(), butina ? butina_live_cap(g, N) : 0);
  }
  int launch(const ClusterGraph &g, int64_t N, DevBuf &work) const {
    if (butina) return launch_butina(g, N, work);
    return density ? launch_dbscan(g, N, min_samples, work) : launch_clusters(g, N, work);
  }
  int n_stats() const { return density || butina ? 8 : 6; }
};
Labelling components() { return {false, 1, "cluster labelling"}; }
Labelling density_based(int64_t min_samples) { return {true, min_samples, "density-based clusters"}; }
Labelling sphere_exclusion() { return {false, 1, "sphere-exclusion clusters", true}; }

// the caller's arrays; core: the density-based form's; degrees: its and the sphere-exclusion form's
struct LabelOut {
  int32_t *labels;
  int64_t *reps, *sizes;
  uint8_t *core;
  int32_t *degrees;
  int64_t *n_clusters;
  bool complete(const Labelling &lab) const {
    return labels && reps && sizes && (!lab.density || core) && (!(lab.density || lab.butina) || degrees);
  }
};

// what one labelling left in the pinned staging area: the result region of the workspace, then `extra` counter words
struct ClusterResult {
  const char *host = nullptr;
  ClusterLayout L{};
  const unsigned long long *status() const { return reinterpret_cast<const unsigned long long *>(host + L.status); }
  const unsigned long long *extra() const { return reinterpret_cast<const unsigned long long *>(host + L.parent); }
};

// labels the graph and brings the result to the host: enqueue, ONE copy chain into pinned memory, one wait.
// counters_dev (may be null): 16 counter words of the prune that travel behind the result.
int label_run(const Labelling &lab, const ClusterGraph &g, int64_t N, DevBuf &work, const void *counters_dev,
              ClusterResult *out) {
  const ClusterLayout L = lab.layout(g, N);
  FC_TRY(work.reserve(L.total));
  FC_TRY(pinned_reserve(L.parent + 16 * sizeof(uint64_t)));
  FC_TRY(lab.launch(g, N, work));
  char *host = static_cast<char *>(ctx().pinned);
  FC_TRY(d2h(host, work.p, L.result_bytes));
  if (counters_dev) FC_TRY(d2h(host + L.parent, counters_dev, 16 * sizeof(uint64_t)));
  FC_TRY(sync());
  out->host = host, out->L = L;
  if (out->status()[kClStatusErr] != 0ull)
    return set_error(FC_E_INTERNAL, "%s: %s on the device", lab.what,
                     lab.butina ? "the rounds ended with conformers undecided" : "a union exceeded its retry bound");
  return FC_OK;
}

// -> the caller's arrays; tail (may be NULL): the density-based form's [0] core points, [1] noise points; the
// sphere-exclusion form's [0] rounds, [1] conformers that went to the finish
void label_unpack(const ClusterResult &r, int64_t N, const LabelOut &o, int64_t *tail) {
  const int64_t K = (int64_t)r.status()[kClStatusK];
  std::memcpy(o.labels, r.host + r.L.labels, (size_t)N * sizeof(int32_t));
  std::memcpy(o.reps, r.host + r.L.reps, (size_t)K * sizeof(int64_t));
  std::memcpy(o.sizes, r.host + r.L.sizes, (size_t)K * sizeof(int64_t));
  if (r.L.core != 0) {  // (the density-based layout)
    std::memcpy(o.core, r.host + r.L.core, (size_t)N * sizeof(uint8_t));
    std::memcpy(o.degrees, r.host + r.L.degrees, (size_t)N * sizeof(int32_t));
  } else if (r.L.degrees != 0) {  // (the sphere-exclusion layout)
    std::memcpy(o.degrees, r.host + r.L.degrees, (size_t)N * sizeof(int32_t));
  }
  *o.n_clusters = K;
  if (tail == nullptr) return;
  if (r.L.core == 0) {
    tail[0] = (int64_t)r.status()[kBuStatusRounds], tail[1] = (int64_t)r.status()[kBuStatusLeft];
    return;
  }
  tail[0] = tail[1] = 0;
  for (int64_t i = 0; i < N; ++i) tail[0] += o.core[i] != 0, tail[1] += o.labels[i] < 0;
}

// The protocol of every resident entry point: list, status, matrix.  A graph source `make(lean)` fills the ensemble's
// pair queue and counters (lean) and, asked again with !lean, its bit matrix.  The labelling runs from the list first; the
// hook / degree kernel itself declines a list that is incomplete (the candidate queue overflowed: counters[6] >
// pairq_cap, read on the device), the host sees that in the status word that comes back with the results, and only then
// asks for the matrix and labels again.  Source::screened: the graph is the prune's own (ScreenSource) -- the similar-pair
// count last seen for these coordinates picks the hook's form as it picks the ladder's (-1: nothing seen yet), and this
// call's counts are noted for the next one.  May return with work in flight (the caller drains on error).
template <class Source>
int label_resident(fc_ensemble *ens, const Source &make, const Labelling &lab, DevBuf &work, const LabelOut &o,
                   int64_t *stats) {
  const int64_t N = ens->N;
  FC_TRY(make(/*lean=*/true));
  auto *cnt = reinterpret_cast<unsigned long long *>(ens->counters.p);
  ClusterGraph g;
  g.pairs_dev = ens->simq.as<uint64_t>(), g.n_pairs_dev = cnt + 2;
  g.n_cand_dev = cnt + 6, g.cand_cap = (unsigned long long)ens->pairq_cap, g.redo_dev = cnt + 12;
  g.known_short = Source::screened && ens->last_similar >= 0 && ens->last_similar < kClShortList;
  ClusterResult res;
  FC_TRY(label_run(lab, g, N, work, cnt, &res));
  int64_t from_bits = 0;
  if (res.status()[kClStatusList] == 0ull) {
    FC_TRY(make(/*lean=*/false));
    ClusterGraph gb;
    gb.bits_dev = ens->bits.as<uint64_t>(), gb.W = ens->W;
    FC_TRY(label_run(lab, gb, N, work, cnt, &res));
    from_bits = 1;
  }
  const unsigned long long *c = res.extra();
  if (Source::screened) note_candidates(ens, c[6], c[2]);
  label_unpack(res, N, o, stats && lab.n_stats() == 8 ? stats + 6 : nullptr);
  if (stats) fill_stats(stats, N * (N - 1) / 2, c, from_bits, *o.n_clusters);
  return FC_OK;
}

// the plain graph, or the enantiomer-aware one under EnantScope: lean first, as fc_prune_rmsd -- only the pair lists; the
// screen and the refine run again for the bit matrix
struct ScreenSource {
  static constexpr bool screened = true;
  fc_ensemble *ens;
  double max_rmsd, max_dev;
  const double *energies;
  double max_dE;
  int operator()(bool lean) const {
    if (lean) FC_TRY(ensemble_shard(ens, 0, 1, default_row_block()));
    return simbits_local(ens, max_rmsd, max_dev, energies, max_dE, true, lean);
  }
};

// what the resident entry points share between their own first checks and the device: two refusals and the outputs of
// an empty call
int label_args(double max_rmsd, double max_dev, const Labelling &lab, const LabelOut &o, int64_t *stats) {
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  if (lab.density) FC_REQUIRE(lab.min_samples >= 1, "min_samples=%lld must be >= 1", (long long)lab.min_samples);
  *o.n_clusters = 0;
  if (stats) std::memset(stats, 0, lab.n_stats() * sizeof(int64_t));
  return FC_OK;
}

// fc_rmsd_clusters, fc_rmsd_dbscan and fc_rmsd_butina behind the API lock
int rmsd_label(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
               const Labelling &lab, const LabelOut &o, int64_t *stats) {
  FC_REQUIRE(ens && o.n_clusters, "NULL pointer argument");
  FC_TRY(label_args(max_rmsd, max_dev, lab, o, stats));
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  FC_REQUIRE(o.complete(lab), "NULL pointer argument");
  FC_REQUIRE(ens->N <= (int64_t)INT32_MAX - 256, "N=%lld: clusters index conformers with 32 bits", (long long)ens->N);
  DevBuf work;
  return drained(label_resident(ens, ScreenSource{ens, max_rmsd, max_dev, energies, max_dE}, lab, work, o, stats));
}

// the symmetry-aware graph: one launch writes the queue AND the matrix, so a declined list costs nothing more
struct SymmSource {
  static constexpr bool screened = false;
  fc_ensemble *ens;
  const std::vector<uint16_t> &table;
  int64_t K;
  DevBuf &dperm;
  double max_rmsd, max_dev;
  const double *energies;
  double max_dE;
  int operator()(bool lean) const {
    return lean ? symm_local(ens, table, K, dperm, max_rmsd, max_dev, energies, max_dE) : FC_OK;
  }
};

// fc_rmsd_clusters_perm, fc_rmsd_dbscan_perm and fc_rmsd_butina_perm behind the API lock
int rmsd_label_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                    const double *energies, double max_dE, const Labelling &lab, const LabelOut &o, int64_t *stats) {
  std::vector<uint16_t> table;
  FC_TRY(perm_table_check(perms, K, A_sel, table));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, true));
  FC_REQUIRE(o.n_clusters != nullptr, "NULL pointer argument");
  FC_TRY(label_args(max_rmsd, max_dev, lab, o, stats));
  if (ens->N > (int64_t)INT32_MAX - 256)  // (FC_E_LIMIT, and judged in front of ensure_init: this form has always done so)
    return set_error(FC_E_LIMIT, "N=%lld: clusters index conformers with 32 bits", (long long)ens->N);
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  FC_REQUIRE(o.complete(lab), "NULL pointer argument");
  DevBuf dperm, work;
  return drained(label_resident(ens, SymmSource{ens, table, K, dperm, max_rmsd, max_dev, energies, max_dE}, lab, work, o, stats));
}

// ---- a caller's graph (fc_clusters_from_* / fc_dbscan_from_*) ------------------------------------------------------------
// one upload, the same labelling (the checks are label_from_pairs' / label_from_bits')
int label_uploaded(const uint64_t *pairs, int64_t n_pairs, const uint64_t *bits, int64_t N, const Labelling &lab,
                   const LabelOut &o) {
  FC_TRY(ensure_init());
  DevBuf graph, work;
  ClusterGraph g;
  ClusterResult res;
  int rc = FC_OK;
  if (bits != nullptr) {
    const int64_t W = ceil_div(N, 64);
    rc = upload(graph, bits, (size_t)N * (size_t)W);
    g.bits_dev = graph.as<uint64_t>(), g.W = W;
  } else {
    rc = upload(graph, pairs, (size_t)n_pairs);  // (n_pairs == 0: an 8-byte block that is never read)
    g.pairs_dev = graph.as<uint64_t>(), g.n_pairs_host = (unsigned long long)n_pairs;
    g.known_short = n_pairs < kClShortList;
  }
  if (rc == FC_OK) rc = label_run(lab, g, N, work, nullptr, &res);
  FC_TRY(drained(rc));
  label_unpack(res, N, o, nullptr);
  return FC_OK;
}

int label_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, const Labelling &lab, const LabelOut &o) {
  FC_REQUIRE(o.n_clusters != nullptr, "n_clusters is NULL");
  FC_REQUIRE(N >= 0 && n_pairs >= 0, "bad arguments N=%lld n_pairs=%lld", (long long)N, (long long)n_pairs);
  if (lab.density) FC_REQUIRE(lab.min_samples >= 1, "min_samples=%lld must be >= 1", (long long)lab.min_samples);
  FC_REQUIRE(N <= (int64_t)INT32_MAX - 256, "N=%lld: clusters index conformers with 32 bits", (long long)N);
  FC_REQUIRE(pairs != nullptr || n_pairs == 0, "pairs is NULL");
  for (int64_t p = 0; p < n_pairs; ++p) {
    const uint64_t i = pairs[p] >> 32, j = pairs[p] & 0xffffffffull;
    FC_REQUIRE(i != j && i < (uint64_t)N && j < (uint64_t)N, "pair %lld = (%llu, %llu): i == j or an index outside [0, %lld)",
               (long long)p, (unsigned long long)i, (unsigned long long)j, (long long)N);
  }
  *o.n_clusters = 0;
  if (N == 0) return FC_OK;
  FC_REQUIRE(o.complete(lab), "NULL pointer argument");
  return label_uploaded(pairs, n_pairs, nullptr, N, lab, o);
}

int label_from_bits(const uint64_t *bits, int64_t N, const Labelling &lab, const LabelOut &o) {
  FC_REQUIRE(o.n_clusters != nullptr, "n_clusters is NULL");
  FC_REQUIRE(N >= 0, "N=%lld < 0", (long long)N);
  if (lab.density) FC_REQUIRE(lab.min_samples >= 1, "min_samples=%lld must be >= 1", (long long)lab.min_samples);
  FC_REQUIRE(N <= (int64_t)INT32_MAX - 256, "N=%lld: clusters index conformers with 32 bits", (long long)N);
  *o.n_clusters = 0;
  if (N == 0) return FC_OK;
  FC_REQUIRE(bits != nullptr && o.complete(lab), "NULL pointer argument");
  return label_uploaded(nullptr, 0, bits, N, lab, o);
}
}  // namespace

extern "C" {

int fc_rmsd_clusters(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                     int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  return rmsd_label(ens, max_rmsd, max_dev, energies, max_dE, components(),
                    {labels_out, reps_out, sizes_out, nullptr, nullptr, n_clusters}, stats);
}

int fc_rmsd_clusters_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                           int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int64_t *n_clusters,
                           int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && n_clusters, "NULL pointer argument");
  EnantScope scope(ens);
  return fc_rmsd_clusters(ens, max_rmsd, max_dev, energies, max_dE, labels_out, reps_out, sizes_out, n_clusters, stats);
}

int fc_rmsd_clusters_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd,
                          double max_dev, const double *energies, double max_dE, int32_t *labels_out, int64_t *reps_out,
                          int64_t *sizes_out, int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  return rmsd_label_perm(ens, perms, K, A_sel, max_rmsd, max_dev, energies, max_dE, components(),
                         {labels_out, reps_out, sizes_out, nullptr, nullptr, n_clusters}, stats);
}

int fc_clusters_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int32_t *labels_out, int64_t *reps_out,
                           int64_t *sizes_out, int64_t *n_clusters) {
  FC_API_LOCK;
  return label_from_pairs(pairs, n_pairs, N, components(), {labels_out, reps_out, sizes_out, nullptr, nullptr, n_clusters});
}

int fc_clusters_from_bits(const uint64_t *bits, int64_t N, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out,
                          int64_t *n_clusters) {
  FC_API_LOCK;
  return label_from_bits(bits, N, components(), {labels_out, reps_out, sizes_out, nullptr, nullptr, n_clusters});
}

// ---- density-based clusters (the contract: include/fc_hip.h; the kernels: fc_clusters.hip, k_db_*) ---------------------
int fc_rmsd_dbscan(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_samples, const double *energies,
                   double max_dE, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, uint8_t *core_out,
                   int32_t *degrees_out, int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  return rmsd_label(ens, max_rmsd, max_dev, energies, max_dE, density_based(min_samples),
                    {labels_out, reps_out, sizes_out, core_out, degrees_out, n_clusters}, stats);
}

int fc_rmsd_dbscan_enant(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_samples, const double *energies,
                         double max_dE, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, uint8_t *core_out,
                         int32_t *degrees_out, int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && n_clusters, "NULL pointer argument");
  EnantScope scope(ens);
  return fc_rmsd_dbscan(ens, max_rmsd, max_dev, min_samples, energies, max_dE, labels_out, reps_out, sizes_out, core_out,
                        degrees_out, n_clusters, stats);
}

int fc_rmsd_dbscan_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                        int64_t min_samples, const double *energies, double max_dE, int32_t *labels_out, int64_t *reps_out,
                        int64_t *sizes_out, uint8_t *core_out, int32_t *degrees_out, int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  return rmsd_label_perm(ens, perms, K, A_sel, max_rmsd, max_dev, energies, max_dE, density_based(min_samples),
                         {labels_out, reps_out, sizes_out, core_out, degrees_out, n_clusters}, stats);
}

int fc_dbscan_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int64_t min_samples, int32_t *labels_out,
                         int64_t *reps_out, int64_t *sizes_out, uint8_t *core_out, int32_t *degrees_out,
                         int64_t *n_clusters) {
  FC_API_LOCK;
  return label_from_pairs(pairs, n_pairs, N, density_based(min_samples),
                          {labels_out, reps_out, sizes_out, core_out, degrees_out, n_clusters});
}

int fc_dbscan_from_bits(const uint64_t *bits, int64_t N, int64_t min_samples, int32_t *labels_out, int64_t *reps_out,
                        int64_t *sizes_out, uint8_t *core_out, int32_t *degrees_out, int64_t *n_clusters) {
  FC_API_LOCK;
  return label_from_bits(bits, N, density_based(min_samples), {labels_out, reps_out, sizes_out, core_out, degrees_out, n_clusters});
}

// ---- sphere-exclusion clusters (the contract: include/fc_hip.h; the kernels: fc_clusters.hip, k_bu_*) ------------------
int fc_rmsd_butina(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                   int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int32_t *degrees_out, int64_t *n_clusters,
                   int64_t *stats) {
  FC_API_LOCK;
  return rmsd_label(ens, max_rmsd, max_dev, energies, max_dE, sphere_exclusion(),
                    {labels_out, reps_out, sizes_out, nullptr, degrees_out, n_clusters}, stats);
}

int fc_rmsd_butina_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                         int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out, int32_t *degrees_out,
                         int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && n_clusters, "NULL pointer argument");
  EnantScope scope(ens);
  return fc_rmsd_butina(ens, max_rmsd, max_dev, energies, max_dE, labels_out, reps_out, sizes_out, degrees_out, n_clusters,
                        stats);
}

int fc_rmsd_butina_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                        const double *energies, double max_dE, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out,
                        int32_t *degrees_out, int64_t *n_clusters, int64_t *stats) {
  FC_API_LOCK;
  return rmsd_label_perm(ens, perms, K, A_sel, max_rmsd, max_dev, energies, max_dE, sphere_exclusion(),
                         {labels_out, reps_out, sizes_out, nullptr, degrees_out, n_clusters}, stats);
}

int fc_butina_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int32_t *labels_out, int64_t *reps_out,
                         int64_t *sizes_out, int32_t *degrees_out, int64_t *n_clusters) {
  FC_API_LOCK;
  return label_from_pairs(pairs, n_pairs, N, sphere_exclusion(), {labels_out, reps_out, sizes_out, nullptr, degrees_out, n_clusters});
}

int fc_butina_from_bits(const uint64_t *bits, int64_t N, int32_t *labels_out, int64_t *reps_out, int64_t *sizes_out,
                        int32_t *degrees_out, int64_t *n_clusters) {
  FC_API_LOCK;
  return label_from_bits(bits, N, sphere_exclusion(), {labels_out, reps_out, sizes_out, nullptr, degrees_out, n_clusters});
}

}  // extern "C"
