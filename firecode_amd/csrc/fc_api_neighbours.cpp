// fc_api_neighbours.cpp -- the extern "C" surface (include/fc_hip.h) of what is read off the exact RMSD of a resident
// ensemble without a threshold graph: the RMSD-diverse selection (greedy max-min; fc_diverse.hip) and the k nearest
// neighbours, within one ensemble or across two (fc_knn.hip), each also under d_sym, and their bench hooks.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "fc_internal.h"

namespace fc {

// (SymArgs, sym_args_check and with_sym_table -- the checked table of the forms under d_sym -- are in fc_internal.h)

// `reps` calls of call(&ms_device) -> the means of the device time they report and of the host time around them
template <class Call>
static int timed_reps(int64_t reps, double *ms_device_mean, double *ms_host_mean, const Call &call) {
  FC_REQUIRE(reps >= 1 && reps <= 4096 && ms_device_mean && ms_host_mean, "bad arguments");
  double dev = 0.0, host = 0.0;
  for (int64_t r = 0; r < reps; ++r) {
    double ms = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    FC_TRY(call(&ms));
    host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    dev += ms;
  }
  *ms_device_mean = dev / (double)reps;
  *ms_host_mean = host / (double)reps;
  return FC_OK;
}

// ---- RMSD-diverse selection (greedy max-min; the contract: include/fc_hip.h, fc_diverse.hip) ----------------------
static int select_diverse_checked(fc_ensemble *ens, int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out,
                                  double *radii_out, int32_t *labels_out, double *dist_out, int64_t *n_selected,
                                  double *ms_device, const SymArgs *sym_args = nullptr) {
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(indices_out != nullptr && n_selected != nullptr, "indices_out / n_selected is NULL");
  FC_REQUIRE(n_max >= 1, "n_max=%lld < 1", (long long)n_max);
  FC_REQUIRE(!(stop_rmsd != stop_rmsd), "stop_rmsd is NaN");
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  *n_selected = 0;
  if (ens->N == 0) return FC_OK;
  FC_REQUIRE(start >= 0 && start < ens->N, "start=%lld outside [0, %lld)", (long long)start, (long long)ens->N);
  FC_REQUIRE(ens->N <= (int64_t)INT32_MAX - 256, "N=%lld: the selection indexes conformers with 32 bits", (long long)ens->N);
  FC_TRY(ensure_init());
  return with_sym_table(sym_args, [&](const SymTable *sym) {
    return select_diverse(ens, n_max, start, stop_rmsd, indices_out, radii_out, labels_out, dist_out, n_selected, ms_device,
                          sym);
  });
}

// the selection under d_sym (the kernel: k_diverse_step_sym); stats (may be NULL): the two counters after the selection
static int select_diverse_perm_checked(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                       int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out, double *radii_out,
                                       int32_t *labels_out, double *dist_out, int64_t *n_selected, double *ms_device,
                                       int64_t *stats) {
  SymArgs a;
  FC_TRY(sym_args_check(perms, K, A_sel, mirror, diverse_sym_lds_bytes, a));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, false));
  if (stats) stats[0] = stats[1] = 0;
  a.stats = stats;
  const bool plain = K == 1 && !mirror;  // d_sym = d: the default's kernels, bit for bit
  return select_diverse_checked(ens, n_max, start, stop_rmsd, indices_out, radii_out, labels_out, dist_out, n_selected,
                                ms_device, plain ? nullptr : &a);
}

// ---- k nearest neighbours under the RMSD (the contract: include/fc_hip.h; the kernels: fc_knn.hip) ------------------
static int knn_k_check(int64_t k) {
  FC_REQUIRE(k >= 1, "k=%lld < 1", (long long)k);
  if (k > FC_KNN_MAX) return set_error(FC_E_LIMIT, "k=%lld neighbours: at most FC_KNN_MAX = %d", (long long)k, FC_KNN_MAX);
  return FC_OK;
}

static int knn_run(fc_ensemble *q, fc_ensemble *r, bool cross, int64_t k, double max_rmsd, int32_t *indices_out,
                   double *dist_out, double *ms_device, int64_t *strips_out, const SymArgs *sym_args) {
  return with_sym_table(sym_args, [&](const SymTable *sym) {
    return knn(q, r, cross, k, max_rmsd, indices_out, dist_out, ms_device, strips_out, sym);
  });
}

static int knn_checked(fc_ensemble *ens, int64_t k, int32_t *indices_out, double *dist_out, double *ms_device,
                       int64_t *strips_out, const SymArgs *sym_args = nullptr) {
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(indices_out != nullptr && dist_out != nullptr, "indices_out / dist_out is NULL");
  FC_TRY(knn_k_check(k));
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  if (strips_out) *strips_out = 0;
  if (ms_device) *ms_device = 0.0;
  if (ens->N == 0) return FC_OK;
  FC_REQUIRE(ens->N <= (int64_t)INT32_MAX - 256, "N=%lld: the lists index conformers with 32 bits", (long long)ens->N);
  FC_TRY(ensure_init());
  return knn_run(ens, ens, false, k, INFINITY, indices_out, dist_out, ms_device, strips_out, sym_args);
}

// the rows of `queries` against the columns of `refs` (the contract: include/fc_hip.h, fc_ensemble_knn_cross); the
// scalar arguments are judged first, so that their refusals do not depend on the handles
static int knn_cross_checked(fc_ensemble *queries, fc_ensemble *refs, int64_t k, double max_rmsd, int32_t *indices_out,
                             double *dist_out, double *ms_device, int64_t *strips_out, const SymArgs *sym_args = nullptr) {
  FC_TRY(knn_k_check(k));
  FC_REQUIRE(max_rmsd > 0.0, "max_rmsd=%g must be positive (+inf: no cap)", max_rmsd);  // (a NaN fails it)
  FC_REQUIRE(queries != nullptr && refs != nullptr, "queries / refs is NULL");
  FC_REQUIRE(indices_out != nullptr && dist_out != nullptr, "indices_out / dist_out is NULL");
  FC_REQUIRE(queries->epoch == ctx().epoch && refs->epoch == ctx().epoch,
             "an ensemble was created before fc_shutdown / a device switch: create it again");
  FC_REQUIRE(queries->A == refs->A, "queries select %lld atoms, refs %lld: one atom selection for both", (long long)queries->A,
             (long long)refs->A);
  if (refs->N > (int64_t)INT32_MAX - 256 || queries->N > (int64_t)INT32_MAX - 256)
    return set_error(FC_E_LIMIT, "Nq=%lld, Nr=%lld: the lists index conformers with 32 bits", (long long)queries->N,
                     (long long)refs->N);
  if (strips_out) *strips_out = 0;
  if (ms_device) *ms_device = 0.0;
  if (queries->N == 0) return FC_OK;
  if (refs->N == 0) {  // no reference: every slot is empty, and no device is needed to say so
    std::fill(indices_out, indices_out + queries->N * k, (int32_t)-1);
    std::fill(dist_out, dist_out + queries->N * k, (double)INFINITY);
    return FC_OK;
  }
  FC_TRY(ensure_init());
  return knn_run(queries, refs, true, k, max_rmsd, indices_out, dist_out, ms_device, strips_out, sym_args);
}

// under d_sym (the kernel: k_knn_tile_sym); stats (may be NULL): the two counters after the call
static int knn_perm_checked(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, int64_t k,
                            int32_t *indices_out, double *dist_out, double *ms_device, int64_t *strips_out, int64_t *stats) {
  SymArgs a;
  FC_TRY(sym_args_check(perms, K, A_sel, mirror, knn_sym_lds_bytes, a));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, false));
  if (stats) stats[0] = stats[1] = 0;
  a.stats = stats;
  const bool plain = K == 1 && !mirror;  // d_sym = d: the default's kernels, bit for bit
  return knn_checked(ens, k, indices_out, dist_out, ms_device, strips_out, plain ? nullptr : &a);
}

static int knn_cross_perm_checked(fc_ensemble *queries, fc_ensemble *refs, const int32_t *perms, int64_t K, int64_t A_sel,
                                  int mirror, int64_t k, double max_rmsd, int32_t *indices_out, double *dist_out,
                                  double *ms_device, int64_t *strips_out, int64_t *stats) {
  SymArgs a;
  FC_TRY(sym_args_check(perms, K, A_sel, mirror, knn_sym_lds_bytes, a));
  FC_REQUIRE(queries != nullptr && refs != nullptr, "queries / refs is NULL");
  FC_TRY(perm_ensemble_check(queries, K, A_sel, false));
  FC_TRY(perm_ensemble_check(refs, K, A_sel, false));
  if (stats) stats[0] = stats[1] = 0;
  a.stats = stats;
  const bool plain = K == 1 && !mirror;
  return knn_cross_checked(queries, refs, k, max_rmsd, indices_out, dist_out, ms_device, strips_out, plain ? nullptr : &a);
}

// The lists of a bench hook, which no caller reads: k entries per row of `rows` (and one more: the pointers are never
// NULL).  Sized in front of the checks, which the hooks leave to the entry point they time -- so without the arguments
// that it is going to refuse.
struct KnnScratch {
  std::vector<int32_t> idx;
  std::vector<double> dist;
  KnnScratch(const fc_ensemble *rows, int64_t k) : idx(entries(rows, k)), dist(entries(rows, k)) {}
  static size_t entries(const fc_ensemble *rows, int64_t k) {
    return rows != nullptr && k >= 1 && k <= FC_KNN_MAX ? (size_t)rows->N * (size_t)k + 1 : 1;
  }
};

}  // namespace fc

using namespace fc;

extern "C" {

int fc_ensemble_select_diverse(fc_ensemble *ens, int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out,
                               double *radii_out, int32_t *labels_out, double *dist_out, int64_t *n_selected) {
  FC_API_LOCK;
  return select_diverse_checked(ens, n_max, start, stop_rmsd, indices_out, radii_out, labels_out, dist_out, n_selected,
                                nullptr);
}

int fc_bench_select_diverse(fc_ensemble *ens, int64_t n_max, int64_t start, double stop_rmsd, int64_t reps,
                            double *ms_device_mean, double *ms_host_mean, int64_t *indices_out, int64_t *n_selected,
                            int64_t *lanes_out) {
  FC_API_LOCK;
  FC_TRY(timed_reps(reps, ms_device_mean, ms_host_mean, [&](double *ms) {
    return select_diverse_checked(ens, n_max, start, stop_rmsd, indices_out, nullptr, nullptr, nullptr, n_selected, ms);
  }));
  if (lanes_out) *lanes_out = diverse_lanes(ens->N);
  return FC_OK;
}

int fc_ensemble_select_diverse_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                    int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out,
                                    double *radii_out, int32_t *labels_out, double *dist_out, int64_t *n_selected) {
  FC_API_LOCK;
  return select_diverse_perm_checked(ens, perms, K, A_sel, mirror, n_max, start, stop_rmsd, indices_out, radii_out,
                                     labels_out, dist_out, n_selected, nullptr, nullptr);
}

// (all three hooks under d_sym: the timed calls run without the counters, which are counted in a call of its own)
int fc_bench_select_diverse_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                 int64_t n_max, int64_t start, double stop_rmsd, int64_t reps, double *ms_device_mean,
                                 double *ms_host_mean, int64_t *indices_out, int64_t *n_selected, int64_t *stats) {
  FC_API_LOCK;
  const auto call = [&](double *ms, int64_t *counted) {
    return select_diverse_perm_checked(ens, perms, K, A_sel, mirror, n_max, start, stop_rmsd, indices_out, nullptr, nullptr,
                                       nullptr, n_selected, ms, counted);
  };
  FC_TRY(timed_reps(reps, ms_device_mean, ms_host_mean, [&](double *ms) { return call(ms, nullptr); }));
  return stats ? call(nullptr, stats) : FC_OK;
}

int fc_ensemble_knn(fc_ensemble *ens, int64_t k, int32_t *indices_out, double *dist_out) {
  FC_API_LOCK;
  return knn_checked(ens, k, indices_out, dist_out, nullptr, nullptr);
}

int fc_bench_knn(fc_ensemble *ens, int64_t k, int64_t reps, double *ms_device_mean, double *ms_host_mean,
                 int64_t *strips_out) {
  FC_API_LOCK;
  KnnScratch out(ens, k);
  return timed_reps(reps, ms_device_mean, ms_host_mean, [&](double *ms) {
    return knn_checked(ens, k, out.idx.data(), out.dist.data(), ms, strips_out);
  });
}

int fc_ensemble_knn_cross(fc_ensemble *queries, fc_ensemble *refs, int64_t k, double max_rmsd, int32_t *indices_out,
                          double *dist_out) {
  FC_API_LOCK;
  return knn_cross_checked(queries, refs, k, max_rmsd, indices_out, dist_out, nullptr, nullptr);
}

int fc_bench_knn_cross(fc_ensemble *queries, fc_ensemble *refs, int64_t k, double max_rmsd, int64_t reps,
                       double *ms_device_mean, double *ms_host_mean, int64_t *strips_out) {
  FC_API_LOCK;
  KnnScratch out(queries, k);
  return timed_reps(reps, ms_device_mean, ms_host_mean, [&](double *ms) {
    // (this hook has always judged the handles in front of max_rmsd, the entry point behind it)
    FC_TRY(knn_k_check(k));
    FC_REQUIRE(queries != nullptr && refs != nullptr, "queries / refs is NULL");
    return knn_cross_checked(queries, refs, k, max_rmsd, out.idx.data(), out.dist.data(), ms, strips_out);
  });
}

int fc_ensemble_knn_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, int64_t k,
                         int32_t *indices_out, double *dist_out) {
  FC_API_LOCK;
  return knn_perm_checked(ens, perms, K, A_sel, mirror, k, indices_out, dist_out, nullptr, nullptr, nullptr);
}

int fc_ensemble_knn_cross_perm(fc_ensemble *queries, fc_ensemble *refs, const int32_t *perms, int64_t K, int64_t A_sel,
                               int mirror, int64_t k, double max_rmsd, int32_t *indices_out, double *dist_out) {
  FC_API_LOCK;
  return knn_cross_perm_checked(queries, refs, perms, K, A_sel, mirror, k, max_rmsd, indices_out, dist_out, nullptr, nullptr,
                                nullptr);
}

int fc_bench_knn_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, int64_t k, int64_t reps,
                      double *ms_device_mean, double *ms_host_mean, int64_t *strips_out, int64_t *stats) {
  FC_API_LOCK;
  KnnScratch out(ens, k);
  const auto call = [&](double *ms, int64_t *strips, int64_t *counted) {
    return knn_perm_checked(ens, perms, K, A_sel, mirror, k, out.idx.data(), out.dist.data(), ms, strips, counted);
  };
  FC_TRY(timed_reps(reps, ms_device_mean, ms_host_mean, [&](double *ms) { return call(ms, strips_out, nullptr); }));
  return stats ? call(nullptr, nullptr, stats) : FC_OK;
}

int fc_bench_knn_cross_perm(fc_ensemble *queries, fc_ensemble *refs, const int32_t *perms, int64_t K, int64_t A_sel,
                            int mirror, int64_t k, double max_rmsd, int64_t reps, double *ms_device_mean,
                            double *ms_host_mean, int64_t *strips_out, int64_t *stats) {
  FC_API_LOCK;
  KnnScratch out(queries, k);
  const auto call = [&](double *ms, int64_t *strips, int64_t *counted) {
    return knn_cross_perm_checked(queries, refs, perms, K, A_sel, mirror, k, max_rmsd, out.idx.data(), out.dist.data(), ms,
                                  strips, counted);
  };
  FC_TRY(timed_reps(reps, ms_device_mean, ms_host_mean, [&](double *ms) { return call(ms, strips_out, nullptr); }));
  return stats ? call(nullptr, nullptr, stats) : FC_OK;
}

}  // extern "C"
