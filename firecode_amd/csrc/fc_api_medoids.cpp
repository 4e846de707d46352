// fc_api_medoids.cpp -- the extern "C" surface (include/fc_hip.h) of "which conformer stands for this group": the medoids
// of given groups under the ensemble's RMSD, the k-medoids selection (the alternating form: assign, move to the medoid)
// and the subset of a resident ensemble that both are built on; and of "how good is this grouping": the silhouettes.
// The kernels: fc_medoid.hip, fc_silhouette.hip; the assignment step is the cross k-NN with k = 1 (fc_knn.hip), the
// default start the diverse selection (fc_diverse.hip).
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>

#include "fc_internal.h"

namespace fc {

// (Grouping: fc_internal.h)  labels (N, or nullptr: everything in group 0), already checked: label < n_groups, negative =
// in no group
void group_by_label(const int32_t *labels, int64_t N, int64_t n_groups, Grouping &g) {
  g.offs.assign((size_t)n_groups + 1, 0);
  if (labels == nullptr) {
    g.offs[1] = N;
  } else {
    for (int64_t i = 0; i < N; ++i)
      if (labels[i] >= 0) ++g.offs[(size_t)labels[i] + 1];
  }
  g.largest = 0;
  for (int64_t c = 0; c < n_groups; ++c) {
    g.largest = std::max(g.largest, g.offs[(size_t)c + 1]);
    g.offs[(size_t)c + 1] += g.offs[(size_t)c];
  }
  g.order.resize((size_t)g.offs[(size_t)n_groups]);
  std::vector<int64_t> at(g.offs.begin(), g.offs.end() - 1);
  for (int64_t i = 0; i < N; ++i) {
    const int64_t c = labels == nullptr ? 0 : labels[i];
    if (c >= 0) g.order[(size_t)at[(size_t)c]++] = (int32_t)i;
  }
}

// a group too large for the 64-bit sum of q(d): d <= sqrt(4 g_max / A), whatever the rotation
static int sum_limit_check(fc_ensemble *ens, int64_t largest) {
  FC_TRY(ensemble_build_finish(ens));
  const double g = ens->g_max;
  if (!(g >= 0.0) || !std::isfinite(g)) return FC_OK;  // (no finite bound to judge by: NaN coordinates give NaN distances)
  const double d_max = std::ceil(std::sqrt(4.0 * g / (double)ens->A)) + 1.0;
  if ((double)largest * d_max >= 2147483648.0)
    return set_error(FC_E_LIMIT, "a group of %lld conformers with distances up to %.3g: the sum of q(d) does not fit 64 bits",
                     (long long)largest, d_max);
  return FC_OK;
}

// S and E of the contract, by conformer (N each; 0 for singletons and unlabelled conformers).  ms_kernel may be NULL;
// sym (may be NULL): under d_sym.
static int group_sums(fc_ensemble *ens, const Grouping &g, std::vector<uint64_t> &S, std::vector<double> &E, double *ms_kernel,
                      const SymTable *sym = nullptr) {
  const int64_t N = ens->N, M = (int64_t)g.order.size();
  S.assign((size_t)N, 0);
  E.assign((size_t)N, 0.0);
  if (ms_kernel) *ms_kernel = 0.0;
  if (g.largest < 2) return FC_OK;  // no pair: no device
  std::vector<int32_t> seg_end((size_t)M);
  for (size_t c = 0; c + 1 < g.offs.size(); ++c)
    for (int64_t p = g.offs[c]; p < g.offs[c + 1]; ++p) seg_end[(size_t)p] = (int32_t)g.offs[c + 1];
  bool identity = M == N;
  for (int64_t p = 0; identity && p < M; ++p) identity = g.order[(size_t)p] == p;
  fc_ensemble sorted;  // the label-sorted copy (not made when the ensemble is in that order already)
  DevBuf d_order, d_end, d_out;
  std::vector<uint64_t> out((size_t)M * 2);
  const auto run = [&]() {
    FC_TRY(upload(d_end, seg_end.data(), (size_t)M));
    const fc_ensemble *e = ens;
    if (!identity) {
      FC_TRY(upload(d_order, g.order.data(), (size_t)M));
      FC_TRY(ensemble_gather(ens, d_order.as<int32_t>(), M, &sorted, false));
      e = &sorted;
    }
    FC_TRY(d_out.reserve((size_t)M * 2 * sizeof(uint64_t)));
    FC_TRY(launch_group_sums(e, d_end.as<int32_t>(), d_out.as<unsigned long long>(), ms_kernel != nullptr, sym));  // S | E
    FC_TRY(d2h(out.data(), d_out.p, (size_t)M * 2 * sizeof(uint64_t)));
    FC_TRY(sync());
    if (ms_kernel) {
      float ms = 0.0f;
      FC_HIP_TRY(hipEventElapsedTime(&ms, ctx().ev0, ctx().ev1));
      *ms_kernel = ms;
    }
    return FC_OK;
  };
  FC_TRY(drained(run()));
  for (int64_t p = 0; p < M; ++p) {
    const size_t i = (size_t)g.order[(size_t)p];
    S[i] = out[(size_t)p];
    std::memcpy(&E[i], &out[(size_t)(M + p)], sizeof(double));
  }
  return FC_OK;
}

// per group: the member with the smallest S, the lowest index on ties (the members come in ascending index)
static void medoids_of(const Grouping &g, const std::vector<uint64_t> &S, const std::vector<double> &E, int64_t *medoids_out,
                       int64_t *sizes_out, double *mean_out, double *radius_out) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t c = 0; c + 1 < g.offs.size(); ++c) {
    const int64_t size = g.offs[c + 1] - g.offs[c];
    int64_t best = -1;
    for (int64_t p = g.offs[c]; p < g.offs[c + 1]; ++p) {
      const int64_t i = g.order[(size_t)p];
      if (best < 0 || S[(size_t)i] < S[(size_t)best]) best = i;
    }
    medoids_out[c] = best;
    if (sizes_out) sizes_out[c] = size;
    if (mean_out) mean_out[c] = size == 0 ? nan : size == 1 ? 0.0 : std::ldexp((double)S[(size_t)best], -32) / (double)(size - 1);
    if (radius_out) radius_out[c] = size == 0 ? nan : E[(size_t)best];
  }
}

int labels_check(const int32_t *labels, int64_t N, int64_t n_groups) {
  if (labels == nullptr) return FC_OK;
  for (int64_t i = 0; i < N; ++i)
    FC_REQUIRE(labels[i] < n_groups, "labels[%lld]=%d is not below n_groups=%lld", (long long)i, (int)labels[i], (long long)n_groups);
  return FC_OK;
}

// sym_args (may be NULL): under d_sym, already checked -- the table goes up only where the device is used
static int medoids_checked(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, int64_t *medoids_out, int64_t *sizes_out,
                           double *mean_out, double *radius_out, uint64_t *sums_q32_out, double *ecc_out, double *ms_kernel,
                           const SymArgs *sym_args = nullptr) {
  // (the scalar arguments are judged first, so that their refusals do not depend on the handle)
  FC_REQUIRE(n_groups >= 1, "n_groups=%lld < 1", (long long)n_groups);
  FC_REQUIRE(n_groups <= (int64_t)INT32_MAX, "n_groups=%lld: labels are 32-bit", (long long)n_groups);
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(medoids_out != nullptr && sizes_out != nullptr && mean_out != nullptr && radius_out != nullptr,
             "medoids_out / sizes_out / mean_out / radius_out is NULL");
  FC_TRY(labels_check(labels, ens->N, n_groups));
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  if (ms_kernel) *ms_kernel = 0.0;
  const int64_t N = ens->N;
  if (N > (int64_t)INT32_MAX - 256)
    return set_error(FC_E_LIMIT, "N=%lld: the sums index conformers with 32 bits", (long long)N);
  Grouping g;
  group_by_label(labels, N, n_groups, g);
  std::vector<uint64_t> S;
  std::vector<double> E;
  const auto sums = [&](const SymTable *sym) { return group_sums(ens, g, S, E, ms_kernel, sym); };
  if (g.largest >= 2) {
    FC_TRY(ensure_init());
    FC_TRY(sum_limit_check(ens, g.largest));
    FC_TRY(with_sym_table(sym_args, sums));
  } else {
    FC_TRY(sums(nullptr));  // (no pair: no device)
  }
  medoids_of(g, S, E, medoids_out, sizes_out, mean_out, radius_out);
  if (sums_q32_out) std::copy(S.begin(), S.end(), sums_q32_out);
  if (ecc_out) std::copy(E.begin(), E.end(), ecc_out);
  return FC_OK;
}

// a, b and nearest of the silhouette's contract for the labelled conformers, by conformer; the unlabelled ones and --
// b, nearest -- everything the device was not needed for keep what the caller put there.  M >= 2 labelled conformers.
// sym (may be NULL): under d_sym.
static int silhouette_device(fc_ensemble *ens, const Grouping &g, const int32_t *labels, double *a_out, double *b_out,
                             int32_t *nearest_out, double *ms_kernel, const SymTable *sym = nullptr) {
  const int64_t N = ens->N, M = (int64_t)g.order.size();
  std::vector<int32_t> seg((size_t)M * 2);  // seg_begin | seg_end
  for (size_t c = 0; c + 1 < g.offs.size(); ++c)
    for (int64_t p = g.offs[c]; p < g.offs[c + 1]; ++p)
      seg[(size_t)p] = (int32_t)g.offs[c], seg[(size_t)(M + p)] = (int32_t)g.offs[c + 1];
  bool identity = M == N;
  for (int64_t p = 0; identity && p < M; ++p) identity = g.order[(size_t)p] == p;
  fc_ensemble sorted;  // the label-sorted copy (not made when the ensemble is in that order already)
  DevBuf d_order, d_seg, d_work;
  const int S = silhouette_strips(M);
  const size_t n_res = silhouette_result_bytes(M);
  std::vector<uint64_t> res((n_res + 7) / 8);  // a | b | nearest
  const auto run = [&]() {
    FC_TRY(upload(d_seg, seg.data(), (size_t)M * 2));
    const fc_ensemble *e = ens;
    if (!identity) {
      FC_TRY(upload(d_order, g.order.data(), (size_t)M));
      FC_TRY(ensemble_gather(ens, d_order.as<int32_t>(), M, &sorted, false));
      e = &sorted;
    }
    FC_TRY(d_work.reserve(silhouette_work_bytes(M, S)));
    FC_TRY(launch_silhouette(e, d_seg.as<int32_t>(), d_seg.as<int32_t>() + M, S, d_work.as<uint8_t>(), ms_kernel != nullptr,
                             sym));
    FC_TRY(d2h(res.data(), d_work.p, n_res));
    FC_TRY(sync());
    if (ms_kernel) {
      float ms = 0.0f;
      FC_HIP_TRY(hipEventElapsedTime(&ms, ctx().ev0, ctx().ev1));
      *ms_kernel = ms;
    }
    return FC_OK;
  };
  FC_TRY(drained(run()));
  const double *a = reinterpret_cast<const double *>(res.data()), *b = a + M;
  const int32_t *near = reinterpret_cast<const int32_t *>(b + M);
  for (int64_t p = 0; p < M; ++p) {
    const size_t i = (size_t)g.order[(size_t)p];
    a_out[i] = a[p];
    b_out[i] = b[p];
    // a group is named by its first position in the sorted copy: back to its label
    nearest_out[i] = near[p] < 0 ? -1 : labels == nullptr ? 0 : labels[(size_t)g.order[(size_t)near[p]]];
  }
  return FC_OK;
}

static int silhouette_checked(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, double *s_out, double *a_out,
                              double *b_out, int32_t *nearest_out, double *cluster_mean_out, int64_t *sizes_out, double *score_out,
                              double *ms_kernel, const SymArgs *sym_args = nullptr) {
  // (the scalar arguments are judged first, so that their refusals do not depend on the handle)
  FC_REQUIRE(n_groups >= 1, "n_groups=%lld < 1", (long long)n_groups);
  FC_REQUIRE(n_groups <= (int64_t)INT32_MAX, "n_groups=%lld: labels are 32-bit", (long long)n_groups);
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(s_out != nullptr && a_out != nullptr && b_out != nullptr && nearest_out != nullptr && cluster_mean_out != nullptr &&
                 sizes_out != nullptr && score_out != nullptr,
             "s_out / a_out / b_out / nearest_out / cluster_mean_out / sizes_out / score_out is NULL");
  FC_TRY(labels_check(labels, ens->N, n_groups));
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  if (ms_kernel) *ms_kernel = 0.0;
  const int64_t N = ens->N;
  if (N > (int64_t)INT32_MAX - 256)
    return set_error(FC_E_LIMIT, "N=%lld: the sums index conformers with 32 bits", (long long)N);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  Grouping g;
  group_by_label(labels, N, n_groups, g);
  const int64_t M = (int64_t)g.order.size();
  int64_t n_nonempty = 0;
  for (int64_t c = 0; c < n_groups; ++c) n_nonempty += g.offs[(size_t)c + 1] > g.offs[(size_t)c];
  for (int64_t i = 0; i < N; ++i) {
    const bool in = labels == nullptr || labels[i] >= 0;
    s_out[i] = b_out[i] = nan;
    a_out[i] = in ? 0.0 : nan;  // (a single labelled conformer: a singleton)
    nearest_out[i] = -1;
  }
  if (M >= 2) {  // a pair: the device
    FC_TRY(ensure_init());
    FC_TRY(sum_limit_check(ens, M));  // (a prefix runs over a whole row)
    FC_TRY(with_sym_table(sym_args, [&](const SymTable *sym) {
      return silhouette_device(ens, g, labels, a_out, b_out, nearest_out, ms_kernel, sym);
    }));
  }
  std::vector<double> sum((size_t)n_groups, 0.0);
  double total = 0.0;
  for (int64_t i = 0; i < N; ++i) {  // (ascending conformer index: the order of the sums of the contract)
    const int64_t c = labels == nullptr ? 0 : labels[i];
    if (c < 0) continue;
    double s;
    if (n_nonempty < 2) {
      s = b_out[i] = nan, nearest_out[i] = -1;
    } else {
      const double a = a_out[i], b = b_out[i], top = a > b ? a : b;
      s = g.offs[(size_t)c + 1] - g.offs[(size_t)c] == 1 || top == 0.0 ? 0.0 : (b - a) / top;
    }
    s_out[i] = s;
    sum[(size_t)c] += s;
    total += s;
  }
  for (int64_t c = 0; c < n_groups; ++c) {
    const int64_t size = g.offs[(size_t)c + 1] - g.offs[(size_t)c];
    sizes_out[c] = size;
    cluster_mean_out[c] = size == 0 ? nan : sum[(size_t)c] / (double)size;
  }
  *score_out = M == 0 ? nan : total / (double)M;
  return FC_OK;
}

static int indices_check(const char *what, const int64_t *idx, int64_t n, int64_t N, bool distinct) {
  std::vector<uint8_t> seen(distinct ? (size_t)N : 0, 0);
  for (int64_t c = 0; c < n; ++c) {
    FC_REQUIRE(idx[c] >= 0 && idx[c] < N, "%s[%lld]=%lld outside [0, %lld)", what, (long long)c, (long long)idx[c], (long long)N);
    if (distinct) {
      FC_REQUIRE(!seen[(size_t)idx[c]], "%s[%lld]=%lld is repeated", what, (long long)c, (long long)idx[c]);
      seen[(size_t)idx[c]] = 1;
    }
  }
  return FC_OK;
}

// the conformers `indices` of ens as a new ensemble (the caller owns it)
static int subset_checked(fc_ensemble *ens, const int64_t *indices, int64_t n, fc_ensemble **out) {
  FC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  FC_REQUIRE(n >= 0, "n=%lld < 0", (long long)n);
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(indices != nullptr || n == 0, "indices is NULL");
  FC_TRY(indices_check("indices", indices, n, ens->N, false));
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  if (n > (int64_t)INT32_MAX - 256) return set_error(FC_E_LIMIT, "n=%lld: conformers are indexed with 32 bits", (long long)n);
  FC_TRY(ensure_init());
  FC_TRY(ensemble_build_finish(ens));
  std::unique_ptr<fc_ensemble> e(new (std::nothrow) fc_ensemble);
  if (!e) return set_error(FC_E_NOMEM, "host allocation failed");
  std::vector<int32_t> idx((size_t)n);
  for (int64_t c = 0; c < n; ++c) idx[(size_t)c] = (int32_t)indices[c];
  DevBuf d_idx;
  const auto run = [&]() {
    FC_TRY(upload(d_idx, idx.data(), (size_t)n));
    return ensemble_gather(ens, d_idx.as<int32_t>(), n, e.get(), true);  // (waits: idx and d_idx outlive the kernel)
  };
  const int rc = drained(run());
  if (rc != FC_OK) {
    (void)sync();  // nothing of the new ensemble's buffers in flight when they go back to the pool
    return rc;
  }
  *out = e.release();
  return FC_OK;
}

static uint64_t q32(double d) { return (uint64_t)std::nearbyint(d * 4294967296.0); }

// one k-medoids state: the representatives, every conformer's position among them and distance to it, the cost
struct KmState {
  std::vector<int64_t> M;
  std::vector<int32_t> lab;
  std::vector<double> dist;
  uint64_t cost = 0;
};

// the assignment step: the k = 1 list of fc_ensemble_knn_cross(ens, subset(ens, M)) -- sym (may be NULL): of
// fc_ensemble_knn_cross_perm; a medoid gets its own position and distance 0, set by index
static int km_assign(fc_ensemble *ens, KmState &s, const SymTable *sym) {
  const int64_t N = ens->N, n = (int64_t)s.M.size();
  std::vector<int32_t> idx((size_t)n);
  for (int64_t c = 0; c < n; ++c) idx[(size_t)c] = (int32_t)s.M[(size_t)c];
  fc_ensemble reps;
  DevBuf d_idx;
  s.lab.resize((size_t)N);
  s.dist.resize((size_t)N);
  const auto run = [&]() {
    FC_TRY(upload(d_idx, idx.data(), (size_t)n));
    FC_TRY(ensemble_gather(ens, d_idx.as<int32_t>(), n, &reps, false));
    return knn(ens, &reps, true, 1, INFINITY, s.lab.data(), s.dist.data(), nullptr, nullptr, sym);  // (ends with a wait)
  };
  FC_TRY(drained(run()));
  for (int64_t c = 0; c < n; ++c) s.lab[(size_t)s.M[(size_t)c]] = (int32_t)c, s.dist[(size_t)s.M[(size_t)c]] = 0.0;
  s.cost = 0;
  for (int64_t j = 0; j < N; ++j) s.cost += q32(s.dist[(size_t)j]);
  return FC_OK;
}

// the loop of the contract behind the checks; sym (may be NULL): under d_sym -- the start, the assignment and the move
static int kmedoids_run(fc_ensemble *ens, const int64_t *init, int64_t n, int64_t max_iter, int64_t *medoids_out,
                        int32_t *labels_out, double *dist_out, uint64_t *cost_q32_out, int64_t *n_iter_out, const SymTable *sym) {
  const int64_t N = ens->N;
  KmState cur, prev;
  cur.M.resize((size_t)n);
  if (init != nullptr) {
    std::copy(init, init + n, cur.M.begin());
  } else {
    int64_t picked = 0;
    FC_TRY(select_diverse(ens, n, 0, -1.0, cur.M.data(), nullptr, nullptr, nullptr, &picked, nullptr, sym));
    if (picked != n) return set_error(FC_E_INTERNAL, "the diverse selection returned %lld of %lld picks", (long long)picked, (long long)n);
  }
  int64_t n_iter = 0;
  const KmState *result = nullptr;
  for (int64_t t = 0;; ++t) {
    FC_TRY(km_assign(ens, cur, sym));
    ++n_iter;
    if (t > 0 && cur.cost >= prev.cost) {
      result = &prev;
      break;
    }
    result = &cur;
    if (t == max_iter) break;
    Grouping g;
    group_by_label(cur.lab.data(), N, n, g);
    std::vector<uint64_t> S;
    std::vector<double> E;
    FC_TRY(group_sums(ens, g, S, E, nullptr, sym));
    std::vector<int64_t> next((size_t)n);
    medoids_of(g, S, E, next.data(), nullptr, nullptr, nullptr);
    if (next == cur.M) break;
    prev = std::move(cur);
    cur = KmState();
    cur.M = std::move(next);
    result = nullptr;
  }
  std::copy(result->M.begin(), result->M.end(), medoids_out);
  std::copy(result->lab.begin(), result->lab.end(), labels_out);
  std::copy(result->dist.begin(), result->dist.end(), dist_out);
  *cost_q32_out = result->cost;
  *n_iter_out = n_iter;
  return FC_OK;
}

// sym_args (may be NULL): under d_sym, already checked -- one upload of the table serves the whole call
static int kmedoids_checked(fc_ensemble *ens, const int64_t *init, int64_t n, int64_t max_iter, int64_t *medoids_out,
                            int32_t *labels_out, double *dist_out, uint64_t *cost_q32_out, int64_t *n_iter_out,
                            const SymArgs *sym_args = nullptr) {
  // (the scalar arguments are judged first, so that their refusals do not depend on the handle)
  FC_REQUIRE(n >= 1, "n=%lld < 1", (long long)n);
  FC_REQUIRE(max_iter >= 0, "max_iter=%lld < 0", (long long)max_iter);
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(medoids_out != nullptr && labels_out != nullptr && dist_out != nullptr && cost_q32_out != nullptr && n_iter_out != nullptr,
             "medoids_out / labels_out / dist_out / cost_q32_out / n_iter_out is NULL");
  *cost_q32_out = 0, *n_iter_out = 0;
  const int64_t N = ens->N;
  if (N == 0) return FC_OK;
  FC_REQUIRE(n <= N, "n=%lld representatives of N=%lld conformers", (long long)n, (long long)N);
  if (init != nullptr) FC_TRY(indices_check("init", init, n, N, true));
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  if (N > (int64_t)INT32_MAX - 256)
    return set_error(FC_E_LIMIT, "N=%lld: the selection indexes conformers with 32 bits", (long long)N);
  FC_TRY(ensure_init());
  FC_TRY(sum_limit_check(ens, N));  // (no group is larger than the ensemble)
  return with_sym_table(sym_args, [&](const SymTable *sym) {
    return kmedoids_run(ens, init, n, max_iter, medoids_out, labels_out, dist_out, cost_q32_out, n_iter_out, sym);
  });
}

// ---- the three under d_sym (include/fc_hip.h): the table's checks where fc_ensemble_knn_perm has
// them, then the plain twin's in its own order.  K = 1 without the flag: d_sym = d, the default's kernels, bit for bit.
static int sums_sym_args(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, int64_t *stats, SymArgs &a) {
  FC_TRY(sym_args_check(perms, K, A_sel, mirror, knn_sym_lds_bytes, a));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, false));
  if (stats) stats[0] = stats[1] = 0;
  a.stats = stats;
  return FC_OK;
}

static int medoids_perm_checked(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, const int32_t *labels,
                                int64_t n_groups, int64_t *medoids_out, int64_t *sizes_out, double *mean_out, double *radius_out,
                                uint64_t *sums_q32_out, double *ecc_out, double *ms_kernel, int64_t *stats) {
  SymArgs a;
  FC_TRY(sums_sym_args(ens, perms, K, A_sel, mirror, stats, a));
  const bool plain = K == 1 && !mirror;
  return medoids_checked(ens, labels, n_groups, medoids_out, sizes_out, mean_out, radius_out, sums_q32_out, ecc_out, ms_kernel,
                         plain ? nullptr : &a);
}

static int kmedoids_perm_checked(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, const int64_t *init,
                                 int64_t n, int64_t max_iter, int64_t *medoids_out, int32_t *labels_out, double *dist_out,
                                 uint64_t *cost_q32_out, int64_t *n_iter_out) {
  SymArgs a;
  FC_TRY(sums_sym_args(ens, perms, K, A_sel, mirror, nullptr, a));
  // (the start under d_sym, k_diverse_step_sym, keeps one conformer and the table in LDS: within the tiles' need)
  const bool plain = K == 1 && !mirror;
  return kmedoids_checked(ens, init, n, max_iter, medoids_out, labels_out, dist_out, cost_q32_out, n_iter_out, plain ? nullptr : &a);
}

static int silhouette_perm_checked(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                   const int32_t *labels, int64_t n_groups, double *s_out, double *a_out, double *b_out,
                                   int32_t *nearest_out, double *cluster_mean_out, int64_t *sizes_out, double *score_out,
                                   double *ms_kernel, int64_t *stats) {
  SymArgs a;
  FC_TRY(sums_sym_args(ens, perms, K, A_sel, mirror, stats, a));
  const bool plain = K == 1 && !mirror;
  return silhouette_checked(ens, labels, n_groups, s_out, a_out, b_out, nearest_out, cluster_mean_out, sizes_out, score_out,
                            ms_kernel, plain ? nullptr : &a);
}

}  // namespace fc

using namespace fc;

extern "C" {

int fc_ensemble_subset(fc_ensemble *ens, const int64_t *indices, int64_t n, fc_ensemble **out) {
  FC_API_LOCK;
  return subset_checked(ens, indices, n, out);
}

int fc_ensemble_medoids(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, int64_t *medoids_out, int64_t *sizes_out,
                        double *mean_out, double *radius_out, uint64_t *sums_q32_out, double *ecc_out, double *ms_kernel) {
  FC_API_LOCK;
  return medoids_checked(ens, labels, n_groups, medoids_out, sizes_out, mean_out, radius_out, sums_q32_out, ecc_out, ms_kernel);
}

int fc_ensemble_kmedoids(fc_ensemble *ens, const int64_t *init, int64_t n, int64_t max_iter, int64_t *medoids_out,
                         int32_t *labels_out, double *dist_out, uint64_t *cost_q32_out, int64_t *n_iter_out) {
  FC_API_LOCK;
  return kmedoids_checked(ens, init, n, max_iter, medoids_out, labels_out, dist_out, cost_q32_out, n_iter_out);
}

int fc_ensemble_silhouette(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, double *s_out, double *a_out, double *b_out,
                           int32_t *nearest_out, double *cluster_mean_out, int64_t *sizes_out, double *score_out,
                           double *ms_kernel) {
  FC_API_LOCK;
  return silhouette_checked(ens, labels, n_groups, s_out, a_out, b_out, nearest_out, cluster_mean_out, sizes_out, score_out,
                            ms_kernel);
}

int fc_ensemble_medoids_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, const int32_t *labels,
                             int64_t n_groups, int64_t *medoids_out, int64_t *sizes_out, double *mean_out, double *radius_out,
                             uint64_t *sums_q32_out, double *ecc_out, double *ms_kernel, int64_t *stats) {
  FC_API_LOCK;
  return medoids_perm_checked(ens, perms, K, A_sel, mirror, labels, n_groups, medoids_out, sizes_out, mean_out, radius_out,
                              sums_q32_out, ecc_out, ms_kernel, stats);
}

int fc_ensemble_kmedoids_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror, const int64_t *init,
                              int64_t n, int64_t max_iter, int64_t *medoids_out, int32_t *labels_out, double *dist_out,
                              uint64_t *cost_q32_out, int64_t *n_iter_out) {
  FC_API_LOCK;
  return kmedoids_perm_checked(ens, perms, K, A_sel, mirror, init, n, max_iter, medoids_out, labels_out, dist_out, cost_q32_out,
                               n_iter_out);
}

int fc_ensemble_silhouette_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, int mirror,
                                const int32_t *labels, int64_t n_groups, double *s_out, double *a_out, double *b_out,
                                int32_t *nearest_out, double *cluster_mean_out, int64_t *sizes_out, double *score_out,
                                double *ms_kernel, int64_t *stats) {
  FC_API_LOCK;
  return silhouette_perm_checked(ens, perms, K, A_sel, mirror, labels, n_groups, s_out, a_out, b_out, nearest_out,
                                 cluster_mean_out, sizes_out, score_out, ms_kernel, stats);
}

}  // extern "C"
