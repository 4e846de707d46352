// fc_api_group_mean.cpp -- the extern "C" surface (include/fc_hip.h) of "what does this group look like": the mean
// structure of every group of conformers with its members superposed on it (generalized Procrustes), the per-atom
// fluctuation about it, every member's RMSD to it and the member closest to it.  The kernels: fc_group_mean.hip; the
// label-sorted copy is the medoids' (group_by_label, ensemble_gather).
#include <algorithm>
#include <cmath>
#include <limits>

#include "fc_internal.h"

namespace fc {

static int group_means_checked(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, const int64_t *refs, int64_t max_iter,
                               double tol, double *means_out, double *rmsf_out, double *dist_out, double *rot_out,
                               int64_t *closest_out, int64_t *sizes_out, int64_t *n_iter_out, double *ms_kernel) {
  // (the scalar arguments are judged first, so that their refusals do not depend on the handle)
  FC_REQUIRE(n_groups >= 1, "n_groups=%lld < 1", (long long)n_groups);
  FC_REQUIRE(n_groups <= (int64_t)INT32_MAX, "n_groups=%lld: labels are 32-bit", (long long)n_groups);
  FC_REQUIRE(max_iter >= 0, "max_iter=%lld < 0", (long long)max_iter);
  FC_REQUIRE(tol >= 0.0, "tol=%g is negative or NaN", tol);
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(means_out != nullptr && rmsf_out != nullptr && dist_out != nullptr && closest_out != nullptr && sizes_out != nullptr &&
                 n_iter_out != nullptr,
             "means_out / rmsf_out / dist_out / closest_out / sizes_out / n_iter_out is NULL");
  const int64_t N = ens->N, A = ens->A, A3 = 3 * A;
  FC_TRY(labels_check(labels, N, n_groups));
  if (ms_kernel) *ms_kernel = 0.0;
  if (N == 0) return FC_OK;  // (writes nothing)
  if (N > (int64_t)INT32_MAX - 256)
    return set_error(FC_E_LIMIT, "N=%lld: the groups index conformers with 32 bits", (long long)N);
  Grouping g;
  group_by_label(labels, N, n_groups, g);
  const int64_t M = (int64_t)g.order.size();
  if (refs != nullptr) {
    for (int64_t c = 0; c < n_groups; ++c) {
      if (g.offs[(size_t)c + 1] == g.offs[(size_t)c]) continue;  // (an empty group's entry is not read)
      const int64_t r = refs[c];
      FC_REQUIRE(r >= 0 && r < N, "refs[%lld]=%lld outside [0, %lld)", (long long)c, (long long)r, (long long)N);
      FC_REQUIRE((labels == nullptr ? 0 : labels[r]) == c, "refs[%lld]=%lld is not a member of group %lld", (long long)c,
                 (long long)r, (long long)c);
    }
  }
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");

  const double nan = std::numeric_limits<double>::quiet_NaN();
  // ---- the tables of the call
  const int chunk = group_mean_chunk();
  std::vector<int32_t> grp((size_t)M), pos_of(refs ? (size_t)N : 0, -1), init, chunks, active;
  std::vector<int32_t> frozen((size_t)n_groups, 1), iters((size_t)n_groups, 0);
  if (refs)
    for (int64_t p = 0; p < M; ++p) pos_of[(size_t)g.order[(size_t)p]] = (int32_t)p;
  int64_t n_chunks = 0;
  for (int64_t c = 0; c < n_groups; ++c) {
    const int64_t b = g.offs[(size_t)c], e = g.offs[(size_t)c + 1], size = e - b;
    sizes_out[c] = size;
    if (size == 0) continue;
    for (int64_t p = b; p < e; ++p) grp[(size_t)p] = (int32_t)c;
    init.push_back((int32_t)c);
    init.push_back(refs ? pos_of[(size_t)refs[c]] : (int32_t)b);  // (the segment starts at its smallest-index member)
    if (size < 2) continue;
    const int64_t nc = ceil_div(size, chunk);
    if (n_chunks + nc > (int64_t)INT32_MAX)
      return set_error(FC_E_LIMIT, "%lld groups: the chunks of the reduction are indexed with 32 bits", (long long)n_groups);
    active.insert(active.end(), {(int32_t)c, (int32_t)n_chunks, (int32_t)nc, (int32_t)size});
    for (int64_t k = 0; k < nc; ++k)
      chunks.insert(chunks.end(), {(int32_t)(b + k * chunk), (int32_t)std::min(e, b + (k + 1) * chunk), (int32_t)c});
    n_chunks += nc;
    frozen[(size_t)c] = 0;
  }
  for (int64_t i = 0; i < N; ++i) dist_out[i] = nan;
  if (rot_out)
    for (int64_t i = 0; i < N; ++i)
      for (int e = 0; e < 9; ++e) rot_out[i * 9 + e] = e % 4 == 0 ? 1.0 : 0.0;
  for (int64_t c = 0; c < n_groups; ++c) {
    closest_out[c] = -1, n_iter_out[c] = 0;
    if (sizes_out[c] == 0) {
      std::fill(means_out + c * A3, means_out + (c + 1) * A3, nan);
      std::fill(rmsf_out + c * A, rmsf_out + (c + 1) * A, nan);
    }
  }
  if (M == 0) return FC_OK;  // (nobody is in a group: no device)

  FC_TRY(ensure_init());
  FC_TRY(ensemble_build_finish(ens));
  bool identity = M == N;
  for (int64_t p = 0; identity && p < M; ++p) identity = g.order[(size_t)p] == p;
  fc_ensemble sorted;  // the label-sorted copy (not made when the ensemble is in that order already)
  DevBuf d_order, d_grp, d_init, d_chunks, d_active;
  GroupMeanWork w;
  std::vector<double> mean((size_t)n_groups * A3), rmsf((size_t)n_groups * A), d((size_t)M), R(rot_out ? (size_t)M * 9 : 0);
  const auto run = [&]() {
    const fc_ensemble *e = ens;
    if (!identity) {
      FC_TRY(upload(d_order, g.order.data(), (size_t)M));
      FC_TRY(ensemble_gather(ens, d_order.as<int32_t>(), M, &sorted, false));
      e = &sorted;
    }
    GroupMeanPlan pl;
    pl.M = M, pl.n_groups = n_groups;
    FC_TRY(upload(d_grp, grp.data(), grp.size()));
    FC_TRY(upload(d_init, init.data(), init.size()));
    FC_TRY(upload(d_chunks, chunks.data(), chunks.size()));
    FC_TRY(upload(d_active, active.data(), active.size()));
    pl.grp_dev = d_grp.as<int32_t>();
    pl.init_dev = d_init.as<int32_t>(), pl.n_init = (int64_t)init.size() / 2;
    pl.chunks_dev = d_chunks.as<int32_t>(), pl.n_chunks = n_chunks;
    pl.active_dev = d_active.as<int32_t>(), pl.n_active = (int64_t)active.size() / 4;
    FC_TRY(w.mean.reserve(mean.size() * sizeof(double)));
    FC_TRY(w.rmsf.reserve(rmsf.size() * sizeof(double)));
    FC_TRY(upload(w.frozen, frozen.data(), frozen.size()));
    FC_TRY(upload(w.n_iter, iters.data(), iters.size()));
    FC_TRY(group_means_run(e, pl, w, max_iter, tol, ms_kernel != nullptr));
    // (rows of empty groups were never written on the device: the host's NaN stand)
    FC_TRY(d2h(mean.data(), w.mean.p, mean.size() * sizeof(double)));
    FC_TRY(d2h(rmsf.data(), w.rmsf.p, rmsf.size() * sizeof(double)));
    FC_TRY(d2h(iters.data(), w.n_iter.p, iters.size() * sizeof(int32_t)));
    FC_TRY(d2h(d.data(), w.d.p, d.size() * sizeof(double)));
    if (rot_out) FC_TRY(d2h(R.data(), w.R.p, R.size() * sizeof(double)));
    FC_TRY(sync());
    if (ms_kernel) {
      float ms = 0.0f;
      FC_HIP_TRY(hipEventElapsedTime(&ms, ctx().ev0, ctx().ev1));
      *ms_kernel = ms;
    }
    return FC_OK;
  };
  FC_TRY(drained(run()));

  for (int64_t c = 0; c < n_groups; ++c) {
    const int64_t b = g.offs[(size_t)c], e = g.offs[(size_t)c + 1], size = e - b;
    if (size == 0) continue;
    std::copy(mean.begin() + c * A3, mean.begin() + (c + 1) * A3, means_out + c * A3);
    n_iter_out[c] = iters[(size_t)c];
    if (size == 1) {  // mean = itself: d = 0, rmsf = 0 and R = identity by definition, not by a rotation's last bits
      std::fill(rmsf_out + c * A, rmsf_out + (c + 1) * A, 0.0);
      dist_out[g.order[(size_t)b]] = 0.0;
      closest_out[c] = g.order[(size_t)b];
      continue;
    }
    std::copy(rmsf.begin() + c * A, rmsf.begin() + (c + 1) * A, rmsf_out + c * A);
    int64_t best = -1;
    double d_best = 0.0;
    for (int64_t p = b; p < e; ++p) {  // (ascending conformer index: the lowest index wins a tie)
      const int64_t i = g.order[(size_t)p];
      dist_out[i] = d[(size_t)p];
      if (rot_out) std::copy(R.begin() + p * 9, R.begin() + (p + 1) * 9, rot_out + i * 9);
      if (best < 0 || d[(size_t)p] < d_best) best = i, d_best = d[(size_t)p];
    }
    closest_out[c] = best;
  }
  return FC_OK;
}

}  // namespace fc

using namespace fc;

extern "C" {

int fc_ensemble_group_means(fc_ensemble *ens, const int32_t *labels, int64_t n_groups, const int64_t *refs, int64_t max_iter,
                            double tol, double *means_out, double *rmsf_out, double *dist_out, double *rot_out,
                            int64_t *closest_out, int64_t *sizes_out, int64_t *n_iter_out, double *ms_kernel) {
  FC_API_LOCK;
  return group_means_checked(ens, labels, n_groups, refs, max_iter, tol, means_out, rmsf_out, dist_out, rot_out, closest_out,
                             sizes_out, n_iter_out, ms_kernel);
}

}  // extern "C"
