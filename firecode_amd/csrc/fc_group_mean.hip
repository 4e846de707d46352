// fc_group_mean.hip -- mean structures and per-atom fluctuations of groups of conformers of a resident ensemble
// (generalized Procrustes per group), for gfx950 (wave64, float64).
//
// The contract (include/fc_hip.h, fc_ensemble_group_means), per non-empty group g of the
// label-sorted copy of the ensemble (positions p, a group = a contiguous segment, members in ascending conformer index):
//
//   M_g = X[ref_g];  turn t < max_iter, g not frozen:  R_p = the Kabsch rotation of X[p] onto M_g,  Y_p = R_p X[p],
//       M' = (sum over the segment of Y_p) / |g|,  c = sqrt(sum_a |M'_a - M_ga|^2 / A),  M_g = M',  frozen when c <= tol
//   final pass: R_p, Y_p, d_p = sqrt(sum_a |Y_pa - M_ga|^2 / A), rmsf_g[a] = sqrt(sum_p |Y_pa - M_ga|^2 / |g|)
//
// Three plain launches per turn on the library's stream (no grid barrier, no spin-wait, no atomics of any kind):
//   k_gm_align       8 lanes per conformer, 32 conformers per workgroup: the covariance of the conformer (read from the
//                    conformer-minor Xs) against ITS group's mean, the rotation (kabsch_rotation_qcp, the Jacobi sweeps of
//                    kabsch_rotation where the eigenvalue is not clearly simple: k_diverse_step's atom loops and sums), and
//                    in the second atom pass the rotated coordinates Y, stored conformer-minor, and -- final pass -- d and R.
//                    The mean comes from LDS when the workgroup's 32 positions lie in one group (one read of it per
//                    workgroup), from global memory through L2 otherwise (a workgroup across several small groups).
//   k_gm_chunk_sums  one wavefront per (chunk, row): a chunk is kGmChunk = 64 consecutive positions of a group's segment,
//                    counted from the segment's start; lane l loads position l of the chunk (0.0 beyond the segment's end),
//                    the 64 values meet in an xor butterfly, distances 1, 2, 4, 8, 16, 32 in that order.  Rows: the 3 A
//                    coordinates of Y; final pass: the A values (dx dx + dy dy) + dz dz of Y - M.
//   k_gm_combine     one workgroup per group, one thread per row: the chunk partials added in ascending chunk order,
//                    divided by |g|; c and the new mean's sum of squares: per thread over its rows r = tid, tid + 256, ...
//                    in ascending order, the butterfly above per wavefront, the four wavefronts' values added in order.
//                    It overwrites the mean in place (a row is read and written by one thread), counts the turn, freezes
//                    the group, or marks the turn's word "a group is still moving".
// Every sum is therefore a fixed expression of the group's own members: the same bits on every run, with the mean staged
// or not (FC_GROUP_MEAN_STAGE=0), for every grid of the two reduction kernels (FC_GROUP_MEAN_GRID=<workgroups>) and
// however often the host reads the word (FC_GROUP_MEAN_BATCH=<turns>).  One lane form only: a second one would have to
// repeat the 8-way split of the atom loops to keep the bits.
// A frozen group is skipped by all three kernels (the final pass takes every group), so its mean is never touched again.
//
// Limits: the mean's A x 24 bytes are staged up to kGroupMeanLdsAtoms atoms (48 KiB); beyond that it is read from global
// memory.  Positions and chunks are 32-bit (N < 2^31 - 256), offsets into Y, the partials and the means 64-bit.
#include "fc_internal.h"
#include "fc_kabsch_math.h"

#include <algorithm>
#include <climits>
#include <cstdlib>

namespace fc {

constexpr int kGmThreads = 256;
constexpr int kGmLanes = 8;                           // lanes per conformer of k_gm_align
constexpr int kGmPerBlock = kGmThreads / kGmLanes;    // conformers per workgroup
constexpr int kGmChunk = 64;                          // positions per chunk of the reduction: one wavefront
constexpr int64_t kGroupMeanLdsAtoms = 2048;          // A x 24 B = 48 KiB of LDS for the mean

int64_t group_mean_stage_atoms() { return kGroupMeanLdsAtoms; }
int group_mean_chunk() { return kGmChunk; }

__device__ __forceinline__ double gm_group8_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// the 64 lanes' values added as a tree of neighbouring pairs: every lane gets the sum
__device__ __forceinline__ double gm_wave_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// the means start as their reference members: init = (group, position) per non-empty group
__global__ void __launch_bounds__(kGmThreads)
k_gm_init(const double *__restrict__ Xa, const double *__restrict__ G, int A3, const int32_t *__restrict__ init, int n_init,
          double *__restrict__ mean, double *__restrict__ Gm) {
  for (int k = blockIdx.x; k < n_init; k += gridDim.x) {
    const int g = init[2 * k], pos = init[2 * k + 1];
    const double *__restrict__ src = Xa + (int64_t)pos * A3;
    double *__restrict__ dst = mean + (int64_t)g * A3;
    for (int t = threadIdx.x; t < A3; t += kGmThreads) dst[t] = src[t];
    if (threadIdx.x == 0) Gm[g] = G[pos];
  }
}

template <bool STAGE>
__global__ void __launch_bounds__(kGmThreads)
k_gm_align(const double *__restrict__ Xs, const double *__restrict__ G, int M, int64_t Mpad, int A,
           const int32_t *__restrict__ grp, const double *__restrict__ mean, const double *__restrict__ Gm,
           const int32_t *__restrict__ frozen, int final_pass, double *__restrict__ Y, double *__restrict__ d_out,
           double *__restrict__ R_out) {
  extern __shared__ double s_mean[];  // [A][3] when STAGE and the workgroup lies in one group
  const int tid = threadIdx.x;
  const int first = blockIdx.x * kGmPerBlock;  // (the grid is ceil(M / kGmPerBlock): first < M)
  const int last = min(first + kGmPerBlock, M) - 1;
  const int g_first = grp[first];
  const bool one_group = g_first == grp[last];  // (positions are sorted by group)
  if (one_group && !final_pass && frozen[g_first]) return;
  const bool staged = STAGE && one_group;  // (the same for the whole workgroup)
  if (staged) {
    const double *__restrict__ src = mean + (int64_t)g_first * A * 3;
    for (int t = tid; t < 3 * A; t += kGmThreads) s_mean[t] = src[t];
    __syncthreads();
  }
  const int sub = tid & (kGmLanes - 1);
  const int p = first + tid / kGmLanes;
  if (p >= M) return;  // (uniform over the 8 lanes of a conformer, as every branch below: the shuffles stay inside them)
  const int g = grp[p];
  if (!final_pass && frozen[g]) return;
  const double *__restrict__ P = staged ? s_mean : mean + (int64_t)g * A * 3;

  double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int a = sub; a < A; a += kGmLanes) {
    const double *__restrict__ qa = Xs + (int64_t)(a * 3) * Mpad + p;
    const double px = P[a * 3], py = P[a * 3 + 1], pz = P[a * 3 + 2];
    const double qx = qa[0], qy = qa[Mpad], qz = qa[2 * Mpad];
    B[0] = fma(px, qx, B[0]); B[1] = fma(px, qy, B[1]); B[2] = fma(px, qz, B[2]);
    B[3] = fma(py, qx, B[3]); B[4] = fma(py, qy, B[4]); B[5] = fma(py, qz, B[5]);
    B[6] = fma(pz, qx, B[6]); B[7] = fma(pz, qy, B[7]); B[8] = fma(pz, qz, B[8]);
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) B[e] = gm_group8_sum(B[e]);
  // (identical in the 8 lanes: xor sums are)
  double R[9];
  if (!kabsch_rotation_qcp(B, Gm[g] + G[p], R)) (void)kabsch_rotation(B, R);
  double ssq = 0.0;
  for (int a = sub; a < A; a += kGmLanes) {
    const int64_t row = (int64_t)(a * 3) * Mpad + p;
    const double *__restrict__ qa = Xs + row;
    const double px = P[a * 3], py = P[a * 3 + 1], pz = P[a * 3 + 2];
    const double qx = qa[0], qy = qa[Mpad], qz = qa[2 * Mpad];
    const double yx = R[0] * qx + R[1] * qy + R[2] * qz;
    const double yy = R[3] * qx + R[4] * qy + R[5] * qz;
    const double yz = R[6] * qx + R[7] * qy + R[8] * qz;
    Y[row] = yx, Y[row + Mpad] = yy, Y[row + 2 * Mpad] = yz;
    const double dx = px - yx, dy = py - yy, dz = pz - yz;
    ssq += dx * dx + dy * dy + dz * dz;
  }
  if (!final_pass) return;
  ssq = gm_group8_sum(ssq);
  if (sub == 0) {
    d_out[p] = sqrt(ssq / (double)A);
#pragma unroll
    for (int e = 0; e < 9; ++e) R_out[(int64_t)p * 9 + e] = R[e];
  }
}

// chunks = (begin, end, group) per chunk; part[chunk][3 A] (the final pass uses the first A of a chunk's slots)
__global__ void __launch_bounds__(kGmThreads)
k_gm_chunk_sums(const double *__restrict__ Y, int64_t Mpad, int A, const int32_t *__restrict__ chunks, int n_chunks,
                const double *__restrict__ mean, const int32_t *__restrict__ frozen, int final_pass,
                double *__restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int A3 = 3 * A, rows = final_pass ? A : A3;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int b = chunks[3 * c], e = chunks[3 * c + 1], g = chunks[3 * c + 2];
    if (!final_pass && frozen[g]) continue;
    const int p = b + lane;
    const bool valid = p < e;
    const double *__restrict__ Mg = mean + (int64_t)g * A3;
    double *__restrict__ out = part + (int64_t)c * A3;
    for (int r = w; r < rows; r += kGmThreads / 64) {  // (wave-uniform)
      double v = 0.0;
      if (valid) {
        if (!final_pass) {
          v = Y[(int64_t)r * Mpad + p];
        } else {
          const double *__restrict__ ya = Y + (int64_t)(r * 3) * Mpad + p;
          const double dx = ya[0] - Mg[r * 3], dy = ya[Mpad] - Mg[r * 3 + 1], dz = ya[2 * Mpad] - Mg[r * 3 + 2];
          v = (dx * dx + dy * dy) + dz * dz;
        }
      }
      v = gm_wave_sum(v);
      if (lane == 0) out[r] = v;
    }
  }
}

// active = (group, first chunk, chunks, members) per group of two or more members
__global__ void __launch_bounds__(kGmThreads)
k_gm_combine(const double *__restrict__ part, int A, const int32_t *__restrict__ active, int n_active, int final_pass,
             int turn, double tol, double *__restrict__ mean, double *__restrict__ Gm, double *__restrict__ rmsf,
             int32_t *__restrict__ frozen, int32_t *__restrict__ n_iter, int32_t *__restrict__ moving) {
  __shared__ double s_c[kGmThreads / 64], s_g[kGmThreads / 64];
  const int tid = threadIdx.x;
  const int A3 = 3 * A, rows = final_pass ? A : A3;
  for (int k = blockIdx.x; k < n_active; k += gridDim.x) {
    const int g = active[4 * k], c0 = active[4 * k + 1], nc = active[4 * k + 2];
    const double size = (double)active[4 * k + 3];
    if (!final_pass && frozen[g]) continue;  // (the same for the whole workgroup)
    double acc_c = 0.0, acc_g = 0.0;
    for (int r = tid; r < rows; r += kGmThreads) {
      const double *__restrict__ src = part + (int64_t)c0 * A3 + r;
      double s = src[0];
      for (int c = 1; c < nc; ++c) s += src[(int64_t)c * A3];
      if (final_pass) {
        rmsf[(int64_t)g * A + r] = sqrt(s / size);
      } else {
        double *__restrict__ m = mean + (int64_t)g * A3 + r;
        const double m_new = s / size, diff = m_new - *m;
        acc_c += diff * diff;
        acc_g += m_new * m_new;
        *m = m_new;
      }
    }
    if (final_pass) continue;
    acc_c = gm_wave_sum(acc_c);
    acc_g = gm_wave_sum(acc_g);
    __syncthreads();  // (s_c / s_g may still be read from the previous group)
    if ((tid & 63) == 0) s_c[tid >> 6] = acc_c, s_g[tid >> 6] = acc_g;
    __syncthreads();
    if (tid == 0) {
      const double c = sqrt((((s_c[0] + s_c[1]) + s_c[2]) + s_c[3]) / (double)A);
      Gm[g] = ((s_g[0] + s_g[1]) + s_g[2]) + s_g[3];
      n_iter[g] = turn + 1;
      if (c <= tol) frozen[g] = 1;
      else *moving = 1;  // (every writer writes the same value)
    }
  }
}

static int env_int(const char *name, int lo, int hi, int dflt) {
  const char *v = getenv(name);
  if (!v || !*v) return dflt;
  char *end = nullptr;
  const long x = strtol(v, &end, 10);
  return (*end != 0 || x < lo || x > hi) ? dflt : (int)x;
}

// FC_GROUP_MEAN_STAGE=0: the mean from global memory everywhere; FC_GROUP_MEAN_GRID=<n>: workgroups of the two
// reduction kernels; FC_GROUP_MEAN_BATCH=<n>: turns enqueued between two reads of the "still moving" word.  Speed and
// tests only: the outputs are the same bits for every value.
bool group_mean_stage(int64_t A) { return A <= kGroupMeanLdsAtoms && env_int("FC_GROUP_MEAN_STAGE", 0, 1, 1) != 0; }
static unsigned gm_grid(int64_t items) {
  const int forced = env_int("FC_GROUP_MEAN_GRID", 1, 1 << 20, 0);
  return (unsigned)std::max<int64_t>(1, forced ? forced : std::min<int64_t>(items, (int64_t)1 << 16));
}
constexpr int kGmBatchMax = 64;
static int gm_batch() { return env_int("FC_GROUP_MEAN_BATCH", 1, kGmBatchMax, 4); }

static int gm_pass(const fc_ensemble *e, const GroupMeanPlan &pl, GroupMeanWork &w, bool stage, int final_pass, int turn,
                   double tol, int32_t *moving) {
  const int M = (int)pl.M, A = (int)e->A;
  const unsigned nb = (unsigned)ceil_div(pl.M, kGmPerBlock);
  if (stage)
    hipLaunchKernelGGL((k_gm_align<true>), dim3(nb), dim3(kGmThreads), (size_t)A * 3 * sizeof(double), ctx().stream,
                       e->Xs.as<double>(), e->G.as<double>(), M, e->Npad, A, pl.grp_dev, w.mean.as<double>(), w.Gm.as<double>(),
                       w.frozen.as<int32_t>(), final_pass, w.Y.as<double>(), w.d.as<double>(), w.R.as<double>());
  else
    hipLaunchKernelGGL((k_gm_align<false>), dim3(nb), dim3(kGmThreads), 0, ctx().stream, e->Xs.as<double>(),
                       e->G.as<double>(), M, e->Npad, A, pl.grp_dev, w.mean.as<double>(), w.Gm.as<double>(),
                       w.frozen.as<int32_t>(), final_pass, w.Y.as<double>(), w.d.as<double>(), w.R.as<double>());
  FC_TRY(check_launch("k_gm_align"));
  if (pl.n_active == 0) return FC_OK;  // (singletons only: nothing to reduce)
  hipLaunchKernelGGL(k_gm_chunk_sums, dim3(gm_grid(pl.n_chunks)), dim3(kGmThreads), 0, ctx().stream, w.Y.as<double>(), e->Npad,
                     A, pl.chunks_dev, (int)pl.n_chunks, w.mean.as<double>(), w.frozen.as<int32_t>(), final_pass,
                     w.part.as<double>());
  FC_TRY(check_launch("k_gm_chunk_sums"));
  hipLaunchKernelGGL(k_gm_combine, dim3(gm_grid(pl.n_active)), dim3(kGmThreads), 0, ctx().stream, w.part.as<double>(), A,
                     pl.active_dev, (int)pl.n_active, final_pass, turn, tol, w.mean.as<double>(), w.Gm.as<double>(),
                     w.rmsf.as<double>(), w.frozen.as<int32_t>(), w.n_iter.as<int32_t>(), moving);
  return check_launch("k_gm_combine");
}

// The turns and the final pass behind fc_ensemble_group_means (arguments checked there).  e: the label-sorted ensemble
// (pl.M = e->N >= 1 positions); w.frozen and w.n_iter uploaded by the caller (1 for singletons and empty groups | 0).
// Enqueued and, every gm_batch() turns, waited for; the results stay on the device.  timed: the context's events ev0 /
// ev1 around everything, for the caller to read behind its wait.
int group_means_run(const fc_ensemble *e, const GroupMeanPlan &pl, GroupMeanWork &w, int64_t max_iter, double tol, bool timed) {
  Context &c = ctx();
  const int A = (int)e->A;
  const bool stage = group_mean_stage(e->A);
  const int batch = gm_batch();
  FC_TRY(w.Y.reserve((size_t)A * 3 * e->Npad * sizeof(double)));
  FC_TRY(w.part.reserve((size_t)std::max<int64_t>(pl.n_chunks, 1) * A * 3 * sizeof(double)));
  FC_TRY(w.d.reserve((size_t)pl.M * sizeof(double)));
  FC_TRY(w.R.reserve((size_t)pl.M * 9 * sizeof(double)));
  FC_TRY(w.Gm.reserve((size_t)pl.n_groups * sizeof(double)));
  FC_TRY(w.words.reserve(kGmBatchMax * sizeof(int32_t)));
  if (timed) FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  hipLaunchKernelGGL(k_gm_init, dim3(gm_grid(pl.n_init)), dim3(kGmThreads), 0, c.stream, e->Xa.as<double>(), e->G.as<double>(),
                     A * 3, pl.init_dev, (int)pl.n_init, w.mean.as<double>(), w.Gm.as<double>());
  FC_TRY(check_launch("k_gm_init"));
  if (pl.n_active > 0) {
    const int64_t turns = std::min<int64_t>(max_iter, (int64_t)INT32_MAX - 1);  // (n_iter is 32-bit on the device)
    for (int64_t t = 0; t < turns;) {
      const int64_t t_end = std::min(turns, t + batch);
      FC_HIP_TRY(hipMemsetAsync(w.words.p, 0, kGmBatchMax * sizeof(int32_t), c.stream));
      int32_t *last = nullptr;
      for (; t < t_end; ++t) {
        last = w.words.as<int32_t>() + (t % batch);
        FC_TRY(gm_pass(e, pl, w, stage, 0, (int)t, tol, last));
      }
      int32_t moving = 0;
      FC_HIP_TRY(hipMemcpyAsync(&moving, last, sizeof moving, hipMemcpyDeviceToHost, c.stream));
      FC_TRY(sync());
      if (!moving) break;  // every group is frozen: further turns would do nothing
    }
  }
  FC_TRY(gm_pass(e, pl, w, stage, 1, 0, tol, nullptr));
  if (timed) FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  return FC_OK;
}

__global__ void k_warm_group_mean() {}
int warm_group_mean() {
  hipLaunchKernelGGL(k_warm_group_mean, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_group_mean");
}

}  // namespace fc
