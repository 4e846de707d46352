// fc_symm.hip -- symmetry-aware RMSD similarity (include/fc_hip.h, "symmetry-aware forms"):
//
//   (r_k, m_k) = rmsd_and_max(X[i], X[j][perms[k]])      k = 0 .. K-1
//   similar_sym(i, j) = any_k (r_k < max_rmsd && m_k < max_dev)      [&& |E_i - E_j| < max_dE]
//
// An all-pairs, exact-fp64 kernel over the resident ensemble.  A workgroup owns a tile of 16 row x 16 column conformers,
// one pair per lane; it keeps its row tile in LDS and walks a strided share of the column tiles at or right of the
// diagonal.  Both coordinate tiles and the permutation table (16-bit indices) sit in LDS, so a permutation is nothing
// but an LDS address: the lane reads p_a and q_{perms[k][a]}.  Per k: the 3 x 3 covariance, the fp64 polynomial test
// (kabsch_may_be_below; Gp + Gq does not depend on k), and only where it passes the exact rotation and the explicit
// deviation pass, summed in the order of pair_exact_aos -- on pairs gathered in LDS until a workgroup's worth waits, so
// that a few candidates per wavefront do not make every wavefront walk the rotation.  The result goes out in the two
// forms the ladder and the union-find already take: the bit matrix and the ensemble's similar-pair queue.
#include "fc_internal.h"
#include "fc_kabsch_math.h"

namespace fc {

namespace {
constexpr int kSymTile = 16;  // conformers per side of a tile: 16 x 16 pairs = the 256 lanes of a workgroup
// doubles between two conformers of a tile: odd, so that the 16 column conformers a wavefront reads start in different banks
__host__ __device__ inline int symm_stride(int A) { return (A * 3) | 1; }

// one tile of kSymTile conformers, first one c0, from the conformer-major copy (rows past N: zeros)
__device__ __forceinline__ void symm_fill(double *__restrict__ dst, const double *__restrict__ Xa, int64_t c0, int64_t N,
                                          int A3, int stride, int tid) {
  const int64_t base = c0 * A3, end = N * (int64_t)A3;
  for (int idx = tid; idx < kSymTile * A3; idx += 256) {
    const int l = idx / A3, rest = idx - l * A3;
    dst[l * stride + rest] = base + idx < end ? Xa[base + idx] : 0.0;
  }
}

// covariance of (p, q[perm]) -- B[x][y] = sum_a p_a[x] q_perm(a)[y], accumulated atom by atom as pair_exact_aos does
template <class Ptr>
__device__ __forceinline__ void symm_covariance(const double *__restrict__ p, const double *__restrict__ q, Ptr perm, int A,
                                                double (&B)[9]) {
#pragma unroll
  for (int e = 0; e < 9; ++e) B[e] = 0.0;
  for (int a = 0; a < A; ++a) {
    const int b = (int)perm[a] * 3;
    const double px = p[a * 3], py = p[a * 3 + 1], pz = p[a * 3 + 2];
    const double qx = q[b], qy = q[b + 1], qz = q[b + 2];
    B[0] = fma(px, qx, B[0]); B[1] = fma(px, qy, B[1]); B[2] = fma(px, qz, B[2]);
    B[3] = fma(py, qx, B[3]); B[4] = fma(py, qy, B[4]); B[5] = fma(py, qz, B[5]);
    B[6] = fma(pz, qx, B[6]); B[7] = fma(pz, qy, B[7]); B[8] = fma(pz, qz, B[8]);
  }
}

// explicit rotated difference of (p, q[perm]) under R -> (rmsd, maxdev); the sums of pair_exact_aos
template <class Ptr>
__device__ __forceinline__ void symm_deviation(const double *__restrict__ p, const double *__restrict__ q, Ptr perm, int A,
                                               const double (&R)[9], double &rmsd, double &maxdev) {
  double ssq = 0.0, mx = 0.0;
  for (int a = 0; a < A; ++a) {
    const int b = (int)perm[a] * 3;
    const double px = p[a * 3], py = p[a * 3 + 1], pz = p[a * 3 + 2];
    const double qx = q[b], qy = q[b + 1], qz = q[b + 2];
    const double rx = R[0] * qx + R[1] * qy + R[2] * qz, ry = R[3] * qx + R[4] * qy + R[5] * qz;
    const double rz = R[6] * qx + R[7] * qy + R[8] * qz;
    const double dx = px - rx, dy = py - ry, dz = pz - rz;
    const double s = dx * dx + dy * dy + dz * dz;
    ssq += s;
    mx = fmax(mx, s);
  }
  rmsd = sqrt(ssq / (double)A);
  maxdev = sqrt(mx);
}
}  // namespace

// candidate pairs wait in LDS for the exact pass: a drain takes 256 of them, a column tile adds at most 256
constexpr int kSymQueue = 512;

size_t symm_lds_bytes(int64_t A, int64_t K) {
  return (size_t)2 * kSymTile * (size_t)symm_stride((int)A) * sizeof(double) + (((size_t)K * (size_t)A * sizeof(uint16_t) + 7) & ~(size_t)7) +
         (size_t)2 * kSymQueue * sizeof(uint64_t) + 8;  // (+ the queue's fill level)
}

// ---------------------------------------------------------------------------
// k_symm_simbits: grid (row tiles, column share).  Two phases per workgroup, so that the expensive one runs on full
// wavefronts whatever the density of similar pairs:
//   screen  every lane owns one pair of the current 16 x 16 tile: per k the covariance from LDS and the fp64 polynomial
//           test; a pair with any passing k is queued in LDS with the 64-bit set of those k
//   exact   whenever 256 pairs wait (and once at the end) every lane takes one: per queued k the covariance again (from
//           the conformer-major copy in memory; the same sums, the same bits), the rotation, the deviation pass.  The
//           k loop ends at the first complete pass that is itself clear of both thresholds: a pair whose verdict could
//           turn on a value within 1e-9 of a threshold has had every queued k looked at.
// counters[1] += queued pairs, [2] and [6] += similar pairs (the queue is complete iff [6] <= simq_cap, as the ladder and
// the union-find check it), [3] += grey pairs (counted once).  bits: zeroed by the launcher, row i word j >> 6, only j > i.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void symm_exact(bool have, uint64_t e, uint64_t kmask, const double *__restrict__ Xa,
                                           const double *__restrict__ G, int A, const uint16_t *__restrict__ pt,
                                           double max_rmsd, double max_dev, const double *__restrict__ energies, double max_dE,
                                           uint64_t *__restrict__ bits, int64_t W, unsigned long long *__restrict__ counters,
                                           uint64_t *__restrict__ simq, unsigned long long simq_cap, int lane) {
  const int64_t i = (int64_t)(e >> 32), j = (int64_t)(e & 0xffffffffull);
  bool sim = false, grey = false;
  if (have) {
    const double *__restrict__ p = Xa + i * (int64_t)A * 3;
    const double *__restrict__ q = Xa + j * (int64_t)A * 3;
    const double Gs = G[i] + G[j];
    while (kmask) {
      const int k = __ffsll((unsigned long long)kmask) - 1;
      kmask &= kmask - 1;
      const uint16_t *__restrict__ pk = pt + k * A;
      double B[9], R[9];
      symm_covariance(p, q, pk, A, B);
      if (!kabsch_rotation_qcp(B, Gs, R)) (void)kabsch_rotation(B, R);
      double rk, mk;
      symm_deviation(p, q, pk, A, R, rk, mk);
      const bool pass = (rk < max_rmsd) && (mk < max_dev);
      const bool g = (fabs(rk - max_rmsd) < 1e-9) || (rk < max_rmsd && fabs(mk - max_dev) < 1e-9);
      sim = sim || pass;
      grey = grey || g;
      if (pass && !g) break;
    }
    if (energies != nullptr) sim = sim && (fabs(energies[i] - energies[j]) < max_dE);
    if (sim) atomicOr(reinterpret_cast<unsigned long long *>(&bits[i * W + (j >> 6)]), 1ull << (j & 63));
  }
  const uint64_t mc = __ballot(have), ms = __ballot(sim), mg = __ballot(grey);
  unsigned long long sbase = 0;
  if (lane == 0) {
    if (mc) atomicAdd(&counters[1], (unsigned long long)__popcll(mc));
    if (ms) {
      sbase = atomicAdd(&counters[2], (unsigned long long)__popcll(ms));
      atomicAdd(&counters[6], (unsigned long long)__popcll(ms));
    }
    if (mg) atomicAdd(&counters[3], (unsigned long long)__popcll(mg));
  }
  sbase = __shfl(sbase, 0);
  if (sim) {
    const unsigned long long at = sbase + (unsigned long long)__popcll(ms & ((1ull << lane) - 1ull));
    if (at < simq_cap) simq[at] = e;
  }
}

__global__ void __launch_bounds__(256)
k_symm_simbits(const double *__restrict__ Xa, const double *__restrict__ G, int64_t N, int A,
               const uint16_t *__restrict__ perms, int K, double max_rmsd, double max_dev,
               const double *__restrict__ energies, double max_dE, uint64_t *__restrict__ bits, int64_t W,
               unsigned long long *__restrict__ counters, uint64_t *__restrict__ simq, unsigned long long simq_cap) {
  extern __shared__ double symm_lds[];
  const int A3 = A * 3, stride = symm_stride(A);
  double *rows = symm_lds, *cols = symm_lds + kSymTile * stride;
  uint64_t *q_pair = reinterpret_cast<uint64_t *>(cols + kSymTile * stride);
  uint64_t *q_mask = q_pair + kSymQueue;
  int &q_n = *reinterpret_cast<int *>(q_mask + kSymQueue);
  uint16_t *pt = reinterpret_cast<uint16_t *>(q_mask + kSymQueue + 1);
  const int tid = threadIdx.x, lane = tid & 63;
  const int r = tid >> 4, c = tid & 15;
  const int64_t rb = blockIdx.x, nct = (N + kSymTile - 1) / kSymTile;
  symm_fill(rows, Xa, rb * kSymTile, N, A3, stride, tid);
  for (int idx = tid; idx < K * A; idx += 256) pt[idx] = perms[idx];
  if (tid == 0) q_n = 0;
  const int64_t i = rb * kSymTile + r;
  const double Gp = i < N ? G[i] : 0.0;
  const double A_thr2 = (double)A * (max_rmsd * max_rmsd + kScreenMargin);
  const double *__restrict__ p = rows + r * stride;
  const double *__restrict__ q = cols + c * stride;
  for (int64_t cb = rb + blockIdx.y; cb < nct; cb += gridDim.y) {
    __syncthreads();  // the previous column tile has been read by every lane; q_n is settled
    symm_fill(cols, Xa, cb * kSymTile, N, A3, stride, tid);
    __syncthreads();
    const int64_t j = cb * kSymTile + c;
    const bool on = i < N && j < N && j > i;
    uint64_t kmask = 0;
    if (on) {
      const double Gs = Gp + G[j];
      for (int k = 0; k < K; ++k) {
        double B[9];
        symm_covariance(p, q, pt + k * A, A, B);
        if (kabsch_may_be_below(B, Gs, A_thr2)) kmask |= 1ull << k;
      }
    }
    const uint64_t mq = __ballot(kmask != 0);
    int qbase = 0;
    if (lane == 0 && mq) qbase = atomicAdd(&q_n, __popcll(mq));
    qbase = __shfl(qbase, 0);
    if (kmask != 0) {
      const int at = qbase + __popcll(mq & ((1ull << lane) - 1ull));  // < kSymQueue: fewer than 256 waited, at most 256 came
      q_pair[at] = ((uint64_t)i << 32) | (uint64_t)j;
      q_mask[at] = kmask;
    }
    __syncthreads();
    const int waiting = q_n;
    if (waiting >= 256) {  // (uniform) the last 256 entries, one per lane
      symm_exact(true, q_pair[waiting - 256 + tid], q_mask[waiting - 256 + tid], Xa, G, A, pt, max_rmsd, max_dev, energies, max_dE,
                 bits, W, counters, simq, simq_cap, lane);
      __syncthreads();
      if (tid == 0) q_n = waiting - 256;
    }
  }
  __syncthreads();
  const int waiting = q_n;
  if (waiting > 0) {
    const bool have = tid < waiting;
    symm_exact(have, have ? q_pair[tid] : 0ull, have ? q_mask[tid] : 0ull, Xa, G, A, pt, max_rmsd, max_dev, energies, max_dE, bits, W,
               counters, simq, simq_cap, lane);
  }
}

// all K values of each requested pair: one lane per (pair, k), straight from the conformer-major copy
__global__ void __launch_bounds__(256)
k_symm_pairs(const double *__restrict__ Xa, int A, const uint16_t *__restrict__ perms, int K,
             const int64_t *__restrict__ pi, const int64_t *__restrict__ pj, int64_t P, double *__restrict__ rmsd,
             double *__restrict__ maxdev) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P * K) return;
  const int64_t pr = t / K;
  const int k = (int)(t - pr * K);
  const double *__restrict__ p = Xa + pi[pr] * (int64_t)A * 3;
  const double *__restrict__ q = Xa + pj[pr] * (int64_t)A * 3;
  const uint16_t *__restrict__ pk = perms + (int64_t)k * A;
  double B[9], R[9];
  symm_covariance(p, q, pk, A, B);
  (void)kabsch_rotation(B, R);
  double rk, mk;
  symm_deviation(p, q, pk, A, R, rk, mk);
  rmsd[t] = rk;
  maxdev[t] = mk;
}

// similarity bits and the similar-pair queue of the whole (unsharded) ensemble; the workspace is ensemble_shard's
int launch_symm_simbits(fc_ensemble *e, const uint16_t *perms_dev, int64_t K, double max_rmsd, double max_dev,
                        const double *energies_dev, double max_dE) {
  const int64_t N = e->N, nt = ceil_div(N, (int64_t)kSymTile);
  const size_t lds = symm_lds_bytes(e->A, K);
  if (lds > kLdsLimit)
    return set_error(FC_E_LIMIT, "A=%lld selected atoms with K=%lld permutations need %zu bytes of LDS per tile (limit %zu)",
                     (long long)e->A, (long long)K, lds, kLdsLimit);
  FC_HIP_TRY(hipMemsetAsync(e->bits.p, 0, (size_t)e->rows_local * e->W * sizeof(uint64_t), ctx().stream));
  if (N < 2) return FC_OK;
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_symm_simbits), lds, "k_symm_simbits"));
  const unsigned share = (unsigned)std::min<int64_t>(nt, 8);  // column tiles are dealt to this many workgroups per row tile
  hipLaunchKernelGGL(k_symm_simbits, dim3((unsigned)nt, share), dim3(256), lds, ctx().stream, e->Xa.as<double>(),
                     e->G.as<double>(), N, (int)e->A, perms_dev, (int)K, max_rmsd, max_dev, energies_dev, max_dE,
                     e->bits.as<uint64_t>(), e->W, reinterpret_cast<unsigned long long *>(e->counters.p),
                     e->simq.as<uint64_t>(), (unsigned long long)e->pairq_cap);
  return check_launch("k_symm_simbits");
}

int launch_symm_pairs(const fc_ensemble *e, const uint16_t *perms_dev, int64_t K, const int64_t *pi_dev,
                      const int64_t *pj_dev, int64_t P, double *rmsd_dev, double *maxdev_dev) {
  if (P == 0) return FC_OK;
  if (!grid_x_fits(ceil_div(P * K, 256), 256))
    return set_error(FC_E_LIMIT, "P=%lld pairs x K=%lld permutations exceed one launch", (long long)P, (long long)K);
  hipLaunchKernelGGL(k_symm_pairs, dim3((unsigned)ceil_div(P * K, 256)), dim3(256), 0, ctx().stream, e->Xa.as<double>(),
                     (int)e->A, perms_dev, (int)K, pi_dev, pj_dev, P, rmsd_dev, maxdev_dev);
  return check_launch("k_symm_pairs");
}

__global__ void k_warm_symm() {}
int warm_symm() {
  hipLaunchKernelGGL(k_warm_symm, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_symm");
}

}  // namespace fc
