// fc_diverse.hip -- RMSD-diverse conformer selection (greedy max-min, farthest point, Gonzalez k-center) over a
// resident ensemble, for gfx950 (wave64, float64).
//
// The contract (include/fc_hip.h, fc_ensemble_select_diverse) -- d(i, j) is the heavy-atom Kabsch
// RMSD of the ensemble, the value fc_ensemble_rmsd_pairs returns for the pair (i, j):
//
//   s[0] = start;  D[j] = d(s0, j);  D[s0] = 0;  L[j] = 0;  radius[0] = +inf
//   for k = 1 .. n_max-1, while fewer than N are selected:
//       m   = max D[j] over the conformers not yet selected;  s_k = the smallest such j with D[j] == m
//       if stop_rmsd >= 0 and m <= stop_rmsd: stop
//       radius[k] = m;  D[s_k] = 0;  L[s_k] = k
//       for all j: t = d(s_k, j); if t < D[j]: D[j] = t; L[j] = k      (strict: ties keep the earlier representative)
//
// One launch of k_diverse_step per selection step k, plain launches on the library's stream (no grid barrier, no graph):
//   1. every workgroup reduces the per-workgroup (max D, index) partials the previous step left -- a few hundred values,
//      read after the kernel boundary -- to s_k and m, redundantly (no hand-off inside a launch); workgroup 0 records
//      indices[k] and radii[k].  The partials are double-buffered by the parity of k.
//   2. s_k's selected atoms (the centred conformer-major copy Xa) are staged in LDS, and every conformer j of the
//      workgroup is aligned against them -- pair_exact_aos (fc_kabsch.hip) with s_k as p and j as q: covariance,
//      rotation, the explicit rotated difference (no max-deviation pass); the rotation by kabsch_rotation_qcp (Newton
//      eigenvalue + adjugate eigenvector, ~300 flops) with the Jacobi sweeps of kabsch_rotation (~7 000) where the
//      eigenvalue is not clearly simple, as the prune's refine does; the conformer's coordinates read from the
//      conformer-minor Xs so that lanes over conformers load coalesced -- and D, L updated.
//   3. the workgroup's partial max over the conformers it owns that are not selected, compared lexicographically on
//      (value, -index) so that the result does not depend on the order of the reduction; padding lanes take no part.
// A device word ends the selection (radius stop): later launches return at once.
//
// Lanes per conformer: 8 up to kDiverseLanes8MaxN conformers (fc_tuning.h) -- the atom loops split over 8 lanes and the
// nine covariance sums and the squared deviation meet through xor shuffles inside the 8-lane group, as in
// pair_exact_group8 -- so that 10^4 conformers fill 1 250 wavefronts instead of 157; 1 lane above it.  Both forms give
// fc_ensemble_rmsd_pairs' values (Jacobi rotation, pair_exact_aos's order of the sums) within a few ulp: the rmsd is
// stationary in the rotation at the optimum, so the QCP rotation's last bits reach it only at second order.
//
// Limits: the representative's A x 24 bytes are staged in LDS up to kDiverseLdsAtoms atoms (48 KiB); beyond that the
// same kernel reads them from global memory (k_diverse_step<.., false>): no size limit of its own besides N < 2^31.
//
// k_diverse_step_sym (further down) is the same step under the smallest rmsd over a table of atom permutations and,
// optionally, both handednesses (fc_ensemble_select_diverse_perm); the host loop is shared, and so
// are parts 1 and 3 and the D / L update (div_pick_rep, div_update, div_write_partial, above the kernels).  The two atom
// loops of part 2 stay written out in each kernel: as shared __forceinline__ functions they compiled to the same
// instruction counts and registers but measured 0.4 % (8 lanes) to 10 % (1 lane, 10^5 conformers, 8 permutations) slower
// per step (tools/bench_diverse.py, tools/bench_diverse_sym.py; docs/rmsd_tile_measurements.md: the parent's spread
// there is 0.2 ... 0.4 %).  One or eight lanes per conformer against one
// representative: not fc_rmsd_tile.h's row tile.
#include "fc_internal.h"
#include "fc_kabsch_math.h"

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>

namespace fc {

constexpr int kDivThreads = 256;
constexpr int64_t kDiverseLdsAtoms = 2048;  // A x 24 B = 48 KiB of LDS for the representative

// (v1, i1) comes before (v2, i2): larger value first, lower index on ties
__device__ __forceinline__ bool div_better(double v1, int i1, double v2, int i2) {
  return v1 > v2 || (v1 == v2 && i1 < i2);
}

__device__ __forceinline__ void div_wave_argmax(double &v, int &i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (div_better(ov, oi, v, i)) v = ov, i = oi;
  }
}

// block-wide lexicographic argmax; every thread of the workgroup gets the result
__device__ __forceinline__ void div_block_argmax(double &v, int &i, double *s_v, int *s_i) {
  div_wave_argmax(v, i);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // (s_v / s_i may still be read from a previous use)
  if ((threadIdx.x & 63) == 0) s_v[w] = v, s_i[w] = i;
  __syncthreads();
  v = s_v[0], i = s_i[0];
#pragma unroll
  for (int k = 1; k < kDivThreads / 64; ++k)
    if (div_better(s_v[k], s_i[k], v, i)) v = s_v[k], i = s_i[k];
}

__device__ __forceinline__ double div_group8_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// Part 1 of a step: the representative s of this step, from the partials the previous step left.  false: the selection
// has ended and the whole workgroup returns.  state[0]: 1 once the radius stop was met; state[1]: number of
// representatives selected
__device__ __forceinline__ bool div_pick_rep(int k, int start, double stop_rmsd, int n_steps, const double *part_v,
                                             const int32_t *part_i, int nb, int64_t *idx_out, double *rad_out, int64_t *state,
                                             double *s_v, int *s_i, int *s_stop, int &s) {
  const int tid = threadIdx.x;
  s = start;
  if (k > 0) {
    // the radius stop was met at an earlier step.  ONE read per workgroup, shared by all its waves: workgroup 0 of the
    // launch that meets the stop writes the word while other workgroups of that launch start, and waves that each read
    // it could disagree -- those that returned would leave their slots of the block reduction below unwritten
    if (tid == 0) *s_stop = *(volatile int64_t *)state != 0;
    __syncthreads();
    if (*s_stop) return false;
    const double *__restrict__ pv = part_v + (size_t)((k - 1) & 1) * nb;
    const int32_t *__restrict__ pi = part_i + (size_t)((k - 1) & 1) * nb;
    double m = -1.0;
    int mi = INT_MAX;
    for (int b = tid; b < nb; b += kDivThreads)
      if (div_better(pv[b], pi[b], m, mi)) m = pv[b], mi = pi[b];
    div_block_argmax(m, mi, s_v, s_i);
    if (mi == INT_MAX || (stop_rmsd >= 0.0 && m <= stop_rmsd)) {  // (no conformer left: the host never asks for that)
      if (blockIdx.x == 0 && tid == 0) state[0] = 1, state[1] = k;
      return false;
    }
    if (blockIdx.x == 0 && tid == 0) idx_out[k] = mi, rad_out[k] = m;
    s = mi;
  } else if (blockIdx.x == 0 && tid == 0) {
    idx_out[0] = start, rad_out[0] = INFINITY;
    state[0] = 0, state[1] = n_steps;
  }
  return true;
}

// D, L and is_rep of conformer j, at distance t from this step's representative, and the lane's candidate for the next
// step's max: the updated D[j] (strict: ties keep the earlier representative).  One lane per conformer calls it.
__device__ __forceinline__ void div_update(int k, int j, double t, double *D, int32_t *L, uint8_t *is_rep, double &cand,
                                           int &cand_i) {
  double d = t;
  if (k == 0) {
    D[j] = t, L[j] = 0, is_rep[j] = 0;
  } else {
    d = D[j];
    if (t < d) D[j] = t, L[j] = k, d = t;
  }
  cand = d, cand_i = j;
}

// Part 3 of a step: this workgroup's partial for the next step
__device__ __forceinline__ void div_write_partial(int k, double cand, int cand_i, double *part_v, int32_t *part_i, int nb,
                                                  double *s_v, int *s_i) {
  div_block_argmax(cand, cand_i, s_v, s_i);
  if (threadIdx.x == 0) {
    part_v[(size_t)(k & 1) * nb + blockIdx.x] = cand;
    part_i[(size_t)(k & 1) * nb + blockIdx.x] = cand_i;
  }
}

template <int LANES, bool STAGE>
__global__ void __launch_bounds__(kDivThreads)
k_diverse_step(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ G, int N, int64_t Npad, int A, int k,
               int start, double stop_rmsd, int n_steps, double *__restrict__ D, int32_t *__restrict__ L,
               uint8_t *__restrict__ is_rep, double *__restrict__ part_v, int32_t *__restrict__ part_i, int nb,
               int64_t *__restrict__ idx_out, double *__restrict__ rad_out, int64_t *__restrict__ state) {
  static_assert(LANES == 1 || LANES == 8, "one or eight lanes per conformer");
  extern __shared__ double s_rep[];  // [A][3] when STAGE
  __shared__ double s_v[kDivThreads / 64];
  __shared__ int s_i[kDivThreads / 64];
  __shared__ int s_stop;
  const int tid = threadIdx.x;

  // ---- 1. the representative of this step
  int s;
  if (!div_pick_rep(k, start, stop_rmsd, n_steps, part_v, part_i, nb, idx_out, rad_out, state, s_v, s_i, &s_stop, s)) return;

  // ---- 2. align s against every conformer of this workgroup
  const double *__restrict__ P;
  if (STAGE) {
    const double *__restrict__ src = Xa + (int64_t)s * A * 3;
    for (int t = tid; t < 3 * A; t += kDivThreads) s_rep[t] = src[t];
    __syncthreads();
    P = s_rep;
  } else {
    P = Xa + (int64_t)s * A * 3;
  }
  constexpr int kPerBlock = kDivThreads / LANES;
  const int sub = LANES == 1 ? 0 : (tid & (LANES - 1));
  const int j = blockIdx.x * kPerBlock + tid / LANES;
  double cand = -1.0;  // this lane's candidate for the next step's max: the updated D[j] of an unselected conformer
  int cand_i = INT_MAX;
  if (j < N) {  // (uniform over the LANES lanes of a conformer: the shuffles below stay inside active groups)
    if (j == s) {
      if (sub == 0) D[j] = 0.0, L[j] = k, is_rep[j] = 1;
    } else if (k == 0 || !is_rep[j]) {
      double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int a = sub; a < A; a += LANES) {
        const double *__restrict__ qa = Xs + (int64_t)(a * 3) * Npad + j;
        const double px = P[a * 3], py = P[a * 3 + 1], pz = P[a * 3 + 2];
        const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
        B[0] = fma(px, qx, B[0]); B[1] = fma(px, qy, B[1]); B[2] = fma(px, qz, B[2]);
        B[3] = fma(py, qx, B[3]); B[4] = fma(py, qy, B[4]); B[5] = fma(py, qz, B[5]);
        B[6] = fma(pz, qx, B[6]); B[7] = fma(pz, qy, B[7]); B[8] = fma(pz, qz, B[8]);
      }
      if (LANES > 1) {
#pragma unroll
        for (int e = 0; e < 9; ++e) B[e] = div_group8_sum(B[e]);
      }
      // rotation: Newton eigenvalue + adjugate eigenvector where the eigenvalue is clearly simple, the Jacobi sweeps
      // otherwise (identical in the lanes of a group: xor sums are)
      double R[9];
      if (!kabsch_rotation_qcp(B, G[s] + G[j], R)) (void)kabsch_rotation(B, R);
      double ssq = 0.0;
      for (int a = sub; a < A; a += LANES) {
        const double *__restrict__ qa = Xs + (int64_t)(a * 3) * Npad + j;
        const double px = P[a * 3], py = P[a * 3 + 1], pz = P[a * 3 + 2];
        const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
        const double dx = px - (R[0] * qx + R[1] * qy + R[2] * qz);
        const double dy = py - (R[3] * qx + R[4] * qy + R[5] * qz);
        const double dz = pz - (R[6] * qx + R[7] * qy + R[8] * qz);
        ssq += dx * dx + dy * dy + dz * dz;
      }
      if (LANES > 1) ssq = div_group8_sum(ssq);
      const double t = sqrt(ssq / (double)A);
      if (sub == 0) div_update(k, j, t, D, L, is_rep, cand, cand_i);
    }
  }

  // ---- 3. this workgroup's partial for the next step
  div_write_partial(k, cand, cand_i, part_v, part_i, nb, s_v, s_i);
}

// ---------------------------------------------------------------------------
// k_diverse_step_sym: the step under d_sym (include/fc_hip.h, fc_ensemble_select_diverse_perm)
//
//   d_sym(s, j) = min over k < K, h in H of rmsd(X[s], h * X[j][perms[k]]),   H = {+1} or, MIRROR, {+1, -1}
//
// The three parts of k_diverse_step, with part 2 walking the table.  The representative AND the table (16-bit indices)
// sit in LDS and the permutation is applied to the representative: sum_a p_a q_pi(a)^T = sum_b p_pi^-1(b) q_b^T and the
// table is closed under inverse, so the minimum over "rows applied to s" is the minimum the contract names, a
// permutation costs an LDS address, and the conformer is still read coalesced from the conformer-minor Xs.
// Per conformer and row k: the covariance B_k (the only atom loop every (pair, k) pays), the Newton eigenvalue of B_k
// and -- MIRROR -- of -B_k (kabsch_lambda_max_both), and for each h the rotation and the explicit deviation pass
// UNLESS the eigenvalue form of its msd, (Gs + Gj - 2 lambda)/A, exceeds the smallest explicit msd seen so far for this
// conformer by more than kScreenMargin (1e-6 A^2: the eigenvalue form is good to ~1e-11 of G/A where the iteration
// has settled on its largest root, a simple one; on a (nearly) double root it may end anywhere, and
// kabsch_lambda_max_both then gives the upper bound (Gs + Gj)/2 -- an msd of 0, which leaves nothing out).  A (k, h)
// left out is therefore not the minimum; the value kept is the explicit sum of the winning (k, h), h = -1 as
// pair_exact_aos<INV> forms it: -B, p + R q.
// The rows are taken in table order against a running best -- not sorted by eigenvalue: that would keep 2 K
// eigenvalues per lane.  Row 0 is the identity, the winner for every conformer that was not relabelled.
// stats (may be NULL): [0] += (k, h) whose eigenvalue was formed, [1] += those that reached the explicit pass.
// ---------------------------------------------------------------------------
constexpr size_t kDiverseSymStaticLds = 64;  // s_v, s_i, s_stop below: 52 bytes, rounded

size_t diverse_sym_lds_bytes(int64_t A, int64_t K) {
  return (size_t)A * 3 * sizeof(double) + (((size_t)K * (size_t)A * sizeof(uint16_t) + 7) & ~(size_t)7) + kDiverseSymStaticLds;
}

template <int LANES, bool MIRROR>
__global__ void __launch_bounds__(kDivThreads)
k_diverse_step_sym(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ G, int N, int64_t Npad,
                   int A, const uint16_t *__restrict__ perms, int K, int k, int start, double stop_rmsd, int n_steps,
                   double *__restrict__ D, int32_t *__restrict__ L, uint8_t *__restrict__ is_rep, double *__restrict__ part_v,
                   int32_t *__restrict__ part_i, int nb, int64_t *__restrict__ idx_out, double *__restrict__ rad_out,
                   int64_t *__restrict__ state, unsigned long long *__restrict__ stats) {
  static_assert(LANES == 1 || LANES == 8, "one or eight lanes per conformer");
  extern __shared__ double s_sym[];  // [A][3] of the representative, then the table [K][A] as uint16_t
  __shared__ double s_v[kDivThreads / 64];
  __shared__ int s_i[kDivThreads / 64];
  __shared__ int s_stop;
  static_assert(sizeof s_v + sizeof s_i + sizeof s_stop <= kDiverseSymStaticLds, "diverse_sym_lds_bytes counts less");
  const int tid = threadIdx.x;

  // ---- 1. the representative of this step
  int s;
  if (!div_pick_rep(k, start, stop_rmsd, n_steps, part_v, part_i, nb, idx_out, rad_out, state, s_v, s_i, &s_stop, s)) return;

  // ---- 2. align s, under every row of the table and either handedness, against every conformer of this workgroup
  uint16_t *pt = reinterpret_cast<uint16_t *>(s_sym + 3 * A);
  {
    const double *__restrict__ src = Xa + (int64_t)s * A * 3;
    for (int t = tid; t < 3 * A; t += kDivThreads) s_sym[t] = src[t];
    for (int t = tid; t < K * A; t += kDivThreads) pt[t] = perms[t];
    __syncthreads();
  }
  const double *__restrict__ P = s_sym;
  constexpr int kPerBlock = kDivThreads / LANES;
  const int sub = LANES == 1 ? 0 : (tid & (LANES - 1));
  const int j = blockIdx.x * kPerBlock + tid / LANES;
  double cand = -1.0;
  int cand_i = INT_MAX;
  unsigned n_formed = 0, n_explicit = 0;
  if (j < N) {  // (uniform over the LANES lanes of a conformer, and so is every branch below: xor sums are)
    if (j == s) {
      if (sub == 0) D[j] = 0.0, L[j] = k, is_rep[j] = 1;
    } else if (k == 0 || !is_rep[j]) {
      const double Gs = G[s] + G[j];
      const double margin = (double)A * kScreenMargin;
      double best = INFINITY;  // the smallest explicit sum of squares so far
      for (int r = 0; r < K; ++r) {
        const uint16_t *__restrict__ pr = pt + r * A;
        double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int a = sub; a < A; a += LANES) {
          const double *__restrict__ qa = Xs + (int64_t)(a * 3) * Npad + j;
          const int b = (int)pr[a] * 3;
          const double px = P[b], py = P[b + 1], pz = P[b + 2];
          const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
          B[0] = fma(px, qx, B[0]); B[1] = fma(px, qy, B[1]); B[2] = fma(px, qz, B[2]);
          B[3] = fma(py, qx, B[3]); B[4] = fma(py, qy, B[4]); B[5] = fma(py, qz, B[5]);
          B[6] = fma(pz, qx, B[6]); B[7] = fma(pz, qy, B[7]); B[8] = fma(pz, qz, B[8]);
        }
        if (LANES > 1) {
#pragma unroll
          for (int e = 0; e < 9; ++e) B[e] = div_group8_sum(B[e]);
        }
        double lam_p, lam_m = 0.0;
        kabsch_lambda_max_both<MIRROR>(B, Gs, lam_p, lam_m);
#pragma nounroll
        for (int h = 0; h < (MIRROR ? 2 : 1); ++h) {
          ++n_formed;
          if (Gs - 2.0 * (h ? lam_m : lam_p) > best + margin) continue;  // (a NaN goes on to the explicit pass)
          ++n_explicit;
          const double sg = h ? -1.0 : 1.0;
          double Bh[9], R[9];
#pragma unroll
          for (int e = 0; e < 9; ++e) Bh[e] = sg * B[e];
          if (!kabsch_rotation_qcp(Bh, Gs, R)) (void)kabsch_rotation(Bh, R);
          double ssq = 0.0;
          for (int a = sub; a < A; a += LANES) {
            const double *__restrict__ qa = Xs + (int64_t)(a * 3) * Npad + j;
            const int b = (int)pr[a] * 3;
            const double px = P[b], py = P[b + 1], pz = P[b + 2];
            const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
            const double dx = px - sg * (R[0] * qx + R[1] * qy + R[2] * qz);
            const double dy = py - sg * (R[3] * qx + R[4] * qy + R[5] * qz);
            const double dz = pz - sg * (R[6] * qx + R[7] * qy + R[8] * qz);
            ssq += dx * dx + dy * dy + dz * dz;
          }
          if (LANES > 1) ssq = div_group8_sum(ssq);
          if (!(ssq >= best)) best = ssq;
        }
      }
      const double t = sqrt(best / (double)A);
      if (sub == 0) div_update(k, j, t, D, L, is_rep, cand, cand_i);
      else n_formed = n_explicit = 0;  // (counted once per conformer)
    }
  }
  if (stats != nullptr) {  // (uniform: a bench hook's counters)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_formed += __shfl_xor(n_formed, o), n_explicit += __shfl_xor(n_explicit, o);
    if ((tid & 63) == 0 && n_formed) {
      atomicAdd(&stats[0], (unsigned long long)n_formed);
      atomicAdd(&stats[1], (unsigned long long)n_explicit);
    }
  }

  // ---- 3. this workgroup's partial for the next step
  div_write_partial(k, cand, cand_i, part_v, part_i, nb, s_v, s_i);
}

int diverse_lanes(int64_t N) {  // lanes per conformer of the step kernel at N conformers (fc_bench_select_diverse reports it)
  if (const char *v = getenv("FC_DIVERSE_LANES")) {  // a measurement of the two forms at one size (tools/bench_diverse.py)
    if (v[0] == '1' && v[1] == 0) return 1;
    if (v[0] == '8' && v[1] == 0) return 8;
  }
  return N <= kDiverseLanes8MaxN ? 8 : 1;
}

template <int LANES, bool STAGE>
static int launch_step(const fc_ensemble *e, int k, int start, double stop, int n_steps, DevBuf &D, DevBuf &L,
                       DevBuf &rep, DevBuf &pv, DevBuf &pi, int nb, DevBuf &idx, DevBuf &rad, DevBuf &state) {
  const size_t lds = STAGE ? (size_t)e->A * 3 * sizeof(double) : 0;
  hipLaunchKernelGGL((k_diverse_step<LANES, STAGE>), dim3((unsigned)nb), dim3(kDivThreads), lds, ctx().stream,
                     e->Xs.as<double>(), e->Xa.as<double>(), e->G.as<double>(), (int)e->N, e->Npad, (int)e->A, k, start, stop, n_steps,
                     D.as<double>(), L.as<int32_t>(), rep.as<uint8_t>(), pv.as<double>(), pi.as<int32_t>(), nb,
                     idx.as<int64_t>(), rad.as<double>(), state.as<int64_t>());
  return check_launch("k_diverse_step");
}

template <int LANES, bool MIRROR>
static const void *step_sym_kernel() {
  return reinterpret_cast<const void *>(k_diverse_step_sym<LANES, MIRROR>);
}

template <int LANES, bool MIRROR>
static int launch_step_sym(const fc_ensemble *e, const SymTable &sym, int k, int start, double stop, int n_steps, DevBuf &D,
                           DevBuf &L, DevBuf &rep, DevBuf &pv, DevBuf &pi, int nb, DevBuf &idx, DevBuf &rad, DevBuf &state) {
  const size_t lds = diverse_sym_lds_bytes(e->A, sym.K) - kDiverseSymStaticLds;
  hipLaunchKernelGGL((k_diverse_step_sym<LANES, MIRROR>), dim3((unsigned)nb), dim3(kDivThreads), lds, ctx().stream,
                     e->Xs.as<double>(), e->Xa.as<double>(), e->G.as<double>(), (int)e->N, e->Npad, (int)e->A, sym.perms_dev,
                     sym.K, k, start, stop, n_steps, D.as<double>(), L.as<int32_t>(), rep.as<uint8_t>(), pv.as<double>(),
                     pi.as<int32_t>(), nb, idx.as<int64_t>(), rad.as<double>(), state.as<int64_t>(), sym.stats_dev);
  return check_launch("k_diverse_step_sym");
}

// The selection behind fc_ensemble_select_diverse (arguments checked there; N >= 1, 1 <= n_max, 0 <= start < N).
// stop_rmsd < 0: n_max steps enqueued at once, one host wait at the end; otherwise batches of kDiverseBatch steps and
// a read of the stop word behind each.  ms_device (may be NULL): HIP-event time from the first launch to the last.
// sym (may be NULL): the steps are k_diverse_step_sym's (fc_ensemble_select_diverse_perm, which has checked that the
// representative and the table fit the LDS).
int select_diverse(fc_ensemble *e, int64_t n_max, int64_t start, double stop_rmsd, int64_t *indices_out,
                   double *radii_out, int32_t *labels_out, double *dist_out, int64_t *n_selected, double *ms_device,
                   const SymTable *sym) {
  constexpr int kDiverseBatch = 64;
  const int64_t N = e->N;
  const int n_steps = (int)std::min<int64_t>(n_max, N);
  const int lanes = diverse_lanes(N);
  const bool stage = e->A <= kDiverseLdsAtoms;
  const int nb = (int)ceil_div(N, kDivThreads / lanes);
  if (sym) {
    const size_t lds = diverse_sym_lds_bytes(e->A, sym->K);
    if (lds > kLdsLimit)
      return set_error(FC_E_LIMIT, "A_sel=%lld selected atoms with K=%lld permutations need %zu bytes of LDS (limit %zu)",
                       (long long)e->A, (long long)sym->K, lds, kLdsLimit);
    const void *fn = lanes == 8 ? (sym->mirror ? step_sym_kernel<8, true>() : step_sym_kernel<8, false>())
                                : (sym->mirror ? step_sym_kernel<1, true>() : step_sym_kernel<1, false>());
    FC_TRY(allow_dynamic_lds(fn, lds - kDiverseSymStaticLds, "k_diverse_step_sym"));
  }
  DevBuf D, L, rep, pv, pi, idx, rad, state;
  FC_TRY(D.reserve((size_t)N * sizeof(double)));
  FC_TRY(L.reserve((size_t)N * sizeof(int32_t)));
  FC_TRY(rep.reserve((size_t)N));
  FC_TRY(pv.reserve((size_t)2 * nb * sizeof(double)));
  FC_TRY(pi.reserve((size_t)2 * nb * sizeof(int32_t)));
  FC_TRY(idx.reserve((size_t)n_steps * sizeof(int64_t)));
  FC_TRY(rad.reserve((size_t)n_steps * sizeof(double)));
  FC_TRY(state.reserve(2 * sizeof(int64_t)));
  Context &c = ctx();
  if (ms_device) FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  int64_t st[2] = {0, n_steps};
  for (int k = 0; k < n_steps;) {
    const int k_end = stop_rmsd < 0.0 ? n_steps : std::min(n_steps, k + kDiverseBatch);
    for (; k < k_end; ++k) {
      int rc;
      if (sym && lanes == 8)
        rc = sym->mirror ? launch_step_sym<8, true>(e, *sym, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state)
                         : launch_step_sym<8, false>(e, *sym, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state);
      else if (sym)
        rc = sym->mirror ? launch_step_sym<1, true>(e, *sym, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state)
                         : launch_step_sym<1, false>(e, *sym, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state);
      else if (lanes == 8)
        rc = stage ? launch_step<8, true>(e, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state)
                   : launch_step<8, false>(e, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state);
      else
        rc = stage ? launch_step<1, true>(e, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state)
                   : launch_step<1, false>(e, k, (int)start, stop_rmsd, n_steps, D, L, rep, pv, pi, nb, idx, rad, state);
      FC_TRY(rc);
    }
    if (ms_device) FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));  // (the last batch's record is the one read)
    FC_HIP_TRY(hipMemcpyAsync(st, state.p, sizeof st, hipMemcpyDeviceToHost, c.stream));
    FC_TRY(sync());
    if (st[0]) break;
  }
  const int64_t K = st[1];
  FC_TRY(d2h(indices_out, idx.p, (size_t)K * sizeof(int64_t)));
  if (radii_out) FC_TRY(d2h(radii_out, rad.p, (size_t)K * sizeof(double)));
  if (labels_out) FC_TRY(d2h(labels_out, L.p, (size_t)N * sizeof(int32_t)));
  if (dist_out) FC_TRY(d2h(dist_out, D.p, (size_t)N * sizeof(double)));
  FC_TRY(sync());
  if (ms_device) {
    float ms = 0.0f;
    FC_HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    *ms_device = ms;
  }
  *n_selected = K;
  return FC_OK;
}

__global__ void k_warm_diverse() {}
int warm_diverse() {
  hipLaunchKernelGGL(k_warm_diverse, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_diverse");
}

}  // namespace fc
