// fc_knn.hip -- k nearest neighbours of every conformer under the ensemble's Kabsch RMSD, over a resident ensemble and
// without an N x N matrix, for gfx950 (wave64, float64).
//
// The contract (include/fc_hip.h, fc_ensemble_knn) -- d(i, j) is the heavy-atom Kabsch RMSD of the
// ensemble, the d of the diverse selection (fc_diverse.hip):
//
//   for every conformer i: the k conformers j != i with the smallest d(i, j), in ascending order of (d(i, j), j) --
//   equal distances: the lower index first, inside the list and at its cut; slots beyond N - 1: index -1, distance +inf.
//
// k_knn_tile -- grid: row tiles x column strips.  The tile is fc_rmsd_tile.h's: a workgroup takes 16 rows, each WAVEFRONT
// owns 4 of them and walks the strip's columns 64 at a time, one lane per column conformer:
//   1. the covariances of the column with the 4 rows in one atom loop (tile_covariance);
//   2. per row, the filter: the Newton eigenvalue of the covariance gives A msd = (Gi + Gj) - 2 lambda, never above the
//      explicit sum by more than rounding WHERE THE ITERATION HAS SETTLED ON ITS LARGEST ROOT, A SIMPLE ONE
//      (kabsch_lambda_is_settled certifies that); on a (nearly) double root -- atoms on a line, two atoms, a symmetric
//      top against its mirror image -- it ends on either side of the root, or on another root altogether, and such a
//      pair is not ruled out (kabsch_lambda_upper gives A msd = 0 for it).  When A msd exceeds A tau^2 -- tau the
//      row's current k-th distance -- by more than the margin for EVERY column of the chunk, none of them can enter
//      the row's list and the rest of the row is skipped (wave-uniform).  The eigenvalue decides nothing else: FC_KNN_FILTER=0 takes every pair through step 3 and gives
//      the same bits;
//   3. otherwise the rotation and the explicit rotated difference in a second atom loop (tile_rmsd): the value that is
//      written out is never the eigenvalue form, which cancels for near neighbours;
//   4. lanes whose (d, j) comes before the row's current k-th entry are found by a ballot and inserted one at a time
//      into the row's running list.
// The running list of a row is a sorted top-64 held ONE SLOT PER LANE in the registers of the wavefront that owns the
// row (4 rows: 12 registers): an insertion is a ballot (the position), one shift by a lane and a select; the threshold
// is slot k - 1.  A row's list within a strip has one owner, so nothing is shared between wavefronts: no atomics, no
// order dependence.  The full square is computed, not the triangle -- d(i, j) is evaluated once as (row i, column j) and
// once as (row j, column i), twice the arithmetic -- for exactly that reason: a triangular form would hand each distance to
// two lists owned by different workgroups.
// d(i, j) is one fixed instruction sequence over the atoms in order: it does not depend on the tile, the strip or the
// lane a pair falls into (rows and columns past the end are computed as copies of conformer N - 1 and dropped), so two
// columns with bitwise-identical coordinates give bitwise-identical distances in a row, and the outputs are the same
// bits for every strip count.
//
// Each (row, strip) writes its sorted partial list; k_knn_merge -- one wavefront per row -- offers the S partial lists
// of the row to one list by the same insertion and writes the outputs (-1 for the unfilled slots).  The entries of a
// row are distinct in j, so the merged list does not depend on the order of the strips.
//
// The cross form (fc_ensemble_knn_cross) is the same kernel with its rows from one resident
// ensemble Q (Xa, G, N) and its columns from another, R (Xs, G, N, Npad): for every conformer of Q its k nearest conformers
// of R.  No pair is left out, every clamp is per side, the tiles come from Nq and the chunks and strips from Nr.  An
// optional cap keeps only d < max_rmsd: the test is made on the value, beside the list, and the filter's tau is the
// smaller of slot k - 1 and the cap from the first chunk on -- whole chunks are ruled out before any list has filled.
// d(i, j) is the same instruction sequence in both forms: an ensemble against a bitwise copy of itself gives the
// distance bits of the one-ensemble form for every i != j.
//
// The symmetry- and mirror-aware forms (fc_ensemble_knn_perm, fc_ensemble_knn_cross_perm) are
// k_knn_tile_sym, further down: the same tiles, strips, lists and merge under
//   d_sym(i, j) = min over p < K, h in H of rmsd(Q[i], h * R[j][perms[p]]),   H = {+1} or {+1, -1}
// with a (pair, p, h) taken through the explicit pass unless its eigenvalue rules it out -- by tau as above, or by the
// pair's smallest explicit sum so far.
// Why the outputs are the same bits with the filter on or off and for every strip count.  The explicit sum of a
// (pair, p, h) is one fixed instruction sequence, so the pair has a fixed smallest explicit sum, that of its argmin
// (p*, h*); the value offered is the minimum over the explicit sums that were VISITED, hence that sum whenever (p*, h*)
// is visited.  (1) The eigenvalue form of (p*, h*) never exceeds its explicit sum by more than rounding (it is used only
// where it is certified as the largest root, and is 0 elsewhere: kabsch_lambda_max_both; the margins cover the
// rounding), and every other explicit sum of the pair is at least as large: (p*, h*) is never above the running best,
// so only tau can rule it out.  (2) When tau rules it out,
// d_sym > tau; whatever else of the pair was visited has an explicit sum >= that of (p*, h*), so the value offered is
// above tau as well and is not inserted (nor under the cap) -- and tau only shrinks, so the pair is in no final list.
// (3) A pair that belongs in the final list has d_sym <= every tau its row ever had in any strip, so (p*, h*) is
// visited and the exact bits are offered.  Visiting MORE (other lanes of the ballot, the filter off) changes no minimum.
#include "fc_rmsd_tile.h"

#include <climits>

namespace fc {

static_assert(FC_KNN_MAX == 64, "a row's list is one slot per lane of a wavefront");
// The filter's margin on A * msd, beside A * kScreenMargin: the eigenvalue form (Gp + Gq) - 2 lambda and the explicit sum
// differ by the rounding of G, of the covariance and of Newton's last step, a few (2 A + 10) u (Gp + Gq) -- 7e-12 of
// (Gp + Gq) at the 32 767 atoms a conformer can have -- and by what a settled iteration can be away from its root,
// 1.1e-11 (Gp + Gq) (kabsch_lambda_is_settled)
constexpr double kKnnFilterRel = 1e-10;

// (d1, j1) comes before (d2, j2): smaller distance first, lower index on ties
__device__ __forceinline__ bool knn_before(double d1, int j1, double d2, int j2) {
  return d1 < d2 || (d1 == d2 && j1 < j2);
}

// Offer each lane's (d, j) -- where ok -- to a row's list: (ld, lj) is this lane's slot of the sorted top-64, (td, tj)
// slot k - 1, the threshold.  Called by all 64 lanes.  Survivors are taken in lane order, each re-tested against the
// threshold the insertions before it left.
__device__ __forceinline__ void knn_offer(double &ld, int &lj, double &td, int &tj, double d, int j, bool ok, int k,
                                          int lane) {
  for (;;) {
    const unsigned long long m = __ballot(ok && knn_before(d, j, td, tj));
    if (m == 0) break;
    const int src = __ffsll((long long)m) - 1;
    const double nd = __shfl(d, src);
    const int nj = __shfl(j, src);
    const int pos = __popcll(__ballot(knn_before(ld, lj, nd, nj)));  // the list is sorted: entries before the new one
    const double pd = __shfl_up(ld, 1);
    const int pj = __shfl_up(lj, 1);
    if (lane == pos) ld = nd, lj = nj;
    else if (lane > pos) ld = pd, lj = pj;
    if (lane == src) ok = false;
    td = __shfl(ld, k - 1);
    tj = __shfl(lj, k - 1);
  }
}

// What the cross form (rows from an ensemble Q, columns from an ensemble R) passes beside the arguments of the
// one-ensemble form, which then describe: Xs, Npad -- R; Xa, G, N -- Q.  The one-ensemble form passes an empty struct
// at the end, so that its own arguments and its code stay as they were.
template <bool CROSS>
struct KnnCross {};
template <>
struct KnnCross<true> {
  const double *Gr;  // R's sums of squares
  int Nr;            // R's conformers
  double cap;        // a list takes only d < cap; +inf: no cap
};

// CROSS = false: one ensemble, the self-pair left out by index.  CROSS = true: no pair left out, the cap.
template <bool STAGE, bool CROSS>
__global__ void __launch_bounds__(kTileThreads)
k_knn_tile(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ Gq, int Nq, int64_t Npad, int A,
           int k, int filter, int n_tiles, int n_chunks, double *__restrict__ part_d, int32_t *__restrict__ part_j,
           const KnnCross<CROSS> x) {
  const double *__restrict__ Gr;
  int Nr;
  double cap;
  if constexpr (CROSS) Gr = x.Gr, Nr = x.Nr, cap = x.cap;
  else Gr = Gq, Nr = Nq, cap = INFINITY;
  extern __shared__ double s_rows[];  // [kTileRows][A][3] when STAGE
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int S = gridDim.y, s = blockIdx.y;
  // the strip's chunks of 64 columns
  const int c0 = (int)((int64_t)s * n_chunks / S), c1 = (int)((int64_t)(s + 1) * n_chunks / S);
  const int A3 = 3 * A;
  const double dA = (double)A;

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * kTileRows;
    if (STAGE) tile_stage_rows(s_rows, Xa, row0, Nq, A3);
    const int wrow = row0 + w * kTileR;
    if (wrow < Nq) {  // (wave-uniform)
      int row[kTileR];
      const double *__restrict__ P[kTileR];
      double Gi[kTileR], ld[kTileR], td[kTileR];
      int lj[kTileR], tj[kTileR];
      tile_rows<STAGE>(s_rows, Xa, Gq, row0, wrow, Nq, A3, row, P, Gi);
#pragma unroll
      for (int r = 0; r < kTileR; ++r) {
        ld[r] = td[r] = INFINITY;
        lj[r] = tj[r] = INT_MAX;
      }
      for (int c = c0; c < c1; ++c) {
        const int j = c * 64 + lane;
        const int jl = min(j, Nr - 1);
        const double *__restrict__ q0 = Xs + jl;
        // ---- 1. covariances with the 4 rows
        double B[kTileR][9];
        tile_covariance(P, q0, Npad, A, TileNoPerm{}, B);
        // ---- 2. per row: the filter, and where a lane passes it the rotation, the explicit rotated difference and the list
        const double Gj = Gr[jl];
#pragma unroll
        for (int r = 0; r < kTileR; ++r) {
          const bool ok = j < Nr && (CROSS || j != row[r]) && row[r] < Nq;  // one ensemble: the self-pair is left out by index
          const double GG = Gi[r] + Gj;
          bool may = ok;
          if (filter) {  // (a NaN passes)
            const double msdA = GG - 2.0 * kabsch_lambda_upper(B[r], GG);  // (0 where the eigenvalue cannot be trusted)
            const double tau = CROSS ? fmin(td[r], cap) : td[r];  // the cap: a smaller tau from the first chunk on
            may = ok && !(msdA > dA * tau * tau + (dA * kScreenMargin + kKnnFilterRel * GG));
          }
          if (__ballot(may) == 0) continue;  // (wave-uniform) no column of this chunk can enter the row's list
          const double d = tile_rmsd(P[r], q0, Npad, A, B[r], GG, dA);
          // (the cap is tested on the value itself, beside the list: slot k - 1, which knn_offer re-reads, never holds it)
          knn_offer(ld[r], lj[r], td[r], tj[r], d, j, CROSS ? ok && d < cap : ok, k, lane);
        }
      }
#pragma unroll
      for (int r = 0; r < kTileR; ++r)
        if (row[r] < Nq && lane < k) {
          const int64_t at = ((int64_t)row[r] * S + s) * k + lane;
          part_d[at] = ld[r];
          part_j[at] = lj[r];
        }
    }
  }
}

__global__ void __launch_bounds__(kTileThreads)
k_knn_merge(const double *__restrict__ part_d, const int32_t *__restrict__ part_j, int N, int S, int k,
            int32_t *__restrict__ idx_out, double *__restrict__ dist_out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int kWaves = kTileThreads / 64;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + w; row < N; row += (int64_t)gridDim.x * kWaves) {  // (wave-uniform)
    double ld = INFINITY, td = INFINITY;
    int lj = INT_MAX, tj = INT_MAX;
    for (int s = 0; s < S; ++s) {
      const int64_t at = (row * S + s) * k + lane;
      const double d = lane < k ? part_d[at] : INFINITY;
      const int j = lane < k ? part_j[at] : INT_MAX;
      if (s == 0) {  // a sorted list as it is
        ld = d, lj = j;
        td = __shfl(ld, k - 1), tj = __shfl(lj, k - 1);
      } else {
        knn_offer(ld, lj, td, tj, d, j, j != INT_MAX, k, lane);
      }
    }
    if (lane < k) {
      idx_out[row * k + lane] = lj == INT_MAX ? -1 : lj;
      dist_out[row * k + lane] = ld;
    }
  }
}

// ---------------------------------------------------------------------------
// k_knn_tile_sym: the tile kernel under d_sym (include/fc_hip.h, fc_ensemble_knn_perm / fc_ensemble_knn_cross_perm;
// DESIGN.md section 21)
//
//   d_sym(i, j) = min over p < K, h in H of rmsd(Q[i], h * R[j][perms[p]]),   H = {+1} or, MIRROR, {+1, -1}
//
// k_knn_tile with its chunk walking the table, as k_diverse_step_sym does for its step: fc_rmsd_tile.h's functions with a
// row of the table and, for the explicit pass, the sign passed in.  The workgroup's 16 row
// conformers AND the table (16-bit indices) sit in LDS -- this form is staged only -- and the permutation is applied to
// the row side: sum_a p_a q_pi(a)^T = sum_b p_pi^-1(b) q_b^T and the table is closed under inverse, so the minimum over
// "rows of the table applied to the row conformer" is the minimum the contract names, a permutation costs one LDS
// address per atom (shared by the rows of the wavefront), and the column conformer is still read coalesced from Xs.
// Per chunk of 64 columns and table row p: the covariances of kKnnSymR of the wavefront's rows with the column in one atom loop; per
// row the Newton eigenvalue of B and -- MIRROR -- of -B (kabsch_lambda_max_both); a (p, h) goes on to the rotation and
// the explicit pass (h = -1 as pair_exact_aos<INV> forms it: -B, p + R q) unless its eigenvalue form of A msd rules it
// out for EVERY lane of the wavefront (a ballot, as k_knn_tile) -- by tau, the smaller of the row's slot k - 1 and the
// cap under k_knn_tile's margins, or by the pair's smallest explicit sum so far plus A kScreenMargin (the rule of
// k_diverse_step_sym).  After the K rows each lane offers (sqrt(best / A), j) once, if it made any explicit pass.
//
// Why the outputs are the same bits with the filter on or off and for every strip count: the head of this file.
//
// stats (may be NULL): [0] += (pair, p, h) whose eigenvalue was formed, [1] += those taken through the explicit pass
// (the lanes of a wavefront that made the pass: a pair rides along when another lane of its chunk needs it).
// ---------------------------------------------------------------------------
size_t knn_sym_lds_bytes(int64_t A, int64_t K) {
  return tile_rows_lds_bytes(A) + (((size_t)K * (size_t)A * sizeof(uint16_t) + 7) & ~(size_t)7);
}

#ifdef FC_KNN_SYM_ROWS  // (a tuning build: fc_tuning.h)
constexpr int kKnnSymR = FC_KNN_SYM_ROWS;
#else
// rows of a wavefront that share an atom loop.  4 (k_knn_tile's) holds 72 covariance registers beside the two eigenvalues
// and the running best: 256 VGPRs + 6 ... 29 AGPRs, one wavefront per SIMD; 2 compiles to 193 / 213 VGPRs (MIRROR), two
// wavefronts per SIMD, and measured 1.2 ... 1.5 x faster at 10 000 x 50 although a column load then serves 2 rows
// instead of 4.  The outputs do not depend on it.
constexpr int kKnnSymR = 2;
#endif
static_assert(kTileR % kKnnSymR == 0, "a wavefront's rows in whole groups");

template <bool CROSS, bool MIRROR>
__global__ void __launch_bounds__(kTileThreads)
k_knn_tile_sym(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ Gq, int Nq, int64_t Npad,
               int A, const uint16_t *__restrict__ perms, int K, int k, int filter, int n_tiles, int n_chunks,
               double *__restrict__ part_d, int32_t *__restrict__ part_j, unsigned long long *__restrict__ stats,
               const KnnCross<CROSS> x) {
  const double *__restrict__ Gr;
  int Nr;
  double cap;
  if constexpr (CROSS) Gr = x.Gr, Nr = x.Nr, cap = x.cap;
  else Gr = Gq, Nr = Nq, cap = INFINITY;
  extern __shared__ double s_rows[];  // [kTileRows][A][3], then the table [K][A] as uint16_t
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int S = gridDim.y, s = blockIdx.y;
  const int c0 = (int)((int64_t)s * n_chunks / S), c1 = (int)((int64_t)(s + 1) * n_chunks / S);
  const int A3 = 3 * A;
  const double dA = (double)A;
  const double margin = dA * kScreenMargin;
  uint16_t *pt = reinterpret_cast<uint16_t *>(s_rows + kTileRows * A3);
  for (int t = tid; t < K * A; t += kTileThreads) pt[t] = perms[t];  // (the first tile's barrier covers it)
  unsigned long long n_formed = 0, n_explicit = 0;  // (wave-uniform: ballots)

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * kTileRows;
    tile_stage_rows(s_rows, Xa, row0, Nq, A3);
    // the wavefront's kTileR rows, kKnnSymR at a time (each group walks the strip: the outputs do not depend on the split)
    for (int wrow = row0 + w * kTileR; wrow < min(row0 + (w + 1) * kTileR, Nq); wrow += kKnnSymR) {  // (wave-uniform)
      int row[kKnnSymR];
      const double *__restrict__ P[kKnnSymR];
      double Gi[kKnnSymR], ld[kKnnSymR], td[kKnnSymR];
      int lj[kKnnSymR], tj[kKnnSymR];
      tile_rows<true>(s_rows, Xa, Gq, row0, wrow, Nq, A3, row, P, Gi);
#pragma unroll
      for (int r = 0; r < kKnnSymR; ++r) {
        ld[r] = td[r] = INFINITY;
        lj[r] = tj[r] = INT_MAX;
      }
      for (int c = c0; c < c1; ++c) {
        const int j = c * 64 + lane;
        const int jl = min(j, Nr - 1);
        const double *__restrict__ q0 = Xs + jl;
        const double Gj = Gr[jl];
        double best[kKnnSymR];  // the pair's smallest explicit sum of squares so far
#pragma unroll
        for (int r = 0; r < kKnnSymR; ++r) best[r] = INFINITY;
#pragma nounroll
        for (int p = 0; p < K; ++p) {
          const uint16_t *__restrict__ pr = pt + p * A;
          // ---- 1. covariances of the column with the rows under row p of the table
          double B[kKnnSymR][9];
          tile_covariance(P, q0, Npad, A, pr, B);
          // ---- 2. per row and handedness: the filter, and where a lane passes it the rotation and the explicit pass
#pragma unroll
          for (int r = 0; r < kKnnSymR; ++r) {
            const bool ok = j < Nr && (CROSS || j != row[r]) && row[r] < Nq;
            const double GG = Gi[r] + Gj;
            double lam_p = 0.0, lam_m = 0.0;
            if (filter) kabsch_lambda_max_both<MIRROR>(B[r], GG, lam_p, lam_m);
            n_formed += (unsigned long long)((MIRROR ? 2 : 1) * __popcll(__ballot(ok)));
#pragma nounroll
            for (int h = 0; h < (MIRROR ? 2 : 1); ++h) {
              bool may = ok;
              if (filter) {  // (a NaN passes)
                const double msdA = GG - 2.0 * (h ? lam_m : lam_p);
                const double tau = CROSS ? fmin(td[r], cap) : td[r];
                may = ok && !(msdA > dA * tau * tau + (margin + kKnnFilterRel * GG)) && !(msdA > best[r] + margin);
              }
              if (__ballot(may) == 0) continue;  // (wave-uniform) this (p, h) is ruled out for every column of the chunk
              n_explicit += (unsigned long long)__popcll(__ballot(ok));
              const double ssq = tile_explicit_ssq<true>(P[r], q0, Npad, A, pr, B[r], GG, h ? -1.0 : 1.0);
              if (!(ssq >= best[r])) best[r] = ssq;
            }
          }
        }
        // ---- 3. one offer per pair: the smallest explicit sum, where any was formed
#pragma unroll
        for (int r = 0; r < kKnnSymR; ++r) {
          const bool ok = j < Nr && (CROSS || j != row[r]) && row[r] < Nq && best[r] != INFINITY;
          const double d = sqrt(best[r] / dA);
          knn_offer(ld[r], lj[r], td[r], tj[r], d, j, CROSS ? ok && d < cap : ok, k, lane);
        }
      }
#pragma unroll
      for (int r = 0; r < kKnnSymR; ++r)
        if (row[r] < Nq && lane < k) {
          const int64_t at = ((int64_t)row[r] * S + s) * k + lane;
          part_d[at] = ld[r];
          part_j[at] = lj[r];
        }
    }
  }
  if (stats != nullptr && lane == 0 && n_formed) {  // (a bench hook's counters)
    atomicAdd(&stats[0], n_formed);
    atomicAdd(&stats[1], n_explicit);
  }
}

// column strips of a launch of Nq rows against Nr columns (speed only: the outputs are the same bits for every value)
int knn_strips(int64_t Nq, int64_t Nr) { return tile_strips("FC_KNN_STRIPS", kKnnWorkgroupsPerCu, kKnnMaxStrips, Nq, Nr); }

// FC_KNN_FILTER=0: the explicit pass for every pair (speed only: the outputs are the same bits either way)
static int knn_filter() {
  const char *v = getenv("FC_KNN_FILTER");
  return !(v && v[0] == '0' && v[1] == 0);
}

// one launch: the rows of q against the columns of r (the self form: q == r, CROSS = false, cap = +inf)
struct KnnLaunch {
  const fc_ensemble *q, *r;
  int k, filter, n_tiles, n_chunks, S;
  double cap;
};

template <bool STAGE, bool CROSS>
static int launch_knn_tile(const KnnLaunch &a, double *part_d, int32_t *part_j) {
  const size_t lds = STAGE ? tile_rows_lds_bytes(a.q->A) : 0;
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_knn_tile<STAGE, CROSS>), lds, "k_knn_tile"));
  const unsigned gx = (unsigned)std::min<int64_t>(a.n_tiles, (int64_t)1 << 20);
  KnnCross<CROSS> x;
  if constexpr (CROSS) x = KnnCross<true>{a.r->G.as<double>(), (int)a.r->N, a.cap};
  hipLaunchKernelGGL((k_knn_tile<STAGE, CROSS>), dim3(gx, (unsigned)a.S), dim3(kTileThreads), lds, ctx().stream,
                     a.r->Xs.as<double>(), a.q->Xa.as<double>(), a.q->G.as<double>(), (int)a.q->N, a.r->Npad, (int)a.q->A, a.k,
                     a.filter, a.n_tiles, a.n_chunks, part_d, part_j, x);
  return check_launch("k_knn_tile");
}

template <bool CROSS, bool MIRROR>
static int launch_knn_tile_sym(const KnnLaunch &a, const SymTable &sym, double *part_d, int32_t *part_j) {
  const size_t lds = knn_sym_lds_bytes(a.q->A, sym.K);
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_knn_tile_sym<CROSS, MIRROR>), lds, "k_knn_tile_sym"));
  const unsigned gx = (unsigned)std::min<int64_t>(a.n_tiles, (int64_t)1 << 20);
  KnnCross<CROSS> x;
  if constexpr (CROSS) x = KnnCross<true>{a.r->G.as<double>(), (int)a.r->N, a.cap};
  hipLaunchKernelGGL((k_knn_tile_sym<CROSS, MIRROR>), dim3(gx, (unsigned)a.S), dim3(kTileThreads), lds, ctx().stream,
                     a.r->Xs.as<double>(), a.q->Xa.as<double>(), a.q->G.as<double>(), (int)a.q->N, a.r->Npad, (int)a.q->A,
                     sym.perms_dev, sym.K, a.k, a.filter, a.n_tiles, a.n_chunks, part_d, part_j, sym.stats_dev, x);
  return check_launch("k_knn_tile_sym");
}

static int knn_enqueue(const fc_ensemble *q, const fc_ensemble *r, bool cross, int k, double cap, int S, int32_t *indices_out,
                       double *dist_out, double *ms_device, DevBuf &pd, DevBuf &pj, DevBuf &oi, DevBuf &od,
                       const SymTable *sym) {
  const int64_t Nq = q->N;
  const KnnLaunch a{q, r, k, knn_filter(), (int)ceil_div(Nq, kTileRows), (int)ceil_div(r->N, 64), S, cap};
  const size_t entries = (size_t)Nq * (size_t)k;
  FC_TRY(pd.reserve(entries * (size_t)S * sizeof(double)));
  FC_TRY(pj.reserve(entries * (size_t)S * sizeof(int32_t)));
  FC_TRY(oi.reserve(entries * sizeof(int32_t)));
  FC_TRY(od.reserve(entries * sizeof(double)));
  Context &c = ctx();
  if (ms_device) FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  const bool stage = q->A <= kTileLdsAtoms;
  const auto tile = cross ? (stage ? launch_knn_tile<true, true> : launch_knn_tile<false, true>)
                         : (stage ? launch_knn_tile<true, false> : launch_knn_tile<false, false>);
  if (sym) {
    const auto tile_sym = cross ? (sym->mirror ? launch_knn_tile_sym<true, true> : launch_knn_tile_sym<true, false>)
                                : (sym->mirror ? launch_knn_tile_sym<false, true> : launch_knn_tile_sym<false, false>);
    FC_TRY(tile_sym(a, *sym, pd.as<double>(), pj.as<int32_t>()));
  } else {
    FC_TRY(tile(a, pd.as<double>(), pj.as<int32_t>()));
  }
  const unsigned gm = (unsigned)std::min<int64_t>(ceil_div(Nq, kTileThreads / 64), (int64_t)1 << 20);
  hipLaunchKernelGGL(k_knn_merge, dim3(gm), dim3(kTileThreads), 0, c.stream, pd.as<double>(), pj.as<int32_t>(), (int)Nq, S, k,
                     oi.as<int32_t>(), od.as<double>());
  FC_TRY(check_launch("k_knn_merge"));
  if (ms_device) FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  FC_TRY(d2h(indices_out, oi.p, entries * sizeof(int32_t)));
  FC_TRY(d2h(dist_out, od.p, entries * sizeof(double)));
  FC_TRY(sync());
  if (ms_device) {
    float ms = 0.0f;
    FC_HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    *ms_device = ms;
  }
  return FC_OK;
}

// The lists behind fc_ensemble_knn (cross = false: q == r, max_rmsd = +inf) and fc_ensemble_knn_cross (cross = true: the
// rows of q against the columns of r, which may be the same handle) -- arguments checked there; both N >= 1, the same A,
// 1 <= k <= FC_KNN_MAX, max_rmsd > 0.  ms_device (may be NULL): HIP-event time from the first launch to the end of the
// merge; strips_out (may be NULL): the strip count used.  sym (may be NULL): the tiles are k_knn_tile_sym's
// (fc_ensemble_knn_perm / fc_ensemble_knn_cross_perm, which have checked that the rows and the table fit the LDS).
int knn(fc_ensemble *q, fc_ensemble *r, bool cross, int64_t k, double max_rmsd, int32_t *indices_out, double *dist_out,
        double *ms_device, int64_t *strips_out, const SymTable *sym) {
  const int S = knn_strips(q->N, r->N);
  if (strips_out) *strips_out = S;
  if (sym && knn_sym_lds_bytes(q->A, sym->K) > kLdsLimit)
    return set_error(FC_E_LIMIT, "A_sel=%lld selected atoms with K=%d permutations need %zu bytes of LDS (limit %zu)",
                     (long long)q->A, sym->K, knn_sym_lds_bytes(q->A, sym->K), kLdsLimit);
  DevBuf pd, pj, oi, od;
  const int rc = knn_enqueue(q, r, cross, (int)k, max_rmsd, S, indices_out, dist_out, ms_device, pd, pj, oi, od, sym);
  // an error behind a launch: nothing of the four buffers may be in flight when they go back to the pool
  if (rc != FC_OK && ctx().ready) (void)hipStreamSynchronize(cur_stream());
  return rc;
}

__global__ void k_warm_knn() {}
int warm_knn() {
  hipLaunchKernelGGL(k_warm_knn, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_knn");
}

}  // namespace fc
