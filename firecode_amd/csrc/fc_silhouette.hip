// fc_silhouette.hip -- per-conformer mean Kabsch RMSD to the conformer's own group and to the nearest other group, the
// two quantities a silhouette is read from, over a resident ensemble and without an N x N matrix or an N x n_groups
// table, for gfx950 (wave64, float64).
//
// The contract (include/fc_hip.h, fc_ensemble_silhouette) -- d(i, j) is the d of fc_ensemble_knn:
// covariance, kabsch_rotation_qcp with the kabsch_rotation fallback, the explicit rotated difference with conformer i
// as the row (p) and j as the column (q), never the eigenvalue form, for every ordered pair i != j;
// q(d) = (uint64) rint(d 2^32):
//
//   T[i, g] = sum of q(d(i, j)) over the members j != i of group g        (64-bit integers)
//   a[i] = (double) T[i, own] 2^-32 / (size_own - 1), 0 for a singleton
//   b[i] = min over the other non-empty groups g of m[i, g] = (double) T[i, g] 2^-32 / size_g, nearest[i] = that g,
//          the lowest on ties
//
// k_silhouette_tile walks fc_rmsd_tile.h's tile, as k_group_sums (fc_medoid.hip) and k_knn_tile (fc_knn.hip) do -- over
// the LABEL-SORTED copy of the labelled
// conformers (the host's stable order by label, one k_ensemble_gather), and over the FULL SQUARE: every row owns its
// results, nothing is handed to a column, no atomics.
// In the sorted copy a group is the contiguous column range [seg_begin[j], seg_end[j]) around any of its columns j, and
// a group is named by its first position (ascending in the label: the host turns it back into the label).  Per row
// and chunk:
//   1. the inclusive prefix over the 64 lanes of q(d(row, j)) -- 0 at j = row and at j >= M -- by a 6-step integer scan;
//      it is exact, so a segment's sum is a difference of two prefixes without cancellation error;
//   2. every lane forms the sum of ITS group's columns up to itself: the difference to the exclusive prefix of the lane
//      at seg_begin[j] where that lies in this chunk, otherwise the prefix plus the row's carry -- the sum over the
//      earlier chunks of the strip of the one group that was open when the chunk began (wave-uniform; only one group
//      can be open across a chunk boundary);
//   3. a lane whose column is the last of its group (seg_end[j] == j + 1) closes the group: the row's own group gives
//      T[i, own], any other a candidate (m, g) that the lane keeps as its best by lexicographic (m, g); a group that
//      began before the strip is not complete and goes out as the strip's HEAD record (group, partial sum) instead;
//   4. the carry for the next chunk is lane 63's sum where its group goes on, 0 otherwise.
// At the end of the strip: one wavefront min-reduction of (m, g) per row, and the carry goes out as the strip's TAIL
// record.  A strip that lies inside one group leaves a tail record only.
// Items are (row tile, strip of the chunk range), one workgroup per item up to 2^20 (grid-stride beyond);
// FC_SILHOUETTE_STRIPS=<n> forces the strips (speed and tests only: the same bits for every value -- the sums are
// integers, m is one expression of a complete sum, and a minimum by (m, g) does not depend on the order).
//
// k_silhouette_join -- one thread per row -- walks the row's strips in order, adds the partial sums of a cut group from
// the tail records up to its head record, forms its m, takes the minimum against the strips' own bests and writes a, b
// and nearest.  No spin-waits, no grid barrier, no float atomics.
#include "fc_rmsd_tile.h"

#include <climits>

namespace fc {

// the mean of a complete integer sum over n distances, in A: the one expression both kernels use
__host__ __device__ __forceinline__ double sil_mean(unsigned long long T, int n) {
  return (double)T * (1.0 / 4294967296.0) / (double)n;
}

__device__ __forceinline__ unsigned long long sil_readlane(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// the per-(strip, row) records, strip-major: part_m / part_g -- the best candidate among the groups that lie wholly in
// the strip; head -- the group that began before the strip and ends in it (head_g = -1, as the host's memset leaves it:
// none); tail -- the group that is open at the strip's end (tail_g = -1: none); own_sum[row]: T[row, own] where the
// row's group lies wholly in one strip (otherwise the join finds it)
struct SilRecords {
  double *part_m;
  int32_t *part_g;
  int32_t *head_g;
  unsigned long long *head_sum;
  int32_t *tail_g;
  unsigned long long *tail_sum;
  unsigned long long *own_sum;
};

template <bool STAGE>
__global__ void __launch_bounds__(kTileThreads)
k_silhouette_tile(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ G, int M, int64_t Npad,
                  int A, const int32_t *__restrict__ seg_begin, const int32_t *__restrict__ seg_end, int n_tiles, int n_chunks,
                  int S, const SilRecords out) {
  extern __shared__ double s_rows[];  // [kTileRows][A][3] when STAGE
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int A3 = 3 * A;
  const double dA = (double)A;
  const int64_t n_items = (int64_t)n_tiles * S;

  for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int tile = (int)(item / S), s = (int)(item % S);
    const int row0 = tile * kTileRows;
    // the strip's chunks of 64 columns (S <= n_chunks: never empty)
    const int c0 = (int)((int64_t)s * n_chunks / S), c1 = (int)((int64_t)(s + 1) * n_chunks / S);
    const int col0 = c0 * 64;
    if (STAGE) tile_stage_rows(s_rows, Xa, row0, M, A3);
    const int wrow = row0 + w * kTileR;
    if (wrow >= M) continue;  // (wave-uniform; no barrier follows in this item)
    int row[kTileR], rsb[kTileR], bg[kTileR];
    const double *__restrict__ P[kTileR];
    double Gi[kTileR], bm[kTileR];
    unsigned long long carry[kTileR];
    tile_rows<STAGE>(s_rows, Xa, G, row0, wrow, M, A3, row, P, Gi);
#pragma unroll
    for (int r = 0; r < kTileR; ++r) {
      rsb[r] = seg_begin[min(row[r], M - 1)];
      carry[r] = 0ull;
      bm[r] = INFINITY;
      bg[r] = INT_MAX;
    }
    int open_g = -1;  // the group that is open behind the chunk just walked (a property of the columns: the same for all rows)
    for (int c = c0; c < c1; ++c) {
      const int cbase = c * 64;
      const int j = cbase + lane;
      const int jl = min(j, M - 1);
      const double *__restrict__ q0 = Xs + jl;
      // ---- 1. covariances with the 4 rows
      double B[kTileR][9];
      tile_covariance(P, q0, Npad, A, TileNoPerm{}, B);
      // ---- 2. the column's group: where it begins, whether this column closes it, whether it goes on behind the chunk
      const double Gj = G[jl];
      const int sb = seg_begin[jl], se = seg_end[jl];  // (sb <= jl < se <= M)
      const bool closes = j < M && se == j + 1;
      const bool in_chunk = sb >= cbase;
      const int src = in_chunk ? sb - cbase : 0;  // (sb <= j: a lane of this chunk, not above this one)
      const int sb63 = __builtin_amdgcn_readlane(sb, 63), se63 = __builtin_amdgcn_readlane(se, 63);
      const bool goes_on = cbase + 64 < M && se63 > cbase + 64;  // (then lane 63's column is below M and not clamped)
      open_g = goes_on ? sb63 : -1;
      // ---- 3. per row: the rotation, the explicit rotated difference, the scan and the groups that close here
#pragma unroll
      for (int r = 0; r < kTileR; ++r) {
        if (row[r] >= M) continue;  // (wave-uniform)
        // tile_rmsd's body, written out: as a call it takes this kernel from 242 / 250 to 248 / 256 VGPRs, the last count
        // at which two wavefronts fit a SIMD (the same instructions and the same speed, but no room for the next change)
        const double GG = Gi[r] + Gj;
        const int64_t step = 3 * Npad;
        double R[9];
        if (!kabsch_rotation_qcp(B[r], GG, R)) (void)kabsch_rotation(B[r], R);
        double ssq = 0.0;
        const double *__restrict__ qa = q0;
#pragma unroll 2
        for (int a = 0; a < A; ++a, qa += step) {
          const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
          const double px = P[r][a * 3], py = P[r][a * 3 + 1], pz = P[r][a * 3 + 2];
          const double dx = px - (R[0] * qx + R[1] * qy + R[2] * qz);
          const double dy = py - (R[3] * qx + R[4] * qy + R[5] * qz);
          const double dz = pz - (R[6] * qx + R[7] * qy + R[8] * qz);
          ssq += dx * dx + dy * dy + dz * dz;
        }
        const double d = sqrt(ssq / dA);
        const unsigned long long qd = (j < M && j != row[r]) ? (unsigned long long)rint(d * 4294967296.0) : 0ull;
        unsigned long long p = qd;  // the inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned long long t = __shfl_up(p, o);
          if (lane >= o) p += t;
        }
        const unsigned long long before = __shfl(p - qd, src);  // the exclusive prefix at the group's first lane
        const unsigned long long gsum = in_chunk ? p - before : p + carry[r];  // this lane's group, up to this lane
        if (closes) {
          if (sb < col0) {  // began before the strip: not complete (at most one lane per row and strip)
            const int64_t rec = (int64_t)s * M + row[r];
            out.head_g[rec] = sb;
            out.head_sum[rec] = gsum;
          } else if (sb == rsb[r]) {
            out.own_sum[row[r]] = gsum;
          } else {
            const double m = sil_mean(gsum, se - sb);
            if (m < bm[r] || (m == bm[r] && sb < bg[r])) bm[r] = m, bg[r] = sb;
          }
        }
        carry[r] = goes_on ? sil_readlane(gsum, 63) : 0ull;
      }
    }
    // ---- 4. the strip's best per row, and what is open at its end
#pragma unroll
    for (int r = 0; r < kTileR; ++r) {
      if (row[r] >= M) continue;  // (wave-uniform)
      double m = bm[r];
      int g = bg[r];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double om = __shfl_xor(m, o);
        const int og = __shfl_xor(g, o);
        if (om < m || (om == m && og < g)) m = om, g = og;
      }
      if (lane == 0) {
        const int64_t rec = (int64_t)s * M + row[r];
        out.part_m[rec] = m;
        out.part_g[rec] = g;
        out.tail_g[rec] = open_g;
        out.tail_sum[rec] = carry[r];
      }
    }
  }
}

// a (M), b (M; +inf where the row has no other group) and nearest (M; the first position of the group, -1 where none)
__global__ void __launch_bounds__(256)
k_silhouette_join(const int32_t *__restrict__ seg_begin, const int32_t *__restrict__ seg_end, int M, int S, const SilRecords in,
                  double *__restrict__ a_out, double *__restrict__ b_out, int32_t *__restrict__ nearest_out) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < M; row += (int64_t)gridDim.x * blockDim.x) {
    const int rsb = seg_begin[row], size = seg_end[row] - rsb;
    double bm = INFINITY;
    int bg = INT_MAX;
    unsigned long long own = 0ull, acc = 0ull;
    bool own_joined = false;
    int acc_g = -1;  // the cut group whose parts are being added up
    for (int s = 0; s < S; ++s) {
      const int64_t rec = (int64_t)s * M + row;
      const int hg = in.head_g[rec];
      if (hg >= 0) {  // the cut group ends in this strip (acc_g == hg: its earlier parts came as tails)
        const unsigned long long T = acc + in.head_sum[rec];
        if (hg == rsb) {
          own = T, own_joined = true;
        } else {
          const double m = sil_mean(T, seg_end[hg] - hg);
          if (m < bm || (m == bm && hg < bg)) bm = m, bg = hg;
        }
        acc_g = -1, acc = 0ull;
      }
      const double m = in.part_m[rec];
      const int g = in.part_g[rec];
      if (m < bm || (m == bm && g < bg)) bm = m, bg = g;
      const int tg = in.tail_g[rec];
      if (tg >= 0) {
        if (tg == acc_g) acc += in.tail_sum[rec];  // the strip lies inside the group
        else acc_g = tg, acc = in.tail_sum[rec];
      }
    }
    if (!own_joined) own = in.own_sum[row];
    a_out[row] = size > 1 ? sil_mean(own, size - 1) : 0.0;
    b_out[row] = bm;
    nearest_out[row] = bg == INT_MAX ? -1 : bg;
  }
}

// ---------------------------------------------------------------------------
// k_silhouette_tile_sym: k_silhouette_tile under d_sym (include/fc_hip.h, fc_ensemble_silhouette_perm; DESIGN.md
// section 28) -- d_sym(i, j) as k_group_sums_sym (fc_medoid.hip) forms it: the value k_knn_tile_sym writes for row i and
// column j, for every ordered pair i != j.  The workgroup's 16 rows AND the table sit in LDS (staged only); kSilSymR of
// the wavefront's rows share an atom loop, and each such group of rows walks the strip on its own -- the records are per
// (strip, row), so k_silhouette_join reads them as it reads k_silhouette_tile's.  Per chunk the K table rows are walked
// first (covariances, the eigenvalue filter against the pair's smallest explicit sum so far, the explicit pass), then
// per row the one q(sqrt(best / A)) of every lane goes through k_silhouette_tile's scan, carry and records unchanged.
// The same bits with the filter on or off (FC_MEDOID_SYM_FILTER=0), for every strip count and every kSilSymR.
// stats (may be NULL): as k_group_sums_sym.
// ---------------------------------------------------------------------------
#ifdef FC_SUM_SYM_ROWS  // (a tuning build: fc_tuning.h)
constexpr int kSilSymR = FC_SUM_SYM_ROWS;
#else
constexpr int kSilSymR = 2;  // as k_knn_tile_sym and k_group_sums_sym (the resource report: DESIGN.md section 28)
#endif
static_assert(kTileR % kSilSymR == 0, "a wavefront's rows in whole groups");

template <bool MIRROR>
__global__ void __launch_bounds__(kTileThreads)
k_silhouette_tile_sym(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ G, int M,
                      int64_t Npad, int A, const uint16_t *__restrict__ perms, int K, int filter,
                      const int32_t *__restrict__ seg_begin, const int32_t *__restrict__ seg_end, int n_tiles, int n_chunks, int S,
                      const SilRecords out, unsigned long long *__restrict__ stats) {
  extern __shared__ double s_rows[];  // [kTileRows][A][3], then the table [K][A] as uint16_t
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int A3 = 3 * A;
  const double dA = (double)A;
  const double margin = dA * kScreenMargin;
  const int64_t n_items = (int64_t)n_tiles * S;
  uint16_t *pt = reinterpret_cast<uint16_t *>(s_rows + kTileRows * A3);
  for (int t = tid; t < K * A; t += kTileThreads) pt[t] = perms[t];  // (the first item's barrier covers it)
  unsigned long long n_formed = 0, n_explicit = 0;  // (wave-uniform: ballots)

  for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int tile = (int)(item / S), s = (int)(item % S);
    const int row0 = tile * kTileRows;
    // the strip's chunks of 64 columns (S <= n_chunks: never empty)
    const int c0 = (int)((int64_t)s * n_chunks / S), c1 = (int)((int64_t)(s + 1) * n_chunks / S);
    const int col0 = c0 * 64;
    tile_stage_rows(s_rows, Xa, row0, M, A3);
    // the wavefront's kTileR rows, kSilSymR at a time (wave-uniform; no barrier follows in this item)
    for (int wrow = row0 + w * kTileR; wrow < min(row0 + (w + 1) * kTileR, M); wrow += kSilSymR) {
      int row[kSilSymR], rsb[kSilSymR], bg[kSilSymR];
      const double *__restrict__ P[kSilSymR];
      double Gi[kSilSymR], bm[kSilSymR];
      unsigned long long carry[kSilSymR];
      tile_rows<true>(s_rows, Xa, G, row0, wrow, M, A3, row, P, Gi);
#pragma unroll
      for (int r = 0; r < kSilSymR; ++r) {
        rsb[r] = seg_begin[min(row[r], M - 1)];
        carry[r] = 0ull;
        bm[r] = INFINITY;
        bg[r] = INT_MAX;
      }
      int open_g = -1;  // the group that is open behind the chunk just walked (a property of the columns)
      for (int c = c0; c < c1; ++c) {
        const int cbase = c * 64;
        const int j = cbase + lane;
        const int jl = min(j, M - 1);
        const double *__restrict__ q0 = Xs + jl;
        const double Gj = G[jl];
        // ---- 1. d_sym of the column with the rows: the K table rows, the filter, the explicit passes
        double best[kSilSymR];  // the pair's smallest explicit sum of squares so far
#pragma unroll
        for (int r = 0; r < kSilSymR; ++r) best[r] = INFINITY;
#pragma nounroll
        for (int p = 0; p < K; ++p) {
          const uint16_t *__restrict__ pr = pt + p * A;
          double B[kSilSymR][9];
          tile_covariance(P, q0, Npad, A, pr, B);
#pragma unroll
          for (int r = 0; r < kSilSymR; ++r) {
            if (row[r] >= M) continue;  // (wave-uniform)
            const bool ok = j < M && j != row[r];
            const double GG = Gi[r] + Gj;
            double lam_p = 0.0, lam_m = 0.0;
            if (filter) kabsch_lambda_max_both<MIRROR>(B[r], GG, lam_p, lam_m);
            n_formed += (unsigned long long)((MIRROR ? 2 : 1) * __popcll(__ballot(ok)));
#pragma nounroll
            for (int h = 0; h < (MIRROR ? 2 : 1); ++h) {
              bool may = ok;
              if (filter) {  // (a NaN passes; best = +inf, the pair's first (p, h), passes)
                const double msdA = GG - 2.0 * (h ? lam_m : lam_p);
                may = ok && !(msdA > best[r] + margin);
              }
              if (__ballot(may) == 0) continue;  // (wave-uniform) this (p, h) is ruled out for every pair of the chunk
              n_explicit += (unsigned long long)__popcll(__ballot(ok));
              const double ssq = tile_explicit_ssq<true>(P[r], q0, Npad, A, pr, B[r], GG, h ? -1.0 : 1.0);
              if (!(ssq >= best[r])) best[r] = ssq;
            }
          }
        }
        // ---- 2. the column's group: where it begins, whether this column closes it, whether it goes on behind the chunk
        const int sb = seg_begin[jl], se = seg_end[jl];  // (sb <= jl < se <= M)
        const bool closes = j < M && se == j + 1;
        const bool in_chunk = sb >= cbase;
        const int src = in_chunk ? sb - cbase : 0;  // (sb <= j: a lane of this chunk, not above this one)
        const int sb63 = __builtin_amdgcn_readlane(sb, 63), se63 = __builtin_amdgcn_readlane(se, 63);
        const bool goes_on = cbase + 64 < M && se63 > cbase + 64;  // (then lane 63's column is below M and not clamped)
        open_g = goes_on ? sb63 : -1;
        // ---- 3. per row: the scan and the groups that close here
#pragma unroll
        for (int r = 0; r < kSilSymR; ++r) {
          if (row[r] >= M) continue;  // (wave-uniform)
          const double d = sqrt(best[r] / dA);
          const unsigned long long qd = (j < M && j != row[r]) ? (unsigned long long)rint(d * 4294967296.0) : 0ull;
          unsigned long long p = qd;  // the inclusive prefix over the lanes
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(p, o);
            if (lane >= o) p += t;
          }
          const unsigned long long before = __shfl(p - qd, src);  // the exclusive prefix at the group's first lane
          const unsigned long long gsum = in_chunk ? p - before : p + carry[r];  // this lane's group, up to this lane
          if (closes) {
            if (sb < col0) {  // began before the strip: not complete (at most one lane per row and strip)
              const int64_t rec = (int64_t)s * M + row[r];
              out.head_g[rec] = sb;
              out.head_sum[rec] = gsum;
            } else if (sb == rsb[r]) {
              out.own_sum[row[r]] = gsum;
            } else {
              const double m = sil_mean(gsum, se - sb);
              if (m < bm[r] || (m == bm[r] && sb < bg[r])) bm[r] = m, bg[r] = sb;
            }
          }
          carry[r] = goes_on ? sil_readlane(gsum, 63) : 0ull;
        }
      }
      // ---- 4. the strip's best per row, and what is open at its end
#pragma unroll
      for (int r = 0; r < kSilSymR; ++r) {
        if (row[r] >= M) continue;  // (wave-uniform)
        double m = bm[r];
        int g = bg[r];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const double om = __shfl_xor(m, o);
          const int og = __shfl_xor(g, o);
          if (om < m || (om == m && og < g)) m = om, g = og;
        }
        if (lane == 0) {
          const int64_t rec = (int64_t)s * M + row[r];
          out.part_m[rec] = m;
          out.part_g[rec] = g;
          out.tail_g[rec] = open_g;
          out.tail_sum[rec] = carry[r];
        }
      }
    }
  }
  if (stats != nullptr && lane == 0 && n_formed) {  // (a bench hook's counters)
    atomicAdd(&stats[0], n_formed);
    atomicAdd(&stats[1], n_explicit);
  }
}

int silhouette_strips(int64_t M) { return tile_strips("FC_SILHOUETTE_STRIPS", kTileItemsPerCu, kTileItemMaxStrips, M, M); }

// bytes of the work block of launch_silhouette for M sorted conformers: the outputs first -- a (M doubles) | b (M
// doubles) | nearest (M int32), the part that travels to the host: silhouette_result_bytes -- then the records of S strips
static size_t sil_up(size_t v) { return (v + 255) & ~(size_t)255; }
size_t silhouette_result_bytes(int64_t M) { return (size_t)M * (8 + 8 + 4); }
size_t silhouette_work_bytes(int64_t M, int S) {
  const size_t ms = (size_t)M * (size_t)S;
  return sil_up(silhouette_result_bytes(M)) + 3 * sil_up(ms * 8) + 3 * sil_up(ms * 4) + sil_up((size_t)M * 8);
}

template <bool STAGE>
static int launch_silhouette_tile_as(const fc_ensemble *e, const int32_t *seg_begin_dev, const int32_t *seg_end_dev, int n_tiles,
                                     int n_chunks, int S, const SilRecords &rec) {
  const size_t lds = STAGE ? tile_rows_lds_bytes(e->A) : 0;
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_silhouette_tile<STAGE>), lds, "k_silhouette_tile"));
  const unsigned gx = (unsigned)std::min<int64_t>((int64_t)n_tiles * S, (int64_t)1 << 20);
  hipLaunchKernelGGL((k_silhouette_tile<STAGE>), dim3(gx), dim3(kTileThreads), lds, ctx().stream, e->Xs.as<double>(),
                     e->Xa.as<double>(), e->G.as<double>(), (int)e->N, e->Npad, (int)e->A, seg_begin_dev, seg_end_dev, n_tiles,
                     n_chunks, S, rec);
  return check_launch("k_silhouette_tile");
}

template <bool MIRROR>
static int launch_silhouette_tile_sym_as(const fc_ensemble *e, const SymTable &sym, const int32_t *seg_begin_dev,
                                         const int32_t *seg_end_dev, int n_tiles, int n_chunks, int S, const SilRecords &rec) {
  const size_t lds = knn_sym_lds_bytes(e->A, sym.K);
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_silhouette_tile_sym<MIRROR>), lds, "k_silhouette_tile_sym"));
  const unsigned gx = (unsigned)std::min<int64_t>((int64_t)n_tiles * S, (int64_t)1 << 20);
  hipLaunchKernelGGL((k_silhouette_tile_sym<MIRROR>), dim3(gx), dim3(kTileThreads), lds, ctx().stream, e->Xs.as<double>(),
                     e->Xa.as<double>(), e->G.as<double>(), (int)e->N, e->Npad, (int)e->A, sym.perms_dev, sym.K, sums_sym_filter(),
                     seg_begin_dev, seg_end_dev, n_tiles, n_chunks, S, rec, sym.stats_dev);
  return check_launch("k_silhouette_tile_sym");
}

// a | b | nearest (silhouette_result_bytes, at the front of work_dev) of the label-sorted ensemble e, 2 <= M = e->N <
// 2^31 - 256, seg_begin_dev / seg_end_dev [i] = the bounds of the group of position i; work_dev holds
// silhouette_work_bytes(M, S) bytes, S = silhouette_strips(M).  Enqueued only; timed: the context's events ev0 / ev1 are
// recorded around the kernel pair and the clearing of the head records, for the caller to read behind its wait.
// sym (may be NULL): under d_sym -- k_silhouette_tile_sym, whose rows and table fit the LDS (refused here otherwise; the
// entry points have refused it before any device use).
int launch_silhouette(const fc_ensemble *e, const int32_t *seg_begin_dev, const int32_t *seg_end_dev, int S, uint8_t *work_dev,
                      bool timed, const SymTable *sym) {
  Context &c = ctx();
  const int64_t M = e->N;
  if (sym && knn_sym_lds_bytes(e->A, sym->K) > kLdsLimit)
    return set_error(FC_E_LIMIT, "A_sel=%lld selected atoms with K=%d permutations need %zu bytes of LDS (limit %zu)",
                     (long long)e->A, sym->K, knn_sym_lds_bytes(e->A, sym->K), kLdsLimit);
  const size_t ms = (size_t)M * (size_t)S;
  uint8_t *at = work_dev;
  const auto take = [&at](size_t bytes) {
    uint8_t *p = at;
    at += sil_up(bytes);
    return p;
  };
  double *a_dev = reinterpret_cast<double *>(take(silhouette_result_bytes(M))), *b_dev = a_dev + M;
  int32_t *nearest_dev = reinterpret_cast<int32_t *>(b_dev + M);
  SilRecords rec;
  rec.part_m = reinterpret_cast<double *>(take(ms * 8));
  rec.head_sum = reinterpret_cast<unsigned long long *>(take(ms * 8));
  rec.tail_sum = reinterpret_cast<unsigned long long *>(take(ms * 8));
  rec.part_g = reinterpret_cast<int32_t *>(take(ms * 4));
  rec.head_g = reinterpret_cast<int32_t *>(take(ms * 4));
  rec.tail_g = reinterpret_cast<int32_t *>(take(ms * 4));
  rec.own_sum = reinterpret_cast<unsigned long long *>(take((size_t)M * 8));
  const int n_tiles = (int)ceil_div(M, kTileRows), n_chunks = (int)ceil_div(M, 64);
  if (timed) FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  FC_HIP_TRY(hipMemsetAsync(rec.head_g, 0xFF, ms * 4, c.stream));  // -1: no head record
  if (sym)
    FC_TRY((sym->mirror ? launch_silhouette_tile_sym_as<true> : launch_silhouette_tile_sym_as<false>)(e, *sym, seg_begin_dev,
                                                                                                     seg_end_dev, n_tiles, n_chunks,
                                                                                                     S, rec));
  else
    FC_TRY((e->A <= kTileLdsAtoms ? launch_silhouette_tile_as<true> : launch_silhouette_tile_as<false>)(e, seg_begin_dev, seg_end_dev,
                                                                                                     n_tiles, n_chunks, S, rec));
  const unsigned gj = (unsigned)std::min<int64_t>(ceil_div(M, 256), (int64_t)1 << 16);
  hipLaunchKernelGGL(k_silhouette_join, dim3(gj), dim3(256), 0, c.stream, seg_begin_dev, seg_end_dev, (int)M, S, rec, a_dev, b_dev,
                     nearest_dev);
  FC_TRY(check_launch("k_silhouette_join"));
  if (timed) FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  return FC_OK;
}

__global__ void k_warm_silhouette() {}
int warm_silhouette() {
  hipLaunchKernelGGL(k_warm_silhouette, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_silhouette");
}

}  // namespace fc
