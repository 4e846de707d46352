// fc_medoid.hip -- per-conformer sums of the ensemble's Kabsch RMSD over the conformers of the same group, the quantity
// a cluster's medoid and the k-medoids update are read from, over a resident ensemble and without an N x N matrix, for
// gfx950 (wave64, float64).
//
// The contract (include/fc_hip.h, fc_ensemble_medoids) -- d(i, j), i < j, is the d of
// fc_ensemble_knn: covariance, kabsch_rotation_qcp with the kabsch_rotation fallback, the explicit rotated difference
// with conformer i as the row (p) and j as the column (q), never the eigenvalue form; q(d) = (uint64) rint(d 2^32):
//
//   S[i] = sum of q(d(i, j)) over j != i of i's group,      E[i] = max of d(i, j) over the same j
//
// d is evaluated ONCE per unordered pair and handed to both partners, so S is exactly symmetric in a pair; the sums are
// 64-bit integers, so they do not depend on the order, the launch shape or the arrival of the atomics.
//
// k_group_sums walks fc_rmsd_tile.h's tile, as k_knn_tile (fc_knn.hip) does, without the filter and the lists.  It
// walks a LABEL-SORTED copy of the ensemble (the host's stable
// order by label, one k_ensemble_gather): the group of a row is then the contiguous range of positions that ends at
// seg_end[row], and the pairs of a row that count are the columns row < j < seg_end[row] -- the upper triangle of its
// group's block.  A wavefront's four rows may belong to several small groups: it walks the union of their ranges
// (seg_end is nondecreasing) and masks per row.  Every pair that counts goes through the explicit pass; a (row, chunk)
// in which no lane counts is skipped by a ballot.
// q(d) goes to the row's sum, kept in registers over the strip's chunks, reduced over the wavefront and flushed by one
// atomicAdd per row and strip; and to the column's sum, the lane's four rows added up first: one 64-bit integer
// atomicAdd per lane and chunk, to consecutive addresses.  E goes the same way by atomicMax on the bit pattern of the
// non-negative double (non-negative doubles order like their bits).  About 4 bytes of atomics per alignment.
// The triangle is balanced over (row tile, column strip) items, heaviest tiles first for a single group: a tile's own
// chunk range -- not the ensemble's -- is cut into S strips, the grid is one workgroup per item up to 2^20 (grid-stride
// beyond), and the hardware hands the items out as workgroups retire.  FC_MEDOID_STRIPS=<n> forces S (speed and tests
// only: the same bits for every value).  No spin-waits, no grid barrier, no float atomics.
//
// k_ensemble_gather copies Xs, Xa and G of chosen conformers into a new ensemble; it computes nothing, so the
// coordinates and G keep their bits: the sorted copy above, the medoid sub-ensemble of the k-medoids assignment and
// fc_ensemble_subset.
#include "fc_rmsd_tile.h"

namespace fc {

template <bool STAGE>
__global__ void __launch_bounds__(kTileThreads)
k_group_sums(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ G, int N, int64_t Npad,
             int A, const int32_t *__restrict__ seg_end, int n_tiles, int S, unsigned long long *__restrict__ sums,
             unsigned long long *__restrict__ ecc) {
  extern __shared__ double s_rows[];  // [kTileRows][A][3] when STAGE
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int A3 = 3 * A;
  const double dA = (double)A;
  const int64_t n_items = (int64_t)n_tiles * S;

  for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int tile = (int)(item / S), s = (int)(item % S);
    const int row0 = tile * kTileRows;
    // the tile's chunks of 64 columns: the columns behind its first row up to the end of its last row's group
    const int tb = (row0 + 1) >> 6, te = (seg_end[min(row0 + kTileRows - 1, N - 1)] + 63) >> 6;
    const int nt = max(te - tb, 0);
    const int c0 = tb + (int)((int64_t)s * nt / S), c1 = tb + (int)((int64_t)(s + 1) * nt / S);
    if (c0 >= c1) continue;  // (the same for the whole workgroup)
    if (STAGE) tile_stage_rows(s_rows, Xa, row0, N, A3);
    const int wrow = row0 + w * kTileR;
    if (wrow >= N) continue;  // (wave-uniform; no barrier follows in this item)
    int row[kTileR], se[kTileR];
    const double *__restrict__ P[kTileR];
    double Gi[kTileR], re[kTileR];
    unsigned long long rs[kTileR];
    tile_rows<STAGE>(s_rows, Xa, G, row0, wrow, N, A3, row, P, Gi);
#pragma unroll
    for (int r = 0; r < kTileR; ++r) {
      const int e = seg_end[min(row[r], N - 1)];
      se[r] = row[r] < N ? e : 0;  // (a row past the end counts nowhere)
      rs[r] = 0ull;
      re[r] = 0.0;
    }
    // the wavefront's own part of the strip: behind its first row, up to the end of its last row's group
    const int wc0 = max(c0, (wrow + 1) >> 6), wc1 = min(c1, (seg_end[min(wrow + kTileR - 1, N - 1)] + 63) >> 6);
    for (int c = wc0; c < wc1; ++c) {
      const int j = c * 64 + lane;
      const int jl = min(j, N - 1);
      const double *__restrict__ q0 = Xs + jl;
      // ---- 1. covariances with the 4 rows
      double B[kTileR][9];
      tile_covariance(P, q0, Npad, A, TileNoPerm{}, B);
      // ---- 2. per row: the rotation and the explicit rotated difference where a lane's pair counts
      const double Gj = G[jl];
      unsigned long long cs = 0ull;  // this column's share of the 4 rows
      double ce = 0.0;
#pragma unroll
      for (int r = 0; r < kTileR; ++r) {
        const bool ok = row[r] < j && j < se[r];  // the upper triangle of the row's group (se <= N)
        if (__ballot(ok) == 0) continue;          // (wave-uniform)
        // tile_rmsd's body, written out: as a call it compiles to the same instruction counts, but this kernel then
        // measured 4 ... 12 % slower (tools/bench_medoids.py; docs/rmsd_tile_measurements.md) -- k_knn_tile does not
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
        if (ok) {
          const unsigned long long qd = (unsigned long long)rint(d * 4294967296.0);
          rs[r] += qd;
          cs += qd;
          re[r] = fmax(re[r], d);
          ce = fmax(ce, d);
        }
      }
      if (cs != 0ull) atomicAdd(&sums[j], cs);  // (cs != 0 only where a pair counted: j < N)
      if (ce > 0.0) atomicMax(&ecc[j], (unsigned long long)__double_as_longlong(ce));
    }
    // ---- 3. the rows' sums over the strip: one atomic per row
#pragma unroll
    for (int r = 0; r < kTileR; ++r) {
      unsigned long long v = rs[r];
      double m = re[r];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        v += __shfl_xor(v, o);
        m = fmax(m, __shfl_xor(m, o));
      }
      if (lane == 0 && row[r] < N) {
        if (v != 0ull) atomicAdd(&sums[row[r]], v);
        if (m > 0.0) atomicMax(&ecc[row[r]], (unsigned long long)__double_as_longlong(m));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// k_group_sums_sym: the same sums under d_sym (include/fc_hip.h, fc_ensemble_medoids_perm)
//
//   d_sym(i, j) = min over p < K, h in H of rmsd(X[i][perms[p]], h * X[j]),   H = {+1} or, MIRROR, {+1, -1}
//
// the value k_knn_tile_sym (fc_knn.hip) writes for row i and column j, evaluated once per unordered pair as (row i,
// column j), i < j.  k_group_sums' items, triangle, ballot skip and integer atomics with the chunk walking the table as
// k_knn_tile_sym's does: the workgroup's 16 rows AND the table (16-bit indices) sit in LDS -- this form is staged only --
// and kSumSymR of the wavefront's rows share an atom loop, each such group of rows walking its own part of the strip.
// Per chunk and table row p: the covariances of the group's rows with the column; per row that counts in the chunk the
// Newton eigenvalue of B and -- MIRROR -- of -B, and a (p, h) goes through the rotation and the explicit pass unless its
// eigenvalue form of A msd exceeds the pair's smallest explicit sum so far by more than A kScreenMargin for EVERY
// counting lane of the wavefront (k_knn_tile_sym's second rule; there is no list, so no tau).  A pair's first (p, h)
// has nothing to be compared with and is always explicit; what is skipped is larger than what is kept, so the minimum
// -- and with it every output -- is the same bits with the filter on or off (FC_MEDOID_SYM_FILTER=0), for every strip
// count and for every kSumSymR.  After the K rows one q(sqrt(best / A)) per counting pair goes where k_group_sums sends it.
//
// stats (may be NULL): [0] += (pair, p, h) whose eigenvalue was formed, [1] += those taken through the explicit pass
// (the counting lanes of a wavefront that made the pass).
// ---------------------------------------------------------------------------
#ifdef FC_SUM_SYM_ROWS  // (a tuning build: fc_tuning.h)
constexpr int kSumSymR = FC_SUM_SYM_ROWS;
#else
// rows of a wavefront that share an atom loop: 2, as k_knn_tile_sym settled on (the resource report: DESIGN.md section 28)
constexpr int kSumSymR = 2;
#endif
static_assert(kTileR % kSumSymR == 0, "a wavefront's rows in whole groups");

template <bool MIRROR>
__global__ void __launch_bounds__(kTileThreads)
k_group_sums_sym(const double *__restrict__ Xs, const double *__restrict__ Xa, const double *__restrict__ G, int N, int64_t Npad,
                 int A, const uint16_t *__restrict__ perms, int K, int filter, const int32_t *__restrict__ seg_end, int n_tiles,
                 int S, unsigned long long *__restrict__ sums, unsigned long long *__restrict__ ecc,
                 unsigned long long *__restrict__ stats) {
  extern __shared__ double s_rows[];  // [kTileRows][A][3], then the table [K][A] as uint16_t
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int A3 = 3 * A;
  const double dA = (double)A;
  const double margin = dA * kScreenMargin;
  const int64_t n_items = (int64_t)n_tiles * S;
  uint16_t *pt = reinterpret_cast<uint16_t *>(s_rows + kTileRows * A3);
  for (int t = tid; t < K * A; t += kTileThreads) pt[t] = perms[t];
  __syncthreads();  // (an item without chunks stages no rows: the table does not wait for the first tile's barrier)
  unsigned long long n_formed = 0, n_explicit = 0;  // (wave-uniform: ballots)

  for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int tile = (int)(item / S), s = (int)(item % S);
    const int row0 = tile * kTileRows;
    // the tile's chunks of 64 columns: the columns behind its first row up to the end of its last row's group
    const int tb = (row0 + 1) >> 6, te = (seg_end[min(row0 + kTileRows - 1, N - 1)] + 63) >> 6;
    const int nt = max(te - tb, 0);
    const int c0 = tb + (int)((int64_t)s * nt / S), c1 = tb + (int)((int64_t)(s + 1) * nt / S);
    if (c0 >= c1) continue;  // (the same for the whole workgroup)
    tile_stage_rows(s_rows, Xa, row0, N, A3);
    // the wavefront's kTileR rows, kSumSymR at a time (wave-uniform; no barrier follows in this item)
    for (int wrow = row0 + w * kTileR; wrow < min(row0 + (w + 1) * kTileR, N); wrow += kSumSymR) {
      int row[kSumSymR], se[kSumSymR];
      const double *__restrict__ P[kSumSymR];
      double Gi[kSumSymR], re[kSumSymR];
      unsigned long long rs[kSumSymR];
      tile_rows<true>(s_rows, Xa, G, row0, wrow, N, A3, row, P, Gi);
#pragma unroll
      for (int r = 0; r < kSumSymR; ++r) {
        const int e = seg_end[min(row[r], N - 1)];
        se[r] = row[r] < N ? e : 0;  // (a row past the end counts nowhere)
        rs[r] = 0ull;
        re[r] = 0.0;
      }
      // the rows' own part of the strip: behind the first of them, up to the end of the last one's group
      const int wc0 = max(c0, (wrow + 1) >> 6), wc1 = min(c1, (seg_end[min(wrow + kSumSymR - 1, N - 1)] + 63) >> 6);
      for (int c = wc0; c < wc1; ++c) {
        const int j = c * 64 + lane;
        const int jl = min(j, N - 1);
        const double *__restrict__ q0 = Xs + jl;
        const double Gj = G[jl];
        bool ok[kSumSymR];
        unsigned long long okb[kSumSymR], any = 0ull;
        double best[kSumSymR];  // the pair's smallest explicit sum of squares so far
#pragma unroll
        for (int r = 0; r < kSumSymR; ++r) {
          ok[r] = row[r] < j && j < se[r];  // the upper triangle of the row's group (se <= N)
          okb[r] = __ballot(ok[r]);
          any |= okb[r];
          best[r] = INFINITY;
        }
        if (any == 0ull) continue;  // (wave-uniform)
#pragma nounroll
        for (int p = 0; p < K; ++p) {
          const uint16_t *__restrict__ pr = pt + p * A;
          // ---- 1. covariances of the column with the rows under row p of the table
          double B[kSumSymR][9];
          tile_covariance(P, q0, Npad, A, pr, B);
          // ---- 2. per row that counts here and handedness: the filter, the rotation and the explicit pass
#pragma unroll
          for (int r = 0; r < kSumSymR; ++r) {
            if (okb[r] == 0ull) continue;  // (wave-uniform)
            const double GG = Gi[r] + Gj;
            double lam_p = 0.0, lam_m = 0.0;
            if (filter) kabsch_lambda_max_both<MIRROR>(B[r], GG, lam_p, lam_m);
            n_formed += (unsigned long long)((MIRROR ? 2 : 1) * __popcll(okb[r]));
#pragma nounroll
            for (int h = 0; h < (MIRROR ? 2 : 1); ++h) {
              bool may = ok[r];
              if (filter) {  // (a NaN passes; best = +inf, the pair's first (p, h), passes)
                const double msdA = GG - 2.0 * (h ? lam_m : lam_p);
                may = ok[r] && !(msdA > best[r] + margin);
              }
              if (__ballot(may) == 0) continue;  // (wave-uniform) this (p, h) is ruled out for every pair of the chunk
              n_explicit += (unsigned long long)__popcll(okb[r]);
              const double ssq = tile_explicit_ssq<true>(P[r], q0, Npad, A, pr, B[r], GG, h ? -1.0 : 1.0);
              if (!(ssq >= best[r])) best[r] = ssq;
            }
          }
        }
        // ---- 3. one q(d_sym) per counting pair: to the row's sum and to the column's
        unsigned long long cs = 0ull;  // this column's share of the rows
        double ce = 0.0;
#pragma unroll
        for (int r = 0; r < kSumSymR; ++r) {
          if (ok[r]) {
            const double d = sqrt(best[r] / dA);
            const unsigned long long qd = (unsigned long long)rint(d * 4294967296.0);
            rs[r] += qd;
            cs += qd;
            re[r] = fmax(re[r], d);
            ce = fmax(ce, d);
          }
        }
        if (cs != 0ull) atomicAdd(&sums[j], cs);  // (cs != 0 only where a pair counted: j < N)
        if (ce > 0.0) atomicMax(&ecc[j], (unsigned long long)__double_as_longlong(ce));
      }
      // ---- 4. the rows' sums over the strip: one atomic per row
#pragma unroll
      for (int r = 0; r < kSumSymR; ++r) {
        unsigned long long v = rs[r];
        double m = re[r];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          v += __shfl_xor(v, o);
          m = fmax(m, __shfl_xor(m, o));
        }
        if (lane == 0 && row[r] < N) {
          if (v != 0ull) atomicAdd(&sums[row[r]], v);
          if (m > 0.0) atomicMax(&ecc[row[r]], (unsigned long long)__double_as_longlong(m));
        }
      }
    }
  }
  if (stats != nullptr && lane == 0 && n_formed) {  // (a bench hook's counters)
    atomicAdd(&stats[0], n_formed);
    atomicAdd(&stats[1], n_explicit);
  }
}

// strips a tile's chunk range is cut into: enough items to hand out evenly
int medoid_strips(int64_t N) { return tile_strips("FC_MEDOID_STRIPS", kTileItemsPerCu, kTileItemMaxStrips, N, N); }

// FC_MEDOID_SYM_FILTER=0: the explicit pass for every (p, h) of k_group_sums_sym and k_silhouette_tile_sym (speed and
// tests only: the outputs are the same bits either way)
int sums_sym_filter() {
  const char *v = getenv("FC_MEDOID_SYM_FILTER");
  return !(v && v[0] == '0' && v[1] == 0);
}

template <bool MIRROR>
static int launch_group_sums_sym_as(const fc_ensemble *e, const SymTable &sym, const int32_t *seg_end_dev, int n_tiles, int S,
                                    unsigned long long *sums_dev, unsigned long long *ecc_dev) {
  const size_t lds = knn_sym_lds_bytes(e->A, sym.K);
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_group_sums_sym<MIRROR>), lds, "k_group_sums_sym"));
  const unsigned gx = (unsigned)std::min<int64_t>((int64_t)n_tiles * S, (int64_t)1 << 20);
  hipLaunchKernelGGL((k_group_sums_sym<MIRROR>), dim3(gx), dim3(kTileThreads), lds, ctx().stream, e->Xs.as<double>(),
                     e->Xa.as<double>(), e->G.as<double>(), (int)e->N, e->Npad, (int)e->A, sym.perms_dev, sym.K, sums_sym_filter(),
                     seg_end_dev, n_tiles, S, sums_dev, ecc_dev, sym.stats_dev);
  return check_launch("k_group_sums_sym");
}

template <bool STAGE>
static int launch_group_sums_as(const fc_ensemble *e, const int32_t *seg_end_dev, int n_tiles, int S, unsigned long long *sums_dev,
                                unsigned long long *ecc_dev) {
  const size_t lds = STAGE ? tile_rows_lds_bytes(e->A) : 0;
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_group_sums<STAGE>), lds, "k_group_sums"));
  const unsigned gx = (unsigned)std::min<int64_t>((int64_t)n_tiles * S, (int64_t)1 << 20);
  hipLaunchKernelGGL((k_group_sums<STAGE>), dim3(gx), dim3(kTileThreads), lds, ctx().stream, e->Xs.as<double>(),
                     e->Xa.as<double>(), e->G.as<double>(), (int)e->N, e->Npad, (int)e->A, seg_end_dev, n_tiles, S, sums_dev,
                     ecc_dev);
  return check_launch("k_group_sums");
}

// S (out_dev[0 .. N)) and E (out_dev[N .. 2 N), the doubles' bit patterns), zeroed here, of the label-sorted ensemble e,
// 1 <= N < 2^31 - 256: seg_end_dev[i] = the end of the group of position i.  Enqueued only; timed: the context's events
// ev0 / ev1 are recorded around the zeroing and the kernel, for the caller to read behind its wait.
// sym (may be NULL): under d_sym -- k_group_sums_sym, whose rows and table fit the LDS (refused here otherwise; the entry
// points have refused it before any device use).
int launch_group_sums(const fc_ensemble *e, const int32_t *seg_end_dev, unsigned long long *out_dev, bool timed,
                      const SymTable *sym) {
  Context &c = ctx();
  const int S = medoid_strips(e->N);
  const int n_tiles = (int)ceil_div(e->N, kTileRows);
  if (sym && knn_sym_lds_bytes(e->A, sym->K) > kLdsLimit)
    return set_error(FC_E_LIMIT, "A_sel=%lld selected atoms with K=%d permutations need %zu bytes of LDS (limit %zu)",
                     (long long)e->A, sym->K, knn_sym_lds_bytes(e->A, sym->K), kLdsLimit);
  if (timed) FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  FC_HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)e->N * 2 * sizeof(unsigned long long), c.stream));
  if (sym)
    FC_TRY((sym->mirror ? launch_group_sums_sym_as<true> : launch_group_sums_sym_as<false>)(e, *sym, seg_end_dev, n_tiles, S, out_dev,
                                                                                         out_dev + e->N));
  else
    FC_TRY((e->A <= kTileLdsAtoms ? launch_group_sums_as<true> : launch_group_sums_as<false>)(e, seg_end_dev, n_tiles, S, out_dev,
                                                                                           out_dev + e->N));
  if (timed) FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  return FC_OK;
}

// ---------------------------------------------------------------------------
// k_ensemble_gather: conformer m of the new ensemble is conformer idx[m] of the old one -- Xs (zero beyond n and beyond
// the selected atoms, as k_prep leaves it), Xa and G, copied; gmax_bits (may be NULL): the largest G of the copy
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ensemble_gather(const double *__restrict__ Xs_in, const double *__restrict__ Xa_in, const double *__restrict__ G_in,
                  int64_t Npad_in, const int32_t *__restrict__ idx, int64_t n, int64_t Npad_out, int64_t A,
                  double *__restrict__ Xs_out, double *__restrict__ Xa_out, double *__restrict__ G_out,
                  unsigned long long *__restrict__ gmax_bits) {
  const int64_t A3 = 3 * A;
  const int64_t n_xs = ((A + 3) & ~(int64_t)3) * 3 * Npad_out, n_xa = n * A3;
  const int64_t total = n_xs > n_xa ? n_xs : n_xa;  // (n_xs >= Npad_out)
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    if (e < n_xs) {
      const int64_t r = e / Npad_out, m = e - r * Npad_out;
      Xs_out[e] = (r < A3 && m < n) ? Xs_in[r * Npad_in + idx[m]] : 0.0;
    }
    if (e < n_xa) {
      const int64_t m = e / A3, t = e - m * A3;
      Xa_out[e] = Xa_in[(int64_t)idx[m] * A3 + t];
    }
    if (e < Npad_out) {
      const double g = e < n ? G_in[idx[e]] : 0.0;
      G_out[e] = g;
      if (gmax_bits != nullptr && g == g) atomicMax(gmax_bits, (unsigned long long)__double_as_longlong(g));
    }
  }
}

// `out` (a fresh fc_ensemble) becomes the ensemble of the conformers idx_dev[0 .. n) of src, 0 <= idx < src->N, n >= 0.
// exact_gmax: the largest G of the copy is found and waited for (fc_ensemble_subset); otherwise src's stands in -- never
// smaller, which is the side every user of g_max is conservative on -- and nothing is waited for.
int ensemble_gather(const fc_ensemble *src, const int32_t *idx_dev, int64_t n, fc_ensemble *out, bool exact_gmax) {
  out->epoch = src->epoch;
  out->N = n, out->A = src->A;
  out->Npad = ceil_div(std::max<int64_t>(n, 1), 64) * 64;
  out->W = out->Npad / 64;
  out->sel_host = src->sel_host;
  FC_TRY(out->Xs.reserve((size_t)((out->A + 3) / 4 * 4) * 3 * out->Npad * sizeof(double)));
  FC_TRY(out->G.reserve((size_t)out->Npad * sizeof(double)));
  FC_TRY(out->Xa.reserve((size_t)std::max<int64_t>(n, 1) * out->A * 3 * sizeof(double)));
  FC_TRY(out->counters.reserve(kCounters * sizeof(uint64_t)));
  FC_HIP_TRY(hipMemsetAsync(out->counters.p, 0, kCounters * sizeof(uint64_t), ctx().stream));
  auto *gmax_dev = reinterpret_cast<unsigned long long *>(out->counters.p) + (kCounters - 1);
  const int64_t total = std::max(((out->A + 3) / 4 * 4) * 3 * out->Npad, n * out->A * 3);
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(total, 256), (int64_t)1 << 16);
  hipLaunchKernelGGL(k_ensemble_gather, dim3(grid), dim3(256), 0, ctx().stream, src->Xs.as<double>(), src->Xa.as<double>(),
                     src->G.as<double>(), src->Npad, idx_dev, n, out->Npad, out->A, out->Xs.as<double>(), out->Xa.as<double>(),
                     out->G.as<double>(), exact_gmax ? gmax_dev : nullptr);
  FC_TRY(check_launch("k_ensemble_gather"));
  out->g_max = src->g_max;
  if (exact_gmax) {
    unsigned long long bits = 0;
    FC_TRY(d2h(&bits, gmax_dev, sizeof bits));
    FC_TRY(sync());
    std::memcpy(&out->g_max, &bits, sizeof(double));
    FC_HIP_TRY(hipMemsetAsync(gmax_dev, 0, sizeof(unsigned long long), ctx().stream));
  }
  return FC_OK;
}

__global__ void k_warm_medoid() {}
int warm_medoid() {
  hipLaunchKernelGGL(k_warm_medoid, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_medoid");
}

}  // namespace fc
