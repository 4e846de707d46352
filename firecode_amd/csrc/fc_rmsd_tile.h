// fc_rmsd_tile.h -- the row tile "for every row conformer, over all column conformers, under the Kabsch RMSD" that
// k_knn_tile / k_knn_tile_sym (fc_knn.hip), k_group_sums / k_group_sums_sym (fc_medoid.hip) and k_silhouette_tile /
// k_silhouette_tile_sym (fc_silhouette.hip) walk, said once (DESIGN.md sections 18, 21, 25, 26 and 28), for gfx950
// (wave64, float64).
//
// A workgroup of kTileThreads = 256 threads takes kTileRows = 16 row conformers from the centred conformer-major copy Xa
// (24 B per atom), staged in LDS up to kTileLdsAtoms atoms and read from global memory beyond; each WAVEFRONT owns
// kTileR = 4 of the rows and walks its columns 64 at a time, one lane per column conformer, the column's coordinates
// read from the conformer-minor Xs (coalesced over conformers).  Per chunk: the covariances of the column with the rows
// in one atom loop (one load of the column's atom serves all of them, the row atoms are wave-uniform), and per row the
// rotation -- kabsch_rotation_qcp, the Jacobi sweeps of kabsch_rotation where the eigenvalue is not clearly simple --
// and the explicit rotated difference in a second atom loop, pair_exact_aos's sums.
// d(i, j) is one fixed instruction sequence over the atoms in order: it does not depend on the kernel, the tile, the
// strip or the lane a pair falls into, which is what the "same bits for every strip count" promises of the four
// kernels rest on.  What a kernel does with d -- lists, sums, scans -- and which pairs it skips stay with the kernel.
#pragma once

#include "fc_internal.h"
#include "fc_kabsch_math.h"

#include <cmath>
#include <cstdlib>

namespace fc {

constexpr int kTileThreads = 256;
constexpr int kTileR = 4;                                      // rows per wavefront
constexpr int kTileRows = (kTileThreads / 64) * kTileR;        // rows per workgroup
constexpr int64_t kTileLdsAtoms = 256;                         // 16 rows x A x 24 B = 96 KiB of LDS
// the tiles that hand out (row tile, strip) items (k_group_sums, k_silhouette_tile): items aimed at per CU -- the largest
// item is then a few percent of a CU's share -- and the most strips
constexpr int kTileItemsPerCu = 32;
constexpr int kTileItemMaxStrips = 64;

inline size_t tile_rows_lds_bytes(int64_t A) { return (size_t)kTileRows * (size_t)A * 3 * sizeof(double); }

// Column strips of `rows` row conformers against `cols` column conformers: enough (row tile, strip) workgroups for
// per_cu of them on every CU where the row tiles alone do not give that, at most max_strips and at most one per chunk
// of 64 columns; the environment variable `knob`=<n> forces it (speed and tests only: the outputs are the same bits
// for every value)
inline int tile_strips(const char *knob, int per_cu, int max_strips, int64_t rows, int64_t cols) {
  const int64_t n_chunks = std::max<int64_t>(1, ceil_div(cols, 64));
  int64_t S = 0;
  if (const char *v = getenv(knob)) {
    char *end = nullptr;
    const long long f = strtoll(v, &end, 10);
    if (end != v && *end == 0 && f >= 1) S = std::min<long long>(f, max_strips);
  }
  if (S == 0) {
    const int64_t tiles = std::max<int64_t>(1, ceil_div(rows, kTileRows));
    S = std::min<int64_t>(max_strips, ceil_div((int64_t)per_cu * std::max(1, ctx().n_cu), tiles));
  }
  return (int)std::max<int64_t>(1, std::min(S, n_chunks));
}

// the atom of the row side that stands against atom a of the column: a itself, or row p of a permutation table
// (uint16_t, in LDS) where one is passed in its place
struct TileNoPerm {
  __device__ __forceinline__ int operator[](int a) const { return a; }
};

// The workgroup's kTileRows rows from row0 on (rows past the end: copies of conformer N - 1) from Xa to s_rows
// [kTileRows][A][3].  Called by the whole workgroup.
__device__ __forceinline__ void tile_stage_rows(double *__restrict__ s_rows, const double *__restrict__ Xa, int row0, int N,
                                                int A3) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();  // (the previous item's readers)
  for (int r = w; r < kTileRows; r += kTileThreads / 64) {
    const double *__restrict__ src = Xa + (int64_t)min(row0 + r, N - 1) * A3;
    for (int t = lane; t < A3; t += 64) s_rows[r * A3 + t] = src[t];
  }
  __syncthreads();
}

// The R rows from wrow on, of the tile that begins at row0: their indices, atoms (STAGE: in s_rows, as tile_stage_rows
// left them) and sums of squares, the last two clamped by N - 1
template <bool STAGE, int R>
__device__ __forceinline__ void tile_rows(const double *__restrict__ s_rows, const double *__restrict__ Xa,
                                          const double *__restrict__ G, int row0, int wrow, int N, int A3, int (&row)[R],
                                          const double *__restrict__ (&P)[R], double (&Gi)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    row[r] = wrow + r;
    const int rl = min(row[r], N - 1);
    P[r] = STAGE ? s_rows + (wrow - row0 + r) * A3 : Xa + (int64_t)rl * A3;
    Gi[r] = G[rl];
  }
}

// B[r] = sum over the atoms a of P[r][perm[a]] q_a^T, q the column conformer at q0 in Xs: one load of q_a serves the R rows
template <int R, class Perm>
__device__ __forceinline__ void tile_covariance(const double *__restrict__ const (&P)[R], const double *__restrict__ q0,
                                                int64_t Npad, int A, Perm perm, double (&B)[R][9]) {
  const int64_t step = 3 * Npad;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 9; ++e) B[r][e] = 0.0;
  const double *__restrict__ qa = q0;
#pragma unroll 2
  for (int a = 0; a < A; ++a, qa += step) {
    const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
    const int b = (int)perm[a] * 3;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double px = P[r][b], py = P[r][b + 1], pz = P[r][b + 2];
      B[r][0] = fma(px, qx, B[r][0]); B[r][1] = fma(px, qy, B[r][1]); B[r][2] = fma(px, qz, B[r][2]);
      B[r][3] = fma(py, qx, B[r][3]); B[r][4] = fma(py, qy, B[r][4]); B[r][5] = fma(py, qz, B[r][5]);
      B[r][6] = fma(pz, qx, B[r][6]); B[r][7] = fma(pz, qy, B[r][7]); B[r][8] = fma(pz, qz, B[r][8]);
    }
  }
}

// The explicit sum of squares of one row against the column under the rotation of its covariance B (GG: the two sums
// of squares).  SIGNED: of (p, sg * q[perm]), sg = +1 or -1, as pair_exact_aos<INV> forms it -- sg B, p - sg R q;
// otherwise sg is not read and nothing is multiplied by it.
template <bool SIGNED, class Perm>
__device__ __forceinline__ double tile_explicit_ssq(const double *__restrict__ P, const double *__restrict__ q0, int64_t Npad, int A,
                                                    Perm perm, const double (&B)[9], double GG, double sg) {
  const int64_t step = 3 * Npad;
  double R[9];
  if constexpr (SIGNED) {
    double Bh[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Bh[e] = sg * B[e];
    if (!kabsch_rotation_qcp(Bh, GG, R)) (void)kabsch_rotation(Bh, R);
  } else {
    if (!kabsch_rotation_qcp(B, GG, R)) (void)kabsch_rotation(B, R);
  }
  double ssq = 0.0;
  const double *__restrict__ qa = q0;
#pragma unroll 2
  for (int a = 0; a < A; ++a, qa += step) {
    const double qx = qa[0], qy = qa[Npad], qz = qa[2 * Npad];
    const int b = (int)perm[a] * 3;
    const double px = P[b], py = P[b + 1], pz = P[b + 2];
    const double rx = R[0] * qx + R[1] * qy + R[2] * qz;
    const double ry = R[3] * qx + R[4] * qy + R[5] * qz;
    const double rz = R[6] * qx + R[7] * qy + R[8] * qz;
    const double dx = px - (SIGNED ? sg * rx : rx), dy = py - (SIGNED ? sg * ry : ry), dz = pz - (SIGNED ? sg * rz : rz);
    ssq += dx * dx + dy * dy + dz * dz;
  }
  return ssq;
}

// d(row, column) of the plain form: the value that is written out, never the eigenvalue form
__device__ __forceinline__ double tile_rmsd(const double *__restrict__ P, const double *__restrict__ q0, int64_t Npad, int A,
                                            const double (&B)[9], double GG, double dA) {
  return sqrt(tile_explicit_ssq<false>(P, q0, Npad, A, TileNoPerm{}, B, GG, 1.0) / dA);
}

}  // namespace fc
