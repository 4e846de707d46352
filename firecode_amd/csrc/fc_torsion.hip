// fc_torsion.hip -- torsion-scan conformer generation and torsion
// fingerprints for gfx950 (wave64, float64).
//
// Replaces the inner loops of clustered_csearch / random_csearch
// (firecode/torsion_module.py:812-856, 514-556): per angle-set apply the
// non-zero dihedral rotations in order -- rotate_dihedral (prism_pruner.utils:
// axis = x[i2]-x[i3], centre x[i3], matrix rot_mat_from_pointer(axis, angle))
// -- test torsion_comp_check (torsion_module.py:894-918: any pair between the
// rotating side `mask` and the rest minus {i2,i3} closer than thresh) and
// back off in -5 degree steps, at most angle//5 times.
//
// One wavefront per angle-set: the conformer lives in the wave's LDS slice
// (A*3 doubles); a rotation is lane-per-atom; a clash test flattens the
// (rest x moving) rectangle over the 64 lanes and reduces with a ballot.
#include <hipcub/hipcub.hpp>

#include "fc_internal.h"
#include "fc_kabsch_math.h"

namespace fc {

// rot_mat_from_pointer: scalar-last quaternion [sin(a/2) n, cos(a/2)] -> matrix.  The sine and cosine of the half
// angle depend on the angle alone: callers that apply the same angle again and again (the 5-degree back-off of the
// scan: up to 60 steps per torsion) take them once (half_angle_sincos) -- same function, same argument, same bits.
__device__ __forceinline__ void half_angle_sincos(double angle_deg, double &sn, double &cs) {
  double a2 = angle_deg / 2.0;
  a2 *= 3.141592653589793 / 180.0;
  sincos(a2, &sn, &cs);
}
__device__ __forceinline__ void rot_from_axis_sincos(double ax, double ay, double az, double sn, double cs, double (&M)[9]) {
  const double nrm = sqrt((ax * ax + ay * ay) + az * az);
  const double q1 = sn * (ax / nrm), q2 = sn * (ay / nrm), q3 = sn * (az / nrm), q0 = cs;
  M[0] = 2.0 * (q0 * q0 + q1 * q1) - 1.0;
  M[1] = 2.0 * (q1 * q2 - q0 * q3);
  M[2] = 2.0 * (q1 * q3 + q0 * q2);
  M[3] = 2.0 * (q1 * q2 + q0 * q3);
  M[4] = 2.0 * (q0 * q0 + q2 * q2) - 1.0;
  M[5] = 2.0 * (q2 * q3 - q0 * q1);
  M[6] = 2.0 * (q1 * q3 - q0 * q2);
  M[7] = 2.0 * (q2 * q3 + q0 * q1);
  M[8] = 2.0 * (q0 * q0 + q3 * q3) - 1.0;
}
__device__ __forceinline__ void rot_from_axis_angle(double ax, double ay, double az,
                                                    double angle_deg, double (&M)[9]) {
  double sn, cs;
  half_angle_sincos(angle_deg, sn, cs);
  rot_from_axis_sincos(ax, ay, az, sn, cs, M);
}

// rotate the atoms flagged in `mask` about the i2 - i3 bond (origin i3) by the angle whose half-angle sine / cosine are
// given.  MaskPtr: global memory, or the level's copy in LDS (k_ts_level)
template <class MaskPtr>
__device__ __forceinline__ void rotate_masked_sc(double *x, int A, MaskPtr mask, int i2, int i3, double sn, double cs, int lane) {
  const double cx = x[i3 * 3], cy = x[i3 * 3 + 1], cz = x[i3 * 3 + 2];
  double M[9];
  rot_from_axis_sincos(x[i2 * 3] - cx, x[i2 * 3 + 1] - cy, x[i2 * 3 + 2] - cz, sn, cs, M);
  __builtin_amdgcn_wave_barrier();
  for (int a = lane; a < A; a += 64) {
    if (mask[a]) {
      const double px = x[a * 3] - cx, py = x[a * 3 + 1] - cy, pz = x[a * 3 + 2] - cz;
      x[a * 3] = ((M[0] * px + M[1] * py) + M[2] * pz) + cx;
      x[a * 3 + 1] = ((M[3] * px + M[4] * py) + M[5] * pz) + cy;
      x[a * 3 + 2] = ((M[6] * px + M[7] * py) + M[8] * pz) + cz;
    }
  }
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void rotate_masked(double *x, int A, const uint8_t *mask, int i2, int i3,
                                              double angle, int lane) {
  double sn, cs;
  half_angle_sincos(angle, sn, cs);
  rotate_masked_sc(x, A, mask, i2, i3, sn, cs, lane);
}

// true when no (rest, moving) pair is closer than thresh (max_clashes = 0 is
// the only value the reference ever passes: torsion_module.py:827,838)
// pre_r / pre_m (may be nullptr): the lane's (rest, moving) atom of the first kPrePairs rounds of 64 pairs, worked out once by
// a caller that checks the same torsion again and again (k_ts_level: one torsion per launch)
#if defined(FC_TFD_STAMPS)
// tuning build: counters of the scan tree's last level (tools/ts_stamps.py)
__device__ unsigned long long g_ts_stamps[16];
#define FC_TS_ADD(k, v) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_ts_stamps[k], (unsigned long long)(v)); } while (0)
#define FC_TS_NOW() wall_clock64()
#else
#define FC_TS_ADD(k, v) do { } while (0)
#define FC_TS_NOW() 0ull
#endif
constexpr int kPrePairs = 4;
template <class IdxPtr>
__device__ __forceinline__ bool comp_check(const double *x, IdxPtr mv, int nmv, IdxPtr rs, int nrs, double thr2, int lane,
                                           const int *pre_r = nullptr, const int *pre_m = nullptr) {
  bool hit = false;
  const int total = nmv * nrs;
  for (int p0 = 0; p0 < total; p0 += 64) {
    const int p = p0 + lane;
    if (p < total) {
      int r, m;
      if (pre_r != nullptr && p0 < kPrePairs * 64) r = pre_r[p0 >> 6], m = pre_m[p0 >> 6];
      else r = rs[p / nmv], m = mv[p % nmv];
      const double dx = x[r * 3] - x[m * 3], dy = x[r * 3 + 1] - x[m * 3 + 1],
                   dz = x[r * 3 + 2] - x[m * 3 + 2];
      const double d2 = ((dx * dx) + dy * dy) + dz * dz;
      hit = hit || (d2 < thr2);
    }
    if (__any(hit)) return false;
  }
  return true;
}


// dihedral (prism_pruner.algebra.dihedral, "praxeolitic" form) per lane
__device__ __forceinline__ double dihedral_deg(const double *p0, const double *p1, const double *p2,
                                               const double *p3) {
  const double b0x = -1.0 * (p1[0] - p0[0]), b0y = -1.0 * (p1[1] - p0[1]), b0z = -1.0 * (p1[2] - p0[2]);
  double b1x = p2[0] - p1[0], b1y = p2[1] - p1[1], b1z = p2[2] - p1[2];
  const double b2x = p3[0] - p2[0], b2y = p3[1] - p2[1], b2z = p3[2] - p2[2];
  const double n1 = sqrt((b1x * b1x + b1y * b1y) + b1z * b1z);
  b1x /= n1; b1y /= n1; b1z /= n1;
  const double d0 = (b0x * b1x + b0y * b1y) + b0z * b1z;
  const double d2 = (b2x * b1x + b2y * b1y) + b2z * b1z;
  const double vx = b0x - d0 * b1x, vy = b0y - d0 * b1y, vz = b0z - d0 * b1z;
  const double wx = b2x - d2 * b1x, wy = b2y - d2 * b1y, wz = b2z - d2 * b1z;
  const double xx = (vx * wx + vy * wy) + vz * wz;
  const double cx = b1y * vz - b1z * vy, cy = b1z * vx - b1x * vz, cz = b1x * vy - b1y * vx;
  const double yy = (cx * wx + cy * wy) + cz * wz;
  return atan2(yy, xx) * (180.0 / 3.141592653589793);
}

// One torsion step of the scan (torsion_module.py:826-846): rotate by `angle`; on a clash step back by `backoff` degrees up
// to angle // backoff times until the clash is gone.  Returns 1 when the bond ends up rotated.
// sc_angle / sc_back (may be nullptr): {sin, cos} of half the angle / of half the back-off step, taken from a table by a
// caller that meets the same few angles again and again (k_ts_level) -- half_angle_sincos of the same argument;
// cs_steps (may be nullptr): {cos, sin} of b back-off angles, b = 1 .. kBackTab (see the closed form below)
constexpr int kBackTab = 64;
template <class MaskPtr, class IdxPtr>
__device__ __forceinline__ int torsion_step(double *x, int A, MaskPtr mask, IdxPtr mv, int nm, IdxPtr rs, int nr, int i2, int i3,
                                            int angle, int backoff, double thr2, int lane, const int *pre_r = nullptr,
                                            const int *pre_m = nullptr, const double *sc_angle = nullptr,
                                            const double *sc_back = nullptr, const double *cs_steps = nullptr) {
  double sn, cs;
  if (sc_angle != nullptr) sn = sc_angle[0], cs = sc_angle[1];
  else half_angle_sincos((double)angle, sn, cs);
  rotate_masked_sc(x, A, mask, i2, i3, sn, cs, lane);
  if (comp_check(x, mv, nm, rs, nr, thr2, lane, pre_r, pre_m)) return 1;
  int steps = angle / backoff;  // Python floor division: range(angle // backoff)
  if ((angle % backoff != 0) && ((angle < 0) != (backoff < 0))) --steps;
  if (steps <= 0) return 0;
  if (sc_back != nullptr) sn = sc_back[0], cs = sc_back[1];
  else half_angle_sincos((double)(-backoff), sn, cs);  // once for all the steps
  if (!mask[i2] && !mask[i3]) {
    // the two axis atoms stay where they are, so every step applies the SAME matrix about the same point: built once
    // (from the same numbers by the same operations: the steps' coordinates keep their bits)
    const double cx = x[i3 * 3], cy = x[i3 * 3 + 1], cz = x[i3 * 3 + 2];
    double M[9];
    rot_from_axis_sincos(x[i2 * 3] - cx, x[i2 * 3 + 1] - cy, x[i2 * 3 + 2] - cz, sn, cs, M);
    // WHICH step ends the loop, without walking it.  A moving atom goes round a circle about the axis, so its squared
    // distance to a resting atom after b steps is  c0 + c1 cos(b d) + c2 sin(b d)  (d = the back-off angle; R, P = the
    // two atoms from the axis point, n the axis:  c0 = |R|^2 + |P|^2 - 2 (R.n)(P.n),  c1 = -2 (R.P - (R.n)(P.n)),
    // c2 = 2 R.(n x P)  for the rotation by -d the matrix above makes).  Every lane holds its pairs' three numbers and
    // tests step after step with two multiply-adds per pair -- against a rotation of the moving atoms through LDS
    // and a clash check of all pairs per step (cfg3: 47 % of the 1.7 M leaves clash, 19 steps each: half the
    // scan's time).  The closed form differs from the walked coordinates by roundings (<= 4e-14 (|R|^2 + |P|^2 + 1)
    // over 60 steps, tools/ check in DESIGN 5.4); a pair within 1e-10 (|R|^2 + |P|^2 + 1) of the threshold at any step
    // looked at sends the node to the loop below, which decides as before.  The step found, the moving atoms are
    // turned that many times by the same operations as the loop's: same coordinates, bit for bit.
    const int total_pairs = nm * nr;
    if (pre_r != nullptr && cs_steps != nullptr && steps <= kBackTab && total_pairs <= kPrePairs * 64) {
      const double ax = x[i2 * 3] - cx, ay = x[i2 * 3 + 1] - cy, az = x[i2 * 3 + 2] - cz;
      const double inv = 1.0 / sqrt((ax * ax + ay * ay) + az * az);  // (the closed form needs the axis to ~1e-15, not to the bit)
      const double nx = ax * inv, ny = ay * inv, nz = az * inv;
      // per pair: c0, c1, c2 and the threshold pulled down / pushed up by the guard: below `lo` a clash for certain,
      // at or above `hi` none for certain
      double c0[kPrePairs], c1[kPrePairs], c2[kPrePairs], lo[kPrePairs], hi[kPrePairs];
#pragma unroll
      for (int q = 0; q < kPrePairs; ++q) {
        c0[q] = 1.0e300, c1[q] = 0.0, c2[q] = 0.0, lo[q] = thr2, hi[q] = thr2;  // (no pair: never a clash, never in doubt)
        if (q * 64 + lane < total_pairs) {
          const int r = pre_r[q], m = pre_m[q];
          const double Rx = x[r * 3] - cx, Ry = x[r * 3 + 1] - cy, Rz = x[r * 3 + 2] - cz;
          const double Px = x[m * 3] - cx, Py = x[m * 3 + 1] - cy, Pz = x[m * 3 + 2] - cz;
          const double Rn = Rx * nx + Ry * ny + Rz * nz, Pn = Px * nx + Py * ny + Pz * nz;
          const double RP = Rx * Px + Ry * Py + Rz * Pz, S = (Rx * Rx + Ry * Ry + Rz * Rz) + (Px * Px + Py * Py + Pz * Pz);
          const double kx = ny * Pz - nz * Py, ky = nz * Px - nx * Pz, kz = nx * Py - ny * Px;
          c0[q] = S - 2.0 * Rn * Pn;
          c1[q] = -2.0 * (RP - Rn * Pn);
          c2[q] = 2.0 * (Rx * kx + Ry * ky + Rz * kz);
          const double gd = 1.0e-10 * (S + 1.0);
          lo[q] = thr2 - gd, hi[q] = thr2 + gd;
        }
      }
      const int rounds = (total_pairs + 63) >> 6;
      int found = 0;  // the first step without a clash; -1: undecided (a pair too near the threshold)
      // A few steps per turn: their table values requested together, the pairs' tests in one straight line (a
      // step at a time the loop was a chain of LDS round trips and branches: 8 us per clashing node at two wavefronts
      // per SIMD).  A step at which SOME pair is below `lo` is a clash whatever the pairs near the threshold do: two
      // multiply-adds and one compare (straight into a lane mask) per pair and step; only the first step without such
      // a pair is looked at again -- every pair must be at or above `hi` there, or the node goes to the walked loop.
#ifndef FC_TS_TURN
#define FC_TS_TURN 4
#endif
      constexpr int kTurn = FC_TS_TURN;  // steps per turn (cfg3's last level: 3.20 ms with 4 or 2; with 8 -- 32 registers of table
                                         // values, 352 B of scratch -- 4.25, slower than the per-pair doubt test it replaced: 3.75)
      for (int b0 = 1; b0 <= steps && found == 0; b0 += kTurn) {
        double cb[kTurn], sb[kTurn];
#pragma unroll
        for (int u = 0; u < kTurn; ++u) {
          const int at = (b0 + u <= kBackTab ? b0 + u : kBackTab) - 1;
          cb[u] = cs_steps[2 * at], sb[u] = cs_steps[2 * at + 1];
        }
        uint64_t sure[kTurn];  // per step: the lanes with a pair below `lo`
#pragma unroll
        for (int u = 0; u < kTurn; ++u) {
          sure[u] = 0ull;
#pragma unroll
          for (int q = 0; q < kPrePairs; ++q) {
            if (q >= rounds) break;  // (uniform)
            sure[u] |= __ballot(fma(c2[q], sb[u], fma(c1[q], cb[u], c0[q])) < lo[q]);
          }
        }
#pragma unroll
        for (int u = 0; u < kTurn; ++u) {
          if (b0 + u > steps) break;  // (uniform)
          if (sure[u] != 0ull) continue;
          bool doubt = false;  // no certain clash at this step: is every pair certainly clear?
#pragma unroll
          for (int q = 0; q < kPrePairs; ++q) {
            if (q >= rounds) break;
            doubt = doubt || fma(c2[q], sb[u], fma(c1[q], cb[u], c0[q])) < hi[q];
          }
          found = __any(doubt) ? -1 : b0 + u;
          break;
        }
      }
      if (found >= 0) {
        const int turns = found > 0 ? found : steps;
        __builtin_amdgcn_wave_barrier();
        for (int a = lane; a < A; a += 64) {
          if (mask[a]) {
            double X0 = x[a * 3], X1 = x[a * 3 + 1], X2 = x[a * 3 + 2];
            for (int b = 0; b < turns; ++b) {
              const double px = X0 - cx, py = X1 - cy, pz = X2 - cz;
              X0 = ((M[0] * px + M[1] * py) + M[2] * pz) + cx;
              X1 = ((M[3] * px + M[4] * py) + M[5] * pz) + cy;
              X2 = ((M[6] * px + M[7] * py) + M[8] * pz) + cz;
            }
            x[a * 3] = X0, x[a * 3 + 1] = X1, x[a * 3 + 2] = X2;
          }
        }
        __builtin_amdgcn_wave_barrier();
        return found > 0 ? 1 : 0;
      }
    }
    for (int b = 0; b < steps; ++b) {
      __builtin_amdgcn_wave_barrier();
      for (int a = lane; a < A; a += 64) {
        if (mask[a]) {
          const double px = x[a * 3] - cx, py = x[a * 3 + 1] - cy, pz = x[a * 3 + 2] - cz;
          x[a * 3] = ((M[0] * px + M[1] * py) + M[2] * pz) + cx;
          x[a * 3 + 1] = ((M[3] * px + M[4] * py) + M[5] * pz) + cy;
          x[a * 3 + 2] = ((M[6] * px + M[7] * py) + M[8] * pz) + cz;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (comp_check(x, mv, nm, rs, nr, thr2, lane, pre_r, pre_m)) return 1;
    }
    return 0;
  }
  for (int b = 0; b < steps; ++b) {
    rotate_masked_sc(x, A, mask, i2, i3, sn, cs, lane);
    if (comp_check(x, mv, nm, rs, nr, thr2, lane, pre_r, pre_m)) return 1;
  }
  return 0;
}

__global__ void __launch_bounds__(256)
k_torsion_scan(const double *__restrict__ base, int A, const int64_t *__restrict__ torsions, int T,
               const uint8_t *__restrict__ rotmasks, const int16_t *__restrict__ mv_idx,
               const int16_t *__restrict__ rs_idx, const int32_t *__restrict__ n_mv,
               const int32_t *__restrict__ n_rs, const int64_t *__restrict__ angles, int64_t S,
               double thr2, int backoff, double *__restrict__ out, int64_t *__restrict__ rotated,
               const int64_t *__restrict__ quads, int Q, double *__restrict__ tf) {
  extern __shared__ double s[];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  double *x = s + (size_t)wv * A * 3;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + wv;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t sidx = wave0; sidx < S; sidx += nwaves) {
    for (int k = lane; k < A * 3; k += 64) x[k] = base[k];
    __builtin_amdgcn_wave_barrier();
    int rot = 0;
    for (int t = 0; t < T; ++t) {
      const int angle = (int)angles[sidx * T + t];
      if (angle == 0) continue;
      const int i2 = (int)torsions[t * 4 + 1], i3 = (int)torsions[t * 4 + 2];
      const uint8_t *mask = rotmasks + (size_t)t * A;
      const int16_t *mv = mv_idx + (size_t)t * A;
      const int16_t *rs = rs_idx + (size_t)t * A;
      const int nm = n_mv[t], nr = n_rs[t];
      rot += torsion_step(x, A, mask, mv, nm, rs, nr, i2, i3, angle, backoff, thr2, lane);
    }
    if (out != nullptr) {
      double *o = out + sidx * (int64_t)A * 3;
      for (int k = lane; k < A * 3; k += 64) o[k] = x[k];
    }
    // torsion fingerprint of the conformer while it is still in LDS (get_torsion_fingerprint,
    // torsion_module.py:1070-1077): the same doubles a separate pass over `out` would read
    if (tf != nullptr)
      for (int q = lane; q < Q; q += 64)
        tf[sidx * (int64_t)Q + q] = dihedral_deg(x + quads[q * 4] * 3, x + quads[q * 4 + 1] * 3,
                                                 x + quads[q * 4 + 2] * 3, x + quads[q * 4 + 3] * 3);
    if (lane == 0) rotated[sidx] = rot;
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------
// k_rotcorr_simbits: similarity bits of prune_by_rmsd_rot_corr (a7,
// prism_pruner.pruner; call sites firecode/ensemble.py:253-260,
// embedder.py:1489-1496).  The third-party source is not in the tree; restated
// after the predecessor's published routine (TSCoDe,
// rotationally_corrected_rmsd_and_max) -- PARITY UNPINNED:
//   for every locally symmetric torsion t (in order), for every angle of its
//   n-fold set (0 first): rotate ONLY atom i4 of the second structure about the
//   i2-i3 bond and take the Kabsch RMSD of the four torsion atoms against the
//   first structure; the first angle with the smallest local RMSD is then
//   applied to the whole rotating side (rotation mask); finally
//   rmsd_and_max over the heavy atoms decides: rmsd < max_rmsd && maxdev < max_dev.
// One wavefront per pair (i, j > i): the second structure lives in the wave's
// LDS slice, lanes = trial angles for the local fit, lanes = atoms for the
// rotations and the final superposition.  X is centred (N, A, 3).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_rotcorr_simbits(const double *__restrict__ X, int64_t N, int A, const uint8_t *__restrict__ heavy,
                  const int64_t *__restrict__ torsions, int T, const uint8_t *__restrict__ rotmasks,
                  const double *__restrict__ angles, const int32_t *__restrict__ n_angles, int max_angles,
                  double max_rmsd, double max_dev, const double *__restrict__ energies, double max_dE,
                  unsigned long long *__restrict__ bits, int64_t W) {
  extern __shared__ double s[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 4 + wv;
  if (j <= i || j >= N) return;
  if (energies != nullptr && !(fabs(energies[i] - energies[j]) < max_dE)) return;
  double *x = s + (size_t)wv * A * 3;
  const double *ref = X + i * (int64_t)A * 3;
  const double *src = X + j * (int64_t)A * 3;
  for (int k = lane; k < A * 3; k += 64) x[k] = src[k];
  __builtin_amdgcn_wave_barrier();
  for (int t = 0; t < T; ++t) {
    const int i1 = (int)torsions[t * 4], i2 = (int)torsions[t * 4 + 1], i3 = (int)torsions[t * 4 + 2],
              i4 = (int)torsions[t * 4 + 3];
    const int na = n_angles[t];
    double local = 1.0e300;
    double my_angle = 0.0;
    if (lane < na) {
      my_angle = angles[(size_t)t * max_angles + lane];
      const int id[4] = {i1, i2, i3, i4};
      double p[4][3], q[4][3];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          p[k][c] = ref[id[k] * 3 + c];
          q[k][c] = x[id[k] * 3 + c];
        }
      double M[9];
      rot_from_axis_angle(q[1][0] - q[2][0], q[1][1] - q[2][1], q[1][2] - q[2][2], my_angle, M);
      const double rx = q[3][0] - q[2][0], ry = q[3][1] - q[2][1], rz = q[3][2] - q[2][2];
      q[3][0] = ((M[0] * rx + M[1] * ry) + M[2] * rz) + q[2][0];
      q[3][1] = ((M[3] * rx + M[4] * ry) + M[5] * rz) + q[2][1];
      q[3][2] = ((M[6] * rx + M[7] * ry) + M[8] * rz) + q[2][2];
      double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) B[a * 3 + b] = fma(p[k][a], q[k][b], B[a * 3 + b]);
      double R[9];
      (void)kabsch_rotation(B, R);
      double ssq = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double dx = p[k][0] - (R[0] * q[k][0] + R[1] * q[k][1] + R[2] * q[k][2]);
        const double dy = p[k][1] - (R[3] * q[k][0] + R[4] * q[k][1] + R[5] * q[k][2]);
        const double dz = p[k][2] - (R[6] * q[k][0] + R[7] * q[k][1] + R[8] * q[k][2]);
        ssq += dx * dx + dy * dy + dz * dz;
      }
      local = sqrt(ssq / 4.0);
    }
    // first angle with the smallest local RMSD (the reference compares with a strict <)
    int best_lane = lane;
    double best = local;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ob = __shfl_xor(best, off);
      const int ol = __shfl_xor(best_lane, off);
      if (ob < best || (ob == best && ol < best_lane)) {
        best = ob;
        best_lane = ol;
      }
    }
    const double corr = __shfl(my_angle, best_lane);
    if (corr != 0.0) rotate_masked(x, A, rotmasks + (size_t)t * A, i2, i3, corr, lane);
  }
  // rmsd_and_max(ref[heavy], x[heavy]) -- Kabsch without centring
  double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int nh = 0;
  for (int a = lane; a < A; a += 64) {
    if (heavy[a]) {
      ++nh;
      const double px = ref[a * 3], py = ref[a * 3 + 1], pz = ref[a * 3 + 2];
      const double qx = x[a * 3], qy = x[a * 3 + 1], qz = x[a * 3 + 2];
      B[0] = fma(px, qx, B[0]); B[1] = fma(px, qy, B[1]); B[2] = fma(px, qz, B[2]);
      B[3] = fma(py, qx, B[3]); B[4] = fma(py, qy, B[4]); B[5] = fma(py, qz, B[5]);
      B[6] = fma(pz, qx, B[6]); B[7] = fma(pz, qy, B[7]); B[8] = fma(pz, qz, B[8]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 9; ++e) B[e] += __shfl_xor(B[e], off);
    nh += __shfl_xor(nh, off);
  }
  double R[9];
  (void)kabsch_rotation(B, R);
  double ssq = 0.0, mx = 0.0;
  for (int a = lane; a < A; a += 64) {
    if (heavy[a]) {
      const double qx = x[a * 3], qy = x[a * 3 + 1], qz = x[a * 3 + 2];
      const double dx = ref[a * 3] - (R[0] * qx + R[1] * qy + R[2] * qz);
      const double dy = ref[a * 3 + 1] - (R[3] * qx + R[4] * qy + R[5] * qz);
      const double dz = ref[a * 3 + 2] - (R[6] * qx + R[7] * qy + R[8] * qz);
      const double d = dx * dx + dy * dy + dz * dz;
      ssq += d;
      mx = fmax(mx, d);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ssq += __shfl_xor(ssq, off);
    mx = fmax(mx, __shfl_xor(mx, off));
  }
  const double rmsd = sqrt(ssq / (double)nh), maxdev = sqrt(mx);
  if (lane == 0 && rmsd < max_rmsd && maxdev < max_dev) atomicOr(&bits[i * W + (j >> 6)], 1ull << (j & 63));
}

__global__ void __launch_bounds__(256)
k_torsion_fingerprint(const double *__restrict__ coords, int64_t N, int64_t A,
                      const int64_t *__restrict__ quads, int Q, double *__restrict__ tf) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N * Q) return;
  const int64_t n = g / Q;
  const int q = (int)(g % Q);
  const double *x = coords + n * A * 3;
  tf[g] = dihedral_deg(x + quads[q * 4] * 3, x + quads[q * 4 + 1] * 3, x + quads[q * 4 + 2] * 3,
                       x + quads[q * 4 + 3] * 3);
}

// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// The scan as a PREFIX TREE.  The conformer after torsion k depends only on the angles of torsions
// 0..k (torsion_module.py:812-856 applies them in that order from the same start structure), so
// angle-sets that share a prefix share that work: for the 6^8 grid of BASELINE configs[2] the tree
// has sum_k 6^k = 2.0e6 single-torsion steps where one wavefront per angle-set does 8 * 6^8 = 13.4e6.
// Built on the device for ANY list of angle-sets (full grids, random subsets, duplicates):
//   1. distinct angle values per torsion column (LDS bitmaps) -> rank tables, bits per column;
//   2. code(row) = mixed-radix number of the column ranks, column 0 most significant; radix sort of
//      (code, row) pairs (hipcub) -- rows that share a prefix become adjacent;
//   3. d[i] = first column in which sorted row i differs from row i-1; node ids of level k are the
//      inclusive scan of (d <= k): node = a run of rows with equal prefix 0..k;
//   4. level k, one wavefront per node: parent state (level k-1, HBM) -> LDS, ONE torsion step with
//      exactly the code of k_torsion_scan (rotate, clash test, back-off), state -> HBM; the last level
//      writes conformer / fingerprint / rotated-bond count of every row of its run instead.
// Same arithmetic in the same order as k_torsion_scan: identical bits.
// ---------------------------------------------------------------------------
constexpr int kAngleOffset = 720, kAngleSpan = 2 * kAngleOffset + 1, kAngleWords = (kAngleSpan + 31) / 32;
constexpr int kMaxTreeT = 16;

struct ScanTreeMeta {
  int n[kMaxTreeT], bits[kMaxTreeT], shift[kMaxTreeT];
  int total_bits, bad;
};

__global__ void __launch_bounds__(256)
k_ts_presence(const int64_t *__restrict__ angles, int64_t S, int T, unsigned *__restrict__ present,
              int *__restrict__ bad) {
  extern __shared__ unsigned pres[];  // T x kAngleWords
  for (int k = threadIdx.x; k < T * kAngleWords; k += 256) pres[k] = 0u;
  __syncthreads();
  const int64_t total = S * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t a = angles[e];
    const int t = (int)(e % T);
    if (a < -kAngleOffset || a > kAngleOffset) {
      *bad = 1;
    } else {
      const int v = (int)a + kAngleOffset;
      atomicOr(&pres[t * kAngleWords + (v >> 5)], 1u << (v & 31));
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < T * kAngleWords; k += 256)
    if (pres[k]) atomicOr(&present[k], pres[k]);
}

// rank[t][v]: number of present angle values below v; one wavefront per torsion (a single thread walking T x 1 441
// values was 0.2 ms of every search), the counts per 32-value word by prefix sum over the wavefront
__global__ void __launch_bounds__(64)
k_ts_ranks(const unsigned *__restrict__ present, int T, uint16_t *__restrict__ rank, ScanTreeMeta *__restrict__ meta,
           const int *__restrict__ bad) {
  __shared__ int s_n[kMaxTreeT];
  const int lane = threadIdx.x;
  for (int t = 0; t < T; ++t) {
    int before = 0;  // present values in the words in front of this lane's
    for (int w0 = 0; w0 < kAngleWords; w0 += 64) {
      const int w = w0 + lane;
      const unsigned bits = w < kAngleWords ? present[t * kAngleWords + w] : 0u;
      int incl = __popc(bits);
      const int mine = incl;
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      int run = before + incl - mine;
      if (w < kAngleWords)
        for (int b = 0; b < 32; ++b) {
          const int v = w * 32 + b;
          if (v < kAngleSpan) rank[t * kAngleSpan + v] = (uint16_t)run;
          run += (int)((bits >> b) & 1u);
        }
      before += __shfl(incl, 63);
    }
    if (lane == 0) s_n[t] = before;
  }
  __syncthreads();
  if (lane != 0) return;
  int total = 0;
  for (int t = 0; t < T; ++t) {
    const int n = s_n[t];
    int b = 1;
    while ((1 << b) < n) ++b;
    meta->n[t] = n;
    meta->bits[t] = b;
    total += b;
  }
  int sh = total;
  for (int t = 0; t < T; ++t) {
    sh -= meta->bits[t];
    meta->shift[t] = sh;
  }
  meta->total_bits = total;
  meta->bad = *bad;
}

__global__ void __launch_bounds__(256)
k_ts_codes(const int64_t *__restrict__ angles, int64_t S, int T, const uint16_t *__restrict__ rank,
           const ScanTreeMeta *__restrict__ meta, uint64_t *__restrict__ code, uint32_t *__restrict__ row) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= S) return;
  uint64_t c = 0;
  for (int t = 0; t < T; ++t)
    c |= (uint64_t)rank[t * kAngleSpan + (int)angles[r * T + t] + kAngleOffset] << meta->shift[t];
  code[r] = c;
  row[r] = (uint32_t)r;
}

// d[i]: first column in which sorted row i differs from sorted row i - 1 (0 for i = 0, T for a duplicate)
__global__ void __launch_bounds__(256)
k_ts_firstdiff(const uint64_t *__restrict__ code, int64_t S, int T, const ScanTreeMeta *__restrict__ meta,
               uint8_t *__restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S) return;
  int lv = 0;
  if (i > 0) {
    const uint64_t x = code[i] ^ code[i - 1];
    lv = T;
    if (x) {
      const int msb = 63 - __clzll((long long)x);
      for (int t = 0; t < T; ++t)
        if (msb >= meta->shift[t]) {
          lv = t;
          break;
        }
    }
  }
  d[i] = (uint8_t)lv;
}

__global__ void __launch_bounds__(256)
k_ts_flags(const uint8_t *__restrict__ d, int64_t S, int level, int *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < S) flag[i] = d[i] <= level ? 1 : 0;
}

// first sorted row of every node of this level; first[M] = S closes the last run
__global__ void __launch_bounds__(256)
k_ts_first(const uint8_t *__restrict__ d, const int *__restrict__ nid, int64_t S, int level, int *__restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S) return;
  if (d[i] <= level) first[nid[i] - 1] = (int)i;
  if (i == S - 1) first[nid[i]] = (int)S;
}

// LDS of k_ts_level beside the four conformers: the level's index lists and mask, a table of the half-angle sines and
// cosines of the level's angles, and per wavefront the points of up to 64 dihedrals waiting for their turn
constexpr int kTsScTab = 64;
__host__ __device__ inline size_t ts_level_lds(int A) {
  return (size_t)4 * A * 3 * sizeof(double)                // conformers
         + (size_t)(kTsScTab + 1) * 2 * sizeof(double)     // sincos table, the back-off step's behind it
         + (size_t)kBackTab * 2 * sizeof(double)           // cos, sin of b back-off angles
         + (size_t)4 * 12 * 64 * sizeof(double)            // dihedral points [wave][12][64]
         + (size_t)4 * 64 * 3 * sizeof(int)                // rows of the waiting conformers [wave][3][64]: run begin, end, row[begin]
         + (size_t)A * 5 + 16;
}

// What a node of a level needs before its work can start, gathered by k_ts_nodes so that k_ts_level reads ONE record
// per node instead of walking first -> nid_prev / row -> angles / rot_prev -> state: four dependent global round
// trips per node, with sixteen wavefronts per CU to hide them, were the kernel (14.7 us per node and wavefront at the
// last level of cfg3 whatever the arithmetic did: neither the closed form of the back-off loop nor the batched
// dihedrals moved it)
struct TsNode {
  int i, i_end;   // the node's run of sorted rows
  int par;        // node of the previous level it continues (state_prev, rot_prev)
  int angle, rot; // the level's angle for this node; bonds rotated so far
  int sc;         // place of the angle in the level's table of half-angle sines and cosines
  unsigned row0;  // row[i]
  int pad;
};

__global__ void __launch_bounds__(256)
k_ts_nodes(const int *__restrict__ first, const int *__restrict__ nid_prev, const int *__restrict__ nid,
           const uint32_t *__restrict__ row, const int64_t *__restrict__ angles, const int *__restrict__ rot_prev,
           const uint16_t *__restrict__ rank, int64_t S, int T, int level, TsNode *__restrict__ nodes) {
  const int64_t M = nid[S - 1];
  const int64_t node = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (node >= M) return;
  TsNode n;
  n.i = first[node];
  n.i_end = first[node + 1];
  n.par = level == 0 ? 0 : nid_prev[n.i] - 1;
  n.row0 = row[n.i];
  n.angle = (int)angles[(int64_t)n.row0 * T + level];
  n.rot = level == 0 ? 0 : rot_prev[n.par];
  const int v = n.angle + kAngleOffset;
  n.sc = (v >= 0 && v < kAngleSpan) ? (int)rank[level * kAngleSpan + v] : 0;
  n.pad = 0;
  nodes[node] = n;
}

#ifndef FC_TS_WGS
#define FC_TS_WGS 4  // workgroups per CU the register budget is set for (128 registers, 272 B of scratch: 3.75 ms for cfg3's last level against 3.97 with three and 5.1 with two)
#endif
// (out of line: the rare fingerprints of more than 64 dihedrals must not cost the common path its registers)
__device__ __attribute__((noinline)) double dihedral_deg_at(const double *x, const int64_t *__restrict__ quad) {
  return dihedral_deg(x + quad[0] * 3, x + quad[1] * 3, x + quad[2] * 3, x + quad[3] * 3);
}

// kTsStateRounds: a node's state travels through registers, KR x 64 coordinates (3: 64 atoms, 6: 128 atoms; 0: not at all)
template <int KR>
__global__ void __launch_bounds__(256, FC_TS_WGS)
k_ts_level(const double *__restrict__ base, int A, const int64_t *__restrict__ torsions, int T, int level,
           const uint8_t *__restrict__ rotmasks, const int16_t *__restrict__ mv_idx, const int16_t *__restrict__ rs_idx,
           const int32_t *__restrict__ n_mv, const int32_t *__restrict__ n_rs, int64_t S, double thr2, int backoff,
           const uint32_t *__restrict__ row, const int *__restrict__ nid, const TsNode *__restrict__ nodes,
           const double *__restrict__ state_prev, double *__restrict__ state, int *__restrict__ rot_out,
           double *__restrict__ out, int64_t *__restrict__ rotated, const int64_t *__restrict__ quads, int Q,
           double *__restrict__ tf, const unsigned *__restrict__ present, const uint16_t *__restrict__ rank, int n_angles,
           int closed_form) {
  extern __shared__ double s[];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double *x = s + (size_t)wv * A * 3;
  double *sc_tab = s + (size_t)4 * A * 3;                       // [kTsScTab + 1][2]
  double *cs_steps = sc_tab + (kTsScTab + 1) * 2;              // [kBackTab][2]
  double *pts = cs_steps + kBackTab * 2 + (size_t)wv * 12 * 64;  // [12][64]
  int *wait_rows = reinterpret_cast<int *>(cs_steps + kBackTab * 2 + (size_t)4 * 12 * 64) + wv * 192;  // [3][64]
  const int64_t M = nid[S - 1];  // inclusive scan: number of nodes of this level
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + wv, nwaves = (int64_t)gridDim.x * 4;
  const int t = level;
  const int i2 = (int)torsions[t * 4 + 1], i3 = (int)torsions[t * 4 + 2];
  const int nm = n_mv[t], nr = n_rs[t];
  // the level's ONE torsion: its rotation mask and its moving / rest index lists are read in every step of every
  // back-off loop (up to 60 per node) -- from LDS, not through the vector cache
  int16_t *mv = reinterpret_cast<int16_t *>(wait_rows - wv * 192 + 4 * 192);
  int16_t *rs = mv + A;
  uint8_t *mask = reinterpret_cast<uint8_t *>(rs + A);
  for (int k = threadIdx.x; k < A; k += 256) {
    mv[k] = mv_idx[(size_t)t * A + k];
    rs[k] = rs_idx[(size_t)t * A + k];
    mask[k] = rotmasks[(size_t)t * A + k];
  }
  // the level's few angles (six in a six-fold scan) meet every node: sine and cosine of half of each once per
  // workgroup instead of once per node, the back-off step's as well (same function, same argument: same bits)
  const bool tab = n_angles <= kTsScTab;
  if (tab)
    for (int v = threadIdx.x; v < kAngleSpan; v += 256)
      if ((present[t * kAngleWords + (v >> 5)] >> (v & 31)) & 1u) {
        double sn, cs;
        half_angle_sincos((double)(v - kAngleOffset), sn, cs);
        sc_tab[2 * rank[t * kAngleSpan + v]] = sn;
        sc_tab[2 * rank[t * kAngleSpan + v] + 1] = cs;
      }
  if (threadIdx.x == 0) {
    double sn, cs;
    half_angle_sincos((double)(-backoff), sn, cs);
    sc_tab[2 * kTsScTab] = sn;
    sc_tab[2 * kTsScTab + 1] = cs;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 64 + kBackTab) {
    const int b = threadIdx.x - 64 + 1;
    double sn, cs;
    sincos((double)b * (double)backoff * (3.141592653589793 / 180.0), &sn, &cs);
    cs_steps[2 * (b - 1)] = cs;
    cs_steps[2 * (b - 1) + 1] = sn;
  }
  __syncthreads();
  int pre_r[kPrePairs], pre_m[kPrePairs];  // this lane's pairs of the first rounds of every clash check of the level
#pragma unroll
  for (int q = 0; q < kPrePairs; ++q) {
    const int p = q * 64 + lane;
    pre_r[q] = p < nm * nr ? rs[p / nm] : 0;
    pre_m[q] = p < nm * nr ? mv[p % nm] : 0;
  }
  const bool last = level == T - 1;
  // fingerprints of the last level: a conformer's Q dihedrals on Q lanes would run the long chain (two square roots,
  // three divisions, atan2) at Q / 64 of the machine; the points of 64 / Q conformers wait in LDS instead and are
  // turned into angles together
  const int per_turn = (tf != nullptr && Q > 0 && Q <= 64) ? 64 / Q : 0;
  int qa[4] = {0, 0, 0, 0};  // this lane's dihedral (lane < Q): its four atoms, once per kernel
  if (per_turn > 0 && lane < Q)
#pragma unroll
    for (int c = 0; c < 4; ++c) qa[c] = (int)quads[lane * 4 + c] * 3;
  int waiting = 0;
  auto flush = [&]() {
    __builtin_amdgcn_wave_barrier();
    if (lane < waiting * Q) {
      double p[12];
#pragma unroll
      for (int c = 0; c < 12; ++c) p[c] = pts[c * 64 + lane];
      const double d = dihedral_deg(p, p + 3, p + 6, p + 9);
      const int slot = lane / Q, q = lane - slot * Q;
      const int ib = wait_rows[slot], ie = wait_rows[64 + slot];
      tf[(int64_t)(unsigned)wait_rows[128 + slot] * Q + q] = d;
      for (int ii = ib + 1; ii < ie; ++ii) tf[(int64_t)row[ii] * Q + q] = d;  // (duplicate angle-sets)
    }
    __builtin_amdgcn_wave_barrier();
    waiting = 0;
  };
  // Two nodes ahead: the record of node n + 2 and the state of node n + 1 (whose record came a turn earlier) travel
  // while node n is worked on -- every global load of the loop is consumed a whole turn after it was issued.
  const int n3 = A * 3;
  constexpr int kTsStateRounds = KR > 0 ? KR : 1;
  const bool regs_ok = KR > 0 && n3 <= KR * 64;
  TsNode cur = {}, nxt = {};
  double st_cur[kTsStateRounds], st_nxt[kTsStateRounds];
  auto load_state = [&](const TsNode &nd, double (&st)[kTsStateRounds]) {
    const double *src = level == 0 ? base : state_prev + (int64_t)nd.par * n3;
#pragma unroll
    for (int r = 0; r < kTsStateRounds; ++r) {
      const int k = r * 64 + lane;
      st[r] = k < n3 ? src[k] : 0.0;
    }
  };
  int64_t node = wave0;
  if (node < M) cur = nodes[node];
  if (node + nwaves < M) nxt = nodes[node + nwaves];
  if (node < M && regs_ok) load_state(cur, st_cur);
  const unsigned long long tw0 = FC_TS_NOW();
  unsigned long long acc_n = 0, acc_a = 0, acc_nz = 0, acc_b = 0, acc_c = 0;
  for (; node < M; node += nwaves) {
    const unsigned long long ts0 = FC_TS_NOW();
    TsNode nn = {};
    if (node + 2 * nwaves < M) nn = nodes[node + 2 * nwaves];
    if (regs_ok && node + nwaves < M) load_state(nxt, st_nxt);
    if (regs_ok) {
#pragma unroll
      for (int r = 0; r < kTsStateRounds; ++r) {
        const int k = r * 64 + lane;
        if (k < n3) x[k] = st_cur[r];
      }
    } else {
      const double *src = level == 0 ? base : state_prev + (int64_t)cur.par * n3;
      for (int k = lane; k < n3; k += 64) x[k] = src[k];
    }
    __builtin_amdgcn_wave_barrier();
    const unsigned long long ts1 = FC_TS_NOW();
    int rot = cur.rot;
    const int angle = cur.angle;
    acc_n += 1; acc_a += ts1 - ts0; acc_nz += angle != 0;
    if (angle != 0)
      rot += torsion_step(x, A, mask, mv, nm, rs, nr, i2, i3, angle, backoff, thr2, lane, pre_r, pre_m,
                          tab ? sc_tab + 2 * cur.sc : nullptr, sc_tab + 2 * kTsScTab, closed_form ? cs_steps : nullptr);
    const unsigned long long ts2 = FC_TS_NOW();
    acc_b += ts2 - ts1;
    if (!last) {
      double *o = state + node * (int64_t)n3;
      for (int k = lane; k < n3; k += 64) o[k] = x[k];
      if (lane == 0) rot_out[node] = rot;
    } else {
      for (int ii = cur.i; ii < cur.i_end; ++ii) {  // every row of the run (more than one only for duplicate angle-sets)
        const int64_t r = ii == cur.i ? (int64_t)cur.row0 : (int64_t)row[ii];
        if (out != nullptr) {
          double *o = out + r * (int64_t)n3;
          for (int k = lane; k < n3; k += 64) o[k] = x[k];
        }
        if (tf != nullptr && per_turn == 0)
          for (int q = lane; q < Q; q += 64)
            tf[r * (int64_t)Q + q] = dihedral_deg_at(x, quads + q * 4);
        if (lane == 0) rotated[r] = rot;
      }
      if (per_turn > 0) {
        if (lane < Q) {
          const int at = waiting * Q + lane;
#pragma unroll
          for (int c = 0; c < 12; ++c) pts[c * 64 + at] = x[qa[c / 3] + c % 3];
        }
        if (lane == 0) wait_rows[waiting] = cur.i, wait_rows[64 + waiting] = cur.i_end, wait_rows[128 + waiting] = (int)cur.row0;
        if (++waiting == per_turn) flush();
      }
    }
    __builtin_amdgcn_wave_barrier();
    acc_c += FC_TS_NOW() - ts2;
    cur = nxt;
    nxt = nn;
#pragma unroll
    for (int r = 0; r < kTsStateRounds; ++r) st_cur[r] = st_nxt[r];
  }
  if (waiting > 0) flush();
  if (last) {
    FC_TS_ADD(8, FC_TS_NOW() - tw0); FC_TS_ADD(9, 1); FC_TS_ADD(0, acc_n); FC_TS_ADD(1, acc_nz); FC_TS_ADD(4, acc_a);
    FC_TS_ADD(5, acc_b); FC_TS_ADD(6, acc_c);
  }
  (void)acc_n; (void)acc_a; (void)acc_nz; (void)acc_b; (void)acc_c; (void)tw0;
}

#if defined(FC_TFD_STAMPS)
extern "C" int fc_debug_ts_stamps(unsigned long long *out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ts_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ts_stamps), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// returns FC_OK when the tree did the scan, 1 when it does not apply (the caller runs k_torsion_scan)
static int torsion_scan_tree(const double *base_dev, int64_t A, const int64_t *torsions_dev, int64_t T,
                             const uint8_t *rotmasks_dev, const int16_t *mv_dev, const int16_t *rs_dev,
                             const int32_t *nmv_dev, const int32_t *nrs_dev, const int64_t *angles_dev, int64_t S,
                             double thr2, int64_t backoff, double *out_dev, int64_t *rot_dev,
                             const int64_t *quads_dev, int64_t Q, double *tf_dev) {
  if (T < 2 || T > kMaxTreeT || S < 4096 || S >= (1ll << 31)) return 1;
  hipStream_t st = ctx().stream;
  DevBuf dpres, dbad, drank, dmeta;
  FC_TRY(dpres.reserve((size_t)T * kAngleWords * sizeof(unsigned)));
  FC_TRY(dbad.reserve(sizeof(int)));
  FC_TRY(drank.reserve((size_t)T * kAngleSpan * sizeof(uint16_t)));
  FC_TRY(dmeta.reserve(sizeof(ScanTreeMeta)));
  FC_HIP_TRY(hipMemsetAsync(dpres.p, 0, (size_t)T * kAngleWords * sizeof(unsigned), st));
  FC_HIP_TRY(hipMemsetAsync(dbad.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_ts_presence, dim3((unsigned)std::min<int64_t>(ceil_div(S * T, 256), ctx().n_cu * 8)), dim3(256),
                     (size_t)T * kAngleWords * sizeof(unsigned), st, angles_dev, S, (int)T, dpres.as<unsigned>(),
                     dbad.as<int>());
  hipLaunchKernelGGL(k_ts_ranks, dim3(1), dim3(64), 0, st, dpres.as<unsigned>(), (int)T, drank.as<uint16_t>(),
                     dmeta.as<ScanTreeMeta>(), dbad.as<int>());
  FC_TRY(check_launch("k_ts_ranks"));
  ScanTreeMeta meta;
  FC_TRY(d2h(&meta, dmeta.p, sizeof meta));
  FC_TRY(sync());
  if (meta.bad || meta.total_bits > 62) return 1;
  // node counts are bounded by the grid of distinct values; a level whose states would not fit
  // comfortably (sparse sets of very many rows) leaves the scan to the one-wave-per-row kernel
  std::vector<int64_t> bound((size_t)T);
  double prod = 1.0;
  for (int64_t t = 0; t < T; ++t) {
    prod = std::min(prod * (double)meta.n[t], (double)S);
    bound[(size_t)t] = (int64_t)prod;
  }
  const int64_t max_state_nodes = T >= 2 ? *std::max_element(bound.begin(), bound.end() - 1) : 0;
  // worth it only when prefixes are shared: total nodes well below S * T
  double total_nodes = 0.0;
  for (int64_t t = 0; t < T; ++t) total_nodes += (double)bound[(size_t)t];
  if (total_nodes > 0.6 * (double)S * (double)T) return 1;
  const size_t state_bytes = (size_t)max_state_nodes * (size_t)A * 3 * sizeof(double);
  if (2 * state_bytes > ((size_t)16 << 30)) return 1;
  DevBuf dcode, dcode2, drow, drow2, dd, dflag, dnid[2], dfirst, dstate[2], drotn[2], dtmp;
  FC_TRY(dcode.reserve((size_t)S * 8));
  FC_TRY(dcode2.reserve((size_t)S * 8));
  FC_TRY(drow.reserve((size_t)S * 4));
  FC_TRY(drow2.reserve((size_t)S * 4));
  FC_TRY(dd.reserve((size_t)S));
  FC_TRY(dflag.reserve((size_t)S * 4));
  FC_TRY(dnid[0].reserve((size_t)S * 4));
  FC_TRY(dnid[1].reserve((size_t)S * 4));
  FC_TRY(dfirst.reserve((size_t)(S + 1) * 4));
  FC_TRY(dstate[0].reserve(std::max<size_t>(state_bytes, 8)));
  FC_TRY(dstate[1].reserve(std::max<size_t>(state_bytes, 8)));
  FC_TRY(drotn[0].reserve((size_t)(max_state_nodes + 1) * 4));
  FC_TRY(drotn[1].reserve((size_t)(max_state_nodes + 1) * 4));
  DevBuf dnodes;
  FC_TRY(dnodes.reserve((size_t)(*std::max_element(bound.begin(), bound.end()) + 1) * sizeof(TsNode)));
  const unsigned gb = (unsigned)ceil_div(S, 256);
  if (ts_level_lds((int)A) > ((size_t)160 << 10)) return 1;
  hipLaunchKernelGGL(k_ts_codes, dim3(gb), dim3(256), 0, st, angles_dev, S, (int)T, drank.as<uint16_t>(),
                     dmeta.as<ScanTreeMeta>(), dcode.as<uint64_t>(), drow.as<uint32_t>());
  FC_TRY(check_launch("k_ts_codes"));
  size_t tmp_bytes = 0, tmp_scan = 0;
  FC_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, dcode.as<uint64_t>(), dcode2.as<uint64_t>(),
                                                drow.as<uint32_t>(), drow2.as<uint32_t>(), (int)S, 0,
                                                std::max(meta.total_bits, 1), st));
  FC_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, dflag.as<int>(), dnid[0].as<int>(), (int)S, st));
  FC_TRY(dtmp.reserve(std::max(tmp_bytes, tmp_scan)));
  size_t tb = dtmp.bytes;
  FC_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(dtmp.p, tb, dcode.as<uint64_t>(), dcode2.as<uint64_t>(),
                                                drow.as<uint32_t>(), drow2.as<uint32_t>(), (int)S, 0,
                                                std::max(meta.total_bits, 1), st));
  hipLaunchKernelGGL(k_ts_firstdiff, dim3(gb), dim3(256), 0, st, dcode2.as<uint64_t>(), S, (int)T,
                     dmeta.as<ScanTreeMeta>(), dd.as<uint8_t>());
  FC_TRY(check_launch("k_ts_firstdiff"));
  int closed_form = 1;  // FC_SCAN_CLOSED_FORM=0: every back-off loop walked step by step (A/B knob, per call)
  if (const char *v = getenv("FC_SCAN_CLOSED_FORM")) closed_form = v[0] != '0';
  for (int level = 0; level < (int)T; ++level) {
    DevBuf &nid = dnid[level & 1], &nid_prev = dnid[(level & 1) ^ 1];
    hipLaunchKernelGGL(k_ts_flags, dim3(gb), dim3(256), 0, st, dd.as<uint8_t>(), S, level, dflag.as<int>());
    tb = dtmp.bytes;
    FC_HIP_TRY(hipcub::DeviceScan::InclusiveSum(dtmp.p, tb, dflag.as<int>(), nid.as<int>(), (int)S, st));
    hipLaunchKernelGGL(k_ts_first, dim3(gb), dim3(256), 0, st, dd.as<uint8_t>(), nid.as<int>(), S, level,
                       dfirst.as<int>());
    const int64_t nodes = bound[(size_t)level];
    hipLaunchKernelGGL(k_ts_nodes, dim3((unsigned)ceil_div(nodes, 256)), dim3(256), 0, st, dfirst.as<int>(), nid_prev.as<int>(),
                       nid.as<int>(), drow2.as<uint32_t>(), angles_dev, drotn[(level & 1) ^ 1].as<int>(), drank.as<uint16_t>(), S,
                       (int)T, level, dnodes.as<TsNode>());
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(ceil_div(nodes, 4), (int64_t)ctx().n_cu * 32));
    auto kfn = A * 3 <= 192 ? k_ts_level<3> : A * 3 <= 384 ? k_ts_level<6> : k_ts_level<0>;
    if (level == 0 && ts_level_lds((int)A) > ((size_t)64 << 10))
      FC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)ts_level_lds((int)A)));
    hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(256), ts_level_lds((int)A), st, base_dev,
                       (int)A, torsions_dev, (int)T, level, rotmasks_dev, mv_dev, rs_dev, nmv_dev, nrs_dev, S,
                       thr2, (int)backoff, drow2.as<uint32_t>(), nid.as<int>(), dnodes.as<TsNode>(),
                       dstate[(level & 1) ^ 1].as<double>(), dstate[level & 1].as<double>(),
                       drotn[level & 1].as<int>(), out_dev, rot_dev, quads_dev, (int)Q, tf_dev, dpres.as<unsigned>(),
                       drank.as<uint16_t>(), meta.n[level], closed_form);
    FC_TRY(check_launch("k_ts_level"));
  }
  return sync();  // the temporaries above go back to the pool only after the kernels have used them
}

int launch_torsion_scan(const double *base_dev, int64_t A, const int64_t *torsions_dev, int64_t T,
                        const uint8_t *rotmasks_dev, const int16_t *mv_dev, const int16_t *rs_dev,
                        const int32_t *nmv_dev, const int32_t *nrs_dev, const int64_t *angles_dev,
                        int64_t S, double thresh, int64_t backoff, double *out_dev,
                        int64_t *rot_dev, const int64_t *quads_dev, int64_t Q, double *tf_dev) {
  if (S == 0) return FC_OK;
  const double thr2 = sq_threshold_lt(thresh);
  {
    const char *v = getenv("FC_SCAN_TREE");  // 0: always one wavefront per angle-set (the round-1 kernel)
    if (!(v && v[0] == '0')) {
      const int rc = torsion_scan_tree(base_dev, A, torsions_dev, T, rotmasks_dev, mv_dev, rs_dev, nmv_dev, nrs_dev,
                                       angles_dev, S, thr2, backoff, out_dev, rot_dev, quads_dev, Q, tf_dev);
      if (rc != 1) return rc;
    }
  }
  int64_t blocks = ceil_div(S, 4);
  const int64_t cap = (int64_t)ctx().n_cu * 32;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k_torsion_scan, dim3((unsigned)blocks), dim3(256),
                     (size_t)4 * A * 3 * sizeof(double), ctx().stream, base_dev, (int)A,
                     torsions_dev, (int)T, rotmasks_dev, mv_dev, rs_dev, nmv_dev, nrs_dev,
                     angles_dev, S, thr2, (int)backoff, out_dev, rot_dev, quads_dev, (int)Q, tf_dev);
  return check_launch("k_torsion_scan");
}

int launch_rotcorr_simbits(const double *X_dev, int64_t N, int64_t A, const uint8_t *heavy_dev,
                           const int64_t *tors_dev, int64_t T, const uint8_t *rotmasks_dev,
                           const double *angles_dev, const int32_t *n_angles_dev, int max_angles,
                           double max_rmsd, double max_dev, const double *energies_dev, double max_dE,
                           uint64_t *bits_dev, int64_t W) {
  if (N < 2) return FC_OK;
  const size_t lds = (size_t)4 * A * 3 * sizeof(double);
  FC_TRY(allow_dynamic_lds(reinterpret_cast<const void *>(k_rotcorr_simbits), lds, "k_rotcorr_simbits"));
  // the row index is blockIdx.y: fc_prune_rmsd_rot_corr refuses N > FC_ROTCORR_MAX_ROWS before it comes here
  hipLaunchKernelGGL(k_rotcorr_simbits, dim3((unsigned)ceil_div(N, 4), (unsigned)N), dim3(256), lds, ctx().stream, X_dev, N, (int)A, heavy_dev, tors_dev,
                     (int)T, rotmasks_dev, angles_dev, n_angles_dev, max_angles, max_rmsd, max_dev, energies_dev,
                     max_dE, reinterpret_cast<unsigned long long *>(bits_dev), W);
  return check_launch("k_rotcorr_simbits");
}

int launch_torsion_fingerprint(const double *coords_dev, int64_t N, int64_t A,
                               const int64_t *quads_dev, int64_t Q, double *tf_dev) {
  if (N * Q == 0) return FC_OK;
  hipLaunchKernelGGL(k_torsion_fingerprint, dim3((unsigned)ceil_div(N * Q, 256)), dim3(256), 0,
                     ctx().stream, coords_dev, N, A, quads_dev, (int)Q, tf_dev);
  return check_launch("k_torsion_fingerprint");
}

// Rows of the reference's cartesian_product(*arrays) (firecode/utils.py:219-221: np.stack(np.meshgrid(*arrays), -1)
// .reshape(-1, T) -- with the default 'xy' indexing array #2 varies slowest, then #1, then #3 ... #T, fastest) written where
// the scan reads them: one thread per row, mixed-radix digits of the row number.  The 1 679 616 x 8 grid of cfg3 is
// 107 MB: 9 ms to build on 16 host threads and ~12 ms to send; here it is never anywhere but in HBM.
__global__ void __launch_bounds__(256)
k_angle_grid(const int64_t *__restrict__ values, const int64_t *__restrict__ first, const int64_t *__restrict__ counts, int T,
             int64_t S, int64_t *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= S) return;
  int64_t rem = r;
  for (int p = T - 1; p >= 0; --p) {  // digit order, slowest first: 1, 0, 2, 3, ... (T == 1: just 0)
    const int t = T >= 2 ? (p == 0 ? 1 : (p == 1 ? 0 : p)) : 0;
    const int64_t c = counts[t];
    out[r * T + t] = values[first[t] + rem % c];
    rem /= c;
  }
}
int launch_angle_grid(const int64_t *values_dev, const int64_t *first_dev, const int64_t *counts_dev, int64_t T, int64_t S,
                      int64_t *out_dev) {
  if (S == 0) return FC_OK;
  hipLaunchKernelGGL(k_angle_grid, dim3((unsigned)ceil_div(S, 256)), dim3(256), 0, ctx().stream, values_dev, first_dev, counts_dev,
                     (int)T, S, out_dev);
  return check_launch("k_angle_grid");
}

// indices of the non-zero entries of rot[0 .. S), in order, and their count (device): the rows clustered_csearch hands to
// the TFD prune, selected where the scan left its counts
struct RotNonZero {
  __device__ __forceinline__ bool operator()(const int64_t &v) const { return v != 0; }
};
// out[q] = idx[rows[q] - 1]: the angle-set behind row rows[q] >= 1 of the TFD problem (row 0 is the starting structure)
__global__ void __launch_bounds__(256)
k_rows_to_sets(const int64_t *__restrict__ idx, const int64_t *__restrict__ rows, int64_t n, int64_t *__restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < n) out[q] = idx[rows[q] - 1];
}
int launch_rows_to_sets(const int64_t *idx_dev, const int64_t *rows_dev, int64_t n, int64_t *out_dev) {
  if (n <= 0) return FC_OK;
  hipLaunchKernelGGL(k_rows_to_sets, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, cur_stream(), idx_dev, rows_dev, n, out_dev);
  return check_launch("k_rows_to_sets");
}

int launch_select_rotated(const int64_t *rot_dev, int64_t S, int64_t *idx_dev, int64_t *count_dev, DevBuf &tmp) {
  if (S >= (1ll << 31)) return set_error(FC_E_LIMIT, "too many angle-sets for the device selection");
  hipcub::CountingInputIterator<int64_t> ids(0);
  hipcub::TransformInputIterator<bool, RotNonZero, const int64_t *> flags(rot_dev, RotNonZero());
  size_t bytes = 0;
  FC_HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, bytes, ids, flags, idx_dev, count_dev, (int)S, ctx().stream));
  FC_TRY(tmp.reserve(bytes));
  FC_HIP_TRY(hipcub::DeviceSelect::Flagged(tmp.p, bytes, ids, flags, idx_dev, count_dev, (int)S, ctx().stream));
  return FC_OK;
}

// fc_warmup(): the first launch from a translation unit makes the runtime load that unit's code object (milliseconds);
// a no-op launch moves that cost out of the first real call
__global__ void k_warm_torsion() {}
int warm_torsion() {
  hipLaunchKernelGGL(k_warm_torsion, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_torsion");
}

}  // namespace fc
