// fc_kabsch_math_probe.h -- every routine of fc_kabsch_math.h that has a __host__ form, run on ONE record, with every
// value, flag and certificate written out.  Test infrastructure shared by tools/kabsch_math_host.cpp (the header on the
// host) and fc_kabsch_math_debug.hip (the same routines on the device, one lane per record): both run THIS text, so a
// difference between their outputs is a difference between the two compilations of the header, nothing else.
// On the device all 64 lanes of a wavefront must be active: qcp_lean_eigenvalues4 and kabsch_quaternion_qcp_lean loop
// until the whole wavefront has converged.
#pragma once
#include "fc_kabsch_math.h"

namespace fc {

// a record: B[9] (row-major, B[x][y] = sum p_x q_y), Gp + Gq, A, A thr^2
constexpr int kProbeIn = 12;
// slots of the output (doubles; flags as 0.0 / 1.0, counts as their value)
enum KabschProbeSlot {
  kPrLam = 0,        // kabsch_lambda_max
  kPrSlope = 1,      //   its slope,
  kPrStep = 2,       //   last step
  kPrNorm2 = 3,      //   and |B|_F^2
  kPrSettled = 4,    // kabsch_lambda_is_settled of those four
  kPrUpper = 5,      // kabsch_lambda_upper
  kPrBothPlus = 6,   // kabsch_lambda_max_both<true>: of B
  kPrBothMinus = 7,  //   and of -B
  kPrBothPlain = 8,  // kabsch_lambda_max_both<false>
  kPrSharp = 9,      // kabsch_lambda_is_sharp(lam, slope, A, (Gp + Gq) - 2 lam)
  kPrBelow = 10,     // kabsch_may_be_below<false>
  kPrBelowEnant = 11,
  kPrP0 = 12,        // kabsch_screen_values<false>: P, P'/4, P''/4
  kPrP1 = 13,
  kPrP2 = 14,
  kPrP0Enant = 15,   // kabsch_screen_values<true>
  kPrP1Enant = 16,
  kPrP2Enant = 17,
  kPrJacobiLam = 18,  // kabsch_rotation: its eigenvalue
  kPrJacobiR = 19,    //   and R[9]
  kPrQcpOk = 28,      // kabsch_rotation_qcp: certified,
  kPrQcpR = 29,       //   R[9] (zeros where it declined)
  kPrQuatOk = 38,     // kabsch_quaternion_qcp: certified,
  kPrQuatQ = 39,      //   Q[4] (zeros where it declined)
  kPrQuatIters = 43,  //   Newton steps
  kPrLeanLam = 44,    // qcp_lean_polynomial + qcp_lean_eigenvalues4: eigenvalue of pair 0,
  kPrLeanDelta = 45,  //   its last step,
  kPrLeanConverged = 46,  // qcp_lean_converged of the two
  kPrLean4Spread = 47,  //   largest difference between the eigenvalues of the four pairs of the lane (four copies of the
                        //   record; the compiler may fuse each copy's arithmetic its own way)
  kPrRawOk = 48,      // qcp_lean_quaternion_raw: certified,
  kPrRawQ = 49,       //   Q[4] not normalised,
  kPrRawNq = 53,      //   its squared length
  kPrCol0Ok = 54,     // qcp_lean_quaternion_col0: certified,
  kPrCol0Q = 55,      //   Q[4],
  kPrCol0Nq = 59,     //   nq
  kPrLean4Ok = 60,    // kabsch_quaternion_qcp_lean4 on four copies: how many of its four flags are set
  kPrLeanOk = 61,     // kabsch_quaternion_qcp_lean: certified,
  kPrLeanQ = 62,      //   Q[4] normalised (fc_rsqrt),
  kPrLeanIters = 66,  //   Newton steps
  kPrRotOfQ = 67,     // rotation_from_quaternion of that Q: R[9]
  kPrNegRotOfQ = 76,  // neg_rotation_from_quaternion of it: -R[9]
  kPrNegRotRaw = 85,  // neg_rotation_from_raw_quaternion of the raw Q and nq: -R[9]
  kProbeOut = 94
};

__host__ __device__ inline void kabsch_math_probe(const double *in, double *out) {
  double B[9];
  for (int k = 0; k < 9; ++k) B[k] = in[k];
  const double GG = in[9], A = in[10], A_thr2 = in[11];
  for (int k = 0; k < kProbeOut; ++k) out[k] = 0.0;

  double slope, step, n2;
  const double lam = kabsch_lambda_max(B, GG, &slope, &step, &n2);
  out[kPrLam] = lam, out[kPrSlope] = slope, out[kPrStep] = step, out[kPrNorm2] = n2;
  out[kPrSettled] = kabsch_lambda_is_settled(lam, slope, step, n2) ? 1.0 : 0.0;
  out[kPrUpper] = kabsch_lambda_upper(B, GG);
  double plus = 0.0, minus = 0.0, plain = 0.0, unused = 0.0;
  kabsch_lambda_max_both<true>(B, GG, plus, minus);
  kabsch_lambda_max_both<false>(B, GG, plain, unused);
  out[kPrBothPlus] = plus, out[kPrBothMinus] = minus, out[kPrBothPlain] = plain;
  out[kPrSharp] = kabsch_lambda_is_sharp(lam, slope, A, GG - 2.0 * lam) ? 1.0 : 0.0;

  out[kPrBelow] = kabsch_may_be_below<false>(B, GG, A_thr2) ? 1.0 : 0.0;
  out[kPrBelowEnant] = kabsch_may_be_below<true>(B, GG, A_thr2) ? 1.0 : 0.0;
  const KabschScreenValues v = kabsch_screen_values<false>(B, GG, A_thr2), w = kabsch_screen_values<true>(B, GG, A_thr2);
  out[kPrP0] = v.P0, out[kPrP1] = v.P1, out[kPrP2] = v.P2;
  out[kPrP0Enant] = w.P0, out[kPrP1Enant] = w.P1, out[kPrP2Enant] = w.P2;

  double R[9];
  out[kPrJacobiLam] = kabsch_rotation(B, R);
  for (int k = 0; k < 9; ++k) out[kPrJacobiR + k] = R[k];
  for (int k = 0; k < 9; ++k) R[k] = 0.0;
  out[kPrQcpOk] = kabsch_rotation_qcp(B, GG, R) ? 1.0 : 0.0;
  for (int k = 0; k < 9; ++k) out[kPrQcpR + k] = out[kPrQcpOk] != 0.0 ? R[k] : 0.0;

  double Q[4] = {0.0, 0.0, 0.0, 0.0};
  int iters = 0;
  out[kPrQuatOk] = kabsch_quaternion_qcp(B, GG, Q, &iters) ? 1.0 : 0.0;
  for (int k = 0; k < 4; ++k) out[kPrQuatQ + k] = out[kPrQuatOk] != 0.0 ? Q[k] : 0.0;
  out[kPrQuatIters] = (double)iters;

  // the lean family: four copies of the record stand for the four pairs of a lane
  double B4[4][9], GG4[4], x4[4], d4[4];
  for (int r = 0; r < 4; ++r) {
    for (int k = 0; k < 9; ++k) B4[r][k] = B[k];
    GG4[r] = GG;
  }
  QcpLeanPoly P4[4];
  qcp_lean_eigenvalues4(B4, GG4, P4, x4, d4);
  out[kPrLeanLam] = x4[0], out[kPrLeanDelta] = d4[0];
  out[kPrLeanConverged] = qcp_lean_converged(x4[0], d4[0]) ? 1.0 : 0.0;
  double spread = 0.0;
  for (int r = 1; r < 4; ++r) spread = fmax(spread, fabs(x4[r] - x4[0]));
  out[kPrLean4Spread] = spread;
  double Qraw[4], nq = 0.0, Qc[4], nqc = 0.0;
  const bool raw_ok = qcp_lean_quaternion_raw(B, P4[0], x4[0], d4[0], Qraw, nq);
  out[kPrRawOk] = raw_ok ? 1.0 : 0.0, out[kPrRawNq] = nq;
  for (int k = 0; k < 4; ++k) out[kPrRawQ + k] = Qraw[k];
  out[kPrCol0Ok] = qcp_lean_quaternion_col0(B, P4[0], x4[0], d4[0], Qc, nqc) ? 1.0 : 0.0, out[kPrCol0Nq] = nqc;
  for (int k = 0; k < 4; ++k) out[kPrCol0Q + k] = Qc[k];
  double Q4[4][4], nq4[4], lam4[4];
  bool ok4[4];
  kabsch_quaternion_qcp_lean4(B4, GG4, Q4, nq4, ok4, lam4);
  out[kPrLean4Ok] = (double)((int)ok4[0] + (int)ok4[1] + (int)ok4[2] + (int)ok4[3]);
  (void)Q4, (void)nq4, (void)lam4;

  double Qn[4] = {0.0, 0.0, 0.0, 0.0};
  iters = 0;
  out[kPrLeanOk] = kabsch_quaternion_qcp_lean(B, GG, Qn, &iters) ? 1.0 : 0.0;
  for (int k = 0; k < 4; ++k) out[kPrLeanQ + k] = Qn[k];
  out[kPrLeanIters] = (double)iters;
  rotation_from_quaternion(Qn, R);
  for (int k = 0; k < 9; ++k) out[kPrRotOfQ + k] = R[k];
  neg_rotation_from_quaternion(Qn, R);
  for (int k = 0; k < 9; ++k) out[kPrNegRotOfQ + k] = R[k];
  neg_rotation_from_raw_quaternion(Qraw, nq, R);
  for (int k = 0; k < 9; ++k) out[kPrNegRotRaw + k] = R[k];
}

}  // namespace fc
