// tools/qcp_col0_check.cpp -- host-side check of qcp_lean_quaternion_col0 (fc_kabsch_math.h), the column-0 form of the
// rotation the complete alignments use in the shared frame, against the general form qcp_lean_quaternion_raw: wherever
// column 0 certifies a pair (converged, simple, nq > 0, a00^2 >= 0.6 nq) the general form must have picked column 0 and
// Q, nq and the flag must be equal BIT FOR BIT.  Cases: 3 ... 416 atoms; rotation angles swept through the certificate's
// boundary (q0^2 from 0.5 to 0.7), arbitrary and small rotations, improper pairs (mirror images), near-duplicates.
// Build (host code only): hipcc -O2 -std=c++17 --offload-host-only -ffp-contract=off -I firecode_amd/csrc
//                         tools/qcp_col0_check.cpp -o qcp_col0_check      (add -mfma where the host has it: the header's
//                         contract(fast) regions then fuse as they do on the device)
// Usage: qcp_col0_check [cases per atom count = 81920]; the last line is "<cases> cases, <certified> certified,
// <n> certified where the general form picked another column, <n> certified with a differing bit, ..."; exit status 1
// when either of the two is not zero.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fc_kabsch_math.h"

namespace {
struct Rng {  // xorshift64*: the shape of the noise does not matter here, its speed does
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
  double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  double sym() { return 2.0 * uniform() - 1.0; }                                     // [-1, 1)
};

// rotation by the unit quaternion (w, u sin): row-major
void rotation_about(const double (&axis)[3], double w, double (&R)[9]) {
  const double s = std::sqrt(std::fmax(0.0, 1.0 - w * w));
  const double Q[4] = {w, s * axis[0], s * axis[1], s * axis[2]};
  fc::rotation_from_quaternion(Q, R);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
}  // namespace

int main(int argc, char **argv) {
  const long per_count = argc > 1 ? std::atol(argv[1]) : 81920;
  const int counts[] = {3, 4, 5, 7, 10, 20, 50, 53, 104, 105, 208, 209, 416};
  Rng rng{0x9E3779B97F4A7C15ull};
  long cases = 0, certified = 0, other_column = 0, bit_differs = 0, general_ok = 0, col0_without_certificate = 0;
  long certified_by_kind[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cases_by_kind[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double q0sq_min_certified = 2.0, q0sq_max_declined_col0 = 0.0;
  for (int A : counts) {
    std::vector<double> p(3 * (size_t)A), q(3 * (size_t)A);
    for (long t = 0; t < per_count; ++t) {
      const int kind = (int)(t & 7);
      for (double &v : p) v = 3.0 * rng.sym();
      double axis[3] = {rng.sym(), rng.sym(), rng.sym()};
      const double an = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]) + 1e-300;
      for (double &v : axis) v /= an;
      // q0^2 of the pair's rotation (before the noise moves it a little) and the displacement per coordinate
      double q0sq, noise;
      switch (kind) {
        case 0: case 1: case 2: q0sq = 0.5 + 0.2 * rng.uniform(), noise = 0.05 + 0.5 * rng.uniform(); break;  // the boundary
        case 3: q0sq = 0.6 + 2e-3 * rng.sym(), noise = 1e-3 * rng.uniform(); break;                            // right at it
        case 4: q0sq = rng.uniform(), noise = 0.6; break;                                                      // any angle
        case 5: q0sq = 1.0 - 3e-3 * rng.uniform(), noise = 0.3; break;                                         // the shared frame: < 6.3 degrees
        case 6: q0sq = 0.5 + 0.5 * rng.uniform(), noise = 0.3; break;                                          // improper (mirrored below)
        default: q0sq = (t & 8) ? 0.5 + 0.2 * rng.uniform() : 1.0 - 1e-3 * rng.uniform();                      // near-duplicates
                 noise = (t & 16) ? 1e-5 : ((t & 32) ? 1e-9 : 0.0);
      }
      double R[9];
      rotation_about(axis, std::sqrt(q0sq), R);
      for (int a = 0; a < A; ++a) {
        const double *x = &p[(size_t)a * 3];
        double *y = &q[(size_t)a * 3];
        // p = R q in the header's convention (R rotates q onto p): q = R^T p
        y[0] = R[0] * x[0] + R[3] * x[1] + R[6] * x[2] + noise * rng.sym();
        y[1] = R[1] * x[0] + R[4] * x[1] + R[7] * x[2] + noise * rng.sym();
        y[2] = R[2] * x[0] + R[5] * x[1] + R[8] * x[2] + noise * rng.sym();
        if (kind == 6) y[0] = -y[0];
      }
      double cp[3] = {0, 0, 0}, cq[3] = {0, 0, 0};
      for (int a = 0; a < A; ++a)
        for (int c = 0; c < 3; ++c) cp[c] += p[(size_t)a * 3 + c] / A, cq[c] += q[(size_t)a * 3 + c] / A;
      double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, G = 0.0;
      for (int a = 0; a < A; ++a) {
        double x[3], y[3];
        for (int c = 0; c < 3; ++c) {
          x[c] = p[(size_t)a * 3 + c] - cp[c];
          y[c] = q[(size_t)a * 3 + c] - cq[c];
          G += x[c] * x[c] + y[c] * y[c];
        }
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) B[i * 3 + j] += x[i] * y[j];
      }
      // the eigenvalue as the kernel finds it, then both forms on the same (B, P, lambda, delta)
      const fc::QcpLeanPoly P = fc::qcp_lean_polynomial(B);
      double lam = 0.5 * G, delta = 0.0;
      for (int it = 0; it < 64; ++it)
        if (!fc::qcp_lean_step(P, lam, delta)) break;
      double Qg[4], nqg, Qc[4], nqc;
      const bool okg = fc::qcp_lean_quaternion_raw(B, P, lam, delta, Qg, nqg);
      const bool cert = fc::qcp_lean_quaternion_col0(B, P, lam, delta, Qc, nqc);
      ++cases;
      ++cases_by_kind[kind];
      general_ok += okg ? 1 : 0;
      const bool picked0 = same_bits(Qg[0], Qc[0]) && same_bits(Qg[1], Qc[1]) && same_bits(Qg[2], Qc[2]) && same_bits(Qg[3], Qc[3]);
      const double ratio = nqc > 0.0 ? Qc[0] * Qc[0] / nqc : 0.0;
      if (cert) {
        ++certified;
        ++certified_by_kind[kind];
        q0sq_min_certified = std::fmin(q0sq_min_certified, ratio);
        if (!picked0) ++other_column;
        if (!picked0 || !same_bits(nqg, nqc) || !okg) ++bit_differs;
      } else if (picked0 && okg) {
        ++col0_without_certificate;  // (allowed: the general form runs there)
        q0sq_max_declined_col0 = std::fmax(q0sq_max_declined_col0, ratio);
      }
    }
  }
  std::printf("certified / cases by kind (0-2 boundary sweep, 3 at the boundary, 4 any angle, 5 frame, 6 improper, 7 near-duplicates):");
  for (int k = 0; k < 8; ++k) std::printf(" %ld/%ld", certified_by_kind[k], cases_by_kind[k]);
  std::printf("\ngeneral form accepted %ld; column 0 picked without a certificate %ld (largest a00^2/nq among them %.6f); "
              "smallest a00^2/nq certified %.6f\n",
              general_ok, col0_without_certificate, q0sq_max_declined_col0, q0sq_min_certified);
  std::printf("%ld cases, %ld certified, %ld certified where the general form picked another column, %ld certified with a differing bit\n",
              cases, certified, other_column, bit_differs);
  return other_column == 0 && bit_differs == 0 ? 0 : 1;
}
