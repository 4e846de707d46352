// fc_kabsch_math_debug.hip -- fc_debug_kabsch_math: the routines of fc_kabsch_math.h on the device, one lane per record,
// for tests/test_gpu_kabsch_math.py (no FIRECODE call maps to it; the kernels of the product are not touched).
//   routine 0  the probe of fc_kabsch_math_probe.h: everything tools/kabsch_math_host.cpp runs on the host, from the same text
//   routine 1  the three fp32 screens, plain and ENANT, under the bounds their launchers pass
//   routine 2  fc_sqrt_nonneg and fc_rsqrt (v_rsq_f64 and their Newton steps exist on the device only)
// Every launch is made of full wavefronts: the records are padded to a multiple of 64 with copies of the last one, because
// qcp_lean_eigenvalues4's loop and kabsch_may_be_below_f32_2t_wave's ballots are wave-wide.  A padding lane writes to a
// padding slot of its own, so no lane branches on its index.
#include <vector>

#include "fc_internal.h"
#include "fc_kabsch_math_probe.h"

namespace fc {

constexpr int kScreenIn = 16, kScreenOut = 16, kRootsIn = 1, kRootsOut = 2;

__global__ void __launch_bounds__(64) k_debug_kabsch_probe(const double *__restrict__ in, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  kabsch_math_probe(in + i * kProbeIn, out + i * kProbeOut);
}

template <bool ENANT>
__device__ __forceinline__ void debug_screens(const float (&B)[9], float s, float half, const KabschF32Bounds &bd, float tiny_floor,
                                              double *out) {
  const int lane = threadIdx.x & 63;
  out[0] = kabsch_may_be_below_f32<ENANT>(B, s, half, bd, s, tiny_floor) ? 1.0 : 0.0;
  bool redo = false;
  out[1] = kabsch_may_be_below_f32_2t<ENANT>(B, s, half, bd, tiny_floor, redo) ? 1.0 : 0.0;
  out[2] = redo ? 1.0 : 0.0;
  uint64_t redo_w = 0;
  const uint64_t may_w = kabsch_may_be_below_f32_2t_wave<ENANT>(B, s, half, bd, tiny_floor, redo_w);
  out[3] = (double)((may_w >> lane) & 1ull);
  out[4] = (double)((redo_w >> lane) & 1ull);
}

// in: B[9], s, A thr^2 / 2, (count, kind: read by the host), tiny_floor -- all exactly representable in fp32; bd: 3 floats
__global__ void __launch_bounds__(64) k_debug_kabsch_screens(const double *__restrict__ in, const float *__restrict__ bd3,
                                                             double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const double *rec = in + i * kScreenIn;
  double *o = out + i * kScreenOut;
  float B[9];
  for (int k = 0; k < 9; ++k) B[k] = (float)rec[k];
  const float s = (float)rec[9], half = (float)rec[10], tiny_floor = (float)rec[13];
  const KabschF32Bounds bd{bd3[3 * i], bd3[3 * i + 1], bd3[3 * i + 2]};
  debug_screens<false>(B, s, half, bd, tiny_floor, o);
  debug_screens<true>(B, s, half, bd, tiny_floor, o + 5);
  o[10] = bd.p0, o[11] = bd.p1, o[12] = bd.p2;
  o[13] = o[14] = o[15] = 0.0;
}

__global__ void __launch_bounds__(64) k_debug_kabsch_roots(const double *__restrict__ in, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  out[2 * i] = fc_sqrt_nonneg(in[i]);
  out[2 * i + 1] = fc_rsqrt(in[i]);
}

}  // namespace fc

using namespace fc;

extern "C" int fc_debug_kabsch_math(int routine, const double *in, int64_t n, double *out) {
  FC_API_LOCK;
  FC_REQUIRE(in && out, "NULL argument");
  FC_REQUIRE(n >= 0 && n <= (1 << 20), "n=%lld outside 0..2^20", (long long)n);
  FC_REQUIRE(routine >= 0 && routine <= 2, "routine=%d: 0 (probe), 1 (fp32 screens) or 2 (roots)", routine);
  const int n_in = routine == 0 ? kProbeIn : routine == 1 ? kScreenIn : kRootsIn;
  const int n_out = routine == 0 ? (int)kProbeOut : routine == 1 ? kScreenOut : kRootsOut;
  const int64_t npad = (n + 63) / 64 * 64;
  std::vector<float> bounds;
  if (routine == 1) {
    // the bounds are the launchers' own: kabsch_f32_bounds(A4) or kabsch_h2_bounds(KS2), evaluated on the host as they do
    bounds.resize((size_t)npad * 3);
    for (int64_t i = 0; i < n; ++i) {
      const double count = in[i * kScreenIn + 11], kind = in[i * kScreenIn + 12];
      FC_REQUIRE(count >= 0.0 && count <= 1048576.0 && (kind == 0.0 || kind == 1.0),
                 "record %lld: count outside 0..2^20 or kind not 0 (kabsch_f32_bounds) / 1 (kabsch_h2_bounds)", (long long)i);
      const KabschF32Bounds bd = kind == 0.0 ? kabsch_f32_bounds((int64_t)count) : kabsch_h2_bounds((int64_t)count);
      bounds[3 * i] = bd.p0, bounds[3 * i + 1] = bd.p1, bounds[3 * i + 2] = bd.p2;
    }
    for (int64_t i = n; i < npad; ++i)
      for (int k = 0; k < 3; ++k) bounds[3 * i + k] = bounds[3 * (n - 1) + k];
  }
  if (n == 0) return FC_OK;
  FC_TRY(ensure_init());
  std::vector<double> padded((size_t)npad * n_in);
  std::memcpy(padded.data(), in, (size_t)n * n_in * sizeof(double));
  for (int64_t i = n; i < npad; ++i) std::memcpy(&padded[(size_t)i * n_in], &in[(size_t)(n - 1) * n_in], n_in * sizeof(double));
  DevBuf din, dbd, dout;
  int rc = upload(din, padded.data(), padded.size());
  if (rc == FC_OK && routine == 1) rc = upload(dbd, bounds.data(), bounds.size());
  if (rc == FC_OK) rc = dout.reserve((size_t)npad * n_out * sizeof(double));
  if (rc == FC_OK) {
    const dim3 grid((unsigned)(npad / 64)), block(64);
    if (routine == 0)
      hipLaunchKernelGGL(k_debug_kabsch_probe, grid, block, 0, ctx().stream, din.as<double>(), dout.as<double>());
    else if (routine == 1)
      hipLaunchKernelGGL(k_debug_kabsch_screens, grid, block, 0, ctx().stream, din.as<double>(), dbd.as<float>(), dout.as<double>());
    else
      hipLaunchKernelGGL(k_debug_kabsch_roots, grid, block, 0, ctx().stream, din.as<double>(), dout.as<double>());
    rc = check_launch("k_debug_kabsch_math");
  }
  if (rc == FC_OK) rc = d2h(out, dout.p, (size_t)n * n_out * sizeof(double));
  if (rc == FC_OK) rc = sync();
  return drained(rc);
}
