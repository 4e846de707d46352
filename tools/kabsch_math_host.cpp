// tools/kabsch_math_host.cpp -- fc_kabsch_math.h itself on the host, record by record (tests/test_kabsch_math_cpu.py).
//
//   kabsch_math_host probe  IN OUT   IN: float64 records of kProbeIn = 12 values (B[9], Gp + Gq, A, A thr^2);
//                                    OUT: kProbeOut float64 per record, the slots of csrc/fc_kabsch_math_probe.h --
//                                    every __host__ routine of the header, flags and certificates included
//   kabsch_math_host bounds IN OUT   IN: float64 counts n (A4 of kabsch_f32_bounds, KS2 of kabsch_h2_bounds);
//                                    OUT: 7 float64 per count: kabsch_f32_bounds(n).p0 p1 p2, kabsch_h2_bounds(n).p0 p1 p2,
//                                    kabsch_h2_entry_bound(n)
//
// Build as tests/test_kabsch_math_cpu.py does: hipcc --offload-host-only -O2 -std=c++17 -ffp-contract=off -Wall -Werror
// (-mfma where the host has it: the header's contract(fast) regions then fuse as they do on the device)
// -I firecode_amd/csrc tools/kabsch_math_host.cpp; the test builds it a second time with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fc_kabsch_math_probe.h"

static bool read_doubles(const char *path, std::vector<double> &v) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes < 0 || bytes % (long)sizeof(double) != 0) {
    std::fclose(f);
    return false;
  }
  v.resize((size_t)bytes / sizeof(double));
  const size_t got = v.empty() ? 0 : std::fread(v.data(), sizeof(double), v.size(), f);
  std::fclose(f);
  return got == v.size();
}

static bool write_doubles(const char *path, const std::vector<double> &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  const size_t put = v.empty() ? 0 : std::fwrite(v.data(), sizeof(double), v.size(), f);
  return std::fclose(f) == 0 && put == v.size();
}

int main(int argc, char **argv) {
  if (argc != 4 || (std::strcmp(argv[1], "probe") != 0 && std::strcmp(argv[1], "bounds") != 0)) {
    std::fprintf(stderr, "usage: %s probe|bounds IN OUT\n", argv[0]);
    return 2;
  }
  std::vector<double> in, out;
  if (!read_doubles(argv[2], in)) {
    std::fprintf(stderr, "cannot read %s as float64\n", argv[2]);
    return 2;
  }
  if (std::strcmp(argv[1], "probe") == 0) {
    if (in.size() % fc::kProbeIn != 0) {
      std::fprintf(stderr, "%s: not a whole number of records of %d float64\n", argv[2], fc::kProbeIn);
      return 2;
    }
    const size_t n = in.size() / fc::kProbeIn;
    out.resize(n * fc::kProbeOut);
    for (size_t i = 0; i < n; ++i) fc::kabsch_math_probe(&in[i * fc::kProbeIn], &out[i * fc::kProbeOut]);
    std::printf("%zu records, %d values each\n", n, (int)fc::kProbeOut);
  } else {
    out.resize(in.size() * 7);
    for (size_t i = 0; i < in.size(); ++i) {
      const int64_t n = (int64_t)in[i];
      const fc::KabschF32Bounds a = fc::kabsch_f32_bounds(n), b = fc::kabsch_h2_bounds(n);
      double *o = &out[i * 7];
      o[0] = a.p0, o[1] = a.p1, o[2] = a.p2, o[3] = b.p0, o[4] = b.p1, o[5] = b.p2, o[6] = fc::kabsch_h2_entry_bound(n);
    }
    std::printf("%zu counts\n", in.size());
  }
  if (!write_doubles(argv[3], out)) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
