// tools/row_tiles_check.cpp -- the layout of Xt, the row-tile-major copy of the ensemble (csrc/fc_items.h), walked on the
// host: c++ -O2 -std=c++17 -I firecode_amd/csrc tools/row_tiles_check.cpp (tests/test_row_tiles_cpu.py builds and runs it).
// For N = 1 ... 40 conformers (or the N given as arguments) and A = 1 ... 9 atoms:
//   * every (row < N, atom < A, coordinate) has an offset of its own inside the buffer;
//   * the 16-byte piece lane r of a wave loads for round u, coordinate c of row tile t -- doubles
//     ((t U + u) 3 + c) 32 + 2 r + {0, 1} -- holds the atoms 2u and 2u + 1 of row 16 t + r, and nothing else is loaded;
//   * what such a piece holds beyond the real elements is a padding row (n >= N) or the padding atom of an odd A: the places
//     the kernel expects zeros in, each of them once, and together with the real elements they fill the buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fc_items.h"

int main(int argc, char **argv) {
  std::vector<int64_t> Ns;
  for (int k = 1; k < argc; ++k) Ns.push_back(std::atoll(argv[k]));
  if (Ns.empty())
    for (int64_t n = 1; n <= 40; ++n) Ns.push_back(n);
  long long configs = 0, elements = 0, failures = 0;
  auto fail = [&](const char *what, int64_t N, int64_t A, int64_t n, int64_t a, int64_t c) {
    if (++failures <= 20) std::printf("FAIL %s: N=%lld A=%lld row=%lld atom=%lld c=%lld\n", what, (long long)N, (long long)A, (long long)n, (long long)a, (long long)c);
  };
  for (int64_t N : Ns)
    for (int64_t A = 1; A <= 9; ++A) {
      ++configs;
      const int64_t Npad = (N + 63) / 64 * 64, U = fc::row_tile_pairs(A), size = fc::row_tile_elems(Npad, A);
      if (2 * U < A || 2 * U > A + 1 || size != Npad / 16 * U * 96) fail("size", N, A, -1, -1, -1);
      std::vector<int> real(size, 0), loaded(size, 0);
      for (int64_t n = 0; n < N; ++n)
        for (int64_t a = 0; a < A; ++a)
          for (int64_t c = 0; c < 3; ++c) {
            const int64_t o = fc::row_tile_offset(n, a, c, A);
            if (o < 0 || o >= size) { fail("outside", N, A, n, a, c); continue; }
            if (real[o]++) fail("twice", N, A, n, a, c);
            ++elements;
          }
      // the kernel's walk: row tile, round, coordinate, lane
      int64_t padding = 0;
      for (int64_t t = 0; t < Npad / 16; ++t)
        for (int64_t u = 0; u < U; ++u)
          for (int64_t c = 0; c < 3; ++c)
            for (int64_t r = 0; r < 16; ++r)
              for (int64_t h = 0; h < 2; ++h) {
                const int64_t o = ((t * U + u) * 3 + c) * 32 + 2 * r + h, n = 16 * t + r, a = 2 * u + h;
                if (o >= size) { fail("walk outside", N, A, n, a, c); continue; }
                if (loaded[o]++) fail("loaded twice", N, A, n, a, c);
                if (o != fc::row_tile_offset(n, a, c, A)) fail("walk and offset differ", N, A, n, a, c);
                const bool is_real = n < N && a < A;
                if (is_real != (real[o] == 1)) fail("zero expected", N, A, n, a, c);
                if (!is_real) {
                  ++padding;
                  if (!(n >= N || (a == A && (A & 1)))) fail("padding of another kind", N, A, n, a, c);
                }
              }
      if (padding + N * A * 3 != size) fail("cover", N, A, -1, -1, -1);
    }
  std::printf("%lld configs, %lld elements, %lld failures\n", configs, elements, failures);
  return failures == 0 ? 0 : 1;
}
