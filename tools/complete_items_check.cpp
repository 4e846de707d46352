// tools/complete_items_check.cpp -- host-only check of the item tables of the complete alignments (fc_items.h): over a
// grid of ensemble sizes, world sizes, chunk lengths and tail lengths, the units (16-row tile x 16-column sub-tile) that
// the items of all ranks visit are exactly the ones that touch the upper triangle with a real column, once each.
// Also: the table of chunk = 1 without the real-column rule is the plain ascending enumeration + halves (the screens').
// Build: c++ -O2 -std=c++17 -I firecode_amd/csrc tools/complete_items_check.cpp -o complete_items_check
// Usage: complete_items_check [N ...]   (prints one line per failure and a summary; exit status 1 on any failure)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fc_items.h"

static long failures = 0;

static void fail(const char *what, const fc::ItemPlan &p, int64_t a, int64_t b) {
  if (++failures <= 20)
    std::printf("FAIL %s: N=%lld world=%lld tc=%lld chunk=%lld tail=%lld order=%d at (%lld, %lld)\n", what, (long long)p.N,
                (long long)p.world, (long long)p.tc, (long long)p.chunk, (long long)p.tail, (int)p.tail_order, (long long)a,
                (long long)b);
}

int main(int argc, char **argv) {
  std::vector<int64_t> sizes = {17, 63, 64, 65, 128, 129, 200, 300, 513, 640, 1041, 2049, 4100, 10000};
  if (argc > 1) {
    sizes.clear();
    for (int k = 1; k < argc; ++k) sizes.push_back(std::atoll(argv[k]));
  }
  long configs = 0, n_items = 0;
  for (int64_t N : sizes)
    for (int64_t world : {1, 2, 3, 8})
      for (int64_t tc : {64, 32, 16})
        for (int64_t chunk : {1, 2, 4, 8})
          for (int64_t tail : {0, 2, 512})
            for (int order = 0; order < 2; ++order) {
              const int64_t Npad = (N + 63) / 64 * 64, nt16 = Npad / 16;
              std::vector<unsigned char> seen((size_t)(nt16 * nt16), 0);
              fc::ItemPlan p;
              for (int64_t rank = 0; rank < world; ++rank) {
                p.N = N; p.rank = rank; p.world = world; p.row_block = 128; p.tc = tc; p.NT = Npad / tc;
                p.n_lblocks = fc::local_block_count((N + 127) / 128, rank, world);
                p.halves = tc == 64; p.tail = tail; p.real_columns_only = true; p.chunk = chunk; p.tail_order = order != 0;
                const std::vector<uint64_t> items = fc::build_items(p);
                n_items += (long)items.size();
                for (uint64_t it : items) {
                  if (fc::item_block(it) + fc::item_blocks(it) > p.n_lblocks) fail("row blocks past the end", p, fc::item_block(it), 0);
                  fc::item_units(it, p, [&](int64_t ib, int64_t c0) {
                    unsigned char &s = seen[(size_t)((ib / 16) * nt16 + c0 / 16)];
                    if (s < 255) ++s;
                  });
                }
              }
              for (int64_t rt = 0; rt < nt16; ++rt)
                for (int64_t ct = 0; ct < nt16; ++ct) {
                  const int64_t ib = rt * 16, c0 = ct * 16;
                  // a pair (i, j), i < j < N, in the unit: its last column lies right of its first row
                  const bool wanted = ib < N && c0 < N && c0 + 15 > ib;
                  const int got = seen[(size_t)(rt * nt16 + ct)];
                  if (c0 >= N && got != 0) fail("padding visited", p, ib, c0);
                  else if (got != (wanted ? 1 : 0)) fail(wanted ? (got ? "visited twice" : "not visited") : "visited for nothing", p, ib, c0);
                }
              ++configs;
            }
  // the screens' tables: ascending (row block, tile), the last `tail` items as halves -- what the builder made before it
  // knew chunks
  for (int64_t N : sizes)
    for (int64_t tc : {64, 32})
      for (int64_t tail : {0, 2, 512}) {
        fc::ItemPlan p;
        const int64_t Npad = (N + 63) / 64 * 64;
        p.N = N; p.row_block = 128; p.tc = tc; p.NT = Npad / tc; p.n_lblocks = (N + 127) / 128; p.halves = tc == 64; p.tail = tail;
        std::vector<uint64_t> want;
        for (int64_t l = 0; l < p.n_lblocks; ++l)
          for (int64_t jt = (128 / tc) * l; jt < p.NT; ++jt) want.push_back(((uint64_t)l << 32) | (uint64_t)jt);
        if (p.halves && tail > 0 && (int64_t)want.size() > 4 * tail) {
          std::vector<uint64_t> h;
          for (size_t k = want.size() - (size_t)tail; k < want.size(); ++k) {
            h.push_back(want[k] | (1ull << 31));
            h.push_back(want[k] | (1ull << 63));
          }
          want.resize(want.size() - (size_t)tail);
          want.insert(want.end(), h.begin(), h.end());
        }
        if (fc::build_items(p) != want) fail("screen table changed", p, 0, 0);
        ++configs;
      }
  std::printf("%ld configurations, %ld items, %ld failures\n", configs, n_items, failures);
  return failures ? 1 : 0;
}
