// fc_items.h -- the items of the tiled all-pairs kernels: which (row blocks, column tile) a workgroup takes, in which
// order.  Pure host arithmetic apart from the two decoders the kernels share; it includes nothing of the GPU runtime, so
// a host compiler builds it alone (tools/complete_items_check.cpp, tests/test_complete_items_cpu.py).
// Also here: the layout of Xt, the row-tile-major copy of the ensemble (row_tile_offset; tools/row_tiles_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FC_ITEMS_HD __host__ __device__
#else
#define FC_ITEMS_HD
#endif

namespace fc {

// Row blocks of the bit matrix are dealt to ranks in snake order (0..W-1,
// W-1..0, 0..W-1, ...): the work of a row block falls linearly with its index,
// so pairs of consecutive cycles carry equal work on every rank.
FC_ITEMS_HD inline int64_t global_block(int64_t local_block, int64_t rank, int64_t world) {
  return local_block * world + ((local_block & 1) ? (world - 1 - rank) : rank);
}
inline int64_t local_block_count(int64_t n_gblocks, int64_t rank, int64_t world) {
  int64_t n = 0;
  while (global_block(n, rank, world) < n_gblocks) ++n;  // strictly increasing in n
  return n;
}

// An entry of the item table:
//   bits  0..30  column tile jt            bit 31  the item covers only the FIRST half of the row block's 16-row tiles
//   bits 32..57  first local row block lb  bit 63  ... only the SECOND half
//   bits 58..61  row blocks beyond the first that share the column tile (the complete alignments: the workgroup fills the
//                tile once and walks the 16-row tiles of local blocks lb .. lb + count; 0 = one row block, the only form
//                the screens' tables hold).  lb < 2^26: a launch has fewer than 2^31 rows, a table's row block at least 32.
constexpr uint64_t kItemFirstHalf = 1ull << 31, kItemSecondHalf = 1ull << 63;
constexpr int kItemChunkShift = 58, kItemChunkMax = 16;
FC_ITEMS_HD inline int64_t item_tile(uint64_t it) { return (int64_t)(it & 0x7fffffffull); }
FC_ITEMS_HD inline int64_t item_block(uint64_t it) { return (int64_t)((it >> 32) & 0x3ffffffull); }
FC_ITEMS_HD inline int item_blocks(uint64_t it) { return (int)((it >> kItemChunkShift) & 15ull) + 1; }

// Xt, the row-tile-major copy of the ensemble that the atom pass of the complete alignments reads its row conformer from
// (fc_ensemble::Xt, made by k_row_tiles): doubles [t][u][c][r][h] -- t the tile of 16 consecutive conformers (row n lies
// in tile n / 16), u the pair of atoms (2u, 2u + 1), c the coordinate, r the row inside the tile, h the atom inside the
// pair.  A wave walks ONE stream of 768 bytes per pair of atoms for its 16 rows: lane r takes its two atoms of a
// coordinate with one 16-byte load.  Rows n >= N are zero, and so is the second atom of the last pair of an odd A.
FC_ITEMS_HD inline int64_t row_tile_pairs(int64_t A) { return (A + 1) / 2; }
FC_ITEMS_HD inline int64_t row_tile_offset(int64_t n, int64_t a, int64_t c, int64_t A) {
  return (((n >> 4) * row_tile_pairs(A) + (a >> 1)) * 3 + c) * 32 + (n & 15) * 2 + (a & 1);
}
// doubles of Xt for Npad (a multiple of 16) rows
FC_ITEMS_HD inline int64_t row_tile_elems(int64_t Npad, int64_t A) { return (Npad >> 4) * row_tile_pairs(A) * 96; }

struct ItemPlan {
  int64_t N = 0, rank = 0, world = 1;  // conformers; the rows are the row blocks dealt to `rank` of `world`
  int64_t row_block = 128, tc = 64;    // rows of a row block (a multiple of tc), columns of a tile
  int64_t NT = 0, n_lblocks = 0;       // column tiles of the padded ensemble, local row blocks
  bool halves = false;                 // the last `tail` single items as two half items each
  int64_t tail = 0;
  // the complete alignments only: tiles without a real column (all columns >= N) are left out, and the items in front
  // of the last 3 * tail single ones keep their column tile for up to `chunk` consecutive local row blocks
  bool real_columns_only = false;
  int64_t chunk = 1;
  bool tail_order = true;  // false (a measurement's arm): chunks up to the last `tail` items, no re-ordering
};

// The (16-row tile, 16-column sub-tile) units the complete-alignment kernel computes for an item, in the kernel's order:
// visit(first row, first column).  This IS the kernel's loop nest (k_simbits_screen_mfma, MODE 2) without the arithmetic;
// row tiles are dealt to the waves round-robin there, which changes the order and nothing else.
template <class F>
inline void item_units(uint64_t it, const ItemPlan &p, F visit) {
  const int64_t jt = item_tile(it), lb = item_block(it), j0 = jt * p.tc, tpb = p.row_block / 16;
  int64_t it_first = 0, it_last = tpb * item_blocks(it);
  if (it & kItemFirstHalf) it_last = tpb / 2;
  if (it & kItemSecondHalf) it_first = tpb / 2;
  const int64_t i0 = global_block(lb, p.rank, p.world) * p.row_block;
  if (i0 >= p.N || j0 + p.tc - 1 <= i0) return;
  for (int64_t t = it_first; t < it_last; ++t) {
    const int64_t ib = global_block(lb + t / tpb, p.rank, p.world) * p.row_block + (t % tpb) * 16;
    if (ib >= p.N) break;               // (ib grows with t: global_block is strictly increasing)
    if (j0 + p.tc - 1 <= ib) break;
    for (int64_t cs = 0; cs < p.tc / 16; ++cs) {
      if (j0 + (cs + 1) * 16 - 1 <= ib) continue;  // at or below the diagonal
      if (j0 + cs * 16 >= p.N) continue;           // no real column
      visit(ib, j0 + cs * 16);
    }
  }
}

// Items in dispatch order.  chunk == 1 and all tiles: row blocks ascending, tiles left to right, the last `tail` items
// as halves (the screens' tables).  The complete alignments (chunk > 1): the leading row blocks in chunks that share a
// column tile; the trailing row blocks -- the smallest number that holds 3 * tail items, about three rounds of what the
// chip holds at once -- as single row blocks, the dearest first (stable: whole items keep their order), so that what is cut
// by the diagonal, the last column tile's few real columns and the partial last row block end the launch, and the last
// `tail` of those as halves.
inline std::vector<uint64_t> build_items(const ItemPlan &p) {
  std::vector<uint64_t> items;
  if (p.row_block % p.tc != 0) return items;
  const int64_t r = p.row_block / p.tc;
  const int64_t nt = p.real_columns_only ? std::min(p.NT, (p.N + p.tc - 1) / p.tc) : p.NT;
  auto first_tile = [&](int64_t l) { return r * global_block(l, p.rank, p.world); };
  auto n_single = [&](int64_t l) { return std::max<int64_t>(0, nt - first_tile(l)); };
  // row blocks [0, n_chunked) go in chunks
  int64_t n_chunked = 0;
  if (p.chunk > 1) {
    int64_t kept = 0;
    n_chunked = p.n_lblocks;
    while (n_chunked > 0 && kept < (p.tail_order ? 3 : 1) * p.tail) kept += n_single(--n_chunked);
    if (n_chunked < 2) n_chunked = 0;
  }
  const int64_t chunk = std::min<int64_t>(p.chunk, kItemChunkMax);
  for (int64_t l = 0; l < n_chunked; l += chunk) {
    const uint64_t more = (uint64_t)(std::min(chunk, n_chunked - l) - 1);
    // (the first block of a chunk is the highest in the triangle: a tile it does not need, none of them needs)
    for (int64_t jt = first_tile(l); jt < nt; ++jt) items.push_back((more << kItemChunkShift) | ((uint64_t)l << 32) | (uint64_t)jt);
  }
  const size_t single0 = items.size();
  for (int64_t l = n_chunked; l < p.n_lblocks; ++l)
    for (int64_t jt = first_tile(l); jt < nt; ++jt) items.push_back(((uint64_t)l << 32) | (uint64_t)jt);
  if (p.chunk > 1 && p.tail_order) {
    auto cost = [&](uint64_t it) {
      int64_t n = 0;
      item_units(it, p, [&](int64_t, int64_t) { ++n; });
      return n;
    };
    std::vector<std::pair<int64_t, uint64_t>> keyed;
    for (size_t k = single0; k < items.size(); ++k) keyed.emplace_back(-cost(items[k]), items[k]);
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t k = single0; k < items.size(); ++k) items[k] = keyed[k - single0].second;
  }
  // the last items of the launch as two half-row-block items each: workgroups finish within
  // half an item of each other instead of a whole one
  if (p.halves && p.tail > 0 && (int64_t)items.size() > 4 * p.tail && (int64_t)(items.size() - single0) >= p.tail) {
    std::vector<uint64_t> halves;
    for (int64_t k = (int64_t)items.size() - p.tail; k < (int64_t)items.size(); ++k) {
      halves.push_back(items[(size_t)k] | kItemFirstHalf);
      halves.push_back(items[(size_t)k] | kItemSecondHalf);
    }
    items.resize(items.size() - (size_t)p.tail);
    items.insert(items.end(), halves.begin(), halves.end());
  }
  return items;
}

}  // namespace fc
