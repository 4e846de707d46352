// fc_prune.hip -- greedy k-ladder replay over similarity bits, moment-of-
// inertia similarity, torsion-fingerprint similarity (gfx950, wave64).
//
// Reference semantics (prism_pruner.pruner as evidenced by
// /root/reference/CHANGELOG.md:120,188,198,206 and the in-tree sibling
// firecode/torsion_module.py:973-992): for every ladder value k the array is
// cut in k contiguous chunks of N//k (last chunk takes the remainder); a
// structure active at the start of the level is removed "at the first
// instance of a similar one", i.e. iff an active j > i of its chunk is
// similar.  Rejections inside a level do not feed back into that level, so a
// level is a data-parallel map over rows of the bit matrix:
//     out[i] = in[i] && !any_{i<j<last(i)} ( in[j] && sim[i][j] )
#include "fc_internal.h"
#include "fc_kabsch_math.h"

namespace fc {

// bytes -> active-flag words + population count (counters[0])
__global__ void __launch_bounds__(256)
k_pack_mask(const uint8_t *__restrict__ mask, int64_t N, uint64_t *__restrict__ mbits, int64_t W,
            unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= W) return;
  const int64_t i = w * 64 + lane;
  const bool on = (i < N) && mask[i];
  const uint64_t word = __ballot(on);
  if (lane == 0) {
    mbits[w] = word;
    if (word) atomicAdd(&counters[0], (unsigned long long)__popcll(word));
  }
}

// one wavefront per owned row; lanes stride over the row's words (coalesced)
__global__ void __launch_bounds__(256)
k_level(const uint64_t *__restrict__ bits, int64_t W, const uint64_t *__restrict__ mbits,
        const uint8_t *__restrict__ mask_in, uint8_t *__restrict__ mask_out, int64_t N, int64_t k,
        int IB, int64_t rank, int64_t world, int64_t rows_local) {
  const int lane = threadIdx.x & 63;
  const int64_t lrow = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (lrow >= rows_local) return;
  const int64_t lb = lrow / IB;
  const int64_t i = global_block(lb, rank, world) * IB + (lrow % IB);
  if (i >= N) return;
  if (!mask_in[i]) {
    if (lane == 0) mask_out[i] = 0;
    return;
  }
  const int64_t chunk = N / k;
  int64_t c = chunk > 0 ? i / chunk : 0;
  if (c > k - 1) c = k - 1;
  const int64_t last = (c == k - 1) ? N : chunk * (c + 1);  // exclusive
  // columns j in (i, last)
  const int64_t w0 = (i + 1) >> 6;
  const int64_t w1 = (last - 1) >> 6;  // inclusive; last >= i+1 always
  bool hit = false;
  const uint64_t *row = bits + lrow * W;
  for (int64_t w = w0 + lane; w <= w1; w += 64) {
    uint64_t x = row[w] & mbits[w];
    if (w == w0) {
      const int s = (int)((i + 1) & 63);
      x &= (~0ull) << s;
    }
    if (w == w1) {
      const int e = (int)((last - 1) & 63);  // keep bits 0..e
      x &= (e == 63) ? ~0ull : ((1ull << (e + 1)) - 1ull);
    }
    hit |= (x != 0);
  }
  const bool any = __any(hit);
  if (lane == 0) mask_out[i] = any ? 0 : 1;
}

// ---------------------------------------------------------------------------
// Single-GPU ladder without host round trips: every level is ONE launch that
// decides on the device whether the reference would run it
// (k == 1 or min_per_group * k < n_active), so the host can enqueue the whole
// ladder behind the similarity kernels and synchronise once.
// mask words: mb_in (read), mb_out (zeroed beforehand, survivors OR their bit).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_mask_init(uint64_t *__restrict__ mb, int64_t N, int64_t W, int64_t total_words) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= total_words) return;
  if (w >= W) {  // the level outputs start from zero (survivors OR their bit in)
    mb[w] = 0;
    return;
  }
  const int64_t lo = w * 64;
  uint64_t v = 0;
  if (lo + 64 <= N) v = ~0ull;
  else if (lo < N) v = (1ull << (N - lo)) - 1ull;
  mb[w] = v;
}

__global__ void __launch_bounds__(256)
k_level_fused(const uint64_t *__restrict__ bits, int64_t W, const uint64_t *__restrict__ mb_in,
              uint64_t *__restrict__ mb_out, int64_t N, int64_t k, int64_t min_per_group,
              unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= N) return;
  const bool active = (mb_in[i >> 6] >> (i & 63)) & 1ull;
  if (!active) return;  // wave-uniform
  // every wave recounts the active set (W words: a few coalesced loads per lane)
  // and learns whether its row is the first active one (it reports the level)
  int cnt = 0;
  bool before = false;
  for (int64_t w = lane; w < W; w += 64) {
    const uint64_t m = mb_in[w];
    cnt += __popcll(m);
    if (w < (i >> 6)) before |= (m != 0);
    else if (w == (i >> 6)) before |= ((m & ((1ull << (i & 63)) - 1ull)) != 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  const bool first = !__any(before);
  const bool run = (k == 1) || (min_per_group * k < (int64_t)cnt);
  bool hit = false;
  if (run) {
    const int64_t chunk = N / k;
    int64_t c = chunk > 0 ? i / chunk : 0;
    if (c > k - 1) c = k - 1;
    const int64_t last = (c == k - 1) ? N : chunk * (c + 1);
    const int64_t w0 = (i + 1) >> 6, w1 = (last - 1) >> 6;
    const uint64_t *row = bits + i * W;
    for (int64_t w = w0 + lane; w <= w1; w += 64) {
      uint64_t x = row[w] & mb_in[w];
      if (w == w0) x &= (~0ull) << (int)((i + 1) & 63);
      if (w == w1) {
        const int e = (int)((last - 1) & 63);
        x &= (e == 63) ? ~0ull : ((1ull << (e + 1)) - 1ull);
      }
      hit |= (x != 0);
    }
  }
  const bool any = __any(hit);
  if (lane == 0) {
    if (!any) atomicOr(reinterpret_cast<unsigned long long *>(&mb_out[i >> 6]), 1ull << (i & 63));
    if (run && first && counters != nullptr) atomicAdd(&counters[8], 1ull);
  }
}

// Per ladder level, the similar pairs that can act at it: i and j share a chunk at ladder value
// ladder[l].  k_pair_buckets (grid wide: the 2 x n_ladder integer divisions per pair cost
// nothing there) copies every pair into the bucket of each such level -- wave-aggregated
// appends, one atomic per wavefront and level -- so that the one-workgroup ladder kernel
// below touches, at a level, only the pairs that matter at it: about 2 P visits in total
// instead of n_ladder x P.  The last level (k = 1: one chunk, every pair) needs no bucket.
// level_cnt = counters + kCntLevel (one counter per 128-byte line); buckets: n_ladder regions of `cap` pairs.
__global__ void __launch_bounds__(256)
k_pair_buckets(const uint64_t *__restrict__ pairs, const unsigned long long *__restrict__ n_pairs_ptr,
               unsigned long long cap, int64_t N, const int64_t *__restrict__ ladder, int n_ladder,
               uint64_t *__restrict__ buckets, unsigned long long *__restrict__ level_cnt,
               const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap) {
  const unsigned long long P = *n_pairs_ptr;
  if (P > cap) return;
  // candidate queue overflow: the refine took the word queue and wrote no pair list -- counters[2]
  // then counts similar pairs the list (sized like the candidate queue) does not hold
  if (n_cand_ptr != nullptr && *n_cand_ptr > cand_cap) return;
  const uint32_t n32 = (uint32_t)N;
  const int lane = threadIdx.x & 63;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < P;
       base += stride) {  // wave-uniform trip count: the ballots below see whole wavefronts
    const unsigned long long p = base + lane;
    const uint64_t e = p < P ? pairs[p] : ~0ull;
    const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
    const bool valid = j > i && j < n32;  // padding / malformed entries never act
    uint32_t mine = 0;                    // bit l: this lane's pair acts at level l
    unsigned long long my_cnt = 0;        // lane l: how many pairs of the wavefront act at level l
    for (int l = 0; l < n_ladder; ++l) {
      const uint32_t k = (uint32_t)ladder[l];
      if (k == 1u) continue;  // served from the list itself
      const uint32_t chunk = n32 / k;
      bool same = false;
      if (valid && chunk != 0) {  // chunk == 0: k > N, the level can never run
        uint32_t ci = i / chunk, cj = j / chunk;
        if (ci > k - 1) ci = k - 1;
        if (cj > k - 1) cj = k - 1;
        same = ci == cj;
      }
      if (same) mine |= 1u << l;
      const unsigned long long c = (unsigned long long)__popcll(__ballot(same));
      if (lane == l) my_cnt = c;
    }
    // ONE atomic instruction reserves the wavefront's slots in every bucket: lane l asks for level l
    unsigned long long my_at = 0;
    if (my_cnt) my_at = atomicAdd(&level_cnt[lane * kCntLevelStride], my_cnt);
    for (int l = 0; l < n_ladder; ++l) {
      const bool same = (mine >> l) & 1u;
      const uint64_t m = __ballot(same);
      if (m == 0) continue;  // wave-uniform
      const unsigned long long at = __shfl(my_at, l);
      if (same) buckets[(unsigned long long)l * cap + at + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = e;
    }
  }
}

// ---------------------------------------------------------------------------
// k_ladder_pairs: the WHOLE k-ladder in one launch when similarity is sparse.
// With the exactly-similar pairs as a list (i < j), a level is
//     for every pair: in[i] && in[j] && chunk_k(i) == chunk_k(j)  ->  out[i] = 0
// so one 1024-thread workgroup keeps the mask words in LDS, walks the level's bucket
// (k_pair_buckets; the list itself at k = 1) and separates levels with __syncthreads(): no
// grid barrier, no host round trip.  `n_pairs_ptr`/`n_cand_ptr` are device
// counters (the refine kernel's outputs); the kernel does nothing -- and leaves
// counters[9] = 0 -- when the list is incomplete (candidate queue overflow) or
// longer than `cap`, in which case the bit-matrix levels launched behind it do
// the work (the host sees the flag with the results and launches them only then);
// otherwise it sets counters[9] = 1.  counters[8] = levels that ran.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_ladder_pairs(const uint64_t *__restrict__ pairs, const uint64_t *__restrict__ buckets,
               const unsigned long long *__restrict__ n_pairs_ptr,
               const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap,
               unsigned long long cap, int64_t N, int64_t W, int64_t min_per_group,
               const int64_t *__restrict__ ladder, int n_ladder, uint64_t *__restrict__ mask_out,
               unsigned long long *__restrict__ counters, int drop_later) {
  extern __shared__ unsigned long long lm[];  // cur[W] | nxt[W]
  __shared__ int s_count;
  __shared__ unsigned long long s_level_cnt[32];
  const int tid = threadIdx.x;
  const unsigned long long P = *n_pairs_ptr;
  if ((n_cand_ptr != nullptr && *n_cand_ptr > cand_cap) || P > cap || counters[12] != 0ull) {  // [12]: the screen's verdict asked for a redo
    if (tid == 0) counters[9] = 0;
    if (tid < 16) mask_out[W + tid] = tid == 9 ? 0ull : counters[tid];
    return;
  }
  if (tid < 32) s_level_cnt[tid] = tid < n_ladder ? counters[kCntLevel + kCntLevelStride * tid] : 0ull;  // one round trip, not one per level
  unsigned long long *cur = lm, *nxt = lm + W;
  for (int64_t w = tid; w < W; w += 1024) {
    const int64_t lo = w * 64;
    cur[w] = (lo + 64 <= N) ? ~0ull : ((lo < N) ? ((1ull << (N - lo)) - 1ull) : 0ull);
  }
  const uint32_t n32 = (uint32_t)N;
  __syncthreads();
  int levels = 0;
  for (int l = 0; l < n_ladder; ++l) {
    const int64_t k = ladder[l];
    if (tid == 0) s_count = 0;
    __syncthreads();
    int c = 0;
    for (int64_t w = tid; w < W; w += 1024) c += __popcll(cur[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0 && c) atomicAdd(&s_count, c);
    __syncthreads();
    const bool run = (k == 1) || (min_per_group * k < (int64_t)s_count);
    if (!run) continue;  // block-uniform
    ++levels;
    for (int64_t w = tid; w < W; w += 1024) nxt[w] = cur[w];
    __syncthreads();
    // the pairs of this level: its bucket, or the whole list at k = 1.  Eight independent
    // loads in flight per lane: a single workgroup cannot hide one L2 round trip per pair
    // behind other waves
    const uint64_t *__restrict__ src = (k == 1) ? pairs : buckets + (unsigned long long)l * cap;
    const unsigned long long n_src = (k == 1) ? P : s_level_cnt[l];
    constexpr int U = 8;
    for (unsigned long long p0 = tid; p0 < n_src; p0 += 1024ull * U) {
      uint64_t ev[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned long long p = p0 + 1024ull * u;
        ev[u] = p < n_src ? src[p] : ~0ull;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t i = (uint32_t)(ev[u] >> 32), j = (uint32_t)(ev[u] & 0xffffffffull);
        if (j > i && j < n32) {  // not padding
          if (((cur[i >> 6] >> (i & 63)) & 1ull) && ((cur[j >> 6] >> (j & 63)) & 1ull)) {
            const uint32_t kill = drop_later ? j : i;  // fc_prune_conventions: which member of a similar pair falls
            atomicAnd(&nxt[kill >> 6], ~(1ull << (kill & 63)));
          }
        }
      }
    }
    __syncthreads();
    unsigned long long *t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int64_t w = tid; w < W; w += 1024) mask_out[w] = cur[w];
  if (tid == 0) {
    counters[8] = (unsigned long long)levels;
    counters[9] = 1;
  }
  // the 16 counters ride behind the mask words so that the host needs ONE copy
  if (tid < 16)
    mask_out[W + tid] = tid == 8 ? (unsigned long long)levels : tid == 9 ? 1ull : counters[tid];
}

// ---------------------------------------------------------------------------
// Device-resident exchange of the sharded prune (fc_prune_export_pairs_dev /
// fc_prune_from_gathered_dev): a rank's message is cap+1 words -- its count
// (kPairsNone when its candidate queue overflowed), its exactly-similar pairs,
// padding -- written straight into the caller's collective buffer; the
// gathered world*(cap+1) words are compacted into one list whose length goes
// to counters[2].  A message that is missing or longer than cap makes the
// length ~0, so the ladder kernel behind declines (counters[9] = 0) and the
// caller takes the host path.
// ---------------------------------------------------------------------------
constexpr unsigned long long kPairsNone = 0xFFFFFFFFFFFFFFFEull;
constexpr unsigned long long kPairsPad = 0xFFFFFFFFFFFFFFFFull;

__global__ void __launch_bounds__(256)
k_export_pairs(const uint64_t *__restrict__ simq, const unsigned long long *__restrict__ counters,
               unsigned long long cand_cap, int64_t cap, uint64_t *__restrict__ out) {
  const unsigned long long n = counters[2];
  // [12]: this rank's speculative screen was voted down in the "decline, redo later" mode of the single-GPU pipeline
  // (Context::optimistic_screen; k_screen_verdict has emptied the queues).  The sharded pipeline redoes such a screen in
  // place and never gets here with [12] set; should that change, the other ranks must not take this rank's EMPTY list
  // for its answer, nor stay on the pair path while this rank leaves it: the message says "none", every rank declines.
  const bool overflow = counters[6] > cand_cap || counters[12] != 0ull;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) out[0] = overflow ? kPairsNone : n;
  for (int64_t p = t; p < cap; p += stride)
    out[1 + p] = (!overflow && (unsigned long long)p < n) ? simq[p] : kPairsPad;
}

__global__ void __launch_bounds__(1024)
k_compact_gathered(const uint64_t *__restrict__ gathered, int world, int64_t cap,
                   uint64_t *__restrict__ list, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long s_off[65];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) {
    unsigned long long off = 0;
    int bad = 0;
    for (int r = 0; r < world; ++r) {
      const unsigned long long c = gathered[(int64_t)r * (cap + 1)];
      if (c > (unsigned long long)cap) bad = 1;  // includes kPairsNone
      s_off[r] = off;
      off += bad ? 0ull : c;
    }
    s_off[world] = off;
    s_bad = bad;
    counters[2] = bad ? ~0ull : off;
    counters[10] = (unsigned long long)bad;
  }
  __syncthreads();
  if (s_bad) return;
  for (int r = 0; r < world; ++r) {
    const uint64_t *src = gathered + (int64_t)r * (cap + 1) + 1;
    const unsigned long long c = s_off[r + 1] - s_off[r];
    uint64_t *dst = list + s_off[r];
    for (unsigned long long p = tid; p < c; p += 1024) dst[p] = src[p];
  }
}

// copy for rows a rank does not own (sharded levels)
__global__ void __launch_bounds__(256)
k_copy_bytes(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// moments of inertia: one lane per conformer; 3x3 symmetric eigenvalues by
// cyclic Jacobi (same rotation as the 4x4 case), sorted ascending.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sym3_eigvals(double a00, double a01, double a02, double a11,
                                             double a12, double a22, double (&w)[3]) {
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(a01) + fabs(a02) + fabs(a12);
    if (off == 0.0) break;
    const bool late = sweep > 3;
    // (0,1)
    {
      const double g = 100.0 * fabs(a01);
      if (late && fabs(a00) + g == fabs(a00) && fabs(a11) + g == fabs(a11)) a01 = 0.0;
      else if (a01 != 0.0) {
        const double h = a11 - a00;
        double t;
        if (fabs(h) + g == fabs(h)) t = a01 / h;
        else { const double th = 0.5 * h / a01; t = 1.0 / (fabs(th) + sqrt(1.0 + th * th)); if (th < 0.0) t = -t; }
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c), hh = t * a01;
        a00 -= hh; a11 += hh; a01 = 0.0;
        const double p = a02, q = a12;
        a02 = p - s * (q + p * tau);
        a12 = q + s * (p - q * tau);
      }
    }
    // (0,2)
    {
      const double g = 100.0 * fabs(a02);
      if (late && fabs(a00) + g == fabs(a00) && fabs(a22) + g == fabs(a22)) a02 = 0.0;
      else if (a02 != 0.0) {
        const double h = a22 - a00;
        double t;
        if (fabs(h) + g == fabs(h)) t = a02 / h;
        else { const double th = 0.5 * h / a02; t = 1.0 / (fabs(th) + sqrt(1.0 + th * th)); if (th < 0.0) t = -t; }
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c), hh = t * a02;
        a00 -= hh; a22 += hh; a02 = 0.0;
        const double p = a01, q = a12;  // a[1][0], a[1][2]
        a01 = p - s * (q + p * tau);
        a12 = q + s * (p - q * tau);
      }
    }
    // (1,2)
    {
      const double g = 100.0 * fabs(a12);
      if (late && fabs(a11) + g == fabs(a11) && fabs(a22) + g == fabs(a22)) a12 = 0.0;
      else if (a12 != 0.0) {
        const double h = a22 - a11;
        double t;
        if (fabs(h) + g == fabs(h)) t = a12 / h;
        else { const double th = 0.5 * h / a12; t = 1.0 / (fabs(th) + sqrt(1.0 + th * th)); if (th < 0.0) t = -t; }
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c), hh = t * a12;
        a11 -= hh; a22 += hh; a12 = 0.0;
        const double p = a01, q = a02;  // a[0][1], a[0][2]
        a01 = p - s * (q + p * tau);
        a02 = q + s * (p - q * tau);
      }
    }
  }
  double x = a00, y = a11, z = a22, t;
  if (x > y) { t = x; x = y; y = t; }
  if (y > z) { t = y; y = z; z = t; }
  if (x > y) { t = x; x = y; y = t; }
  w[0] = x; w[1] = y; w[2] = z;
}

__global__ void __launch_bounds__(256)
k_inertia_moments(const double *__restrict__ coords, int64_t N, int64_t A,
                  const double *__restrict__ masses, double *__restrict__ moments) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const double *x = coords + n * A * 3;
  double mt = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
  for (int64_t a = 0; a < A; ++a) {
    const double m = masses[a];
    mt += m;
    cx += x[a * 3] * m;
    cy += x[a * 3 + 1] * m;
    cz += x[a * 3 + 2] * m;
  }
  cx /= mt; cy /= mt; cz /= mt;
  double ixx = 0, iyy = 0, izz = 0, ixy = 0, ixz = 0, iyz = 0;
  for (int64_t a = 0; a < A; ++a) {
    const double m = masses[a];
    const double rx = x[a * 3] - cx, ry = x[a * 3 + 1] - cy, rz = x[a * 3 + 2] - cz;
    const double r2 = rx * rx + ry * ry + rz * rz;
    ixx += m * (r2 - rx * rx);
    iyy += m * (r2 - ry * ry);
    izz += m * (r2 - rz * rz);
    ixy += m * (0.0 - rx * ry);
    ixz += m * (0.0 - rx * rz);
    iyz += m * (0.0 - ry * rz);
  }
  double w[3];
  sym3_eigvals(ixx, ixy, ixz, iyy, iyz, izz, w);
  moments[n * 3 + 0] = w[0];
  moments[n * 3 + 1] = w[1];
  moments[n * 3 + 2] = w[2];
}

// MOI similarity bits: bit j of row i (j > i) = all_k !(|I_i[k]-I_j[k]| / I_i[k] >= tol)
// [&& |E_i - E_j| < max_dE].  One wavefront per (row, 64-column word).
// The negated >= is the oracle's early exit, not the same as < : 0/0 (two zero moments: linear
// molecules on an axis, single atoms) is not a number, fails >= and leaves the pair similar
// ("MOI prune: zero moments").
__global__ void __launch_bounds__(256)
k_moi_simbits(const double *__restrict__ moments, int64_t N, double tol,
              const double *__restrict__ energies, double max_dE, uint64_t *__restrict__ bits,
              int64_t W) {
  const int lane = threadIdx.x & 63;
  // row in blockIdx.x, four words of it per workgroup in blockIdx.y: a flat index over the N * W wavefronts
  // passes 2^32 threads at N = 65 536, more than one grid dimension takes
  const int64_t i = blockIdx.x, jt = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
  if (jt >= W) return;
  if (jt * 64 + 63 <= i) return;
  const int64_t j = jt * 64 + lane;
  bool sim = false;
  if (j < N && j > i) {
    const double a0 = moments[i * 3], a1 = moments[i * 3 + 1], a2 = moments[i * 3 + 2];
    const double b0 = moments[j * 3], b1 = moments[j * 3 + 1], b2 = moments[j * 3 + 2];
    sim = !(fabs(a0 - b0) / a0 >= tol) && !(fabs(a1 - b1) / a1 >= tol) && !(fabs(a2 - b2) / a2 >= tol);
    if (energies != nullptr) sim = sim && (fabs(energies[i] - energies[j]) < max_dE);
  }
  const uint64_t word = __ballot(sim);
  if (lane == 0) bits[i * W + jt] = word;
}

// TFD similarity (firecode/torsion_module.py:1056-1067):
//   deltas = |tf_i - tf_j|; deltas = |deltas - (deltas > 180)*360|; np.sum(deltas) < thresh
// np.sum adds a contiguous float64 vector in its "pairwise" order: plain
// left-to-right below 8 elements, otherwise 8 running lanes r[k] += a[8m+k]
// combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the n%8 tail added one
// by one (verified against np.sum bit for bit for n <= 128; the launcher
// refuses Q > 128, where NumPy starts to recurse).
__device__ __forceinline__ double tfd_delta(const double *__restrict__ ti, const double *__restrict__ tj,
                                            int q, int64_t si, int64_t sj) {
  double d = fabs(ti[q * si] - tj[q * sj]);
  return fabs(d - (d > 180.0 ? 360.0 : 0.0));
}

// ti / tj: fingerprint of one structure with element stride si / sj
__device__ __forceinline__ double tfd_sum(const double *__restrict__ ti, int64_t si,
                                          const double *__restrict__ tj, int64_t sj, int Q) {
  if (Q < 8) {
    double res = 0.0;
    for (int q = 0; q < Q; ++q) res += tfd_delta(ti, tj, q, si, sj);
    return res;
  }
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = tfd_delta(ti, tj, k, si, sj);
  int i = 8;
  for (; i < Q - (Q % 8); i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] += tfd_delta(ti, tj, i + k, si, sj);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < Q; ++i) res += tfd_delta(ti, tj, i, si, sj);
  return res;
}

// bits over all j != i, rows [row_begin, row_end): one wavefront per (row, word)
__global__ void __launch_bounds__(256)
k_tfd_simbits(const double *__restrict__ tf, int64_t N, int Q, double thresh, int64_t row_begin,
              int64_t row_end, uint64_t *__restrict__ bits, int64_t W) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t r = wave / W, jt = wave % W;
  const int64_t i = row_begin + r;
  if (i >= row_end) return;
  const int64_t j = jt * 64 + lane;
  bool sim = false;
  if (j < N && j != i) sim = tfd_sum(tf + i * Q, 1, tf + j * Q, 1, Q) < thresh;
  const uint64_t word = __ballot(sim);
  if (lane == 0) bits[r * W + jt] = word;
}

// first_match[i] = min{ j > i : tfd_similar(i, j) } (or -1): everything the
// k-ladder of prune_conformers_tfd needs, in N integers instead of N^2 bits.
// tfT is fingerprint-major (tfT[q*Npad + n]) so that lanes owning consecutive
// columns load coalesced.  Workgroup = 64 rows (fingerprints in LDS) x a
// running window of 256 columns; a row retires at its first hit and the
// workgroup stops when all its rows have.
template <int QT>  // QT > 0: fingerprint length known at compile time (column kept in VGPRs)
__global__ void __launch_bounds__(256)
k_tfd_first_match(const double *__restrict__ tfT, int64_t N, int64_t Npad, int Qrt, double thresh,
                  int64_t *__restrict__ first_match, const float *__restrict__ tfF, int64_t max_ahead,
                  unsigned long long *__restrict__ left_count, int64_t *__restrict__ left_rows,
                  int64_t *__restrict__ left_from) {
  const int Q = QT > 0 ? QT : Qrt;
  extern __shared__ double rows[];              // [64][Q]
  __shared__ long long best[64];
  __shared__ int n_open;
  // Pre-filter in single precision on the first (up to) four angles: the deltas are non-negative, so a
  // pair whose partial sum already reaches the threshold cannot be similar; only pairs below
  // thresh + 0.01 (fp32 error of four terms <= 360: < 1e-4) get the exact fp64 sum in NumPy's order.
  // On a systematic scan one pair in ~10^3 passes, i.e. 19 wavefront-instructions in 20 skip the fp64 sum.
  constexpr int QF = 8;  // (eight angles: in a systematic scan the first ones are EQUAL over long runs of columns,
                         // with four every column of such a run went on to the fp64 sum)
  __shared__ float rowsF[64][QF];
  const int qf = Q < QF ? Q : QF;
  const float threshF = (float)thresh + 0.01f;
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * 64;
  for (int k = tid; k < 64 * Q; k += 256) {
    const int r = k / Q, q = k % Q;
    rows[k] = (i0 + r < N) ? tfT[(int64_t)q * Npad + i0 + r] : 0.0;
    if (q < QF) rowsF[r][q] = (float)rows[k];
  }
  if (tid < 64) best[tid] = (i0 + tid < N) ? (long long)N : -2;  // N = none yet, -2 = no such row
  if (tid == 0) n_open = (int)((N - i0 < 64) ? (N - i0) : 64);
  __syncthreads();
  // Rows retire at very different distances (in a systematic scan the first match of a
  // conformer can be 10^5 columns away), so the window loop works on the COMPACTED list of
  // rows that are still open and widens the window as that list shrinks: a workgroup left
  // with one open row covers 4096 columns per pair of barriers instead of 256.
  __shared__ int open_rows[64];
  int64_t jb = i0 + 1;
  // max_ahead > 0: the workgroup gives up max_ahead columns past its rows; what is still open then goes to
  // the leftover list (row, first column not looked at) for k_tfd_first_match_rest.  A workgroup that walks
  // the whole array for a row without a match is one latency-bound chain of ~3 000 windows: at 1.7 M
  // structures that chain, not the arithmetic, was the kernel's 50 ms.
  const int64_t j_stop = max_ahead > 0 ? (i0 + 64 + max_ahead < N ? i0 + 64 + max_ahead : N) : N;
  while (jb < j_stop) {
    if (tid < 64) {  // wave 0: compact the open rows (ballot order = row order)
      const bool is_open = best[tid] == (long long)N;
      const uint64_t m = __ballot(is_open);
      if (is_open) open_rows[__popcll(m & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) n_open = __popcll(m);
    }
    __syncthreads();
    const int R = n_open;
    if (R == 0) break;
    const int cpt = R >= 32 ? 1 : R >= 16 ? 2 : R >= 8 ? 4 : R >= 4 ? 8 : 16;  // columns per thread
    if (tfF != nullptr) {
      // four columns per thread at a time, their pre-filter values requested TOGETHER: with one column per
      // trip of a loop full of branches the loads are issued one latency after the other, and a workgroup
      // down to its last open row (most of them, most of the time) is nothing but those latencies
      for (int c0 = 0; c0 < cpt; c0 += 4) {
        float cf4[4][QF];
        int64_t j4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          j4[u] = jb + (int64_t)(c0 + u) * 256 + tid;
          const bool on = c0 + u < cpt && j4[u] < N;
          const int64_t jl = on ? j4[u] : N - 1;
#pragma unroll
          for (int q = 0; q < QF; ++q) cf4[u][q] = q < qf ? tfF[(int64_t)q * Npad + jl] : 0.f;
          if (!on) j4[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t j = j4[u];
          if (j < 0) continue;
          for (int k = 0; k < R; ++k) {
            const int r = open_rows[k];
            const int64_t i = i0 + r;
            if (j <= i) continue;
            float part;
            {
              const float d = fabsf(rowsF[r][0] - cf4[u][0]);
              part = fabsf(d - (d > 180.f ? 360.f : 0.f));
            }
            if (!(part < threshF)) continue;
#pragma unroll
            for (int q = 1; q < QF; ++q)
              if (q < qf) {
                const float d = fabsf(rowsF[r][q] - cf4[u][q]);
                part += fabsf(d - (d > 180.f ? 360.f : 0.f));
              }
            if (!(part < threshF)) continue;
            const double sum = tfd_sum(rows + r * Q, 1, tfT + j, Npad, Q);
            if (sum < thresh) atomicMin(&best[r], (long long)j);
          }
        }
      }
    } else
    for (int c = 0; c < cpt; ++c) {
      const int64_t j = jb + (int64_t)c * 256 + tid;
      if (j < N) {
        // tfF: single-precision copy of the first four angles (16 B per column instead of 8 Q): a workgroup
        // whose last open row has no match reads every later column, and nearly every workgroup of a
        // systematic scan has such a row -- the kernel is bound by that traffic, not by its arithmetic;
        // the fp64 column is read only for the pairs the pre-filter lets through
        double cj[QT > 0 ? QT : 1];
        if (QT > 0 && tfF == nullptr) {
#pragma unroll
          for (int q = 0; q < QT; ++q) cj[q] = tfT[(int64_t)q * Npad + j];
        }
        float cf[QF];
#pragma unroll
        for (int q = 0; q < QF; ++q)
          cf[q] = q < qf ? (tfF != nullptr ? tfF[(int64_t)q * Npad + j]
                                           : (float)(QT > 0 ? cj[q < (QT > 0 ? QT : 1) ? q : 0] : tfT[(int64_t)q * Npad + j]))
                         : 0.f;
        for (int k = 0; k < R; ++k) {
          const int r = open_rows[k];
          const int64_t i = i0 + r;
          // a hit in an earlier window is final (the row is no longer in the list); hits inside
          // this window are resolved with atomicMin
          if (j <= i) continue;
          // the deltas are non-negative and fp32 addition is monotone: the partial sum after any prefix
          // already decides.  In a systematic scan the first angles vary slowest -- whole windows of columns
          // share them -- so the test on the first angle alone sends most WAVEFRONTS past the rest
          float part;
          {
            const float d = fabsf(rowsF[r][0] - cf[0]);
            part = fabsf(d - (d > 180.f ? 360.f : 0.f));
          }
          if (!(part < threshF)) continue;
#pragma unroll
          for (int q = 1; q < QF; ++q)
            if (q < qf) {
              const float d = fabsf(rowsF[r][q] - cf[q]);
              part += fabsf(d - (d > 180.f ? 360.f : 0.f));
            }
          if (!(part < threshF)) continue;
          const double sum = (QT > 0 && tfF == nullptr) ? tfd_sum(rows + r * Q, 1, cj, 1, QT)
                                                        : tfd_sum(rows + r * Q, 1, tfT + j, Npad, Q);
          if (sum < thresh) atomicMin(&best[r], (long long)j);
        }
      }
    }
    jb += (int64_t)cpt * 256;
    __syncthreads();
  }
  if (tid < 64 && i0 + tid < N) {
    const bool open = best[tid] >= (long long)N;
    first_match[i0 + tid] = open ? -1 : best[tid];
    if (open && jb < N) {  // stopped at the look-ahead limit: somebody else scans [jb, N) for this row
      const unsigned long long slot = atomicAdd(left_count, 1ull);
      left_rows[slot] = i0 + tid;
      left_from[slot] = jb;
    }
  }
}

// Bounding box of the first (up to) four angles over every window of 1024 columns: wlo / whi[q * n_win + w].
__global__ void __launch_bounds__(256)
k_tfd_window_bounds(const float *__restrict__ tfF, int64_t N, int64_t Npad, int qf, int64_t n_win,
                    float *__restrict__ wlo, float *__restrict__ whi) {
  __shared__ float slo[4][4], shi[4][4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int64_t w = blockIdx.x, j0 = w * 1024;
  for (int q = 0; q < qf; ++q) {
    float lo = 1e30f, hi = -1e30f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = j0 + (int64_t)u * 256 + tid;
      if (j < N) {
        const float v = tfF[(int64_t)q * Npad + j];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, off));
      hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if (lane == 0) slo[q][wv] = lo, shi[q][wv] = hi;
  }
  __syncthreads();
  if (tid < qf) {
    wlo[(int64_t)tid * n_win + w] = fminf(fminf(slo[tid][0], slo[tid][1]), fminf(slo[tid][2], slo[tid][3]));
    whi[(int64_t)tid * n_win + w] = fmaxf(fmaxf(shi[tid][0], shi[tid][1]), fmaxf(shi[tid][2], shi[tid][3]));
  }
}

// The rows k_tfd_first_match gave up on (no match within its look-ahead), 64 of them per workgroup in list order,
// against ONE chunk of columns: the rectangle (leftover rows) x (all later columns) cut into independent pieces,
// first match = atomicMin over the pieces.  best[slot]: initialised to ~0, holds the smallest matching column.
// Most of the rectangle is never looked at: a row takes part in a window of 1024 columns only if the window's
// bounding box of the first angles comes within the threshold of its own (a lower bound of every column's TFD:
// the distance of the row's angle to the window's interval, wrap-around included, summed over the angles).  In a
// systematic scan the first angles vary slowest -- a window holds ONE value of each of the first three -- so a row
// meets about one window in 6^3.
template <int QT>
__global__ void __launch_bounds__(256)
k_tfd_first_match_rest(const double *__restrict__ tfT, const float *__restrict__ tfF, int64_t N, int64_t Npad, int Qrt,
                       double thresh, const unsigned long long *__restrict__ left_count,
                       const int64_t *__restrict__ left_rows, const int64_t *__restrict__ left_from, int64_t chunk,
                       unsigned long long *__restrict__ best, const float *__restrict__ wlo,
                       const float *__restrict__ whi, int64_t n_win) {
  const int Q = QT > 0 ? QT : Qrt;
  extern __shared__ double rows[];  // [64][Q]
  constexpr int QF = 8, QB = 4;  // angles of the fp32 pre-filter / of the window boxes
  __shared__ float rowsF[64][QF];
  __shared__ long long row_i[64], row_from[64];
  __shared__ unsigned long long wmask[64];  // per window of the chunk: the rows that take part
  const int qf = Q < QF ? Q : QF, qb = Q < QB ? Q : QB;
  const float threshF = (float)thresh + 0.01f;
  const int tid = threadIdx.x;
  const unsigned long long n_left = *left_count;
  const unsigned long long g0 = (unsigned long long)blockIdx.x * 64ull;
  if (g0 >= n_left) return;  // block-uniform
  const int64_t c_lo = (int64_t)blockIdx.y * chunk, c_hi = c_lo + chunk < N ? c_lo + chunk : N;
  __shared__ float blo[QB][64], bhi[QB][64];  // the chunk's window boxes
  __shared__ long long from_min_s;
  const int n_w = (int)((c_hi - c_lo + 1023) / 1024);  // <= 64 (chunk = 65536)
  if (tid < 64) {
    const bool on = g0 + tid < n_left;
    row_i[tid] = on ? left_rows[g0 + tid] : -1;
    const long long from = on ? left_from[g0 + tid] : (long long)N;
    row_from[tid] = from;
    wmask[tid] = 0ull;
    long long fm_ = from;
    for (int off = 32; off > 0; off >>= 1) {
      const long long o = __shfl_xor(fm_, off);
      fm_ = o < fm_ ? o : fm_;
    }
    if (tid == 0) from_min_s = fm_;
  }
  __syncthreads();
  if (from_min_s >= (long long)c_hi) return;  // block-uniform: every row of the group starts behind this chunk
  for (int k = tid; k < 64 * Q; k += 256) {
    const int r = k / Q, q = k % Q;
    rows[k] = row_i[r] >= 0 ? tfT[(int64_t)q * Npad + row_i[r]] : 0.0;
    if (q < QF) rowsF[r][q] = (float)rows[k];
  }
  for (int t = tid; t < QB * n_w; t += 256) {
    const int q = t / n_w, wl = t % n_w;
    const bool have = q < qb;
    blo[q][wl] = have ? wlo[(int64_t)q * n_win + (c_lo >> 10) + wl] : 0.f;
    bhi[q][wl] = have ? whi[(int64_t)q * n_win + (c_lo >> 10) + wl] : 0.f;
  }
  __syncthreads();
  // which rows meet which window: 64 windows x 64 rows, 16 tests per thread
  for (int t = tid; t < 64 * n_w; t += 256) {
    const int wl = t >> 6, r = t & 63;
    const int64_t w = (c_lo >> 10) + wl, w_end = (w + 1) * 1024 < c_hi ? (w + 1) * 1024 : c_hi;
    bool on = row_from[r] < (long long)w_end;
    if (on) {
      float lb = 0.f;
      for (int q = 0; q < qb; ++q) {
        const float a = rowsF[r][q], lo = blo[q][wl], hi = bhi[q][wl];
        const float d0 = fmaxf(fmaxf(lo - a, a - hi), 0.f);
        const float ap = a + 360.f, am = a - 360.f;
        const float d1 = fmaxf(fmaxf(lo - ap, ap - hi), 0.f), d2 = fmaxf(fmaxf(lo - am, am - hi), 0.f);
        lb += fminf(d0, fminf(d1, d2));
      }
      on = lb < threshF + 0.01f;  // (+ 0.01: roundings of the wrapped copies, far below it)
    }
    if (on) atomicOr(&wmask[wl], 1ull << r);
  }
  __syncthreads();
  for (int wl = 0; wl < n_w; ++wl) {
    unsigned long long m = wmask[wl];
    if (m == 0ull) continue;  // block-uniform
    const int64_t jb = c_lo + (int64_t)wl * 1024;
    float cf4[4][QF];
    int64_t j4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      j4[u] = jb + (int64_t)u * 256 + tid;
      const bool on = j4[u] < c_hi;
      const int64_t jl = on ? j4[u] : N - 1;
#pragma unroll
      for (int q = 0; q < QF; ++q) cf4[u][q] = q < qf ? tfF[(int64_t)q * Npad + jl] : 0.f;
      if (!on) j4[u] = -1;
    }
    while (m) {  // the rows of this window, in row order (uniform loop)
      const int r = __builtin_ctzll(m);
      m &= m - 1ull;
      const long long from = row_from[r];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = j4[u];
        if (j < from) continue;  // (also j < 0: from > row >= 0; already looked at, or not later than the row)
        float part;
        {
          const float d = fabsf(rowsF[r][0] - cf4[u][0]);
          part = fabsf(d - (d > 180.f ? 360.f : 0.f));
        }
        if (!(part < threshF)) continue;
#pragma unroll
        for (int q = 1; q < QF; ++q)
          if (q < qf) {
            const float d = fabsf(rowsF[r][q] - cf4[u][q]);
            part += fabsf(d - (d > 180.f ? 360.f : 0.f));
          }
        if (!(part < threshF)) continue;
        const double sum = tfd_sum(rows + r * Q, 1, tfT + j, Npad, Q);
        if (sum < thresh) atomicMin(&best[g0 + r], (unsigned long long)j);
      }
    }
  }
}

__global__ void __launch_bounds__(256)
k_tfd_first_match_merge(const unsigned long long *__restrict__ left_count, const int64_t *__restrict__ left_rows,
                        const unsigned long long *__restrict__ best, int64_t *__restrict__ first_match) {
  const unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= *left_count) return;
  const unsigned long long b = best[k];
  first_match[left_rows[k]] = b == ~0ull ? -1 : (int64_t)b;
}

// ---------------------------------------------------------------------------
// First match with 16-bit angles (round 5).  An angle becomes u = rint(a * 65536 / 360) mod 65536 -- the full circle
// on the full range, so the wrap-around of the reference's delta (|d| or |d - 360|: torsion_module.py:1056-1067) is
// the wrap-around of the 16-bit subtraction.  Eight angles of a structure are one 16-byte load (tfU[j]), the test
// of a (row, column) pair is four v_pk_sub_i16 + four v_sad_u16 against the bias 0x8000 (the row is stored with
// that bias, so that the column's angle lands at 0x8000 +- distance and the unsigned |x - 0x8000| is the circular
// distance) where the fp32 pre-filter above spends ~45 vector instructions -- and the first-match kernels at
// 1.7 M structures are bound by exactly those (1.5e9 pair tests in the look-ahead phase).
//   Rounding: |u - a s| <= 0.5 per angle, <= 1 unit per distance, <= 8 units (0.044 deg) over eight angles.  So
//   SAD <  floor(thresh s) - 10  => similar in exact arithmetic too  (only if ALL angles are in the eight: Q <= 8),
//   SAD >= ceil(thresh s) + 10   => not similar (the eight are a lower bound of the sum for any Q),
//   in between (never, on a systematic scan: its angles differ by whole steps) the fp64 sum in NumPy's order decides.
// Valid while the reference's delta IS the circular distance: every |angle| <= 270 (|a - b| <= 540) and finite;
// k_tfd_pack_u16 raises flags[kFmShards] otherwise, the kernels return at once and the host runs the fp32 kernels above.
// ---------------------------------------------------------------------------
typedef unsigned short fc_us2 __attribute__((ext_vector_type(2)));

// The rows the dense phase leaves open go to kFmShards lists, eight consecutive row blocks to the same one: one list
// means one returning atomic per workgroup on ONE address (2.6e4 of them: 0.3 ms by themselves), a list per block
// means walk workgroups of 25 rows instead of 64.  List s holds at most fm_shard_cap(N) rows.
constexpr int kFmShards = 16;
__host__ __device__ inline int64_t fm_shard_cap(int64_t N) {
  const int64_t blocks = (N + 63) / 64, groups = (blocks + 7) / 8;
  return ((groups + kFmShards - 1) / kFmShards) * 8 * 64;
}
struct FmShards {
  unsigned wg_begin[kFmShards + 1];  // walk workgroups [wg_begin[s], wg_begin[s + 1]) take list s
  unsigned count[kFmShards];
};


__device__ __forceinline__ unsigned pk_sub_u16(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, (fc_us2)(__builtin_bit_cast(fc_us2, a) - __builtin_bit_cast(fc_us2, b)));
}

template <int ND>  // dwords that hold angles (two each)
__device__ __forceinline__ unsigned sad_u16x8(const uint4 c, const uint4 row_biased) {
  unsigned s = __builtin_amdgcn_sad_u16(pk_sub_u16(c.x, row_biased.x), 0x80008000u, 0u);
  if (ND > 1) s = __builtin_amdgcn_sad_u16(pk_sub_u16(c.y, row_biased.y), 0x80008000u, s);
  if (ND > 2) s = __builtin_amdgcn_sad_u16(pk_sub_u16(c.z, row_biased.z), 0x80008000u, s);
  if (ND > 3) s = __builtin_amdgcn_sad_u16(pk_sub_u16(c.w, row_biased.w), 0x80008000u, s);
  return s;
}

__global__ void __launch_bounds__(256)
k_tfd_pack_u16(const double *__restrict__ tfT, int64_t N, int64_t Npad, int Q, uint4 *__restrict__ tfU,
               unsigned long long *__restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Npad) return;
  unsigned h[8];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double a = (q < Q && j < N) ? tfT[(int64_t)q * Npad + j] : 0.0;
    if (!(fabs(a) <= 270.0)) bad = true;
    h[q] = bad ? 0u : ((unsigned)(long long)rint(a * (65536.0 / 360.0)) & 0xffffu);
  }
  tfU[j] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  if (bad) atomicOr(&flags[kFmShards], 1ull);
}

constexpr unsigned kFmOpen = 0xffffffffu;

// The pairs of the undecided band take the fp64 sum out of line (never on a systematic scan; inlined at every test
// it cost the kernels half their wavefronts per SIMD).  row / col: fingerprints with element strides rs / cs.
__device__ __attribute__((noinline)) bool tfd_similar_exact(const double *row, int64_t rs, const double *col, int64_t cs,
                                                            int Q, double thresh) {
  return tfd_sum(row, rs, col, cs, Q) < thresh;
}

// Phase 1, dense: the columns right behind a block of 64 rows -- where half the rows of a systematic scan find their
// match -- with LANES = ROWS: the column is the same for the whole wavefront (a scalar load of 16 bytes), every lane
// tests its own row and keeps its first hit in a register.  No LDS reads, ballots or atomics per test: ~14 vector
// instructions per column and 64 rows, where the lanes = columns form (k_tfd_first_match, and the walk below) pays
// ~25 per OPEN row and 64 columns -- the better trade once fewer than ~35 of the 64 rows are open, i.e. past `ahead`
// columns.  The four wavefronts take the columns in turns of four; what is open at the end goes to the leftover list.
template <int QT>
__global__ void __launch_bounds__(256)
k_tfd_first_match_dense_u16(const double *__restrict__ tfT, const uint4 *__restrict__ tfU, int64_t N, int64_t Npad,
                            int Qrt, double thresh, int t_lo, int t_hi, int64_t *__restrict__ first_match,
                            int64_t ahead, unsigned long long *__restrict__ left_count,
                            int64_t *__restrict__ left_rows, int64_t *__restrict__ left_from) {
  const int Q = QT > 0 ? QT : Qrt;
  constexpr int ND = QT > 0 ? (QT >= 7 ? 4 : (QT + 1) / 2) : 4;
  if (left_count[kFmShards] != 0ull) return;  // (grid-uniform: angles the 16 bits cannot stand for)
  __shared__ unsigned best[64];               // column - i0 of the first match
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * 64, i = i0 + lane;
  const bool row = i < N;
  uint4 rw = tfU[row ? i : N - 1];
  rw = make_uint4(rw.x ^ 0x80008000u, rw.y ^ 0x80008000u, rw.z ^ 0x80008000u, rw.w ^ 0x80008000u);
  if (tid < 64) best[tid] = row ? kFmOpen : 0u;
  __syncthreads();
  const int64_t e = i0 + 64 + ahead < N ? i0 + 64 + ahead : N;  // columns [i0 + 1, e)
  const int e_rel = (int)(e - i0);
  unsigned mine = row ? kFmOpen : 0u;
  // (the columns of the next turn are requested before this turn's tests; the tests themselves without branches:
  // the rare pair of the undecided band is noted and looked at after the turn)
  uint4 cur[4], nxt[4];
  int64_t j0 = i0 + 1 + 4 * wv;
#pragma unroll
  for (int u = 0; u < 4; ++u) cur[u] = tfU[j0 + u < N ? j0 + u : N - 1];
  for (; j0 < e; j0 += 16) {
#pragma unroll
    for (int u = 0; u < 4; ++u) nxt[u] = tfU[j0 + 16 + u < N ? j0 + 16 + u : N - 1];
    const int jrel0 = (int)(j0 - i0);
    unsigned und = 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jrel = jrel0 + u;  // (uniform)
      const int s = (int)sad_u16x8<ND>(cur[u], rw);
      const bool valid = jrel > lane && jrel < e_rel;
      const unsigned cand = (valid && s < t_lo) ? (unsigned)jrel : kFmOpen;
      mine = mine < cand ? mine : cand;
      und |= (valid && s >= t_lo && s < t_hi) ? 1u << u : 0u;
    }
    if (__ballot(und != 0u) != 0ull) {
#pragma unroll 1
      for (int u = 0; u < 4; ++u)
        if (((und >> u) & 1u) && (unsigned)(jrel0 + u) < mine &&
            tfd_similar_exact(tfT + i, Npad, tfT + j0 + u, Npad, Q, thresh))
          mine = (unsigned)(jrel0 + u);
    }
    if (__ballot(mine == kFmOpen) == 0ull) break;  // every row has a match among this wavefront's columns
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
  }
  if (row && mine != kFmOpen) atomicMin(&best[lane], mine);
  __syncthreads();
  if (tid < 64) {  // (the first wavefront, whole)
    const bool open = row && best[tid] == kFmOpen;
    if (row) first_match[i] = open ? -1 : i0 + (int64_t)best[tid];
    const uint64_t lm = __ballot(open && e < N);
    if (lm != 0ull) {
      const int sh = (int)((blockIdx.x >> 3) & (kFmShards - 1));
      unsigned long long base = 0ull;
      if (tid == 0) base = atomicAdd(&left_count[sh], (unsigned long long)__popcll(lm));
      base = __shfl(base, 0);
      if ((lm >> tid) & 1ull) {
        const int64_t slot = (int64_t)sh * fm_shard_cap(N) + (int64_t)base + __popcll(lm & ((1ull << tid) - 1ull));
        left_rows[slot] = i;
        left_from[slot] = e;
      }
    }
  }
}

// Bounding boxes of the first (up to) eight angles over every window of 256 columns: wlo / whi[q * n_win + w]
// and, for the walk's per-row test, as packed 16-bit (centre, half width + 2) per angle: wbu[2 w], wbu[2 w + 1] -- the
// distance of a row's angle to the interval is then max(0, |a - c| - h) in the wrapping 16-bit arithmetic, five packed
// instructions per two angles (the float form with its three wrapped copies: forty), rounded so that it never
// exceeds the true one; a box of 359 degrees or more is the whole circle (h = 0x8000)
__global__ void __launch_bounds__(256)
k_tfd_window_bounds_f64(const double *__restrict__ tfT, int64_t N, int64_t Npad, int qf, int64_t n_win,
                        float *__restrict__ wlo, float *__restrict__ whi, uint4 *__restrict__ wbu) {
  __shared__ float slo[8][4], shi[8][4];
  __shared__ unsigned sc[8], sh[8];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int64_t w = blockIdx.x, j = w * 256 + tid;
  for (int q = 0; q < qf; ++q) {
    double lo = 1e30, hi = -1e30;
    if (j < N) lo = hi = tfT[(int64_t)q * Npad + j];
    for (int off = 32; off > 0; off >>= 1) {
      lo = fmin(lo, __shfl_xor(lo, off));
      hi = fmax(hi, __shfl_xor(hi, off));
    }
    // outward in fp32: the box must hold every column's fp64 angle
    if (lane == 0) slo[q][wv] = __double2float_rd(lo), shi[q][wv] = __double2float_ru(hi);
  }
  __syncthreads();
  if (tid < 8) {
    unsigned c = 0u, h = 0x8000u;  // (an angle the fingerprint does not have: every row is "inside")
    if (tid < qf) {
      const float lo = fminf(fminf(slo[tid][0], slo[tid][1]), fminf(slo[tid][2], slo[tid][3]));
      const float hi = fmaxf(fmaxf(shi[tid][0], shi[tid][1]), fmaxf(shi[tid][2], shi[tid][3]));
      wlo[(int64_t)tid * n_win + w] = lo;
      whi[(int64_t)tid * n_win + w] = hi;
      if (hi - lo < 359.f) {
        c = (unsigned)(long long)rint(0.5 * ((double)lo + (double)hi) * (65536.0 / 360.0)) & 0xffffu;
        h = (unsigned)ceil(0.5 * ((double)hi - (double)lo) * (65536.0 / 360.0)) + 2u;
      }
    }
    sc[tid] = c;
    sh[tid] = h;
  }
  __syncthreads();
  if (tid == 0 && wbu != nullptr) {
    wbu[2 * w] = make_uint4(sc[0] | (sc[1] << 16), sc[2] | (sc[3] << 16), sc[4] | (sc[5] << 16), sc[6] | (sc[7] << 16));
    wbu[2 * w + 1] = make_uint4(sh[0] | (sh[1] << 16), sh[2] | (sh[3] << 16), sh[4] | (sh[5] << 16), sh[6] | (sh[7] << 16));
  }
}

typedef short fc_s2 __attribute__((ext_vector_type(2)));
// sum over two angles of max(0, |a - c| - h), 16-bit wrapping distance, saturating
__device__ __forceinline__ fc_us2 box_gap_u16x2(unsigned a, unsigned c, unsigned h, fc_us2 acc) {
  const fc_s2 d = __builtin_bit_cast(fc_s2, a) - __builtin_bit_cast(fc_s2, c);
  const fc_s2 ad = __builtin_elementwise_max(d, (fc_s2)(0) - d);  // (|-32768| stays 0x8000: half the circle, unsigned)
  const fc_us2 g = __builtin_elementwise_sub_sat(__builtin_bit_cast(fc_us2, ad), __builtin_bit_cast(fc_us2, h));
  return __builtin_elementwise_add_sat(acc, g);
}

// distance of the intervals [alo, ahi] and [blo, bhi] on the circle of 360 (a lower bound of the reference's delta
// between any member of one and any member of the other, for angles within [-270, 270])
__device__ __forceinline__ float interval_gap_360(float alo, float ahi, float blo, float bhi) {
  const float d0 = fmaxf(fmaxf(blo - ahi, alo - bhi), 0.f);
  const float d1 = fmaxf(fmaxf(blo - (ahi + 360.f), (alo + 360.f) - bhi), 0.f);
  const float d2 = fmaxf(fmaxf(blo - (ahi - 360.f), (alo - 360.f) - bhi), 0.f);
  return fminf(d0, fminf(d1, d2));
}

#if defined(FC_TFD_STAMPS)
// tuning build: ticks (s_memtime, 100 MHz) per phase of the walk, summed over workgroups by thread 0 (tools/fm_stamps.py)
__device__ unsigned long long g_fm_stamps[16];
#define FC_FM_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define FC_FM_ADD(k, v) do { if (threadIdx.x == 0) atomicAdd(&g_fm_stamps[k], (unsigned long long)(v)); } while (0)
#define FC_FM_MAX(k, v) do { if (threadIdx.x == 0) atomicMax(&g_fm_stamps[k], (unsigned long long)(v)); } while (0)
#define FC_FM_MIN(k, v) do { if (threadIdx.x == 0) atomicMin(&g_fm_stamps[k], (unsigned long long)(v)); } while (0)
#else
#define FC_FM_T(var) do { } while (0)
#define FC_FM_ADD(k, v) do { } while (0)
#define FC_FM_MAX(k, v) do { } while (0)
#define FC_FM_MIN(k, v) do { } while (0)
#endif

// Phase 2, the walk: the rows the dense phase left open, 64 per workgroup in list order, against ALL later columns,
// window by window of 256 columns IN ORDER -- a row retires at its first window with a match (the chunked
// k_tfd_first_match_rest cannot stop: at 1.7 M structures it looked at 19 x the (row, window) pairs an ordered walk
// needs, `tools/fm_probe.py`).  Windows are skipped by the bounding boxes of their angles twice: against the box of the
// workgroup's rows (256 windows per step, one per thread), then per row.  In a systematic scan the angles vary like
// the digits of a counter, so a window holds few values of the slow ones and most windows are far from a given row.
// The windows that remain are taken FOUR at a time, one per wavefront (four columns per lane): a visit is one load
// latency and two barriers whatever it tests, and a workgroup with a row that matches nowhere makes a hundred of
// them -- one after the other they were the kernel (tools/fm_stamps.py).  A row that retires in the first window of
// such a turn is still tested in the other three; the first match is the minimum either way.
template <int QT>
__global__ void __launch_bounds__(256)
k_tfd_first_match_walk_u16(const double *__restrict__ tfT, const uint4 *__restrict__ tfU, int64_t N, int64_t Npad,
                           int Qrt, double thresh, int t_lo, int t_hi, const FmShards sh,
                           const int64_t *__restrict__ left_rows, const int64_t *__restrict__ left_from,
                           const float *__restrict__ wlo, const float *__restrict__ whi,
                           const uint4 *__restrict__ wbu, int64_t n_win, int64_t *__restrict__ first_match) {
  const int Q = QT > 0 ? QT : Qrt;
  constexpr int ND = QT > 0 ? (QT >= 7 ? 4 : (QT + 1) / 2) : 4;
  constexpr int QB = 8, WIN = 256, WSH = 8;
  extern __shared__ double rows[];  // [64][Q]
  __shared__ uint4 rowsU[64];
  __shared__ float rowsF[64][QB];
  __shared__ long long row_i[64], row_from[64];
  __shared__ unsigned long long lbest[64];  // first matching column so far, ~0: none
  __shared__ float glo[QB], ghi[QB];
  __shared__ long long from_min_s;
  __shared__ int cand[256], act[256];
  __shared__ uint4 cbox[256][2];  // the candidate windows' boxes in 16 bits: centres, half widths
  __shared__ unsigned long long wmask[256];
  __shared__ int wave_n[4];
  __shared__ unsigned long long alive_s;
  const int qb = QT > 0 ? (QT < QB ? QT : QB) : (Q < QB ? Q : QB);
  const float lim = (float)thresh + 0.03f;  // (fp32 roundings of the boxes and of the wrapped copies: far below)
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int shard = 0;
  while (shard + 1 < kFmShards && blockIdx.x >= sh.wg_begin[shard + 1]) ++shard;
  const unsigned long long g0 = (unsigned long long)(blockIdx.x - sh.wg_begin[shard]) * 64ull, n_left = sh.count[shard];
  left_rows += (int64_t)shard * fm_shard_cap(N);
  left_from += (int64_t)shard * fm_shard_cap(N);
  FC_FM_T(st0);
  if (tid < 64) {
    const bool on = g0 + tid < n_left;
    const long long ri = on ? left_rows[g0 + tid] : -1;
    const long long from = on ? left_from[g0 + tid] : (long long)N;
    row_i[tid] = ri;
    row_from[tid] = from;
    lbest[tid] = ~0ull;
    const uint4 a = tfU[on ? ri : 0];
    rowsU[tid] = make_uint4(a.x ^ 0x80008000u, a.y ^ 0x80008000u, a.z ^ 0x80008000u, a.w ^ 0x80008000u);
    long long fm_ = from;
    for (int off = 32; off > 0; off >>= 1) {
      const long long o = __shfl_xor(fm_, off);
      fm_ = o < fm_ ? o : fm_;
    }
    const unsigned long long al = __ballot(on && from < (long long)N);
    if (tid == 0) from_min_s = fm_, alive_s = al;
  }
  __syncthreads();
  for (int k = tid; k < 64 * Q; k += 256) {
    const int r = k / Q, q = k % Q;
    const double v = row_i[r] >= 0 ? tfT[(int64_t)q * Npad + row_i[r]] : 0.0;
    rows[k] = v;
    if (q < QB) rowsF[r][q] = (float)v;
  }
  __syncthreads();
  if (tid < 64) {  // the box of the workgroup's rows
    const bool on = row_i[tid] >= 0;
    for (int q = 0; q < qb; ++q) {
      float lo = on ? rowsF[tid][q] : 1e30f, hi = on ? rowsF[tid][q] : -1e30f;
      for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
      }
      if (tid == 0) glo[q] = lo - 1e-3f, ghi[q] = hi + 1e-3f;  // ((float) of the fp64 angle: within 2e-5 of it)
    }
  }
  __syncthreads();
  unsigned long long alive = alive_s;
  FC_FM_T(st1);
  FC_FM_ADD(0, 1);
  FC_FM_ADD(1, st1 - st0);
  uint4 my_u = rowsU[lane];  // (lane = row in step (2))
  my_u = make_uint4(my_u.x ^ 0x80008000u, my_u.y ^ 0x80008000u, my_u.z ^ 0x80008000u, my_u.w ^ 0x80008000u);
  const long long my_from = row_from[lane];
  for (int64_t wb = from_min_s >> WSH; wb < n_win && alive != 0ull; wb += 256) {
    // (1) the windows of this step the workgroup's box comes near, compacted in order, their boxes kept in LDS
    // (the loads of a window's sixteen numbers are issued together: one after the other, per angle and again per
    // candidate and row, they were most of this kernel's time)
    FC_FM_T(sa);
    const int64_t w = wb + tid;
    float wl[QB], wh[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const bool have = q < qb && w < n_win;
      wl[q] = have ? wlo[(int64_t)q * n_win + w] : 0.f;
      wh[q] = have ? whi[(int64_t)q * n_win + w] : 0.f;
    }
    const uint4 wc_u = wbu[2 * (w < n_win ? w : n_win - 1)], wh_u = wbu[2 * (w < n_win ? w : n_win - 1) + 1];
    bool near = false;
    if (w < n_win) {
      float lb = 0.f;
#pragma unroll
      for (int q = 0; q < QB; ++q)
        if (q < qb) lb += interval_gap_360(glo[q], ghi[q], wl[q], wh[q]);
      near = lb < lim;
    }
    uint64_t nb = __ballot(near);
    if (lane == 0) wave_n[wv] = __popcll(nb);
    __syncthreads();
    int base = 0, nc = 0;
    for (int v = 0; v < 4; ++v) {
      if (v < wv) base += wave_n[v];
      nc += wave_n[v];
    }
    if (near) {
      const int at = base + __popcll(nb & ((1ull << lane) - 1ull));
      cand[at] = (int)(w - wb);
      cbox[at][0] = wc_u;
      cbox[at][1] = wh_u;
    }
    __syncthreads();
    FC_FM_T(sb);
    FC_FM_ADD(2, sb - sa);
    FC_FM_ADD(5, 1);
    FC_FM_ADD(6, nc);
    // (2) per candidate window: the rows that come near it (lane = row)
    for (int c = wv; c < nc; c += 4) {
      const int64_t wc = wb + cand[c];
      const int64_t w_end = (wc + 1) * WIN < N ? (wc + 1) * WIN : N;
      // (a lower bound, in 16-bit units, of the TFD of the row to any column of the window: see k_tfd_window_bounds_f64)
      const uint4 bc = cbox[c][0], bh = cbox[c][1];
      fc_us2 acc = box_gap_u16x2(my_u.x, bc.x, bh.x, (fc_us2)(0));
      acc = box_gap_u16x2(my_u.y, bc.y, bh.y, acc);
      acc = box_gap_u16x2(my_u.z, bc.z, bh.z, acc);
      acc = box_gap_u16x2(my_u.w, bc.w, bh.w, acc);
      const int lbu = (int)acc.x + (int)acc.y;
      const uint64_t m = __ballot(my_from < (long long)w_end && lbu < t_hi);
      if (lane == 0) wmask[c] = m;
    }
    __syncthreads();
    // ... and of those the ones that have a row (a few of two hundred), compacted in order: act
    {
      const bool has = tid < nc && (wmask[tid] & alive) != 0ull;
      nb = __ballot(has);
      if (lane == 0) wave_n[wv] = __popcll(nb);
      __syncthreads();
      int abase = 0;
      for (int v = 0; v < wv; ++v) abase += wave_n[v];
      if (has) act[abase + __popcll(nb & ((1ull << lane) - 1ull))] = tid;
    }
    __syncthreads();
    const int na = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    FC_FM_T(sc);
    FC_FM_ADD(3, sc - sb);
    // (3) the windows with rows, four per turn
    for (int a0 = 0; a0 < na; a0 += 4) {
      const int c = a0 + wv < na ? act[a0 + wv] : -1;  // (wave-uniform)
      unsigned long long m = c >= 0 ? (wmask[c] & alive) : 0ull;
      if (m != 0ull) {
        FC_FM_ADD(7, 1);
        const int64_t jb = (wb + cand[c]) * WIN;
        uint4 cu[4];
        int jrel[4];  // column - jb, -1: none
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t j = jb + u * 64 + lane;
          const bool on = j < N;
          cu[u] = tfU[on ? j : N - 1];
          jrel[u] = on ? u * 64 + lane : -1;
        }
        while (m) {
          const int r = __builtin_ctzll(m);
          m &= m - 1ull;
          // (columns before the row's `from` were looked at by the dense phase)
          const long long fr = row_from[r] - jb - 1;
          const int fr_rel = fr < -1 ? -1 : (int)fr;
          const uint4 rw = rowsU[r];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            bool hit = false;
            if (jrel[u] > fr_rel) {
              const int s = (int)sad_u16x8<ND>(cu[u], rw);
              hit = s < t_lo || (s < t_hi && tfd_similar_exact(rows + r * Q, 1, tfT + jb + jrel[u], Npad, Q, thresh));
            }
            const uint64_t b = __ballot(hit);  // columns increase with u, then with the lane: the first hit is the lowest
            if (b != 0ull) {
              if (lane == __builtin_ctzll(b)) atomicMin(&lbest[r], (unsigned long long)(jb + jrel[u]));
              break;  // (uniform)
            }
          }
        }
      }
      __syncthreads();
      if (tid < 64) {
        const unsigned long long al = __ballot(lbest[tid] == ~0ull) & alive;
        if (tid == 0) alive_s = al;
      }
      __syncthreads();
      alive = alive_s;
      if (alive == 0ull) break;
    }
    __syncthreads();  // (cand / wmask / act are rewritten by the next step)
    FC_FM_T(sd);
    FC_FM_ADD(4, sd - sc);
  }
  if (tid < 64 && row_i[tid] >= 0) first_match[row_i[tid]] = lbest[tid] == ~0ull ? -1 : (int64_t)lbest[tid];
  FC_FM_T(se);
  FC_FM_ADD(9, se - st0);
  FC_FM_MAX(8, se - st0);
  FC_FM_MIN(11, st0);
  FC_FM_MAX(12, se);
}

// ---------------------------------------------------------------------------
// Sequential "is_new_structure" filter of string_embed (embeds.py:59-84): a pose
// that passed the clash test is kept iff its fingerprint is not TFD-similar to
// any fingerprint KEPT so far (the cache is never trimmed).  Exact, chunked:
// for the next 256 poses (in order) (1) every pose is compared with all
// fingerprints kept before the chunk -- one workgroup per pose, lanes stride
// the kept list; (2) one wavefront walks the chunk in order and compares each
// still-alive pose with the ones kept inside the chunk.  accT: kept fingerprints,
// fingerprint-major with stride cap.  n_acc: device counter.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_leader_vs_kept(const double *__restrict__ tf, int Q, int64_t chunk0, int64_t P,
                 const uint8_t *__restrict__ pass, const double *__restrict__ accT, int64_t cap,
                 const unsigned long long *__restrict__ n_acc, double thresh,
                 uint8_t *__restrict__ rejected) {
  __shared__ int found;
  const int64_t p = chunk0 + blockIdx.x;
  if (p >= P) return;
  if (threadIdx.x == 0) found = 0;
  __syncthreads();
  if (!pass[p]) return;
  const int64_t n = (int64_t)*n_acc;
  const double *ti = tf + p * Q;
  for (int64_t j0 = 0; j0 < n; j0 += 256) {
    const int64_t j = j0 + threadIdx.x;
    if (j < n && tfd_sum(ti, 1, accT + j, cap, Q) < thresh) found = 1;
    __syncthreads();
    const int stop = found;  // every thread reads the flag of THIS trip ...
    __syncthreads();         // ... before any thread of the next trip may set it: the break is workgroup-uniform
    if (stop) break;
  }
  if (threadIdx.x == 0) rejected[blockIdx.x] = (uint8_t)found;
}

__global__ void __launch_bounds__(64)
k_leader_within_chunk(const double *__restrict__ tf, int Q, int64_t chunk0, int64_t P,
                      const uint8_t *__restrict__ pass, const uint8_t *__restrict__ rejected,
                      double *__restrict__ accT, int64_t cap, unsigned long long *__restrict__ n_acc,
                      double thresh, uint8_t *__restrict__ accept) {
  __shared__ int kept[256];
  const int lane = threadIdx.x;
  int n_kept = 0;
  unsigned long long base = *n_acc;
  const int64_t n_in = (P - chunk0 < 256) ? (P - chunk0) : 256;
  for (int c = 0; c < (int)n_in; ++c) {
    const int64_t p = chunk0 + c;
    bool ok = pass[p] && !rejected[c];  // wave-uniform
    if (ok) {
      bool hit = false;
      for (int k0 = 0; k0 < n_kept; k0 += 64) {
        const int k = k0 + lane;
        if (k < n_kept && tfd_sum(tf + p * Q, 1, tf + (chunk0 + kept[k]) * Q, 1, Q) < thresh) hit = true;
      }
      ok = !__any(hit);
    }
    if (ok) {
      if (lane == 0) kept[n_kept] = c;
      for (int q = lane; q < Q; q += 64) accT[(int64_t)q * cap + (int64_t)(base + n_kept)] = tf[p * Q + q];
      ++n_kept;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);
    }
    if (lane == 0) accept[p] = ok ? 1 : 0;
  }
  if (lane == 0) *n_acc = base + (unsigned long long)n_kept;
}

int launch_leader_chunk(const double *tf_dev, int64_t Q, int64_t chunk0, int64_t P, const uint8_t *pass_dev,
                        double *accT_dev, int64_t cap, unsigned long long *n_acc_dev, double thresh,
                        uint8_t *rejected_dev, uint8_t *accept_dev) {
  const int64_t n_in = (P - chunk0 < 256) ? (P - chunk0) : 256;
  if (n_in <= 0) return FC_OK;
  hipLaunchKernelGGL(k_leader_vs_kept, dim3((unsigned)n_in), dim3(256), 0, ctx().stream, tf_dev, (int)Q, chunk0,
                     P, pass_dev, accT_dev, cap, n_acc_dev, thresh, rejected_dev);
  FC_TRY(check_launch("k_leader_vs_kept"));
  hipLaunchKernelGGL(k_leader_within_chunk, dim3(1), dim3(64), 0, ctx().stream, tf_dev, (int)Q, chunk0, P,
                     pass_dev, rejected_dev, accT_dev, cap, n_acc_dev, thresh, accept_dev);
  return check_launch("k_leader_within_chunk");
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_pack_mask(const uint8_t *mask_dev, int64_t N, uint64_t *mbits_dev, int64_t W,
                     unsigned long long *counters_dev) {
  hipLaunchKernelGGL(k_pack_mask, dim3((unsigned)ceil_div(W, 4)), dim3(256), 0, ctx().stream,
                     mask_dev, N, mbits_dev, W, counters_dev);
  return check_launch("k_pack_mask");
}

int launch_level(const uint64_t *bits_dev, int64_t W, const uint64_t *mbits_dev,
                 const uint8_t *mask_in, uint8_t *mask_out, int64_t N, int64_t k, int64_t IB,
                 int64_t rank, int64_t world, int64_t rows_local) {
  if (rows_local == 0) return FC_OK;
  hipLaunchKernelGGL(k_level, dim3((unsigned)ceil_div(rows_local, 4)), dim3(256), 0, ctx().stream,
                     bits_dev, W, mbits_dev, mask_in, mask_out, N, k, (int)IB, rank, world,
                     rows_local);
  return check_launch("k_level");
}

int launch_mask_init(uint64_t *mb_dev, int64_t N, int64_t W, int64_t total_words) {
  hipLaunchKernelGGL(k_mask_init, dim3((unsigned)ceil_div(total_words, 256)), dim3(256), 0, ctx().stream,
                     mb_dev, N, W, total_words);
  return check_launch("k_mask_init");
}

int launch_level_fused(const uint64_t *bits_dev, int64_t W, const uint64_t *mb_in, uint64_t *mb_out,
                       int64_t N, int64_t k, int64_t min_per_group, unsigned long long *counters) {
  hipLaunchKernelGGL(k_level_fused, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, ctx().stream,
                     bits_dev, W, mb_in, mb_out, N, k, min_per_group, counters);
  return check_launch("k_level_fused");
}

// fc_prune_conventions: "a structure is removed at the first LATER similar one" (0, default) or the
// mirror rule (1); only the pair ladder implements the mirror rule
static int g_drop_later = 0;
void prune_conventions_set(int drop_later) { g_drop_later = drop_later ? 1 : 0; }
int prune_drop_later() { return g_drop_later; }

// ---------------------------------------------------------------------------
// The same ladder for LONG pair lists, on the whole chip (round 4).  k_ladder_pairs is ONE workgroup streaming every
// level's bucket: 7.6e5 similar pairs (the ensemble without clusters of the bench's `secondary` block) are ~3 M pair
// visits = 24 MB through one CU: 0.38 ms, with k_pair_buckets' 0.10 ms (one wave-wide atomic per 64 pairs on each
// level's counter: 1.2e4 per counter, serialised at the L2) most of the lane's time per prune.  Here a level is a
// launch: every workgroup takes the current mask into LDS, walks its share of the level's pairs with LDS atomics on a
// private copy of the next mask and ANDs that copy into the global one; the LAST workgroup to finish (a ticket) flips
// the current / next roles and resets the old current mask to all-ones -- what the next level ANDs into.  Whether a level
// runs (min_per_group * k < active) every workgroup decides for itself from the same current mask.  State: counters[32]
// = which of the two mask buffers is current, [33] = tickets, [8] = levels run.  Levels that cannot run at this N are
// not launched.  Chosen on the host from the last similar-pair count seen for these coordinates (a launch per level costs
// a short list more than the one-workgroup walk).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool ladder_declined(const unsigned long long *n_pairs_ptr, const unsigned long long *n_cand_ptr,
                                                unsigned long long cand_cap, unsigned long long cap,
                                                const unsigned long long *counters) {
  return (n_cand_ptr != nullptr && *n_cand_ptr > cand_cap) || *n_pairs_ptr > cap || counters[12] != 0ull;
}

__global__ void __launch_bounds__(256)
k_ladder_many_init(uint64_t *__restrict__ buf_a, uint64_t *__restrict__ buf_b, int64_t N, int64_t W,
                   unsigned long long *__restrict__ counters) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w < W) {
    const int64_t lo = w * 64;
    buf_a[w] = (lo + 64 <= N) ? ~0ull : ((lo < N) ? ((1ull << (N - lo)) - 1ull) : 0ull);
    buf_b[w] = ~0ull;
  }
  if (w == 0) counters[32] = 0ull, counters[33] = 0ull, counters[8] = 0ull;
}

constexpr int kLadderManyThreads = 1024;
__global__ void __launch_bounds__(kLadderManyThreads)
k_ladder_many_level(const uint64_t *__restrict__ src, const unsigned long long *__restrict__ n_src_ptr, int64_t k, int64_t N,
                    int64_t W, int64_t min_per_group, uint64_t *__restrict__ buf_a, uint64_t *__restrict__ buf_b,
                    unsigned long long *__restrict__ counters, int drop_later, const unsigned long long *__restrict__ n_pairs_ptr,
                    const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap, unsigned long long cap) {
  extern __shared__ unsigned long long lm[];  // cur[W] | nxt[W]
  __shared__ int s_count;
  __shared__ unsigned s_last;
  if (ladder_declined(n_pairs_ptr, n_cand_ptr, cand_cap, cap, counters)) return;
  const int tid = threadIdx.x;
  const unsigned long long which = counters[32];
  uint64_t *__restrict__ cur_g = which ? buf_b : buf_a, *__restrict__ nxt_g = which ? buf_a : buf_b;
  unsigned long long *cur = lm, *nxt = lm + W;
  if (tid == 0) s_count = 0;
  __syncthreads();
  int c = 0;
  for (int64_t w = tid; w < W; w += kLadderManyThreads) {
    const unsigned long long v = cur_g[w];
    cur[w] = v;
    nxt[w] = ~0ull;
    c += __popcll(v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((tid & 63) == 0 && c) atomicAdd(&s_count, c);
  __syncthreads();
  if (!((k == 1) || (min_per_group * k < (int64_t)s_count))) return;  // the same decision in every workgroup
  const unsigned long long n_src = *n_src_ptr;
  const uint32_t n32 = (uint32_t)N;
  for (unsigned long long p = (unsigned long long)blockIdx.x * kLadderManyThreads + tid; p < n_src; p += (unsigned long long)gridDim.x * kLadderManyThreads) {
    const uint64_t e = src[p];
    const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
    if (j > i && j < n32 && ((cur[i >> 6] >> (i & 63)) & 1ull) && ((cur[j >> 6] >> (j & 63)) & 1ull)) {
      const uint32_t kill = drop_later ? j : i;
      atomicAnd(&nxt[kill >> 6], ~(1ull << (kill & 63)));
    }
  }
  __syncthreads();
  for (int64_t w = tid; w < W; w += kLadderManyThreads) {
    const unsigned long long v = blockIdx.x == 0 ? (nxt[w] & cur[w]) : nxt[w];  // (workgroup 0 carries the current mask over)
    if (v != ~0ull) atomicAnd(reinterpret_cast<unsigned long long *>(&nxt_g[w]), v);
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(&counters[33], 1ull) == (unsigned long long)gridDim.x - 1ull ? 1u : 0u;
  __syncthreads();
  if (s_last) {  // everyone else has read the current mask and added its part: swap the roles
    for (int64_t w = tid; w < W; w += kLadderManyThreads) cur_g[w] = ~0ull;
    if (tid == 0) {
      counters[32] = 1ull - which;
      counters[33] = 0ull;
      counters[8] += 1ull;
    }
  }
}

__global__ void __launch_bounds__(256)
k_ladder_many_finish(const uint64_t *__restrict__ buf_a, const uint64_t *__restrict__ buf_b, int64_t W,
                     uint64_t *__restrict__ mask_out, unsigned long long *__restrict__ counters,
                     const unsigned long long *__restrict__ n_pairs_ptr, const unsigned long long *__restrict__ n_cand_ptr,
                     unsigned long long cand_cap, unsigned long long cap) {
  const int tid = threadIdx.x;
  const bool declined = ladder_declined(n_pairs_ptr, n_cand_ptr, cand_cap, cap, counters);
  if (!declined) {
    const uint64_t *__restrict__ cur = counters[32] ? buf_b : buf_a;
    for (int64_t w = tid; w < W; w += 256) mask_out[w] = cur[w];
  }
  __syncthreads();
  if (tid == 0) counters[9] = declined ? 0ull : 1ull;
  if (tid < 16) mask_out[W + tid] = tid == 9 ? (declined ? 0ull : 1ull) : counters[tid];  // ([8] = levels run, kept by the levels)
}

// k_pair_buckets for long lists: the slots of a level are reserved once per WORKGROUP of sixteen wavefronts (the
// one-atomic-per-wavefront form serialises 1.2e4 atomics per level counter at 7.6e5 pairs: 0.10 ms)
__global__ void __launch_bounds__(1024)
k_pair_buckets_many(const uint64_t *__restrict__ pairs, const unsigned long long *__restrict__ n_pairs_ptr,
                    unsigned long long cap, int64_t N, const int64_t *__restrict__ ladder, int n_ladder,
                    uint64_t *__restrict__ buckets, unsigned long long *__restrict__ level_cnt,
                    const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap) {
  __shared__ unsigned s_wcnt[16][32];
  __shared__ unsigned long long s_base[32];
  const unsigned long long P = *n_pairs_ptr;
  if (P > cap) return;
  if (n_cand_ptr != nullptr && *n_cand_ptr > cand_cap) return;
  const uint32_t n32 = (uint32_t)N;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long stride = (unsigned long long)gridDim.x * 1024ull;
  for (unsigned long long base = (unsigned long long)blockIdx.x * 1024ull; base < P; base += stride) {  // block-uniform
    const unsigned long long p = base + tid;
    const uint64_t e = p < P ? pairs[p] : ~0ull;
    const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
    const bool valid = j > i && j < n32;
    uint32_t mine = 0;
    for (int l = 0; l < n_ladder; ++l) {
      const uint32_t k = (uint32_t)ladder[l];
      bool same = false;
      if (k != 1u) {
        const uint32_t chunk = n32 / k;
        if (valid && chunk != 0) {
          uint32_t ci = i / chunk, cj = j / chunk;
          if (ci > k - 1) ci = k - 1;
          if (cj > k - 1) cj = k - 1;
          same = ci == cj;
        }
      }
      if (same) mine |= 1u << l;
      const unsigned c = (unsigned)__popcll(__ballot(same));
      if (lane == l) s_wcnt[wv][l] = c;
    }
    __syncthreads();
    if (tid < n_ladder) {
      unsigned tot = 0;
      for (int w = 0; w < 16; ++w) tot += s_wcnt[w][tid];
      s_base[tid] = tot ? atomicAdd(&level_cnt[tid * kCntLevelStride], (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    for (int l = 0; l < n_ladder; ++l) {
      const bool same = (mine >> l) & 1u;
      const uint64_t m = __ballot(same);
      if (m == 0) continue;  // wave-uniform
      unsigned before = 0;
      for (int w = 0; w < wv; ++w) before += s_wcnt[w][l];
      if (same) buckets[(unsigned long long)l * cap + s_base[l] + before + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = e;
    }
    __syncthreads();  // (the counts are overwritten by the next round)
  }
}

// workgroups per level launch of the prunes (tuning knob FC_LADDER_MANY_GRID, read once per process)
unsigned ladder_many_grid() {
  static const unsigned many_grid = [] {
    const char *v = getenv("FC_LADDER_MANY_GRID");
    const long g = v ? std::strtol(v, nullptr, 10) : 16;  // (2 .. 256 measured at 7.6e5 pairs: 16-32 best; many workgroups pay in global atomics and tickets)
    return (unsigned)(g >= 1 && g <= kLadderManyGridMax ? g : 16);
  }();
  return many_grid;
}

// grid: workgroups per level launch, 1 .. kLadderManyGridMax (the caller's check)
int launch_ladder_pairs_many(const uint64_t *pairs_dev, uint64_t *buckets_dev, const unsigned long long *n_pairs_dev,
                             const unsigned long long *n_cand_dev, unsigned long long cand_cap, unsigned long long cap,
                             int64_t N, int64_t W, int64_t min_per_group, const int64_t *ladder_dev, const int64_t *ladder_host,
                             int n_ladder, uint64_t *mask_bufs_dev, uint64_t *mask_out_dev, unsigned long long *counters_dev,
                             unsigned grid) {
  hipStream_t st = ctx().stream;
  hipLaunchKernelGGL(k_pair_buckets_many, dim3((unsigned)ctx().n_cu), dim3(1024), 0, st, pairs_dev, n_pairs_dev, cap, N,
                     ladder_dev, n_ladder, buckets_dev, counters_dev + kCntLevel, n_cand_dev, cand_cap);
  FC_TRY(check_launch("k_pair_buckets_many"));
  uint64_t *buf_a = mask_bufs_dev, *buf_b = mask_bufs_dev + W;
  hipLaunchKernelGGL(k_ladder_many_init, dim3((unsigned)ceil_div(W, 256)), dim3(256), 0, st, buf_a, buf_b, N, W, counters_dev);
  FC_TRY(check_launch("k_ladder_many_init"));
  const size_t lds = (size_t)2 * W * sizeof(uint64_t);
  for (int l = 0; l < n_ladder; ++l) {
    const int64_t k = ladder_host[l];
    const uint64_t *src = k == 1 ? pairs_dev : buckets_dev + (unsigned long long)l * cap;
    const unsigned long long *n_src = k == 1 ? n_pairs_dev : counters_dev + kCntLevel + kCntLevelStride * l;
    hipLaunchKernelGGL(k_ladder_many_level, dim3(grid), dim3(kLadderManyThreads), lds, st, src, n_src, k, N, W, min_per_group,
                       buf_a, buf_b, counters_dev, g_drop_later, n_pairs_dev, n_cand_dev, cand_cap, cap);
    FC_TRY(check_launch("k_ladder_many_level"));
  }
  hipLaunchKernelGGL(k_ladder_many_finish, dim3(1), dim3(256), 0, st, buf_a, buf_b, W, mask_out_dev, counters_dev, n_pairs_dev,
                     n_cand_dev, cand_cap, cap);
  return check_launch("k_ladder_many_finish");
}

int launch_ladder_pairs(const uint64_t *pairs_dev, uint64_t *buckets_dev,
                        const unsigned long long *n_pairs_dev, const unsigned long long *n_cand_dev,
                        unsigned long long cand_cap, unsigned long long cap, int64_t N, int64_t W,
                        int64_t min_per_group, const int64_t *ladder_dev, int n_ladder,
                        uint64_t *mask_out_dev, unsigned long long *counters_dev) {
  // counters_dev[kCntLevel + kCntLevelStride * l] = bucket fill levels (zero on entry: the caller's reset)
  hipLaunchKernelGGL(k_pair_buckets, dim3((unsigned)(ctx().n_cu * 8)), dim3(256), 0, ctx().stream,
                     pairs_dev, n_pairs_dev, cap, N, ladder_dev, n_ladder, buckets_dev, counters_dev + kCntLevel, n_cand_dev,
                     cand_cap);
  FC_TRY(check_launch("k_pair_buckets"));
  const size_t lds = (size_t)2 * W * sizeof(uint64_t);
  hipLaunchKernelGGL(k_ladder_pairs, dim3(1), dim3(1024), lds, ctx().stream, pairs_dev, buckets_dev,
                     n_pairs_dev, n_cand_dev, cand_cap, cap, N, W, min_per_group, ladder_dev, n_ladder,
                     mask_out_dev, counters_dev, g_drop_later);
  return check_launch("k_ladder_pairs");
}

int launch_export_pairs(const uint64_t *simq_dev, const unsigned long long *counters_dev,
                        unsigned long long cand_cap, int64_t cap, uint64_t *out_dev) {
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(cap, 256), 64));
  hipLaunchKernelGGL(k_export_pairs, dim3(blocks), dim3(256), 0, ctx().stream, simq_dev, counters_dev,
                     cand_cap, cap, out_dev);
  return check_launch("k_export_pairs");
}

int launch_compact_gathered(const uint64_t *gathered_dev, int world, int64_t cap, uint64_t *list_dev,
                            unsigned long long *counters_dev) {
  hipLaunchKernelGGL(k_compact_gathered, dim3(1), dim3(1024), 0, ctx().stream, gathered_dev, world, cap,
                     list_dev, counters_dev);
  return check_launch("k_compact_gathered");
}

int launch_copy_bytes(const uint8_t *src, uint8_t *dst, int64_t n) {
  if (n == 0) return FC_OK;
  hipLaunchKernelGGL(k_copy_bytes, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx().stream,
                     src, dst, n);
  return check_launch("k_copy_bytes");
}

int launch_inertia_moments(const double *coords_dev, int64_t N, int64_t A, const double *masses_dev,
                           double *moments_dev) {
  if (N == 0) return FC_OK;
  hipLaunchKernelGGL(k_inertia_moments, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0,
                     ctx().stream, coords_dev, N, A, masses_dev, moments_dev);
  return check_launch("k_inertia_moments");
}

int launch_moi_simbits(const double *moments_dev, int64_t N, double tol, const double *energies_dev,
                       double max_dE, uint64_t *bits_dev, int64_t W) {
  if (N * W == 0) return FC_OK;
  // (N * 256 threads along x, W / 4 blocks along y: N < 2^24 and W <= 4 * 65535; a bit matrix of that size is 35 TB)
  if (N >= ((int64_t)1 << 24) || ceil_div(W, 4) > 65535)
    return set_error(FC_E_LIMIT, "N=%lld structures exceed the grid of the MOI similarity kernel", (long long)N);
  hipLaunchKernelGGL(k_moi_simbits, dim3((unsigned)N, (unsigned)ceil_div(W, 4)), dim3(256), 0, ctx().stream,
                     moments_dev, N, tol, energies_dev, max_dE, bits_dev, W);
  return check_launch("k_moi_simbits");
}

// (N, Q) row-major -> (Q, Npad) fingerprint-major, zero padded: thread n reads its Q contiguous values,
// the stores of a wavefront are coalesced per fingerprint
__global__ void __launch_bounds__(256)
k_transpose_pad(const double *__restrict__ in, int64_t N, int64_t Q, int64_t Npad, double *__restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= Npad) return;
  for (int64_t q = 0; q < Q; ++q) out[q * Npad + n] = n < N ? in[n * Q + q] : 0.0;
}

int launch_transpose_pad(const double *in_dev, int64_t N, int64_t Q, int64_t Npad, double *out_dev) {
  if (Npad == 0 || Q == 0) return FC_OK;
  hipLaunchKernelGGL(k_transpose_pad, dim3((unsigned)ceil_div(Npad, 256)), dim3(256), 0, ctx().stream, in_dev, N, Q,
                     Npad, out_dev);
  return check_launch("k_transpose_pad");
}

// the same with a row selection: out row 0 = `first` (Q values), out row 1 + k = in[idx[k]]; the rest zeros
// (fc_torsion_scan_tfd: the fingerprints of a scan stay on the device, the starting structure leads the list)
__global__ void __launch_bounds__(256)
k_gather_transpose_pad(const double *__restrict__ in, const double *__restrict__ first, const int64_t *__restrict__ idx,
                       int64_t M, int64_t Q, int64_t Npad, double *__restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= Npad) return;
  const double *__restrict__ row = n == 0 ? first : (n <= M ? in + idx[n - 1] * Q : nullptr);
  for (int64_t q = 0; q < Q; ++q) out[q * Npad + n] = row ? row[q] : 0.0;
}

int launch_gather_transpose_pad(const double *in_dev, const double *first_dev, const int64_t *idx_dev, int64_t M,
                                int64_t Q, int64_t Npad, double *out_dev) {
  if (Npad == 0 || Q == 0) return FC_OK;
  hipLaunchKernelGGL(k_gather_transpose_pad, dim3((unsigned)ceil_div(Npad, 256)), dim3(256), 0, ctx().stream, in_dev,
                     first_dev, idx_dev, M, Q, Npad, out_dev);
  return check_launch("k_gather_transpose_pad");
}

// fp32 copy of the first (up to) four fingerprint-major rows for the pre-filter of k_tfd_first_match
__global__ void __launch_bounds__(256)
k_tfd_prefilter_copy(const double *__restrict__ tfT, int64_t n, float *__restrict__ tfF) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) tfF[i] = (float)tfT[i];
}

// Which device form the last launch_tfd_first_match took (fc_tfd_last_form): bit 0 one-phase fp32, bit 1 fp32 look-ahead
// + column chunks, bit 2 16-bit dense phase, bit 3 16-bit walk launched, bit 4 the 16-bit path refused its angles and
// the fp32 kernels redid the array; and the rows still open after phase 1.  Host bookkeeping only.
static int g_tfd_last_form = 0;
static int64_t g_tfd_last_open = 0;
int tfd_last_form(int64_t *n_open_out) {
  if (n_open_out != nullptr) *n_open_out = g_tfd_last_open;
  return g_tfd_last_form;
}

// tfF_scratch: min(Q, 8) * Npad floats owned by the caller until the stream has run the kernel (nullptr, or
// FC_TFD_F32_COPY=0: the kernel reads the fp64 columns for its pre-filter as well)
int launch_tfd_first_match(const double *tfT_dev, int64_t N, int64_t Npad, int64_t Q, double thresh,
                           int64_t *fm_dev, float *tfF_scratch) {
  g_tfd_last_form = 0;
  g_tfd_last_open = 0;
  if (N == 0) return FC_OK;
  const dim3 grid((unsigned)ceil_div(N, 64)), block(256);
  const size_t lds = (size_t)64 * Q * sizeof(double);
  // (the conversion rounds each angle to fp32 exactly as the kernel's own (float) of the fp64 value does)
  const float *tfF_dev = nullptr;
  static const bool use_copy = [] {
    const char *v = getenv("FC_TFD_F32_COPY");
    return !(v && v[0] == '0');
  }();
  // two phases for long arrays: bounded look-ahead per row block, then the rows still open against column
  // chunks (FC_TFD_LOOKAHEAD: columns, 0 = one phase; needs the fp32 copy)
  // (measured at 1.7 M structures, whole call incl. the upload: one phase 59 ms; look-ahead 4 096: 11.7 ms,
  // 32 768: 15.8, 131 072: 16.3)
  int64_t lookahead_env = 4096;
  bool forced = false;
  if (const char *v = getenv("FC_TFD_LOOKAHEAD")) lookahead_env = (int64_t)std::strtoll(v, nullptr, 10), forced = true;  // (per call: test knob)
  const bool two_phase = tfF_scratch != nullptr && use_copy && lookahead_env > 0 && (forced ? N > 8 * lookahead_env : N >= 65536);
  const int64_t max_ahead = two_phase ? lookahead_env : 0;
  DevBuf left;  // [counts, flag | rows | from | best x N | boxes | 16-bit angles]: released to the pool at return
  unsigned long long *left_count = nullptr, *best_dev = nullptr;
  int64_t *left_rows = nullptr, *left_from = nullptr;
  const int64_t n_win = ceil_div(N, 1024);
  const int qf4 = (int)std::min<int64_t>(Q, 4);
  float *wlo = nullptr, *whi = nullptr;
  bool use_u16 = true;
  if (const char *v = getenv("FC_TFD_U16")) use_u16 = v[0] != '0';  // 0: the fp32 pre-filter kernels (per call: test knob)
  const bool u16 = two_phase && use_u16 && N < ((int64_t)1 << 31) - (1 << 20);
  constexpr int kHead = 32;  // counters (one, or kFmShards) and the flag of the 16-bit path
  const int64_t list_cap = u16 ? std::max<int64_t>(N, kFmShards * fm_shard_cap(N)) : N;
  const int64_t n_winw = ceil_div(N, 256);
  if (two_phase) {
    const size_t boxes = (size_t)(16 * n_winw + 32) * sizeof(float) + (size_t)(2 * n_winw + 2) * sizeof(uint4);  // (those of the 16-bit walk)
    FC_TRY(left.reserve((size_t)(2 * list_cap + N + kHead) * sizeof(int64_t) + boxes + (u16 ? (size_t)Npad * sizeof(uint4) + 16 : 0)));
    left_count = left.as<unsigned long long>();
    left_rows = reinterpret_cast<int64_t *>(left_count + kHead);
    left_from = left_rows + list_cap;
    best_dev = reinterpret_cast<unsigned long long *>(left_from + list_cap);
    wlo = reinterpret_cast<float *>(best_dev + N), whi = wlo + 4 * n_win;
    FC_HIP_TRY(hipMemsetAsync(left_count, 0, kHead * sizeof(unsigned long long), ctx().stream));
  }
  if (u16) {
    // 16-bit angles (see k_tfd_pack_u16): a dense phase right behind every block of rows, then ONE ordered walk per
    // 64 open rows over windows of 256 columns
    // (dense phase of 32 / 64 / 128 / 256 columns at 1.7 M structures: 0.33 + 1.03 / 0.35 + 0.96 / 0.39 + 0.92 /
    // 0.51 + 0.82 ms for the two kernels)
    const int64_t ahead = forced ? lookahead_env : 128;
    const int qf8 = (int)std::min<int64_t>(Q, 8);
    float *blo = wlo, *bhi = blo + 8 * n_winw;
    uint4 *wbu = reinterpret_cast<uint4 *>((reinterpret_cast<uintptr_t>(bhi + 8 * n_winw + 16) + 15) & ~(uintptr_t)15);
    uint4 *tfU = wbu + 2 * n_winw;
    hipLaunchKernelGGL(k_tfd_pack_u16, dim3((unsigned)ceil_div(Npad, 256)), block, 0, ctx().stream, tfT_dev, N, Npad, (int)Q,
                       tfU, left_count);
    FC_TRY(check_launch("k_tfd_pack_u16"));
    hipLaunchKernelGGL(k_tfd_window_bounds_f64, dim3((unsigned)n_winw), block, 0, ctx().stream, tfT_dev, N, Npad, qf8, n_winw,
                       blo, bhi, wbu);
    FC_TRY(check_launch("k_tfd_window_bounds_f64"));
    // thresholds in 16-bit units (the bounds are derived at k_tfd_pack_u16)
    int t_lo = 0, t_hi = 0;
    if (thresh > 0.0) {
      const double ts = std::min(thresh * (65536.0 / 360.0), 300000.0);
      t_hi = (int)std::ceil(ts) + 10;
      t_lo = Q <= 8 ? std::max(0, (int)std::floor(ts) - 10) : 0;
    }
#define FC_FMU(QT)                                                                                                   \
  case QT:                                                                                                           \
    hipLaunchKernelGGL(k_tfd_first_match_dense_u16<QT>, grid, block, 0, ctx().stream, tfT_dev, tfU, N, Npad, (int)Q, \
                       thresh, t_lo, t_hi, fm_dev, ahead, left_count, left_rows, left_from);                         \
    break;
    switch (Q) {
      FC_FMU(1) FC_FMU(2) FC_FMU(3) FC_FMU(4) FC_FMU(5) FC_FMU(6) FC_FMU(7) FC_FMU(8)
      default:
        hipLaunchKernelGGL(k_tfd_first_match_dense_u16<0>, grid, block, 0, ctx().stream, tfT_dev, tfU, N, Npad, (int)Q,
                           thresh, t_lo, t_hi, fm_dev, ahead, left_count, left_rows, left_from);
    }
#undef FC_FMU
    FC_TRY(check_launch("k_tfd_first_match_dense_u16"));
    unsigned long long head[kFmShards + 1] = {0};
    FC_TRY(d2h(head, left_count, sizeof head));
    FC_TRY(sync());
    FmShards sh;
    unsigned long long n_left = 0;
    sh.wg_begin[0] = 0;
    for (int k = 0; k < kFmShards; ++k) {
      sh.count[k] = (unsigned)head[k];
      sh.wg_begin[k + 1] = sh.wg_begin[k] + (unsigned)ceil_div((int64_t)head[k], 64);
      n_left += head[k];
    }
    if (getenv("FC_DEBUG"))
      fprintf(stderr, "[fc] tfd first match (16-bit angles%s): %llu of %lld rows open after the dense phase of %lld columns\n",
              head[kFmShards] ? ": REFUSED, angles beyond +-270 or not finite" : "", n_left, (long long)N, (long long)ahead);
    if (head[kFmShards] == 0ull) {
      g_tfd_last_form = 4;
      g_tfd_last_open = (int64_t)n_left;
      if (n_left == 0) return FC_OK;
      g_tfd_last_form |= 8;
      const dim3 rgrid(sh.wg_begin[kFmShards]);
#define FC_FMW(QT)                                                                                                      \
  case QT:                                                                                                              \
    hipLaunchKernelGGL(k_tfd_first_match_walk_u16<QT>, rgrid, block, lds, ctx().stream, tfT_dev, tfU, N, Npad, (int)Q,  \
                       thresh, t_lo, t_hi, sh, left_rows, left_from, blo, bhi, wbu, n_winw, fm_dev);                         \
    break;
      switch (Q) {
        FC_FMW(1) FC_FMW(2) FC_FMW(3) FC_FMW(4) FC_FMW(5) FC_FMW(6) FC_FMW(7) FC_FMW(8)
        default:
          hipLaunchKernelGGL(k_tfd_first_match_walk_u16<0>, rgrid, block, lds, ctx().stream, tfT_dev, tfU, N, Npad, (int)Q,
                             thresh, t_lo, t_hi, sh, left_rows, left_from, blo, bhi, wbu, n_winw, fm_dev);
      }
#undef FC_FMW
      return check_launch("k_tfd_first_match_walk_u16");
    }
    // refused: the fp32 kernels below redo the whole array
    g_tfd_last_form = 16;
    FC_HIP_TRY(hipMemsetAsync(left_count, 0, kHead * sizeof(unsigned long long), ctx().stream));
  }
  if (use_copy && tfF_scratch != nullptr) {
    const int64_t n = std::min<int64_t>(Q, 8) * Npad;
    hipLaunchKernelGGL(k_tfd_prefilter_copy, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx().stream, tfT_dev, n,
                       tfF_scratch);
    FC_TRY(check_launch("k_tfd_prefilter_copy"));
    tfF_dev = tfF_scratch;
  }
#define FC_FM(QT)                                                                                  \
  case QT:                                                                                         \
    hipLaunchKernelGGL(k_tfd_first_match<QT>, grid, block, lds, ctx().stream, tfT_dev, N, Npad,    \
                       (int)Q, thresh, fm_dev, tfF_dev, max_ahead, left_count, left_rows, left_from); \
    break;
  switch (Q) {
    FC_FM(1) FC_FM(2) FC_FM(3) FC_FM(4) FC_FM(5) FC_FM(6) FC_FM(7) FC_FM(8) FC_FM(9) FC_FM(10)
    FC_FM(11) FC_FM(12) FC_FM(13) FC_FM(14) FC_FM(15) FC_FM(16)
    default:
      hipLaunchKernelGGL(k_tfd_first_match<0>, grid, block, lds, ctx().stream, tfT_dev, N, Npad, (int)Q,
                         thresh, fm_dev, tfF_dev, max_ahead, left_count, left_rows, left_from);
  }
#undef FC_FM
  FC_TRY(check_launch("k_tfd_first_match"));
  g_tfd_last_form |= two_phase ? 2 : 1;
  if (!two_phase) return FC_OK;
  unsigned long long n_left = 0;
  FC_TRY(d2h(&n_left, left_count, sizeof n_left));
  FC_TRY(sync());
  g_tfd_last_open = (int64_t)n_left;
  if (getenv("FC_DEBUG")) fprintf(stderr, "[fc] tfd first match: %llu of %lld rows open after a look-ahead of %lld columns\n", n_left, (long long)N, (long long)max_ahead);
  if (n_left == 0) return FC_OK;
  FC_HIP_TRY(hipMemsetAsync(best_dev, 0xff, (size_t)n_left * sizeof(unsigned long long), ctx().stream));
  const int64_t chunk = 65536;
  const dim3 rgrid((unsigned)ceil_div((int64_t)n_left, 64), (unsigned)ceil_div(N, chunk));
  // bounding boxes of the pre-filter angles per window of 1024 columns (behind `best` in the same block)
  hipLaunchKernelGGL(k_tfd_window_bounds, dim3((unsigned)n_win), block, 0, ctx().stream, tfF_dev, N, Npad, qf4, n_win, wlo, whi);
  FC_TRY(check_launch("k_tfd_window_bounds"));
#define FC_FMR(QT)                                                                                          \
  case QT:                                                                                                  \
    hipLaunchKernelGGL(k_tfd_first_match_rest<QT>, rgrid, block, lds, ctx().stream, tfT_dev, tfF_dev, N, Npad, \
                       (int)Q, thresh, left_count, left_rows, left_from, chunk, best_dev, wlo, whi, n_win); \
    break;
  switch (Q) {
    FC_FMR(1) FC_FMR(2) FC_FMR(3) FC_FMR(4) FC_FMR(5) FC_FMR(6) FC_FMR(7) FC_FMR(8) FC_FMR(9) FC_FMR(10)
    FC_FMR(11) FC_FMR(12) FC_FMR(13) FC_FMR(14) FC_FMR(15) FC_FMR(16)
    default:
      hipLaunchKernelGGL(k_tfd_first_match_rest<0>, rgrid, block, lds, ctx().stream, tfT_dev, tfF_dev, N, Npad, (int)Q,
                         thresh, left_count, left_rows, left_from, chunk, best_dev, wlo, whi, n_win);
  }
#undef FC_FMR
  FC_TRY(check_launch("k_tfd_first_match_rest"));
  hipLaunchKernelGGL(k_tfd_first_match_merge, dim3((unsigned)ceil_div((int64_t)n_left, 256)), block, 0, ctx().stream, left_count,
                     left_rows, best_dev, fm_dev);
  return check_launch("k_tfd_first_match_merge");
}

#if defined(FC_TFD_STAMPS)
extern "C" int fc_debug_fm_stamps(unsigned long long *out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_fm_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {0};
    z[11] = ~0ull;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_fm_stamps), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
#endif

int launch_tfd_simbits(const double *tf_dev, int64_t N, int64_t Q, double thresh, int64_t row_begin,
                       int64_t row_end, uint64_t *bits_dev, int64_t W) {
  const int64_t waves = (row_end - row_begin) * W;
  if (waves <= 0) return FC_OK;
  if (!grid_x_fits(ceil_div(waves, 4), 256))
    return set_error(FC_E_LIMIT, "%lld rows x %lld words exceed one launch of the TFD bit kernel: pass fewer rows per call",
                     (long long)(row_end - row_begin), (long long)W);
  hipLaunchKernelGGL(k_tfd_simbits, dim3((unsigned)ceil_div(waves, 4)), dim3(256), 0, ctx().stream,
                     tf_dev, N, (int)Q, thresh, row_begin, row_end, bits_dev, W);
  return check_launch("k_tfd_simbits");
}

// fc_warmup(): the first launch from a translation unit makes the runtime load that unit's code object (milliseconds);
// a no-op launch moves that cost out of the first real call
__global__ void k_warm_prune() {}
int warm_prune() {
  hipLaunchKernelGGL(k_warm_prune, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_prune");
}

}  // namespace fc
