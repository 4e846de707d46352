// fc_clusters.hip -- connected components of a similarity graph on the device (include/fc_hip.h, "similarity clusters";
// DESIGN.md section 13): labels, representatives and sizes from the exactly-similar pair list of the RMSD stage, from its
// bit matrix, or from a caller's graph in either form.
//
// A lock-free union-find over parent[N] (int32).  The LARGER root is always hooked under the SMALLER one, so
//   - a non-root's parent is strictly smaller than its index: every walk ends, whatever it reads on the way;
//   - a component's final root is its smallest member: the representative the contract asks for, without a second pass.
// Launches: init -> hook (pairs or bits; long lists in phases with a compression between them, below) -> flatten +
// root flags -> scan -> label.  Only the hook kernels have threads that read what other workgroups of the SAME launch
// write; they read and write parent[] with agent-scope atomics only (below).  Behind a kernel boundary plain loads are
// enough.
#include "fc_internal.h"

namespace fc {

namespace {

constexpr int kClThreads = 256;

// Inside the hook kernel every access to parent[] is an agent-scope atomic: the L2s of the eight XCDs are not coherent
// for plain loads within a launch, and a retry that re-read a stale parent from its own XCD's L2 could spin for as
// long as the line stays resident.
__device__ __forceinline__ int32_t cl_load(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cl_store(int32_t *p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving.  A halving store that loses against another one costs time only: whatever lands in
// parent[x] was an ancestor of x when it was read, so it is smaller than x and in x's tree for good (trees only merge).
// At most x steps: every step moves to a strictly smaller index.
__device__ __forceinline__ int32_t cl_find(int32_t *parent, int32_t x) {
  for (;;) {
    const int32_t p = cl_load(parent + x);
    if (p == x) return x;
    const int32_t g = cl_load(parent + p);
    if (g == p) return p;
    cl_store(parent + x, g);
    x = g;
  }
}

// One union.  Every successful CAS removes a root, every failed one means that another thread's CAS on the same word
// succeeded: at most N - 1 failures over the whole launch.  The cap is a multiple of that; reaching it is a bug in this
// file and ends as an error word (FC_E_INTERNAL on the host), never as a hang.
__device__ __forceinline__ void cl_unite(int32_t *parent, int32_t a, int32_t b, int64_t retry_cap,
                                         unsigned long long *status) {
  // both ends under one parent already: the same tree, and nothing to write (what the later phases of a long list mostly
  // finds: two loads of words that nobody writes any more)
  if (cl_load(parent + a) == cl_load(parent + b)) return;
  for (int64_t tries = 0;; ++tries) {
    a = cl_find(parent, a);
    b = cl_find(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    int32_t expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    if (tries >= retry_cap) {
      status[kClStatusErr] = 1ull;
      return;
    }
    a = expected;  // what hi was hooked under meanwhile
    b = lo;
  }
}

// Long lists in phases.  With every edge of a dense graph in flight at once, hundreds of unions per vertex meet on the
// few words near the root of the giant component: CAS retries, halving stores and dependent agent-scope loads of lines
// that every atomic drops from the L2s serialise (7.6e5 edges on 10^4 conformers: one launch took 5 ms).  What costs is
// the number of unions in flight that meet on the same words, so the forest is grown under little contention first:
//   seed    parent[larger end] = min(itself, smaller end) for EVERY entry: one atomic that returns nothing -- no read, no
//           retry (25 us for that list).  It unites nothing by the hooking rule; it leaves every vertex pointing at its
//           smallest smaller neighbour, a forest inside the components whose roots are the local minima of the graph
//           (about N / degree of them instead of N).  A launch of its own in front of any CAS: the invariants (parent
//           <= index, parent in the same component) hold throughout;
//   coarse  the hooking rule on 1/1024 of the entries: enough to join most of those few trees (42 us);
//   fine    on the next 31/1024, then on the rest (7 us each): after a compression nearly every union starts with
//           "both ends under one parent already" -- two loads of words that nobody writes any more.
// k_cl_compress (parent[i] = root(i)) runs between the phases.  An entry's class is a multiplicative hash of its position,
// so that no stride of the list or of the bit rows lines up with it.  Which entries a phase takes changes the order of
// the unions, never the components.
__device__ __forceinline__ void cl_seed(int32_t *parent, int32_t hi, int32_t lo) {
  (void)__hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// an entry's sampling class, 0 .. 1023: the phases take [0, 1), [1, 32) and [32, 1024)
__device__ __forceinline__ unsigned cl_class(unsigned long long idx) { return ((uint32_t)idx * 2654435761u) >> 22; }
constexpr unsigned kClClasses = 1024, kClCoarse = 1, kClFine = 32;
constexpr unsigned long long kClSplitMin = (unsigned long long)kClShortList;  // entries from which a list is split
constexpr unsigned long long kClNeverSplit = ~0ull;

__global__ void __launch_bounds__(kClThreads)
k_cl_init(int32_t *__restrict__ parent, int64_t N, unsigned long long *__restrict__ status, unsigned long long n_pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) parent[i] = (int32_t)i;
  if (i == 0) {
    status[kClStatusErr] = 0ull;
    status[kClStatusList] = 1ull;
    status[kClStatusK] = 0ull;
    status[kClStatusPairs] = n_pairs;
  }
}

// One thread per entry of a device pair list ((i << 32) | j, either order, duplicates allowed) whose length is a
// device word: counters[2] of the refine, read here as the ladder reads it, with no host round trip.  The list is
// declined -- status[kClStatusList] = 0, nothing hooked -- when the refine's candidate queue overflowed (it then wrote no
// complete list; n_cand_ptr / cand_cap) or the screen's verdict asked for a redo (redo_ptr): the same conditions, decided
// in the same place, as k_ladder_pairs' counters[9].  Entries with i == j or an index >= N are padding and never act.
// seed: the seed launch; otherwise the entries of the classes [c_lo, c_hi).  A list shorter than split_min is not split:
// the launch that takes the last classes hooks ALL of it and the others return -- decided here from the device's
// length, so every launch sequence is right for any list.
__global__ void __launch_bounds__(kClThreads)
k_cl_hook_pairs(const uint64_t *__restrict__ pairs, const unsigned long long *__restrict__ n_pairs_ptr,
                const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap,
                const unsigned long long *__restrict__ redo_ptr, int64_t N, int32_t *parent,
                unsigned long long *status, bool seed, unsigned c_lo, unsigned c_hi, unsigned long long split_min) {
  const unsigned long long P = *n_pairs_ptr;
  const bool declined = (n_cand_ptr != nullptr && (*n_cand_ptr > cand_cap || P > cand_cap)) ||
                        (redo_ptr != nullptr && *redo_ptr != 0ull);
  if (declined) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[kClStatusList] = 0ull;
    return;
  }
  const bool split = P >= split_min;
  const bool last = !seed && c_hi == kClClasses;
  if (!last && !split) return;
  const uint32_t n32 = (uint32_t)N;
  const int64_t retry_cap = 4 * N + 1024;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    if (!seed && split && (cl_class(p) < c_lo || cl_class(p) >= c_hi)) continue;
    const uint64_t e = pairs[p];
    const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
    if (i == j || i >= n32 || j >= n32) continue;
    if (seed) {
      cl_seed(parent, (int32_t)(i > j ? i : j), (int32_t)(i > j ? j : i));
      continue;
    }
    cl_unite(parent, (int32_t)i, (int32_t)j, retry_cap, status);
  }
}

// One thread per 64-bit word of the bit matrix (row i, word w; row stride W words), walking its set bits.  Only bits
// j > i are read: words left of the diagonal word are skipped (the RMSD stage never writes them), the diagonal word is
// masked.  seed: the seed launch (one seed per word: its first neighbour); otherwise the words of the classes [c_lo, c_hi).
__global__ void __launch_bounds__(kClThreads)
k_cl_hook_bits(const uint64_t *__restrict__ bits, int64_t W, int64_t N, int32_t *parent, unsigned long long *status,
               bool seed, unsigned c_lo, unsigned c_hi) {
  const int64_t total = N * W;
  const int64_t retry_cap = 4 * N + 1024;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / W, w = t - i * W;
    if (w < (i >> 6)) continue;
    if (!seed && (cl_class((unsigned long long)t) < c_lo || cl_class((unsigned long long)t) >= c_hi)) continue;
    uint64_t word = bits[t];
    if (w == (i >> 6)) word &= (i & 63) == 63 ? 0ull : ~0ull << ((i & 63) + 1);
    if (seed) {
      const int64_t j = w * 64 + __ffsll((unsigned long long)word) - 1;
      if (word && j < N) cl_seed(parent, (int32_t)j, (int32_t)i);
      continue;
    }
    while (word) {
      const int b = __ffsll((unsigned long long)word) - 1;
      word &= word - 1;
      const int64_t j = w * 64 + b;
      if (j < N) cl_unite(parent, (int32_t)i, (int32_t)j, retry_cap, status);
    }
  }
}

// between the phases of a long list: parent[i] = root of i, in place.  Other threads walk through parent[i] while it is
// rewritten; old and new value are both ancestors of i, and no root changes in this launch.
__global__ void __launch_bounds__(kClThreads)
k_cl_compress(int32_t *parent, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int32_t x = (int32_t)i;
  for (int32_t p = cl_load(parent + x); p != x; p = cl_load(parent + x)) x = p;
  cl_store(parent + i, x);
}

// root[i] = root of i (out of place: nothing this launch reads is written by it), and the root flags of 64 consecutive
// conformers packed into one word with the wave64 ballot.
__global__ void __launch_bounds__(kClThreads)
k_cl_flatten(const int32_t *__restrict__ parent, int64_t N, int32_t *__restrict__ root, uint64_t *__restrict__ flags,
             int64_t W) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool is_root = false;
  if (i < N) {
    int32_t x = (int32_t)i;
    for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[i] = x;
    is_root = x == (int32_t)i;
  }
  const uint64_t m = __ballot(is_root);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < W) flags[i >> 6] = m;
}

// exclusive prefix of the per-word root counts; one workgroup loops over the W words (15 625 at 10^6 conformers)
__global__ void __launch_bounds__(1024)
k_cl_scan(const uint64_t *__restrict__ flags, int64_t W, int32_t *__restrict__ prefix,
          unsigned long long *__restrict__ status) {
  __shared__ int s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int64_t base = 0; base < W; base += 1024) {
    const int64_t w = base + tid;
    const int c = w < W ? __popcll(flags[w]) : 0;
    int v = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int s = s_wave[q];
      if (q < wave) before += s;
      all += s;
    }
    if (w < W) prefix[w] = carry + before + v - c;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) status[kClStatusK] = (unsigned long long)carry;
}

// label[i] = rank of i's root among the roots; the root itself writes reps[rank]; sizes[rank] counts members.  The
// adds are aggregated within the wavefront first (up to four distinct clusters per wavefront through a ballot each,
// the rest one by one): one giant cluster costs N / 64 adds to its word, not N.  Integer adds: the order does not show.
__global__ void __launch_bounds__(kClThreads)
k_cl_label(const int32_t *__restrict__ root, int64_t N, const uint64_t *__restrict__ flags,
           const int32_t *__restrict__ prefix, int32_t *__restrict__ labels, int64_t *__restrict__ reps,
           unsigned long long *__restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool pending = i < N;
  int32_t rank = -1;
  if (pending) {
    const int32_t r = root[i];
    rank = prefix[r >> 6] + __popcll(flags[r >> 6] & ((1ull << (r & 63)) - 1ull));
    labels[i] = rank;
    if ((int64_t)r == i) reps[rank] = i;
  }
  for (int round = 0; round < 4; ++round) {
    const uint64_t mp = __ballot(pending);
    if (mp == 0) break;  // wave-uniform
    const int leader = __ffsll((unsigned long long)mp) - 1;
    const int32_t lr = __shfl(rank, leader);
    const bool same = pending && rank == lr;
    const uint64_t ms = __ballot(same);
    if (lane == leader) atomicAdd(&sizes[lr], (unsigned long long)__popcll(ms));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&sizes[rank], 1ull);
}

int cl_blocks(int64_t items, int per_cu) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, kClThreads), (int64_t)ctx().n_cu * per_cu));
}

// what the launchers carve out of `work` (cluster_layout) and what every launch of theirs is sized by
struct ClWork {
  int32_t *labels;
  int64_t *reps;
  unsigned long long *sizes, *status;
  int32_t *parent, *root;
  uint64_t *flags;
  int32_t *prefix;
  uint8_t *core;     // core, deg, attach: the density-based form's
  int32_t *deg;      // (and the sphere-exclusion form's)
  uint32_t *attach;
  uint64_t *key, *owner;  // from here to live_e: the sphere-exclusion form's
  int32_t *state, *claim, *stamp, *live_v;
  unsigned long long *und;
  uint64_t *live_e;
  int64_t W;
  unsigned per_n;
  hipStream_t st;
};

// the head of every launcher: the argument checks, the carving, the memsets and k_cl_init.  kind: whose block it is
int cl_begin(const ClusterGraph &g, int64_t N, ClKind kind, int64_t min_samples, DevBuf &work, ClWork *w, size_t live_cap = 0) {
  const bool density = kind == kClDensity;
  const ClusterLayout L = cluster_layout(N, kind, live_cap);
  if (work.p == nullptr || work.bytes < L.total) return set_error(FC_E_INVALID, "cluster workspace too small");
  if (N < 1 || N > (int64_t)INT32_MAX - 256) return set_error(FC_E_LIMIT, "N=%lld: clusters index conformers with 32 bits", (long long)N);
  if (density && min_samples < 1) return set_error(FC_E_INVALID, "min_samples=%lld < 1", (long long)min_samples);
  if ((g.pairs_dev != nullptr) == (g.bits_dev != nullptr)) return set_error(FC_E_INVALID, "one of pair list / bit matrix");
  char *base = static_cast<char *>(work.p);
  w->labels = reinterpret_cast<int32_t *>(base + L.labels);
  w->reps = reinterpret_cast<int64_t *>(base + L.reps);
  w->sizes = reinterpret_cast<unsigned long long *>(base + L.sizes);
  w->core = reinterpret_cast<uint8_t *>(base + L.core);
  w->deg = reinterpret_cast<int32_t *>(base + L.degrees);
  w->status = reinterpret_cast<unsigned long long *>(base + L.status);
  w->parent = reinterpret_cast<int32_t *>(base + L.parent);
  w->root = reinterpret_cast<int32_t *>(base + L.root);
  w->flags = reinterpret_cast<uint64_t *>(base + L.flags);
  w->prefix = reinterpret_cast<int32_t *>(base + L.prefix);
  w->attach = reinterpret_cast<uint32_t *>(base + L.attach);
  w->key = reinterpret_cast<uint64_t *>(base + L.bu_key);
  w->owner = reinterpret_cast<uint64_t *>(base + L.bu_owner);
  w->state = reinterpret_cast<int32_t *>(base + L.bu_state);
  w->claim = reinterpret_cast<int32_t *>(base + L.bu_claim);
  w->stamp = reinterpret_cast<int32_t *>(base + L.bu_stamp);
  w->live_v = reinterpret_cast<int32_t *>(base + L.bu_live_v);
  w->und = reinterpret_cast<unsigned long long *>(base + L.bu_words);
  w->live_e = reinterpret_cast<uint64_t *>(base + L.bu_live_e);
  w->W = ceil_div(N, 64);
  w->st = cur_stream();
  w->per_n = (unsigned)ceil_div(N, kClThreads);
  FC_HIP_TRY(hipMemsetAsync(w->sizes, 0, (size_t)N * sizeof(unsigned long long), w->st));
  if (kind != kClComponents) FC_HIP_TRY(hipMemsetAsync(w->deg, 0, (size_t)N * sizeof(int32_t), w->st));
  if (density) FC_HIP_TRY(hipMemsetAsync(w->attach, 0xff, (size_t)N * sizeof(uint32_t), w->st));
  hipLaunchKernelGGL(k_cl_init, dim3(w->per_n), dim3(kClThreads), 0, w->st, w->parent, N, w->status, g.n_pairs_host);
  return check_launch("k_cl_init");
}

// the hook launches of one graph, hook(seed, first class, end class).  phased: seed | [0, coarse) | [coarse, fine) with a
// compression behind each, then the rest; else one launch over the classes from last_lo on
template <class Hook>
int hook_phases(const ClWork &w, int64_t N, bool phased, unsigned last_lo, const Hook &hook) {
  const auto compress = [&]() {
    hipLaunchKernelGGL(k_cl_compress, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.parent, N);
    return check_launch("k_cl_compress");
  };
  if (phased) {
    FC_TRY(hook(true, 0u, 0u));
    FC_TRY(compress());
    FC_TRY(hook(false, 0u, kClCoarse));
    FC_TRY(compress());
    FC_TRY(hook(false, kClCoarse, kClFine));
    FC_TRY(compress());
  }
  return hook(false, last_lo, kClClasses);
}

// the size of the pair-list launches (the list's length is on the device only: the grid is sized for the chip, the kernels
// stride) and of the bit-matrix ones; the bit matrix is the dense case, split from 1024 words on
dim3 cl_grid_pairs() { return dim3((unsigned)(ctx().n_cu * 8)); }
dim3 cl_grid_bits(int64_t N, int64_t W) { return dim3((unsigned)cl_blocks(N * W, 16)); }
bool cl_split_bits(int64_t N, int64_t W) { return (unsigned long long)N * (unsigned long long)W >= 1024ull; }

}  // namespace

// Everything behind the graph: the caller has reserved `work` (cluster_layout(N, kClComponents).total bytes) and, for the pair
// form, left the list where `g` says.  Enqueues only; the result region of `work` is complete when the stream has drained.
int launch_clusters(const ClusterGraph &g, int64_t N, DevBuf &work) {
  ClWork w;
  FC_TRY(cl_begin(g, N, kClComponents, 1, work, &w));
  if (g.pairs_dev != nullptr) {
    const unsigned long long *n_pairs_dev = g.n_pairs_dev != nullptr ? g.n_pairs_dev : w.status + kClStatusPairs;
    // g.known_short: the caller has seen this list's length (or a recent one of these coordinates) -- the launches that
    // would find nothing to do are left out; a list that is long after all is then hooked in one launch, slowly and correctly
    const dim3 grid = cl_grid_pairs();
    const unsigned long long split_min = g.known_short ? kClNeverSplit : kClSplitMin;
    FC_TRY(hook_phases(w, N, !g.known_short, kClFine, [&](bool seed, unsigned c_lo, unsigned c_hi) {
      hipLaunchKernelGGL(k_cl_hook_pairs, grid, dim3(kClThreads), 0, w.st, g.pairs_dev, n_pairs_dev, g.n_cand_dev, g.cand_cap,
                         g.redo_dev, N, w.parent, w.status, seed, c_lo, c_hi, split_min);
      return check_launch("k_cl_hook_pairs");
    }));  // (the last launch: all of a list that is not split)
  } else {
    if (g.W < w.W) return set_error(FC_E_INVALID, "bit rows of %lld words, %lld needed", (long long)g.W, (long long)w.W);
    const dim3 grid = cl_grid_bits(N, g.W);
    const bool split = cl_split_bits(N, g.W);
    FC_TRY(hook_phases(w, N, split, split ? kClFine : 0u, [&](bool seed, unsigned c_lo, unsigned c_hi) {
      hipLaunchKernelGGL(k_cl_hook_bits, grid, dim3(kClThreads), 0, w.st, g.bits_dev, g.W, N, w.parent, w.status, seed, c_lo, c_hi);
      return check_launch("k_cl_hook_bits");
    }));
  }
  hipLaunchKernelGGL(k_cl_flatten, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.parent, N, w.root, w.flags, w.W);
  FC_TRY(check_launch("k_cl_flatten"));
  hipLaunchKernelGGL(k_cl_scan, dim3(1), dim3(1024), 0, w.st, w.flags, w.W, w.prefix, w.status);
  FC_TRY(check_launch("k_cl_scan"));
  hipLaunchKernelGGL(k_cl_label, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.root, N, w.flags, w.prefix, w.labels, w.reps, w.sizes);
  return check_launch("k_cl_label");
}

// ---- density-based clusters (include/fc_hip.h, "density-based clusters") ---------------------------
// The same union-find restricted to the CORE vertices (degree + 1 >= min_samples): only core-core edges unite, an edge
// with exactly one core end leaves that end in attach[the other] (the smallest one wins), and the labelling counts a root
// only when it is core.  The kernels of the components above are not touched: every step that differs has a kernel of
// its own here (k_db_*), the steps that do not (k_cl_init, k_cl_compress, k_cl_scan) are shared.
// Launches: init -> degrees -> hook (the phases of the components; borders attached by the launch that sees every
// entry) -> flatten + core flags -> scan -> label.  deg[] is complete when its launch has ended and attach[] is only
// written (an agent-scope atomic that returns nothing) inside the hook launches: plain loads of both are enough
// behind the kernel boundary.  parent[] inside the hook launches: as above, agent-scope atomics only.
namespace {

constexpr uint32_t kDbNone = 0xffffffffu;  // attach[i]: no core neighbour seen (hipMemsetAsync 0xff)

__device__ __forceinline__ bool db_core(const int32_t *__restrict__ deg, uint32_t i, int64_t min_samples) {
  return (int64_t)deg[i] + 1 >= min_samples;
}

// deg[dest] += 1 for every lane that is `on`, equal destinations of the wavefront added once: up to four distinct ones
// through a ballot each (a hub, or the run of one row in the refine's list), the rest one by one.  The caller keeps
// the wavefront converged.  Integer adds that return nothing: the order does not show.
__device__ __forceinline__ void db_count(int32_t *deg, bool on, uint32_t dest, int lane) {
  bool pending = on;
  for (int round = 0; round < 4; ++round) {
    const uint64_t mp = __ballot(pending);
    if (mp == 0) return;  // wave-uniform
    const int leader = __ffsll((unsigned long long)mp) - 1;
    const uint32_t ld = __shfl(dest, leader);
    const bool same = pending && dest == ld;
    const uint64_t ms = __ballot(same);
    if (lane == leader) (void)__hip_atomic_fetch_add(deg + ld, (int32_t)__popcll(ms), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pending = pending && !same;
  }
  if (pending) (void)__hip_atomic_fetch_add(deg + dest, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the conditions on which k_cl_hook_pairs declines the refine's list, word for word
__device__ __forceinline__ bool db_declined(unsigned long long P, const unsigned long long *__restrict__ n_cand_ptr,
                                            unsigned long long cand_cap, const unsigned long long *__restrict__ redo_ptr) {
  return (n_cand_ptr != nullptr && (*n_cand_ptr > cand_cap || P > cand_cap)) || (redo_ptr != nullptr && *redo_ptr != 0ull);
}

// Degrees from the pair list: every entry adds 1 to both of its ends (so an unordered pair must be listed once).  The
// length is the device's word; a declined list counts nothing and clears status[kClStatusList].  deg[] zeroed by the launcher.
__global__ void __launch_bounds__(kClThreads)
k_db_degree_pairs(const uint64_t *__restrict__ pairs, const unsigned long long *__restrict__ n_pairs_ptr,
                  const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap,
                  const unsigned long long *__restrict__ redo_ptr, int64_t N, int32_t *deg, unsigned long long *status) {
  const unsigned long long P = *n_pairs_ptr;
  if (db_declined(P, n_cand_ptr, cand_cap, redo_ptr)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[kClStatusList] = 0ull;
    return;
  }
  const uint32_t n32 = (uint32_t)N;
  const int lane = threadIdx.x & 63;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  // (the bound is the wavefront's first entry: all 64 lanes stay in the loop together)
  for (unsigned long long p0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); p0 < P; p0 += stride) {
    const unsigned long long p = p0 + (unsigned)lane;
    uint32_t i = 0, j = 0;
    bool on = p < P;
    if (on) {
      const uint64_t e = pairs[p];
      i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
      on = i != j && i < n32 && j < n32;
    }
    db_count(deg, on, i, lane);
    db_count(deg, on, j, lane);
  }
}

// Degrees from the bit matrix, no atomics: workgroup c owns the 64 conformers of word column c.
//   column part  the four wavefronts share the rows above the diagonal; all lanes read the same word (row i, word c)
//                and lane l counts bit l, for i < 64 c + l only, in a register;
//   row part     each wavefront takes 16 of the 64 rows: the popcount of the row's words from the diagonal word
//                rightwards, masked as k_cl_hook_bits masks it and cut at N.
// Each part reads the upper triangle once; the sum is exact and has no order.
__global__ void __launch_bounds__(kClThreads)
k_db_degree_bits(const uint64_t *__restrict__ bits, int64_t W, int64_t N, int32_t *__restrict__ deg) {
  __shared__ int s_col[kClThreads / 64][64];
  __shared__ int s_row[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x, Wn = (N + 63) >> 6;
  const int64_t j = c * 64 + lane;
  const int64_t rows = N < c * 64 + 64 ? N : c * 64 + 64;
  int cnt = 0;
#pragma unroll 8
  for (int64_t i = wave; i < rows; i += kClThreads / 64) {
    const uint64_t word = bits[i * W + c];
    cnt += (int)((word >> lane) & 1ull) & (int)(i < j);
  }
  s_col[wave][lane] = cnt;
  for (int r = 0; r < 16; ++r) {
    const int64_t i = c * 64 + wave * 16 + r;  // (wave-uniform)
    int rc = 0;
    if (i < N) {
      for (int64_t w = c + lane; w < Wn; w += 64) {
        uint64_t word = bits[i * W + w];
        if (w == c) word &= (i & 63) == 63 ? 0ull : ~0ull << ((i & 63) + 1);
        if (w == Wn - 1 && (N & 63) != 0) word &= (1ull << (N & 63)) - 1ull;
        rc += __popcll(word);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rc += __shfl_xor(rc, o);
    if (lane == 0) s_row[wave * 16 + r] = rc;
  }
  __syncthreads();
  if (tid < 64 && j < N) deg[j] = s_col[0][tid] + s_col[1][tid] + s_col[2][tid] + s_col[3][tid] + s_row[tid];
}

// one edge under the core rule.  unite: the hooking rule for a core-core edge (seed: its seed); attach: an edge with
// exactly one core end offers that end to the other
__device__ __forceinline__ void db_edge(uint32_t i, uint32_t j, const int32_t *__restrict__ deg, int64_t min_samples,
                                        int32_t *parent, uint32_t *attach, bool seed, bool unite, bool do_attach,
                                        int64_t retry_cap, unsigned long long *status) {
  const bool ci = db_core(deg, i, min_samples), cj = db_core(deg, j, min_samples);
  if (ci && cj) {
    if (!unite) return;
    if (seed)
      cl_seed(parent, (int32_t)(i > j ? i : j), (int32_t)(i > j ? j : i));
    else
      cl_unite(parent, (int32_t)i, (int32_t)j, retry_cap, status);
  } else if (do_attach && (ci || cj)) {
    (void)__hip_atomic_fetch_min(attach + (ci ? j : i), ci ? i : j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// k_cl_hook_pairs under the core rule: the same phases, the same split decided from the device's length, the same
// retry cap and error word.  Borders are attached by the one launch that visits every entry: the seed launch of a split
// list, the last launch of a list that is not split.
__global__ void __launch_bounds__(kClThreads)
k_db_hook_pairs(const uint64_t *__restrict__ pairs, const unsigned long long *__restrict__ n_pairs_ptr,
                const unsigned long long *__restrict__ n_cand_ptr, unsigned long long cand_cap,
                const unsigned long long *__restrict__ redo_ptr, int64_t N, const int32_t *__restrict__ deg,
                int64_t min_samples, int32_t *parent, uint32_t *attach, unsigned long long *status, bool seed, unsigned c_lo,
                unsigned c_hi, unsigned long long split_min) {
  const unsigned long long P = *n_pairs_ptr;
  if (db_declined(P, n_cand_ptr, cand_cap, redo_ptr)) return;  // (k_db_degree_pairs has said so in status[])
  const bool split = P >= split_min;
  const bool last = !seed && c_hi == kClClasses;
  if (!last && !split) return;
  const bool do_attach = seed ? split : !split;
  const uint32_t n32 = (uint32_t)N;
  const int64_t retry_cap = 4 * N + 1024;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    const bool mine = seed || !split || (cl_class(p) >= c_lo && cl_class(p) < c_hi);
    if (!mine && !do_attach) continue;
    const uint64_t e = pairs[p];
    const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
    if (i == j || i >= n32 || j >= n32) continue;
    db_edge(i, j, deg, min_samples, parent, attach, seed, mine, do_attach, retry_cap, status);
  }
}

// k_cl_hook_bits under the core rule.  The seed launch walks every set bit (the borders are attached there) and seeds
// each core row with its first core neighbour of the word.
__global__ void __launch_bounds__(kClThreads)
k_db_hook_bits(const uint64_t *__restrict__ bits, int64_t W, int64_t N, const int32_t *__restrict__ deg, int64_t min_samples,
               int32_t *parent, uint32_t *attach, unsigned long long *status, bool seed, bool do_attach, unsigned c_lo,
               unsigned c_hi) {
  const int64_t total = N * W;
  const int64_t retry_cap = 4 * N + 1024;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / W, w = t - i * W;
    if (w < (i >> 6)) continue;
    if (!seed && (cl_class((unsigned long long)t) < c_lo || cl_class((unsigned long long)t) >= c_hi)) continue;
    uint64_t word = bits[t];
    if (w == (i >> 6)) word &= (i & 63) == 63 ? 0ull : ~0ull << ((i & 63) + 1);
    bool seeded = false;
    while (word) {
      const int b = __ffsll((unsigned long long)word) - 1;
      word &= word - 1;
      const int64_t j = w * 64 + b;
      if (j >= N) break;  // (ascending: nothing behind it is a conformer)
      const bool both = db_core(deg, (uint32_t)i, min_samples) && db_core(deg, (uint32_t)j, min_samples);
      db_edge((uint32_t)i, (uint32_t)j, deg, min_samples, parent, attach, seed, !(seed && seeded), do_attach, retry_cap, status);
      seeded = seeded || both;
    }
  }
}

// k_cl_flatten under the core rule: a vertex that is not core was never hooked and is its own root, so a root is
// flagged only when it is core.  The core flags travel to the host from here.
__global__ void __launch_bounds__(kClThreads)
k_db_flatten(const int32_t *__restrict__ parent, int64_t N, const int32_t *__restrict__ deg, int64_t min_samples,
             int32_t *__restrict__ root, uint64_t *__restrict__ flags, int64_t W, uint8_t *__restrict__ core) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool is_root = false;
  if (i < N) {
    int32_t x = (int32_t)i;
    for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[i] = x;
    const bool c = db_core(deg, (uint32_t)i, min_samples);
    core[i] = c ? 1 : 0;
    is_root = c && x == (int32_t)i;
  }
  const uint64_t m = __ballot(is_root);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < W) flags[i >> 6] = m;
}

// k_cl_label with noise: a core vertex takes the rank of its root, a border vertex that of the root of attach[i] (a
// core vertex: its root is a flagged one), everything else -1.  sizes count both kinds, aggregated as in k_cl_label.
__global__ void __launch_bounds__(kClThreads)
k_db_label(const int32_t *__restrict__ root, int64_t N, const uint8_t *__restrict__ core, const uint32_t *__restrict__ attach,
           const uint64_t *__restrict__ flags, const int32_t *__restrict__ prefix, int32_t *__restrict__ labels,
           int64_t *__restrict__ reps, unsigned long long *__restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool pending = false;
  int32_t rank = -1;
  if (i < N) {
    int32_t r = -1;
    if (core[i])
      r = root[i];
    else if (attach[i] != kDbNone)
      r = root[attach[i]];
    if (r >= 0) {
      rank = prefix[r >> 6] + __popcll(flags[r >> 6] & ((1ull << (r & 63)) - 1ull));
      if ((int64_t)r == i) reps[rank] = i;
      pending = true;
    }
    labels[i] = rank;
  }
  for (int round = 0; round < 4; ++round) {
    const uint64_t mp = __ballot(pending);
    if (mp == 0) break;  // wave-uniform
    const int leader = __ffsll((unsigned long long)mp) - 1;
    const int32_t lr = __shfl(rank, leader);
    const bool same = pending && rank == lr;
    const uint64_t ms = __ballot(same);
    if (lane == leader) atomicAdd(&sizes[lr], (unsigned long long)__popcll(ms));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&sizes[rank], 1ull);
}

}  // namespace

// launch_clusters under the core rule; `work` holds cluster_layout(N, kClDensity).total bytes
int launch_dbscan(const ClusterGraph &g, int64_t N, int64_t min_samples, DevBuf &work) {
  ClWork w;
  FC_TRY(cl_begin(g, N, kClDensity, min_samples, work, &w));
  if (g.pairs_dev != nullptr) {
    const unsigned long long *n_pairs_dev = g.n_pairs_dev != nullptr ? g.n_pairs_dev : w.status + kClStatusPairs;
    const dim3 grid = cl_grid_pairs();
    const unsigned long long split_min = g.known_short ? kClNeverSplit : kClSplitMin;
    hipLaunchKernelGGL(k_db_degree_pairs, grid, dim3(kClThreads), 0, w.st, g.pairs_dev, n_pairs_dev, g.n_cand_dev, g.cand_cap,
                       g.redo_dev, N, w.deg, w.status);
    FC_TRY(check_launch("k_db_degree_pairs"));
    FC_TRY(hook_phases(w, N, !g.known_short, kClFine, [&](bool seed, unsigned c_lo, unsigned c_hi) {
      hipLaunchKernelGGL(k_db_hook_pairs, grid, dim3(kClThreads), 0, w.st, g.pairs_dev, n_pairs_dev, g.n_cand_dev, g.cand_cap,
                         g.redo_dev, N, w.deg, min_samples, w.parent, w.attach, w.status, seed, c_lo, c_hi, split_min);
      return check_launch("k_db_hook_pairs");
    }));
  } else {
    if (g.W < w.W) return set_error(FC_E_INVALID, "bit rows of %lld words, %lld needed", (long long)g.W, (long long)w.W);
    hipLaunchKernelGGL(k_db_degree_bits, dim3((unsigned)w.W), dim3(kClThreads), 0, w.st, g.bits_dev, g.W, N, w.deg);
    FC_TRY(check_launch("k_db_degree_bits"));
    const dim3 grid = cl_grid_bits(N, g.W);
    const bool split = cl_split_bits(N, g.W);
    FC_TRY(hook_phases(w, N, split, split ? kClFine : 0u, [&](bool seed, unsigned c_lo, unsigned c_hi) {
      hipLaunchKernelGGL(k_db_hook_bits, grid, dim3(kClThreads), 0, w.st, g.bits_dev, g.W, N, w.deg, min_samples, w.parent,
                         w.attach, w.status, seed, /*do_attach=*/seed || !split, c_lo, c_hi);
      return check_launch("k_db_hook_bits");
    }));
  }
  hipLaunchKernelGGL(k_db_flatten, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.parent, N, w.deg, min_samples, w.root, w.flags,
                     w.W, w.core);
  FC_TRY(check_launch("k_db_flatten"));
  hipLaunchKernelGGL(k_cl_scan, dim3(1), dim3(1024), 0, w.st, w.flags, w.W, w.prefix, w.status);
  FC_TRY(check_launch("k_cl_scan"));
  hipLaunchKernelGGL(k_db_label, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.root, N, w.core, w.attach, w.flags, w.prefix,
                     w.labels, w.reps, w.sizes);
  return check_launch("k_db_label");
}

// ---- sphere-exclusion clusters (include/fc_hip.h, "sphere-exclusion clusters") --------------------
// Butina's walk in its fixed order is the lexicographically-first maximal independent set of the graph under the
// priority key[v] = ((0x7fffffff - d(v)) << 32) | v (smaller first): v is a centroid exactly when none of its neighbours
// with a smaller key is one.  It is decided in synchronous rounds over state[N] (undecided, centroid, member).  Round r:
//   edge pass    for an edge (a, b), key[a] < key[b]: a centroid and b undecided -> claim[b] = 1; both undecided ->
//                stamp[b] = r ("blocked in round r": an earlier neighbour may still become a centroid);
//   vertex pass  an undecided v that is claimed becomes a member; one that is not stamped r has only members before it
//                and becomes a centroid; the rest is counted into und[r].
// Two launches, so that nothing one workgroup writes is read by another in the same launch: the edge pass reads key[]
// and state[] and writes claim[] and stamp[] (plain stores: every writer of a word writes the same value), the vertex
// pass reads those and writes state[i] from thread i alone.  A round that finds und[r - 1] == 0 returns at once.  The
// first undecided vertex in key order is never stamped, so every round decides at least one vertex.
// Launches: init -> degrees (the density-based form's two kernels, unchanged) -> keys -> R rounds -> one more round that
// also writes down the live subgraph (the vertices it leaves undecided; the edges it found with two undecided ends,
// which are all the edges the remaining rounds can act on) -> finish: ONE workgroup goes on with the same two passes
// over the live lists, __syncthreads() between them, until nothing is undecided -> owners -> roots + centroid flags ->
// k_cl_scan -> k_cl_label (both unchanged).  No thread waits for another workgroup anywhere.
// The live-edge list has live_cap entries.  When the graph left more than that, the list is not used and the finish
// walks the graph itself (the caller's list or the bit matrix): slower, the same rounds.
namespace {

constexpr int32_t kBuUndecided = 0, kBuCentroid = 1, kBuMember = 2;
constexpr int kBuLiveE = kBuRoundsMax + 2;  // und[kBuLiveE]: edges offered to the live list (more than live_cap: not used)
constexpr int kBuFinishThreads = 1024;

// The edge sources.  each(first, stride, f) calls f(on, i, j) with the wavefront CONVERGED (the loop bounds are the
// wavefront's, a lane without an edge passes on = false), so that f may ballot.  first: the thread's index in the launch.

// the edges of a pair list whose length is a device word; declined on k_db_degree_pairs' conditions (no edges then)
struct BuPairs {
  const uint64_t *pairs;
  const unsigned long long *n_pairs_ptr, *n_cand_ptr;
  unsigned long long cand_cap;
  const unsigned long long *redo_ptr;
  uint32_t n32;
  template <class F>
  __device__ __forceinline__ void each(unsigned long long first, unsigned long long stride, const F &f) const {
    const unsigned long long P = *n_pairs_ptr;
    if (db_declined(P, n_cand_ptr, cand_cap, redo_ptr)) return;
    const unsigned lane = (unsigned)(first & 63ull);
    for (unsigned long long p0 = first - lane; p0 < P; p0 += stride) {
      const unsigned long long p = p0 + lane;
      uint32_t i = 0, j = 0;
      bool on = p < P;
      if (on) {
        const uint64_t e = pairs[p];
        i = (uint32_t)(e >> 32), j = (uint32_t)(e & 0xffffffffull);
        on = i != j && i < n32 && j < n32;
      }
      f(on, i, j);
    }
  }
};

// the edges of a bit matrix, walked as k_cl_hook_bits walks it: bits j > i only, the diagonal word masked, cut at N
struct BuBits {
  const uint64_t *bits;
  int64_t W, N;
  template <class F>
  __device__ __forceinline__ void each(unsigned long long first, unsigned long long stride, const F &f) const {
    const int64_t total = N * W;
    const int64_t lane = (int64_t)(first & 63ull);
    for (int64_t t0 = (int64_t)first - lane; t0 < total; t0 += (int64_t)stride) {
      const int64_t t = t0 + lane;
      int64_t i = 0, w = 0;
      uint64_t word = 0ull;
      if (t < total) {
        i = t / W, w = t - i * W;
        if (w >= (i >> 6)) word = bits[t];
        if (w == (i >> 6)) word &= (i & 63) == 63 ? 0ull : ~0ull << ((i & 63) + 1);
      }
      while (__any(word != 0ull)) {  // wave-uniform
        int64_t j = 0;
        bool on = word != 0ull;
        if (on) {
          j = w * 64 + __ffsll((unsigned long long)word) - 1;
          word &= word - 1;
          if (j >= N) on = false, word = 0ull;  // (ascending: nothing behind it is a conformer)
        }
        f(on, (uint32_t)i, (uint32_t)j);
      }
    }
  }
};

// the edge pass on one edge (on: this lane has one; the wavefront is converged).  live_e != nullptr: an edge with two
// undecided ends is also written to the live list as (a << 32) | b, a before b in key order -- one add per wavefront
__device__ __forceinline__ void bu_edge(bool on, uint32_t i, uint32_t j, const uint64_t *key, const int32_t *state,
                                        int32_t *claim, int32_t *stamp, int32_t r, uint64_t *live_e,
                                        unsigned long long *live_n, unsigned long long live_cap) {
  uint32_t a = 0, b = 0;
  bool both = false;
  if (on) {
    const bool first = key[i] < key[j];
    a = first ? i : j, b = first ? j : i;
    if (state[b] == kBuUndecided) {
      const int32_t sa = state[a];
      if (sa == kBuCentroid) claim[b] = 1;
      both = sa == kBuUndecided;
      if (both) stamp[b] = r;
    }
  }
  if (live_e == nullptr) return;  // (uniform)
  const uint64_t m = __ballot(both);
  if (m == 0ull) return;  // wave-uniform
  const int lane = (int)(__lane_id());
  const int leader = __ffsll((unsigned long long)m) - 1;
  unsigned long long base = 0ull;
  if (lane == leader) base = atomicAdd(live_n, (unsigned long long)__popcll(m));
  base = __shfl(base, leader);
  const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
  if (both && slot < live_cap) live_e[slot] = ((uint64_t)a << 32) | (uint64_t)b;
}

// the vertex pass on one vertex; true: it stays undecided
__device__ __forceinline__ bool bu_vertex(uint32_t v, int32_t *state, const int32_t *claim, const int32_t *stamp, int32_t r) {
  if (state[v] != kBuUndecided) return false;
  if (claim[v] != 0)
    state[v] = kBuMember;
  else if (stamp[v] != r)
    state[v] = kBuCentroid;
  else
    return true;
  return false;
}

// key[], the cleared per-vertex words and the round words: und[0] = N, everything else 0
__global__ void __launch_bounds__(kClThreads)
k_bu_keys(const int32_t *__restrict__ deg, int64_t N, uint64_t *__restrict__ key, uint64_t *__restrict__ owner,
          int32_t *__restrict__ state, int32_t *__restrict__ claim, int32_t *__restrict__ stamp,
          unsigned long long *__restrict__ und, unsigned long long *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    key[i] = ((uint64_t)(0x7fffffff - deg[i]) << 32) | (uint64_t)i;
    owner[i] = ~0ull;
    state[i] = kBuUndecided;
    claim[i] = 0;
    stamp[i] = 0;
  }
  if (blockIdx.x == 0) {
    for (int k = threadIdx.x; k < kBuWords; k += kClThreads) und[k] = k == 0 ? (unsigned long long)N : 0ull;
    if (threadIdx.x == 0) status[kBuStatusRounds] = 0ull, status[kBuStatusLeft] = 0ull;
  }
}

// the edge pass of round r >= 1 (und[r - 1]: what the round before left).  live_e != nullptr: the round that writes the
// live lists
template <class Src>
__global__ void __launch_bounds__(kClThreads)
k_bu_edges(const Src src, const uint64_t *__restrict__ key, const int32_t *__restrict__ state, int32_t *claim, int32_t *stamp,
           unsigned long long *und, int32_t r, uint64_t *live_e, unsigned long long live_cap) {
  if (und[r - 1] == 0ull) return;
  src.each((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, (unsigned long long)gridDim.x * blockDim.x,
           [&](bool on, uint32_t i, uint32_t j) { bu_edge(on, i, j, key, state, claim, stamp, r, live_e, und + kBuLiveE, live_cap); });
}

// the vertex pass of round r.  What stays undecided is counted into und[r], one add per wavefront; live_v != nullptr:
// and written there, at the slots the add returned (any order: the finish takes the list as a set)
__global__ void __launch_bounds__(kClThreads)
k_bu_vertices(int64_t N, int32_t *state, const int32_t *__restrict__ claim, const int32_t *__restrict__ stamp, int32_t r,
              unsigned long long *und, int32_t *__restrict__ live_v, unsigned long long *__restrict__ status) {
  if (und[r - 1] == 0ull) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool left = i < N && bu_vertex((uint32_t)i, state, claim, stamp, r);
  const uint64_t m = __ballot(left);
  if (m != 0ull) {  // wave-uniform
    const int leader = __ffsll((unsigned long long)m) - 1;
    unsigned long long base = 0ull;
    if (lane == leader) base = atomicAdd(und + r, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (left && live_v != nullptr) live_v[base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
  }
  if (i == 0) status[kBuStatusRounds] = (unsigned long long)r;
}

// The finish: ONE workgroup, rounds r0, r0 + 1, ... over the live vertices (und[r0 - 1] of them, left by round r0 - 1)
// and the live edges, the two passes separated by __syncthreads().  Thread t owns the list entries t, t + 1024, ... and
// keeps them compact in place, on its own: an edge stays only while both ends are undecided (nothing else can act
// again), a vertex while it is undecided, so a round costs what is left, not what there was.  The entries are
// (a << 32) | b with a before b already: no key is read here.  Every round decides at least the first undecided vertex
// in key order, so as many rounds as there are live vertices are enough; not done after that is a bug in this file
// and ends as the error word, never as a hang.  Returns at once when the live-edge list overflowed (k_bu_finish_graph).
__global__ void __launch_bounds__(kBuFinishThreads)
k_bu_finish(uint64_t *live_e, unsigned long long live_cap, int32_t *state, int32_t *claim, int32_t *stamp, int32_t *live_v,
            const unsigned long long *und, int32_t r0, unsigned long long *status) {
  const unsigned long long nv = und[r0 - 1], ne = und[kBuLiveE];
  if (nv == 0ull || ne > live_cap) return;
  const unsigned tid = threadIdx.x;
  constexpr unsigned long long T = kBuFinishThreads;
  // s_left[it % 3] != 0: round it left something undecided.  Three words in turn: the one of round it + 1 is cleared in
  // round it ahead of the first barrier, when its readers (after the second barrier of round it - 2) are all through
  __shared__ int s_left[3];
  if (tid == 0) status[kBuStatusLeft] = nv, s_left[0] = 0;
  unsigned long long ecnt = ne > tid ? (ne - tid + T - 1) / T : 0ull, vcnt = nv > tid ? (nv - tid + T - 1) / T : 0ull;
  bool done = false;
  int32_t r = r0;
  for (unsigned long long it = 0; it < nv; ++it, ++r) {
    if (tid == 0) s_left[(it + 1) % 3] = 0;
    unsigned long long kept = 0ull;
    for (unsigned long long k = 0; k < ecnt; k += 4) {  // four entries in flight; all four are read before one is written back
      uint64_t e[4];
      int32_t sa[4], sb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) e[q] = k + q < ecnt ? live_e[tid + T * (k + q)] : ~0ull;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool on = e[q] != ~0ull;
        sb[q] = on ? state[(uint32_t)(e[q] & 0xffffffffull)] : kBuMember;
        sa[q] = on ? state[(uint32_t)(e[q] >> 32)] : kBuMember;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (sb[q] != kBuUndecided) continue;
        const uint32_t b = (uint32_t)(e[q] & 0xffffffffull);
        if (sa[q] == kBuCentroid) {
          claim[b] = 1;
        } else if (sa[q] == kBuUndecided) {
          stamp[b] = r;
          live_e[tid + T * kept++] = e[q];
        }
      }
    }
    ecnt = kept;
    __syncthreads();
    kept = 0ull;
    for (unsigned long long k = 0; k < vcnt; ++k) {
      const int32_t v = live_v[tid + T * k];
      if (bu_vertex((uint32_t)v, state, claim, stamp, r)) live_v[tid + T * kept++] = v;
    }
    vcnt = kept;
    if (kept != 0ull) s_left[it % 3] = 1;
    __syncthreads();  // (also the barrier between this round's state and the next edge pass)
    done = s_left[it % 3] == 0;
    if (done) break;
  }
  if (tid == 0) {
    if (done)
      status[kBuStatusRounds] = (unsigned long long)r;
    else
      status[kClStatusErr] = 1ull;
  }
}

// The finish when the live-edge list overflowed: the same rounds with the edge pass over the graph itself (the live
// vertices always fit).  Slower -- every round walks every edge -- and the same result.
template <class Src>
__global__ void __launch_bounds__(kBuFinishThreads)
k_bu_finish_graph(const Src src, unsigned long long live_cap, const uint64_t *key, int32_t *state, int32_t *claim,
                  int32_t *stamp, int32_t *live_v, const unsigned long long *und, int32_t r0, unsigned long long *status) {
  const unsigned long long nv = und[r0 - 1];
  if (nv == 0ull || und[kBuLiveE] <= live_cap) return;
  const unsigned tid = threadIdx.x;
  constexpr unsigned long long T = kBuFinishThreads;
  // s_left[it % 3] != 0: round it left something undecided.  Three words in turn: the one of round it + 1 is cleared in
  // round it ahead of the first barrier, when its readers (after the second barrier of round it - 2) are all through
  __shared__ int s_left[3];
  if (tid == 0) status[kBuStatusLeft] = nv, s_left[0] = 0;
  unsigned long long vcnt = nv > tid ? (nv - tid + T - 1) / T : 0ull;
  bool done = false;
  int32_t r = r0;
  for (unsigned long long it = 0; it < nv; ++it, ++r) {
    if (tid == 0) s_left[(it + 1) % 3] = 0;
    src.each((unsigned long long)tid, T,
             [&](bool on, uint32_t i, uint32_t j) { bu_edge(on, i, j, key, state, claim, stamp, r, nullptr, nullptr, 0ull); });
    __syncthreads();
    unsigned long long kept = 0ull;
    for (unsigned long long k = 0; k < vcnt; ++k) {
      const int32_t v = live_v[tid + T * k];
      if (bu_vertex((uint32_t)v, state, claim, stamp, r)) live_v[tid + T * kept++] = v;
    }
    vcnt = kept;
    if (kept != 0ull) s_left[it % 3] = 1;
    __syncthreads();
    done = s_left[it % 3] == 0;
    if (done) break;
  }
  if (tid == 0) {
    if (done)
      status[kBuStatusRounds] = (unsigned long long)r;
    else
      status[kClStatusErr] = 1ull;
  }
}

// Owners: the centroid of a member is the first centroid, in key order, among its neighbours.  A pass of its own over
// every edge, after the last round: the centroid that claimed a member first need not be that one (an earlier centroid
// can be decided in a later round).  owner[] starts as all ones.
template <class Src>
__global__ void __launch_bounds__(kClThreads)
k_bu_owners(const Src src, const uint64_t *__restrict__ key, const int32_t *__restrict__ state, uint64_t *owner) {
  src.each((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, (unsigned long long)gridDim.x * blockDim.x,
           [&](bool on, uint32_t i, uint32_t j) {
             if (!on) return;
             const int32_t si = state[i], sj = state[j];
             if (si == kBuCentroid && sj == kBuMember)
               (void)__hip_atomic_fetch_min(owner + j, key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
             else if (sj == kBuCentroid && si == kBuMember)
               (void)__hip_atomic_fetch_min(owner + i, key[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
           });
}

// k_cl_flatten's outputs from state[] and owner[]: root[i] = the centroid's index, flags = the centroid ballot.  A vertex
// that is neither a centroid nor owned (possible only behind the error word) is flagged as its own root, so that the
// labelling stays inside its arrays, and raises the error word itself.
__global__ void __launch_bounds__(kClThreads)
k_bu_roots(const int32_t *__restrict__ state, const uint64_t *__restrict__ owner, int64_t N, int32_t *__restrict__ root,
           uint64_t *__restrict__ flags, int64_t W, unsigned long long *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool is_root = false;
  if (i < N) {
    const uint64_t o = owner[i];
    is_root = state[i] == kBuCentroid || o == ~0ull;
    if (state[i] != kBuCentroid && o == ~0ull) status[kClStatusErr] = 1ull;
    root[i] = is_root ? (int32_t)i : (int32_t)(o & 0xffffffffull);
  }
  const uint64_t m = __ballot(is_root);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < W) flags[i >> 6] = m;
}

// parallel rounds ahead of the finish (fc_tuning.h; FC_BUTINA_ROUNDS, read per call: the tests compare several values)
int bu_rounds() {
  long long r = kButinaRounds;
  if (const char *v = getenv("FC_BUTINA_ROUNDS")) {
    char *end = nullptr;
    const long long f = strtoll(v, &end, 10);
    if (end != v && *end == 0 && f >= 0) r = f;
  }
  return (int)std::min<long long>(r, kBuRoundsMax);
}

// everything behind the degrees, for either kind of edge source
template <class Src>
int bu_run(const ClWork &w, const Src &src, dim3 grid, int64_t N, size_t live_cap) {
  const unsigned long long cap = (unsigned long long)live_cap;
  hipLaunchKernelGGL(k_bu_keys, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.deg, N, w.key, w.owner, w.state, w.claim, w.stamp,
                     w.und, w.status);
  FC_TRY(check_launch("k_bu_keys"));
  const int R = bu_rounds();
  for (int r = 1; r <= R + 1; ++r) {
    const bool last = r == R + 1;
    hipLaunchKernelGGL(k_bu_edges<Src>, grid, dim3(kClThreads), 0, w.st, src, w.key, w.state, w.claim, w.stamp, w.und, r,
                       last ? w.live_e : nullptr, cap);
    FC_TRY(check_launch("k_bu_edges"));
    hipLaunchKernelGGL(k_bu_vertices, dim3(w.per_n), dim3(kClThreads), 0, w.st, N, w.state, w.claim, w.stamp, r, w.und,
                       last ? w.live_v : nullptr, w.status);
    FC_TRY(check_launch("k_bu_vertices"));
  }
  hipLaunchKernelGGL(k_bu_finish, dim3(1), dim3(kBuFinishThreads), 0, w.st, w.live_e, cap, w.state, w.claim, w.stamp, w.live_v,
                     w.und, R + 2, w.status);
  FC_TRY(check_launch("k_bu_finish"));
  hipLaunchKernelGGL(k_bu_finish_graph<Src>, dim3(1), dim3(kBuFinishThreads), 0, w.st, src, cap, w.key, w.state, w.claim,
                     w.stamp, w.live_v, w.und, R + 2, w.status);
  FC_TRY(check_launch("k_bu_finish_graph"));
  hipLaunchKernelGGL(k_bu_owners<Src>, grid, dim3(kClThreads), 0, w.st, src, w.key, w.state, w.owner);
  FC_TRY(check_launch("k_bu_owners"));
  hipLaunchKernelGGL(k_bu_roots, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.state, w.owner, N, w.root, w.flags, w.W, w.status);
  FC_TRY(check_launch("k_bu_roots"));
  hipLaunchKernelGGL(k_cl_scan, dim3(1), dim3(1024), 0, w.st, w.flags, w.W, w.prefix, w.status);
  FC_TRY(check_launch("k_cl_scan"));
  hipLaunchKernelGGL(k_cl_label, dim3(w.per_n), dim3(kClThreads), 0, w.st, w.root, N, w.flags, w.prefix, w.labels, w.reps, w.sizes);
  return check_launch("k_cl_label");
}

}  // namespace

// entries of the live-edge list: no more than the graph can have, at most kButinaLiveEdges (fc_tuning.h;
// FC_BUTINA_LIVE_CAP: test knob, forces the finish over the graph itself)
size_t butina_live_cap(const ClusterGraph &g, int64_t N) {
  const unsigned long long n = (unsigned long long)(N > 0 ? N : 1), all = n * (n - 1) / 2;
  unsigned long long bound = g.pairs_dev == nullptr ? all : (g.n_pairs_dev != nullptr ? g.cand_cap : g.n_pairs_host);
  bound = std::min<unsigned long long>(std::min(bound, all), (unsigned long long)kButinaLiveEdges);
  if (const char *v = getenv("FC_BUTINA_LIVE_CAP")) {
    char *end = nullptr;
    const long long f = strtoll(v, &end, 10);
    if (end != v && *end == 0 && f >= 1) bound = std::min<unsigned long long>(bound, (unsigned long long)f);
  }
  return (size_t)std::max<unsigned long long>(bound, 1ull);
}

// launch_clusters for the sphere-exclusion clusters
int launch_butina(const ClusterGraph &g, int64_t N, DevBuf &work) {
  ClWork w;
  const size_t live_cap = butina_live_cap(g, N);
  FC_TRY(cl_begin(g, N, kClButina, 1, work, &w, live_cap));
  if (g.pairs_dev != nullptr) {
    const unsigned long long *n_pairs_dev = g.n_pairs_dev != nullptr ? g.n_pairs_dev : w.status + kClStatusPairs;
    const dim3 grid = cl_grid_pairs();
    hipLaunchKernelGGL(k_db_degree_pairs, grid, dim3(kClThreads), 0, w.st, g.pairs_dev, n_pairs_dev, g.n_cand_dev, g.cand_cap,
                       g.redo_dev, N, w.deg, w.status);
    FC_TRY(check_launch("k_db_degree_pairs"));
    return bu_run(w, BuPairs{g.pairs_dev, n_pairs_dev, g.n_cand_dev, g.cand_cap, g.redo_dev, (uint32_t)N}, grid, N, live_cap);
  }
  if (g.W < w.W) return set_error(FC_E_INVALID, "bit rows of %lld words, %lld needed", (long long)g.W, (long long)w.W);
  hipLaunchKernelGGL(k_db_degree_bits, dim3((unsigned)w.W), dim3(kClThreads), 0, w.st, g.bits_dev, g.W, N, w.deg);
  FC_TRY(check_launch("k_db_degree_bits"));
  return bu_run(w, BuBits{g.bits_dev, g.W, N}, cl_grid_bits(N, g.W), N, live_cap);
}

__global__ void k_warm_clusters() {}
int warm_clusters() {
  hipLaunchKernelGGL(k_warm_clusters, dim3(1), dim3(64), 0, ctx().stream);
  return check_launch("k_warm_clusters");
}

}  // namespace fc
