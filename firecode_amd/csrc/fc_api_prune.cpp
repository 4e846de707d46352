// fc_api_prune.cpp -- the extern "C" surface (include/fc_hip.h) of every prune that ends in a mask: the similarity bits
// (plain, enantiomer- and symmetry-aware), the ladder in its device forms, the pipelines (staged, async, many, sharded)
// and their bench and debug hooks: argument checks, host<->HBM staging, kernel sequencing.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <memory>

#include "fc_internal.h"
#include "fc_kabsch_math.h"

namespace fc {

struct LadderKs {
  int n;
  int64_t k[24];
};
__global__ void k_store_ladder_ks(LadderKs a, int64_t *__restrict__ out) {
  if ((int)threadIdx.x < a.n) out[threadIdx.x] = a.k[threadIdx.x];
}

// rows of the bit matrix per workgroup (tuning knob FC_ROW_BLOCK, multiple of 128)
int64_t default_row_block() {
  const char *v = getenv("FC_ROW_BLOCK");
  if (v) {
    const long r = std::strtol(v, nullptr, 10);
    if (r >= 64 && r <= 4096 && r % 64 == 0) return r;
  }
  return 128;  // measured best on cfg2 (tail and balance beat the extra LDS fills)
}

// similarity bits of this rank's rows: screen + exact refine; counters[1..3]
int simbits_local(fc_ensemble *e, double max_rmsd, double max_dev, const double *energies,
                  double max_dE, bool zero_counters, bool lean) {
  e->lean = lean;
  const double *en_dev = nullptr;
  if (energies != nullptr) {
    FC_TRY(upload(e->energies, energies, (size_t)e->N));
    en_dev = e->energies.as<double>();
  }
  if (zero_counters)
    FC_HIP_TRY(hipMemsetAsync(e->counters.p, 0, kCounters * sizeof(uint64_t), ctx().stream));
  // HIP events bracket the screen kernel (the dominant one) on the library's stream
  FC_HIP_TRY(hipEventRecord(ctx().ev2, ctx().stream));
  ctx().mark_after_screen = ctx().ev3;  // recorded by the launcher right behind the screen kernel
  const int rc_screen = launch_simbits_screen(e, max_rmsd * max_rmsd + kScreenMargin);
  ctx().mark_after_screen = nullptr;
  FC_TRY(rc_screen);
  FC_TRY(launch_simbits_refine(e, max_rmsd, max_dev, en_dev, max_dE));
  e->bits_valid = true;
  return FC_OK;
}

// duration of the last screen kernel enqueued by simbits_local, after a sync
static int64_t last_screen_ns() {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ctx().ev2, ctx().ev3) != hipSuccess) {
    (void)hipGetLastError();  // (no screen has run in this process, the events were never recorded: the refusal must not
                              // stay behind for the next launch's check to find)
    return 0;
  }
  return (int64_t)(ms * 1e6);
}

static const int64_t kLadder[] = {500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000,
                                  500,    200,    100,    50,    20,    10,    5,    2,    1};

// whole ladder on one device (world == 1), enqueued without host round trips:
// one fused launch per ladder value that can still apply (the first ones are
// ruled out on the host from N alone), one sync at the end.
// pairs_dev != nullptr: a device list of the exactly-similar pairs whose length is the device
// counter counters[2] (refine output; complete iff counters[6] <= pairq_cap) or, with
// pairs_are_final, counters[2] alone (list uploaded by the caller).  Then the one-launch
// k_ladder_pairs runs first and the bit-matrix levels behind it return at once.
static const unsigned long long kPairLadderCap = 1ull << 20;
// the one-launch pair ladder keeps two masks of W words in LDS
static bool fits_pair_ladder(int64_t W) { return (size_t)2 * W * sizeof(uint64_t) <= 60 * 1024; }

// Pinned result slots of the ladder (Context::pinned): n slots of `stride` words -- the W mask words of a prune, then the
// 16 counters the ladder kernel wrote behind them (stride 0: W + 16; larger when the prunes of a batch differ in size) --
// and behind the n slots, for the prunes over gathered lists, 8 words per slot of that rank's own counters
static uint64_t *slot_words(int64_t slot, int64_t W, int64_t stride = 0) {
  return static_cast<uint64_t *>(ctx().pinned) + (size_t)slot * (size_t)(stride > 0 ? stride : W + 16);
}
static uint64_t *slot_counters(int64_t slot, int64_t W, int64_t stride = 0) { return slot_words(slot, W, stride) + W; }
static unsigned long long *slot_local_counters(int64_t slot, int64_t n_slots, int64_t W) {
  return reinterpret_cast<unsigned long long *>(slot_words(n_slots, W)) + (size_t)slot * 8;
}
static size_t slot_bytes(int64_t n_slots, int64_t W) { return (size_t)n_slots * (size_t)(W + 16 + 8) * sizeof(uint64_t); }

// what a ladder takes beside the ensemble and what it hands back; every field is optional
struct LadderJob {
  const uint64_t *bits_dev = nullptr;   // bit matrix for the level-by-level form (dense similarity / no pair list)
  const uint64_t *pairs_dev = nullptr;  // device list of the exactly-similar pairs (see ladder_single)
  bool pairs_are_final = false;         // the list is complete as it stands (uploaded or gathered by the caller): no candidate count to check
  // where the list's length stands on the device (nullptr: counters[2]).  A caller's own list brings a word of its own:
  // counters[2] stays the length of the ensemble's simq, which fc_prune_similar_pairs and the export read afterwards
  const unsigned long long *n_pairs_dev = nullptr;
  bool counters_zeroed = false;         // counters[8 ..) are already zero on the stream
  // which device form of the ladder runs: -1 the prune's own choice (below); 0 the bit-matrix levels, 1 the one-workgroup
  // pair ladder, 2 the launch-per-level pair ladder -- exactly that one or FC_E_LIMIT (fc_debug_ladder_from_pairs)
  int form = -1;
  unsigned many_grid = 0;               // workgroups per level launch of form 2 (0: ladder_many_grid())
  int64_t defer_slot = -1, slot_stride = 0;
  uint8_t *mask_out = nullptr;
  int64_t *levels = nullptr, *survivors = nullptr;
  unsigned long long *counters_out = nullptr;  // counters[0..8)
};

// mask words and the counters behind them -> the outputs of a LadderJob
static void unpack_ladder_result(const fc_ensemble *e, const uint64_t *words, const uint64_t *cnt_host, uint8_t *mask_out,
                                 int64_t *levels, int64_t *survivors, unsigned long long *counters_out) {
  const int64_t N = e->N, W = e->W;
  int64_t alive = 0;
  for (int64_t w = 0; w < W; ++w) alive += __builtin_popcountll(words[w]);
  if (mask_out)
    for (int64_t i = 0; i < N; ++i) mask_out[i] = (uint8_t)((words[(size_t)(i >> 6)] >> (i & 63)) & 1ull);
  if (levels) *levels = (int64_t)cnt_host[8];
  if (survivors) *survivors = alive;
  if (counters_out)
    for (int k = 0; k < 8; ++k) counters_out[k] = cnt_host[k];
}

static int ladder_single(fc_ensemble *e, int64_t min_per_group, const LadderJob &job) {
  // defer_slot >= 0: enqueue the pair ladder and the copy of its result into slot `defer_slot` of
  // the pinned staging area and return WITHOUT waiting (the caller synchronises once for many
  // prunes and reads the slots with ladder_collect; pinned memory for all slots is the caller's;
  // slot_stride: words per slot when the prunes differ in size, default W + 16)
  const uint64_t *const pairs_dev = job.pairs_dev;
  const int64_t defer_slot = job.defer_slot;
  const int64_t N = e->N, W = e->W;
  const int n_ladder = (int)(sizeof(kLadder) / sizeof(kLadder[0]));
  FC_TRY(e->ladder.reserve(((size_t)(n_ladder + 1) * W + 16) * sizeof(uint64_t)));
  if (defer_slot < 0) FC_TRY(pinned_reserve((size_t)(W + 16) * sizeof(uint64_t)));
  uint64_t *mb = e->ladder.as<uint64_t>();
  auto *cnt = reinterpret_cast<unsigned long long *>(e->counters.p);
  const unsigned long long *const n_pairs_dev = job.n_pairs_dev ? job.n_pairs_dev : cnt + 2;
  // ladder values that can ever run (n_active <= N) -- decided here, the rest on the device
  std::vector<int64_t> ks;
  for (int64_t k : kLadder)
    if (k == 1 || min_per_group * k < N) ks.push_back(k);
  const int n_lv = (int)ks.size();
  // counters[8] = levels run, counters[9] = "k_ladder_pairs produced the mask"
  // [8], [9]: ladder flags; [10], [11]: spare; [16 ..): bucket fill levels of the pair ladder
  if (!job.counters_zeroed) FC_HIP_TRY(hipMemsetAsync(cnt + 8, 0, (kCounters - 8) * sizeof(uint64_t), ctx().stream));
  uint64_t *words = slot_words(std::max<int64_t>(defer_slot, 0), W, job.slot_stride);
  uint64_t *cnt_host = words + W;
  bool have_mask = false;
  const bool pair_form_asked = job.form == 1 || job.form == 2;
  if (pair_form_asked && (pairs_dev == nullptr || !fits_pair_ladder(W)))
    return set_error(FC_E_LIMIT, "N = %lld: the pair ladder keeps two masks of %lld words in LDS, 3840 words at the most",
                     (long long)N, (long long)W);
  if (pairs_dev != nullptr && fits_pair_ladder(W) && job.form != 0) {
    // sparse similarity (the usual case): the whole ladder is ONE launch over the pair list
    // the values that can run at this N are a suffix of kLadder: they sit on the device once per context (a launch of
    // k_store_ladder_ks per fresh ensemble -- every drop-in call -- was 5 us of an otherwise empty device)
    const int64_t *ks_dev = nullptr;
    {
      bool suffix = n_lv >= 1 && n_lv <= n_ladder;
      for (int q = 0; suffix && q < n_lv; ++q) suffix = ks[(size_t)q] == kLadder[n_ladder - n_lv + q];
      Context &c = ctx();
      if (suffix && c.ladder_all == nullptr) {
        if (hipMalloc(reinterpret_cast<void **>(&c.ladder_all), sizeof kLadder) == hipSuccess) {
          // (a blocking copy, once per context: the first ladder may run on a lane of a pipeline, whose other lanes must not
          // find the values still in flight)
          if (hipMemcpy(c.ladder_all, kLadder, sizeof kLadder, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(c.ladder_all);
            c.ladder_all = nullptr;
          }
        } else {
          (void)hipGetLastError();
          c.ladder_all = nullptr;
        }
      }
      if (suffix && c.ladder_all != nullptr) ks_dev = c.ladder_all + (n_ladder - n_lv);
    }
    if (ks_dev == nullptr && (e->ladder_k_n != n_lv || e->ladder_k_mpg != min_per_group)) {
      // the source of the (asynchronous) copy lives with the ensemble: no host wait here -- a wait at this point sat
      // between the refine and the ladder of every drop-in call (each creates its ensemble) and cost it ~45 us
      // (the values travel as kernel arguments: an asynchronous copy out of a pageable vector could be overtaken by the next
      // prune's reassignment of that vector, or by the ensemble's destruction)
      e->ladder_k_host = ks;
      FC_TRY(e->ladder_k.reserve(ks.size() * sizeof(int64_t)));
      LadderKs args{};
      args.n = (int)std::min<size_t>(ks.size(), 24);
      for (int q = 0; q < args.n; ++q) args.k[q] = ks[(size_t)q];
      hipLaunchKernelGGL(k_store_ladder_ks, dim3(1), dim3(32), 0, ctx().stream, args, e->ladder_k.as<int64_t>());
      FC_TRY(check_launch("k_store_ladder_ks"));
      e->ladder_k_n = n_lv;
      e->ladder_k_mpg = min_per_group;
    }
    // level buckets: one per level, each as long as the longest list the ladder accepts
    const unsigned long long ladder_cap =
        std::min<unsigned long long>(kPairLadderCap, std::max<unsigned long long>(1024, (unsigned long long)N * (N - 1) / 2));
    FC_TRY(e->levelmask.reserve((size_t)ladder_cap * (size_t)n_lv * sizeof(uint64_t)));
    // long lists: a launch per level over the whole chip instead of one workgroup (fc_prune.hip); a host decision from
    // the last similar-pair count seen for these coordinates -- either form is correct for any list
    static const bool many_ok = [] {
      const char *v = getenv("FC_LADDER_MANY");  // 0: always the one-workgroup ladder
      return !(v && atoi(v) == 0);
    }();
    const bool many = pair_form_asked ? job.form == 2 : many_ok && n_lv >= 2 && e->last_similar > ((int64_t)1 << 17);
    // (the two masks of the launch-per-level form sit in the first 2 W words: its result goes behind them also when k = 1
    // is the only level, which the prunes never send there)
    uint64_t *const result_dev = mb + (size_t)std::max(n_lv, 2) * W;
    if (many)
      FC_TRY(launch_ladder_pairs_many(pairs_dev, e->levelmask.as<uint64_t>(), n_pairs_dev, job.pairs_are_final ? nullptr : cnt + 6,
                                      (unsigned long long)e->pairq_cap, ladder_cap, N, W, min_per_group,
                                      ks_dev ? ks_dev : e->ladder_k.as<int64_t>(), ks.data(), n_lv, mb, result_dev, cnt,
                                      job.many_grid ? job.many_grid : ladder_many_grid()));
    else
      FC_TRY(launch_ladder_pairs(pairs_dev, e->levelmask.as<uint64_t>(), n_pairs_dev,
                                 job.pairs_are_final ? nullptr : cnt + 6,
                                 (unsigned long long)e->pairq_cap, ladder_cap, N, W, min_per_group,
                                 ks_dev ? ks_dev : e->ladder_k.as<int64_t>(), n_lv, result_dev, cnt));
    // mask words and the 16 counters behind them (written by the kernel): one copy
    FC_TRY(d2h(words, result_dev, (size_t)(W + 16) * sizeof(uint64_t)));
    if (defer_slot >= 0) return FC_OK;
    FC_TRY(sync());
    have_mask = cnt_host[9] != 0;
    if (pair_form_asked && !have_mask)
      return set_error(FC_E_LIMIT, "the pair ladder declined the list: more than %llu entries", ladder_cap);
  }
  if (defer_slot >= 0) return set_error(FC_E_INVALID, "deferred ladder needs the pair list");
  if (!have_mask) {
    // dense similarity / no pair list: one fused launch per level over the bit matrix
    if (prune_drop_later())
      return set_error(FC_E_INVALID, "fc_prune_conventions(drop_later = 1) is implemented by the pair ladder only; "
                       "this prune needs the bit-matrix levels (dense similarity or no pair list)");
    if (job.bits_dev == nullptr) return set_error(FC_E_LIMIT, "pair list too long for the one-launch ladder and no bit matrix given");
    FC_TRY(launch_mask_init(mb, N, W, (int64_t)(n_lv + 1) * W));
    int cur = 0;
    for (int64_t k : ks) {
      FC_TRY(launch_level_fused(job.bits_dev, W, mb + (size_t)cur * W, mb + (size_t)(cur + 1) * W, N, k,
                                min_per_group, cnt));
      ++cur;
    }
    FC_TRY(d2h(words, mb + (size_t)n_lv * W, (size_t)W * sizeof(uint64_t)));
    FC_TRY(d2h(cnt_host, cnt, 16 * sizeof(uint64_t)));
    FC_TRY(sync());
  }
  unpack_ladder_result(e, words, cnt_host, job.mask_out, job.levels, job.survivors, job.counters_out);
  return FC_OK;
}

// result of a deferred pair ladder (after the caller's synchronisation); false: the kernel
// declined (queue overflow / list too long) and the prune has to be redone synchronously
// what a finished prune says about the length of this ensemble's candidate queue -> every workspace over its coordinates
void note_candidates(fc_ensemble *e, unsigned long long refined, unsigned long long similar) {
  // (every workspace of the chain, whichever lane the prune ran on: the choice of the refine's and the ladder's form must not
  // depend on which lane finished last)
  int guard = 0;
  for (fc_ensemble *w = e->head ? e->head : e; w != nullptr && guard < 8; w = w->twin, ++guard) {
    w->last_candidates = (int64_t)refined;
    w->last_similar = (int64_t)similar;
  }
  Context &c = ctx();
  c.hint_A = e->A, c.hint_N = e->N, c.hint_candidates = (int64_t)refined, c.hint_similar = (int64_t)similar;
}

static bool ladder_collect(fc_ensemble *e, int64_t slot, uint8_t *mask_out, int64_t *levels,
                           int64_t *survivors, unsigned long long *counters_out, int64_t slot_stride = 0) {
  const uint64_t *words = slot_words(slot, e->W, slot_stride), *cnt_host = slot_counters(slot, e->W, slot_stride);
  note_candidates(e, cnt_host[6], cnt_host[2]);  // (pairs the screen queued; valid also when the ladder declined)
  if (cnt_host[9] == 0) return false;
  unpack_ladder_result(e, words, cnt_host, mask_out, levels, survivors, counters_out);
  return true;
}

static int64_t owned_pairs(const fc_ensemble *ens) { return owned_pairs(ens->N, ens->row_block, ens->rank, ens->world); }

// stats[0..5] of a prune: pairs looked at, candidates / similar / grey pairs from the counters, and two slots whose
// meaning belongs to the entry point (include/fc_hip.h)
void fill_stats(int64_t *stats, int64_t pairs, const unsigned long long *cnt, int64_t s4, int64_t s5) {
  stats[0] = pairs, stats[1] = (int64_t)cnt[1], stats[2] = (int64_t)cnt[2], stats[3] = (int64_t)cnt[3];
  stats[4] = s4, stats[5] = s5;
}

// the bare ladder workspace over a bit matrix that is not the RMSD screen's (the caller's bits, MOI, rot-corr)
// (with_bits = false: the pair ladders alone, which need no bit matrix)
static int ladder_workspace(fc_ensemble *e, int64_t N, size_t *bits_bytes = nullptr, bool with_bits = true) {
  e->N = N, e->Npad = ceil_div(N, 64) * 64, e->W = e->Npad / 64;
  e->row_block = 64;
  FC_TRY(e->maskA.reserve((size_t)e->Npad));
  FC_TRY(e->maskB.reserve((size_t)e->Npad));
  FC_TRY(e->mbits.reserve((size_t)e->W * sizeof(uint64_t)));
  FC_TRY(e->counters.reserve(kCounters * sizeof(uint64_t)));
  // rows padded to a multiple of the row block so k_level's local row == global row
  const int64_t rows = ceil_div(N, e->row_block) * e->row_block;
  const size_t bytes = (size_t)rows * e->W * sizeof(uint64_t);
  if (bits_bytes) *bits_bytes = bytes;
  return with_bits ? e->bits.reserve(bytes) : FC_OK;
}

// principal moments of coordinates that are already on the device
static int moi_moments(const double *coords_dev, int64_t N, int64_t A, const double *masses, DevBuf &dm, DevBuf &dmom) {
  FC_TRY(upload(dm, masses, (size_t)A));
  FC_TRY(dmom.reserve((size_t)N * 3 * sizeof(double)));
  return launch_inertia_moments(coords_dev, N, A, dm.as<double>(), dmom.as<double>());
}

// the MOI stage: moments -> similarity bits -> ladder
static int moi_stage(const double *coords_dev, int64_t N, int64_t A, const double *masses, double tol, const double *energies,
                     double max_dE, int64_t min_per_group, uint8_t *mask_out) {
  fc_ensemble e;
  FC_TRY(ladder_workspace(&e, N));
  DevBuf dm, dmom;
  const double *en_dev = nullptr;
  if (energies) {
    FC_TRY(upload(e.energies, energies, (size_t)N));
    en_dev = e.energies.as<double>();
  }
  FC_TRY(moi_moments(coords_dev, N, A, masses, dm, dmom));
  FC_TRY(launch_moi_simbits(dmom.as<double>(), N, tol, en_dev, max_dE, e.bits.as<uint64_t>(), e.W));
  LadderJob job;
  job.bits_dev = e.bits.as<uint64_t>(), job.mask_out = mask_out;
  return ladder_single(&e, min_per_group, job);
}

// puts the context's stream back when a multi-stream region ends, also on its error paths
struct StreamRestore {
  Context &c;
  hipStream_t s;
  ~StreamRestore() { c.stream = s; }
};

// the pipelines time the screen kernel of every stride-th prune only (read once per process)
static int64_t bench_event_stride() {
  static const int64_t stride_ev = [] {
    const char *v = getenv("FC_BENCH_EVENT_STRIDE");
    const long k = v ? std::strtol(v, nullptr, 10) : 8;
    return (int64_t)(k >= 1 && k <= 4096 ? k : 8);
  }();
  return stride_ev;
}

// bits, similar-pair queue and counters of the whole ensemble under similar_sym; `dperm` lives until the caller's wait
int symm_local(fc_ensemble *e, const std::vector<uint16_t> &table, int64_t K, DevBuf &dperm, double max_rmsd, double max_dev,
               const double *energies, double max_dE) {
  FC_TRY(ensemble_shard(e, 0, 1, default_row_block()));
  e->lean = false;
  const double *en_dev = nullptr;
  if (energies != nullptr) {
    FC_TRY(upload(e->energies, energies, (size_t)e->N));
    en_dev = e->energies.as<double>();
  }
  FC_TRY(upload(dperm, table.data(), table.size()));
  FC_HIP_TRY(hipMemsetAsync(e->counters.p, 0, kCounters * sizeof(uint64_t), ctx().stream));
  FC_TRY(launch_symm_simbits(e, dperm.as<uint16_t>(), K, max_rmsd, max_dev, en_dev, max_dE));
  e->bits_valid = true;
  return FC_OK;
}

static int prune_rmsd_perm_run(fc_ensemble *ens, const std::vector<uint16_t> &table, int64_t K, DevBuf &dperm,
                               double max_rmsd, double max_dev, const double *energies, double max_dE,
                               int64_t min_per_group, uint8_t *mask_out, int64_t *stats) {
  FC_TRY(symm_local(ens, table, K, dperm, max_rmsd, max_dev, energies, max_dE));
  // the pair ladder over the queue; it declines a queue that overflowed or is too long for it, and the bit-matrix levels
  // take over from the matrix the same launch wrote
  unsigned long long cnt[8];
  int64_t levels = 0, survivors = 0;
  LadderJob job;
  job.pairs_dev = ens->simq.as<uint64_t>(), job.bits_dev = ens->bits.as<uint64_t>(), job.counters_zeroed = true;
  job.mask_out = mask_out, job.levels = &levels, job.survivors = &survivors, job.counters_out = cnt;
  FC_TRY(ladder_single(ens, min_per_group, job));
  if (stats) fill_stats(stats, ens->N * (ens->N - 1) / 2, cnt, levels, survivors);
  return FC_OK;
}

}  // namespace fc

using namespace fc;

extern "C" {

// ---- a5 ------------------------------------------------------------------------
int fc_rmsd_simbits(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies,
                    double max_dE, int64_t row_begin, int64_t row_end, uint64_t *bits_out,
                    int64_t *n_grey) {
  FC_API_LOCK;
  FC_REQUIRE(ens && bits_out, "NULL pointer argument");
  FC_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= ens->N, "bad row range");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  FC_TRY(ensemble_shard(ens, 0, 1, default_row_block()));
  FC_TRY(simbits_local(ens, max_rmsd, max_dev, energies, max_dE, true));
  const int64_t W = ens->W;
  std::vector<uint64_t> all((size_t)ens->rows_local * W);
  unsigned long long cnt[8];
  FC_TRY(d2h(all.data(), ens->bits.p, all.size() * sizeof(uint64_t)));
  FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
  FC_TRY(sync());
  note_candidates(ens, cnt[6], cnt[2]);
  // words at or below the diagonal were never produced: define them as 0
  for (int64_t i = row_begin; i < row_end; ++i)
    for (int64_t w = 0; w < W; ++w)
      bits_out[(i - row_begin) * W + w] = (w * 64 + 63 > i) ? all[(size_t)i * W + w] : 0ull;
  if (n_grey) *n_grey = (int64_t)cnt[3];
  return FC_OK;
}

int fc_prune_rmsd(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies,
                  double max_dE, int64_t min_per_group, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && mask_out, "NULL pointer argument");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_REQUIRE(min_per_group >= 1, "min_per_group must be >= 1");
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  FC_TRY(ensemble_shard(ens, 0, 1, default_row_block()));
  // lean first: only the pair lists (no bit matrix); the pair ladder declines when the candidate
  // queue overflowed or the list is too long for it -- then the same prune again with the bits
  FC_TRY(simbits_local(ens, max_rmsd, max_dev, energies, max_dE, true, /*lean=*/true));
  unsigned long long cnt[8];
  int64_t levels = 0, survivors = 0;
  LadderJob job;
  job.pairs_dev = ens->simq.as<uint64_t>(), job.counters_zeroed = true;
  job.mask_out = mask_out, job.levels = &levels, job.survivors = &survivors, job.counters_out = cnt;
  int rc = ladder_single(ens, min_per_group, job);
  if (rc == FC_E_LIMIT) {
    FC_TRY(simbits_local(ens, max_rmsd, max_dev, energies, max_dE, true, /*lean=*/false));
    job.bits_dev = ens->bits.as<uint64_t>();
    rc = ladder_single(ens, min_per_group, job);
  }
  FC_TRY(rc);
  note_candidates(ens, cnt[6], cnt[2]);
  if (stats) fill_stats(stats, ens->N * (ens->N - 1) / 2, cnt, levels, survivors);
  return FC_OK;
}

// ---- enantiomer-aware forms (include/fc_hip.h): the same entry points under an EnantScope ----------------------------
int fc_rmsd_simbits_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                          int64_t row_begin, int64_t row_end, uint64_t *bits_out, int64_t *n_grey) {
  FC_API_LOCK;
  FC_REQUIRE(ens && bits_out, "NULL pointer argument");
  EnantScope scope(ens);
  return fc_rmsd_simbits(ens, max_rmsd, max_dev, energies, max_dE, row_begin, row_end, bits_out, n_grey);
}

int fc_prune_rmsd_enant(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies, double max_dE,
                        int64_t min_per_group, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && mask_out, "NULL pointer argument");
  EnantScope scope(ens);
  return fc_prune_rmsd(ens, max_rmsd, max_dev, energies, max_dE, min_per_group, mask_out, stats);
}

// prune_by_rmsd(host arrays) as ONE call (firecode/ensemble.py:230-235, firecode/embedder.py:1472-1474): upload, preparation,
// prune, mask -- what a caller got from fc_ensemble_create + fc_prune_rmsd + fc_ensemble_destroy, under one lock and with
// one crossing of the language boundary
int fc_prune_rmsd_host(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask, int center, double max_rmsd,
                       double max_dev, const double *energies, double max_dE, int64_t min_per_group, uint8_t *mask_out,
                       int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape N=%lld A=%lld", (long long)N, (long long)A);
  FC_REQUIRE(A <= 32767, "A=%lld exceeds 32767 atoms", (long long)A);
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_REQUIRE(min_per_group >= 1, "min_per_group must be >= 1");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords != nullptr && mask_out != nullptr, "NULL pointer argument");
  FC_TRY(ensure_init());
  fc_ensemble e;
  e.epoch = ctx().epoch;
  // the last piece's DMA and the preparation kernel are still running when ensemble_build returns: the prune's reserves and
  // the screen's item table (host work + one small copy) go under them instead of behind the wait for the largest G
  // a small ensemble: the largest G from the caller's array, no copy of the device's and no wait for it (the counters are
  // reset in front of the screen)
  const bool host_gmax = N * A * 3 <= kHostGmaxDoubles;
  int rc = ensemble_build(coords, N, A, atom_mask, center, &e, /*defer_wait=*/true, host_gmax);
  if (rc == FC_OK && host_gmax) {
    const double g = host_largest_g(coords, N, A, e.sel_host, center);
    e.g_max = std::isfinite(g) ? g * (1.0 + 1e-12) : g;  // (not finite: every screen that needs it declines, as with the device's)
  }
  if (rc == FC_OK) rc = ensemble_shard(&e, 0, 1, default_row_block());
  if (rc == FC_OK) rc = prebuild_screen_items(&e);
  const int rc_fin = ensemble_build_finish(&e);  // (always: nothing of `e` may be in flight when it goes out of scope)
  if (rc != FC_OK || rc_fin != FC_OK) return drained(rc != FC_OK ? rc : rc_fin);
  return fc_prune_rmsd(&e, max_rmsd, max_dev, energies, max_dE, min_per_group, mask_out, stats);
}

int fc_greedy_prune_from_bits(const uint64_t *bits, int64_t N, int64_t min_per_group,
                              uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && min_per_group >= 1, "bad arguments");
  if (N == 0) return FC_OK;
  FC_REQUIRE(bits && mask_out, "NULL pointer argument");
  FC_TRY(ensure_init());
  fc_ensemble e;
  FC_TRY(ladder_workspace(&e, N));
  FC_TRY(h2d(e.bits.p, bits, (size_t)N * e.W * sizeof(uint64_t)));
  LadderJob job;
  job.bits_dev = e.bits.as<uint64_t>(), job.mask_out = mask_out;
  return ladder_single(&e, min_per_group, job);
}

// test hook: the ladder over a caller's pair list in ONE chosen device form (include/fc_hip.h)
int fc_debug_ladder_from_pairs(const uint64_t *pairs, int64_t n_pairs, int64_t N, int64_t min_per_group, int form,
                               int64_t grid, uint8_t *mask_out, int64_t *levels_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 1 && N <= (int64_t)INT32_MAX && n_pairs >= 0 && min_per_group >= 1, "bad arguments");
  FC_REQUIRE(mask_out && (pairs || n_pairs == 0), "NULL pointer argument");
  FC_REQUIRE(form >= 0 && form <= 2, "form %d: 0 (bit-matrix levels), 1 (one-workgroup pair ladder) or 2 (launch per level)", form);
  FC_REQUIRE(form != 2 || (grid >= 1 && grid <= kLadderManyGridMax), "grid %lld outside [1, %ld]", (long long)grid,
             kLadderManyGridMax);
  FC_TRY(ensure_init());
  fc_ensemble e;
  size_t bits_bytes = 0;
  FC_TRY(ladder_workspace(&e, N, &bits_bytes, /*with_bits=*/form == 0));
  auto *cnt = reinterpret_cast<unsigned long long *>(e.counters.p);
  DevBuf dp;
  FC_TRY(upload(dp, pairs, (size_t)n_pairs));
  LadderJob job;
  job.mask_out = mask_out, job.levels = levels_out, job.form = form, job.many_grid = (unsigned)grid;
  if (form == 0) {
    FC_HIP_TRY(hipMemsetAsync(e.bits.p, 0, bits_bytes, ctx().stream));
    FC_TRY(launch_scatter_pairs(dp.as<uint64_t>(), n_pairs, N, e.W, e.bits.as<uint64_t>()));
    job.bits_dev = e.bits.as<uint64_t>();
  } else {
    const unsigned long long np = (unsigned long long)n_pairs;
    FC_TRY(h2d(cnt + 2, &np, sizeof np));  // (the pair ladders read the list's length from counters[2])
    job.pairs_dev = dp.as<uint64_t>(), job.pairs_are_final = true;
  }
  return ladder_single(&e, min_per_group, job);
}

// ---- symmetry-aware forms (include/fc_hip.h; the kernels: fc_symm.hip) -----------------------------------------------
int fc_rmsd_simbits_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                         const double *energies, double max_dE, int64_t row_begin, int64_t row_end, uint64_t *bits_out,
                         int64_t *n_grey) {
  FC_API_LOCK;
  std::vector<uint16_t> table;
  FC_TRY(perm_table_check(perms, K, A_sel, table));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, true));
  FC_REQUIRE(bits_out != nullptr, "NULL pointer argument");
  FC_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= ens->N, "bad row range");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  DevBuf dperm;
  const int64_t W = ens->W;
  std::vector<uint64_t> all;
  unsigned long long cnt[8];
  const auto run = [&]() -> int {
    FC_TRY(symm_local(ens, table, K, dperm, max_rmsd, max_dev, energies, max_dE));
    all.resize((size_t)ens->rows_local * W);
    FC_TRY(d2h(all.data(), ens->bits.p, all.size() * sizeof(uint64_t)));
    FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
    return sync();
  };
  FC_TRY(drained(run()));
  for (int64_t i = row_begin; i < row_end; ++i)
    for (int64_t w = 0; w < W; ++w) bits_out[(i - row_begin) * W + w] = all[(size_t)i * W + w];
  if (n_grey) *n_grey = (int64_t)cnt[3];
  return FC_OK;
}

int fc_prune_rmsd_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, double max_rmsd, double max_dev,
                       const double *energies, double max_dE, int64_t min_per_group, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  std::vector<uint16_t> table;
  FC_TRY(perm_table_check(perms, K, A_sel, table));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, true));
  FC_REQUIRE(mask_out != nullptr, "NULL pointer argument");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_REQUIRE(min_per_group >= 1, "min_per_group must be >= 1");
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  DevBuf dperm;
  return drained(prune_rmsd_perm_run(ens, table, K, dperm, max_rmsd, max_dev, energies, max_dE, min_per_group, mask_out, stats));
}

int fc_prune_rmsd_begin(fc_ensemble *ens, double max_rmsd, double max_dev, const double *energies,
                        double max_dE, int64_t rank, int64_t world, int64_t row_block,
                        int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_TRY(ensure_init());
  FC_TRY(ensemble_shard(ens, rank, world, row_block));
  if (ens->N == 0) return FC_OK;
  FC_TRY(simbits_local(ens, max_rmsd, max_dev, energies, max_dE, true));
  unsigned long long cnt[8];
  FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
  FC_TRY(sync());
  if (stats) fill_stats(stats, owned_pairs(ens), cnt, last_screen_ns() /* screen-kernel duration (ns) of this rank */, 0);
  return FC_OK;
}

int fc_prune_level(fc_ensemble *ens, int64_t k, const uint8_t *mask_in, uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(ens && mask_in && mask_out, "NULL pointer argument");
  FC_REQUIRE(ens->bits_valid && !ens->lean, "fc_prune_rmsd_begin has not been called on this ensemble");
  FC_REQUIRE(k >= 1, "k must be >= 1");
  FC_TRY(ensure_init());
  const int64_t N = ens->N;
  if (N == 0) return FC_OK;
  auto *cnt = reinterpret_cast<unsigned long long *>(ens->counters.p);
  FC_TRY(h2d(ens->maskA.p, mask_in, (size_t)N));
  FC_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(uint64_t), ctx().stream));
  FC_TRY(launch_pack_mask(ens->maskA.as<uint8_t>(), N, ens->mbits.as<uint64_t>(), ens->W, cnt));
  FC_TRY(launch_copy_bytes(ens->maskA.as<uint8_t>(), ens->maskB.as<uint8_t>(), N));
  FC_TRY(launch_level(ens->bits.as<uint64_t>(), ens->W, ens->mbits.as<uint64_t>(),
                      ens->maskA.as<uint8_t>(), ens->maskB.as<uint8_t>(), N, k, ens->row_block,
                      ens->rank, ens->world, ens->rows_local));
  FC_TRY(d2h(mask_out, ens->maskB.p, (size_t)N));
  return sync();
}

int fc_prune_similar_pairs(fc_ensemble *ens, uint64_t *pairs_out, int64_t capacity, int64_t *n_out) {
  FC_API_LOCK;
  FC_REQUIRE(ens && n_out, "NULL pointer argument");
  FC_REQUIRE(ens->bits_valid, "fc_prune_rmsd_begin has not been called on this ensemble");
  FC_TRY(ensure_init());
  *n_out = 0;
  if (ens->N == 0) return FC_OK;
  unsigned long long cnt[8];
  FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
  FC_TRY(sync());
  if ((int64_t)cnt[6] > ens->pairq_cap)
    return set_error(FC_E_LIMIT, "candidate queue overflow (%llu > %lld): similar-pair list unavailable",
                     cnt[6], (long long)ens->pairq_cap);
  *n_out = (int64_t)cnt[2];
  if (pairs_out == nullptr) return FC_OK;  // size query
  FC_REQUIRE(capacity >= (int64_t)cnt[2], "pairs_out holds %lld entries, %llu needed", (long long)capacity, cnt[2]);
  FC_TRY(d2h(pairs_out, ens->simq.p, (size_t)cnt[2] * sizeof(uint64_t)));
  return sync();
}

int fc_prune_from_pairs(fc_ensemble *ens, const uint64_t *pairs, int64_t n_pairs,
                        int64_t min_per_group, uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(ens && mask_out && (pairs || n_pairs == 0), "NULL pointer argument");
  FC_REQUIRE(n_pairs >= 0 && min_per_group >= 1, "bad arguments");
  FC_TRY(ensure_init());
  const int64_t N = ens->N, W = ens->W;
  if (N == 0) return FC_OK;
  FC_TRY(ens->counters.reserve(kCounters * sizeof(uint64_t)));
  DevBuf dp, dn;
  FC_TRY(upload(dp, pairs, (size_t)n_pairs));
  // the length of the caller's list travels in a word of its own: counters[2] is the length of this ensemble's simq (the
  // list fc_prune_similar_pairs and fc_prune_export_pairs_dev hand out), which a prune from another list must not change
  const unsigned long long np = (unsigned long long)n_pairs;
  FC_TRY(upload(dn, &np, 1));
  LadderJob job;
  job.mask_out = mask_out;
  if (np <= kPairLadderCap && fits_pair_ladder(W)) {  // sparse: one launch over the pair list; no bit matrix needed
    job.pairs_dev = dp.as<uint64_t>(), job.pairs_are_final = true, job.n_pairs_dev = dn.as<unsigned long long>();
    return ladder_single(ens, min_per_group, job);
  }
  // dense: rebuild the whole bit matrix (rows padded like ladder_single expects) and run the levels
  const int64_t rb = ens->row_block > 0 ? ens->row_block : 64;
  const size_t bytes = (size_t)(ceil_div(N, rb) * rb) * W * sizeof(uint64_t);
  FC_TRY(ens->bits_full.reserve(bytes));
  FC_HIP_TRY(hipMemsetAsync(ens->bits_full.p, 0, bytes, ctx().stream));
  FC_TRY(launch_scatter_pairs(dp.as<uint64_t>(), n_pairs, N, W, ens->bits_full.as<uint64_t>()));
  job.bits_dev = ens->bits_full.as<uint64_t>();
  return ladder_single(ens, min_per_group, job);
}

// ---- device-resident exchange (no host round trip between screen and mask) --------------
int fc_prune_rmsd_begin_async(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t rank,
                              int64_t world, int64_t row_block) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_TRY(ensure_init());
  FC_TRY(ensemble_shard(ens, rank, world, row_block));
  if (ens->N == 0) return FC_OK;
  return simbits_local(ens, max_rmsd, max_dev, nullptr, 0.0, true, /*lean=*/true);  // consumer: the exported pair list
}

// counters reset on the current stream (behind the last user of this workspace), the screen on
// `scr` (behind the previous screen), the refine back on the current stream; ev_a / ev_b (may be
// null): timing events recorded right around the main screen kernel
static int begin_split(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t rank, int64_t world,
                       int64_t row_block, hipStream_t scr, hipEvent_t ev_a, hipEvent_t ev_b) {
  FC_TRY(ensemble_shard(ens, rank, world, row_block));
  if (ens->N == 0) return FC_OK;
  Context &c = ctx();
  FC_TRY(side_streams());
  hipStream_t const tail = c.stream;
  StreamRestore restore{c, tail};
  FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, kCounters * sizeof(uint64_t), tail));
  FC_HIP_TRY(hipEventRecord(c.ev_reset, tail));
  FC_HIP_TRY(hipStreamWaitEvent(scr, c.ev_reset, 0));
  ens->lean = true;  // consumer: the exported pair list
  c.stream = scr;
  if (ev_a) FC_HIP_TRY(hipEventRecord(ev_a, scr));  // the pair costs the stream ~14 us: not every step needs it
  c.mark_after_screen = ev_a ? ev_b : nullptr;
  const int rc_screen = launch_simbits_screen(ens, max_rmsd * max_rmsd + kScreenMargin);
  c.mark_after_screen = nullptr;
  FC_TRY(rc_screen);
  FC_HIP_TRY(hipEventRecord(c.ev_screened, scr));  // behind the verdict and the gated fp64 screen, too
  FC_HIP_TRY(hipStreamWaitEvent(tail, c.ev_screened, 0));
  c.stream = tail;
  FC_TRY(launch_simbits_refine(ens, max_rmsd, max_dev, nullptr, 0.0));
  ens->bits_valid = true;
  return FC_OK;
}

int fc_prune_rmsd_begin_split_async(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t rank,
                                    int64_t world, int64_t row_block, void *screen_stream, int timed) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(screen_stream != nullptr, "screen_stream is NULL");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_TRY(ensure_init());
  return begin_split(ens, max_rmsd, max_dev, rank, world, row_block, static_cast<hipStream_t>(screen_stream),
                     timed ? ctx().ev2 : nullptr, timed ? ctx().ev3 : nullptr);
}

int fc_prune_export_pairs_dev(fc_ensemble *ens, uint64_t *dev_out, int64_t cap) {
  FC_API_LOCK;
  FC_REQUIRE(ens && dev_out, "NULL pointer argument");
  FC_REQUIRE(cap >= 0, "cap must be >= 0");
  FC_REQUIRE(ens->bits_valid, "fc_prune_rmsd_begin has not been called on this ensemble");
  FC_TRY(ensure_init());
  return launch_export_pairs(ens->simq.as<uint64_t>(),
                             reinterpret_cast<const unsigned long long *>(ens->counters.p),
                             (unsigned long long)ens->pairq_cap, cap, dev_out);
}

int fc_prune_from_gathered_dev(fc_ensemble *ens, const uint64_t *dev_gathered, int64_t world, int64_t cap,
                               int64_t min_per_group, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && dev_gathered && mask_out, "NULL pointer argument");
  FC_REQUIRE(world >= 1 && world <= 64 && cap >= 0 && min_per_group >= 1, "bad arguments");
  FC_TRY(ensure_init());
  const int64_t N = ens->N, W = ens->W;
  if (N == 0) return FC_OK;
  if ((uint64_t)world * (uint64_t)cap > kPairLadderCap || !fits_pair_ladder(W))
    return set_error(FC_E_LIMIT, "exchange too large for the one-launch ladder (world*cap = %lld, N = %lld)",
                     (long long)(world * cap), (long long)N);
  FC_TRY(ens->counters.reserve(kCounters * sizeof(uint64_t)));
  FC_TRY(ens->gathered.reserve((size_t)std::max<int64_t>(world * cap, 1) * sizeof(uint64_t)));
  auto *cnt = reinterpret_cast<unsigned long long *>(ens->counters.p);
  FC_TRY(pinned_reserve(slot_bytes(1, W)));
  // this rank's own counters (candidates, similar, grey) before counters[2] becomes the global length
  unsigned long long *local_host = slot_local_counters(0, 1, W);
  FC_TRY(d2h(local_host, cnt, 8 * sizeof(uint64_t)));
  FC_TRY(launch_compact_gathered(dev_gathered, (int)world, cap, ens->gathered.as<uint64_t>(), cnt));
  int64_t survivors = 0;
  LadderJob job;
  job.pairs_dev = ens->gathered.as<uint64_t>(), job.pairs_are_final = true;
  job.mask_out = mask_out, job.survivors = &survivors;
  FC_TRY(ladder_single(ens, min_per_group, job));  // FC_E_LIMIT: some rank's list was missing or longer than cap
  if (stats) fill_stats(stats, owned_pairs(ens), local_host, last_screen_ns(), survivors);
  return FC_OK;
}

// The same, stream-ordered: enqueue prune number `slot` of `n_slots` and return without waiting;
// fc_prune_collect waits for the stream and reads that prune's result.  Lets a caller keep the
// GPU busy across prunes (the next screen starts while the host is still in Python).
int fc_prune_from_gathered_dev_enqueue(fc_ensemble *ens, const uint64_t *dev_gathered, int64_t world,
                                       int64_t cap, int64_t min_per_group, int64_t slot, int64_t n_slots) {
  FC_API_LOCK;
  FC_REQUIRE(ens && dev_gathered, "NULL pointer argument");
  FC_REQUIRE(world >= 1 && world <= 64 && cap >= 0 && min_per_group >= 1, "bad arguments");
  FC_REQUIRE(n_slots >= 1 && n_slots <= 4096 && slot >= 0 && slot < n_slots, "bad slot %lld of %lld", (long long)slot,
             (long long)n_slots);
  FC_TRY(ensure_init());
  const int64_t N = ens->N, W = ens->W;
  FC_REQUIRE(N > 0, "empty ensemble");
  if ((uint64_t)world * (uint64_t)cap > kPairLadderCap || !fits_pair_ladder(W))
    return set_error(FC_E_LIMIT, "exchange too large for the one-launch ladder (world*cap = %lld, N = %lld)",
                     (long long)(world * cap), (long long)N);
  FC_TRY(ens->counters.reserve(kCounters * sizeof(uint64_t)));
  FC_TRY(ens->gathered.reserve((size_t)std::max<int64_t>(world * cap, 1) * sizeof(uint64_t)));
  auto *cnt = reinterpret_cast<unsigned long long *>(ens->counters.p);
  // pinned layout: n_slots x (W + 16) ladder results, then n_slots x 8 local counters; sized by
  // the first prune of a batch (growing it later would move results that are still in flight)
  const size_t need = slot_bytes(n_slots, W);
  if (slot == 0) FC_TRY(pinned_reserve(need));
  FC_REQUIRE(ctx().pinned_bytes >= need, "slot 0 of this batch has not been enqueued");
  FC_TRY(d2h(slot_local_counters(slot, n_slots, W), cnt, 8 * sizeof(uint64_t)));
  FC_TRY(launch_compact_gathered(dev_gathered, (int)world, cap, ens->gathered.as<uint64_t>(), cnt));
  LadderJob job;
  job.pairs_dev = ens->gathered.as<uint64_t>(), job.pairs_are_final = true, job.defer_slot = slot;
  return ladder_single(ens, min_per_group, job);
}

int fc_prune_collect(fc_ensemble *ens, int64_t slot, int64_t n_slots, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && mask_out, "NULL pointer argument");
  FC_REQUIRE(n_slots >= 1 && slot >= 0 && slot < n_slots, "bad slot");
  FC_TRY(ensure_init());
  FC_TRY(sync());
  int64_t survivors = 0;
  if (!ladder_collect(ens, slot, mask_out, nullptr, &survivors, nullptr))
    return set_error(FC_E_LIMIT, "prune %lld: a rank's pair list was missing or too long for the device ladder",
                     (long long)slot);
  if (stats)
    fill_stats(stats, owned_pairs(ens), slot_local_counters(slot, n_slots, ens->W),
               last_screen_ns() /* the most recent screen kernel of this rank */, survivors);
  return FC_OK;
}

int fc_prune_moi(const double *coords, int64_t N, int64_t A, const double *masses,
                 double max_deviation, const double *energies, double max_dE,
                 int64_t min_per_group, uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1 && min_per_group >= 1, "bad arguments");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && masses && mask_out, "NULL pointer argument");
  FC_TRY(ensure_init());
  DevBuf dc;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  return moi_stage(dc.as<double>(), N, A, masses, max_deviation, energies, max_dE, min_per_group, mask_out);
}

// the similarity bits the MOI ladder replays, for callers (and tests) that want the matrix itself
int fc_moi_simbits(const double *coords, int64_t N, int64_t A, const double *masses, double max_deviation,
                   const double *energies, double max_dE, uint64_t *bits_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && masses && bits_out, "NULL pointer argument");
  FC_TRY(ensure_init());
  const int64_t W = ceil_div(N, 64);
  DevBuf dc, dm, dmom, den, dbits;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  if (energies) FC_TRY(upload(den, energies, (size_t)N));
  const size_t bytes = (size_t)N * W * sizeof(uint64_t);
  FC_TRY(dbits.reserve(bytes));
  FC_HIP_TRY(hipMemsetAsync(dbits.p, 0, bytes, ctx().stream));  // the kernel skips the words left of the diagonal
  FC_TRY(moi_moments(dc.as<double>(), N, A, masses, dm, dmom));
  FC_TRY(launch_moi_simbits(dmom.as<double>(), N, max_deviation, energies ? den.as<double>() : nullptr, max_dE,
                            dbits.as<uint64_t>(), W));
  FC_TRY(d2h(bits_out, dbits.p, bytes));
  return sync();
}

// ---- the similarity stages of the drivers on ONE upload --------------------------
// firecode/ensemble.py:205-235 and embedder.py:1445-1474 run prune_by_moment_of_inertia, apply its mask,
// then prune_by_rmsd on the survivors; each call of the reference re-reads host arrays.  Here the
// coordinates go to HBM once: the MOI stage works on them, the survivors are GATHERED on the device
// into the RMSD stage's prepared layout (k_prep_tile with an index list), and the stage masks are
// composed on the way out.  Per stage the result equals the stand-alone entry point's.
int fc_prune_similarity(const double *coords, int64_t N, int64_t A, const uint8_t *heavy_mask, const double *masses,
                        int do_moi, double moi_tol, int do_rmsd, double max_rmsd, double max_dev,
                        const double *energies, double max_dE, int64_t min_per_group, uint8_t *mask_moi_out,
                        uint8_t *mask_out, int64_t *counts) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1 && A <= 32767 && min_per_group >= 1, "bad arguments");
  if (counts) counts[0] = N, counts[1] = N, counts[2] = N;
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && mask_out, "NULL pointer argument");
  FC_REQUIRE(!do_moi || (masses != nullptr && moi_tol > 0.0), "the MOI stage needs masses and a positive tolerance");
  FC_REQUIRE(!do_rmsd || (max_rmsd > 0.0 && max_dev > 0.0), "thresholds must be positive");
  FC_TRY(ensure_init());
  DevBuf raw;
  FC_TRY(upload(raw, coords, (size_t)N * A * 3));  // the one upload of the coordinates
  std::vector<uint8_t> m1((size_t)N, 1);
  if (do_moi) FC_TRY(moi_stage(raw.as<double>(), N, A, masses, moi_tol, energies, max_dE, min_per_group, m1.data()));
  if (mask_moi_out) std::memcpy(mask_moi_out, m1.data(), (size_t)N);
  std::vector<int32_t> idx;
  idx.reserve((size_t)N);
  for (int64_t i = 0; i < N; ++i)
    if (m1[(size_t)i]) idx.push_back((int32_t)i);
  const int64_t N1 = (int64_t)idx.size();
  if (counts) counts[1] = N1, counts[2] = N1;
  if (!do_rmsd || N1 == 0) {
    std::memcpy(mask_out, m1.data(), (size_t)N);
    return FC_OK;
  }
  // survivors gathered into the RMSD stage's layout on the device (no second upload of coordinates)
  DevBuf didx;
  const bool gather = N1 != N;
  if (gather) FC_TRY(upload(didx, idx.data(), idx.size()));
  std::unique_ptr<fc_ensemble> e2(new (std::nothrow) fc_ensemble);
  if (!e2) return set_error(FC_E_NOMEM, "host allocation failed");
  e2->epoch = ctx().epoch;
  FC_TRY(ensemble_build_dev(raw.as<double>(), N1, A, heavy_mask, 1, gather ? didx.as<int32_t>() : nullptr, e2.get()));
  std::vector<double> en1;
  if (energies) {
    en1.resize((size_t)N1);
    for (int64_t k = 0; k < N1; ++k) en1[(size_t)k] = energies[idx[(size_t)k]];
  }
  std::vector<uint8_t> m2((size_t)N1, 0);
  int64_t st[6] = {0};
  FC_TRY(fc_prune_rmsd(e2.get(), max_rmsd, max_dev, energies ? en1.data() : nullptr, max_dE, min_per_group, m2.data(), st));
  std::memset(mask_out, 0, (size_t)N);
  int64_t alive = 0;
  for (int64_t k = 0; k < N1; ++k)
    if (m2[(size_t)k]) {
      mask_out[idx[(size_t)k]] = 1;
      ++alive;
    }
  if (counts) counts[2] = alive;
  return FC_OK;
}

// ---- a7: prune_by_rmsd_rot_corr (prism_pruner.pruner; firecode/ensemble.py:253-260) ----------
int fc_prune_rmsd_rot_corr(const double *coords, int64_t N, int64_t A, const uint8_t *heavy_mask,
                           const int64_t *torsions, int64_t T, const uint8_t *rotation_masks,
                           const double *angles, const int32_t *n_angles, int64_t max_angles,
                           double max_rmsd, double max_dev, const double *energies, double max_dE,
                           int64_t min_per_group, uint8_t *mask_out, uint64_t *bits_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1 && T >= 0 && min_per_group >= 1, "bad arguments");
  if (N == 0) return FC_OK;
  FC_REQUIRE(coords && heavy_mask && mask_out, "NULL pointer argument");
  FC_REQUIRE(T == 0 || (torsions && rotation_masks && angles && n_angles), "NULL torsion arrays");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_REQUIRE(max_angles >= 1 && max_angles <= 64, "1..64 trial angles per torsion");
  int64_t n_heavy = 0;
  for (int64_t a = 0; a < A; ++a) n_heavy += heavy_mask[a] ? 1 : 0;
  FC_REQUIRE(n_heavy >= 1, "the heavy-atom mask selects no atom");
  for (int64_t t = 0; t < T; ++t) {
    for (int k = 0; k < 4; ++k)
      FC_REQUIRE(torsions[t * 4 + k] >= 0 && torsions[t * 4 + k] < A, "torsion %lld: atom index out of range", (long long)t);
    FC_REQUIRE(n_angles[t] >= 1 && n_angles[t] <= max_angles, "torsion %lld: bad angle count", (long long)t);
  }
  if ((size_t)4 * A * 24 > kLdsLimit) return set_error(FC_E_LIMIT, "A=%lld too large for the LDS slice", (long long)A);
  // k_rotcorr_simbits has the row in blockIdx.y, whose extent is 65 535 on every HIP device
  if (N > FC_ROTCORR_MAX_ROWS)
    return set_error(FC_E_LIMIT, "N=%lld exceeds FC_ROTCORR_MAX_ROWS=%d structures: thin the ensemble with the MOI / RMSD stages first",
                     (long long)N, FC_ROTCORR_MAX_ROWS);
  FC_TRY(ensure_init());
  fc_ensemble e;
  size_t bits_bytes = 0;
  FC_TRY(ladder_workspace(&e, N, &bits_bytes));
  FC_HIP_TRY(hipMemsetAsync(e.bits.p, 0, bits_bytes, ctx().stream));
  DevBuf dc, dcen, dh, dt, dm, da, dn;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(dcen.reserve((size_t)N * A * 3 * sizeof(double)));
  FC_TRY(upload(dh, heavy_mask, (size_t)A));
  if (T > 0) {
    FC_TRY(upload(dt, torsions, (size_t)T * 4));
    FC_TRY(upload(dm, rotation_masks, (size_t)T * A));
    FC_TRY(upload(da, angles, (size_t)T * max_angles));
    FC_TRY(upload(dn, n_angles, (size_t)T));
  }
  const double *en_dev = nullptr;
  if (energies) {
    FC_TRY(upload(e.energies, energies, (size_t)N));
    en_dev = e.energies.as<double>();
  }
  FC_TRY(launch_center_structures(dc.as<double>(), N, A, dcen.as<double>()));
  FC_TRY(launch_rotcorr_simbits(dcen.as<double>(), N, A, dh.as<uint8_t>(), dt.as<int64_t>(), T, dm.as<uint8_t>(),
                                da.as<double>(), dn.as<int32_t>(), (int)max_angles, max_rmsd, max_dev, en_dev,
                                max_dE, e.bits.as<uint64_t>(), e.W));
  if (bits_out) FC_TRY(d2h(bits_out, e.bits.p, (size_t)N * e.W * sizeof(uint64_t)));
  LadderJob job;
  job.bits_dev = e.bits.as<uint64_t>(), job.mask_out = mask_out;
  return ladder_single(&e, min_per_group, job);
}

// ---- many prunes in flight -----------------------------------------------------------
// Enqueues the prunes work[0..n) -- counters reset, screen, refine, level buckets, ladder, copy
// of the survivor words + counters into pinned slot r -- and waits ONCE.  Every prune runs in
// full and delivers its mask words to host memory; what goes away is the host round trip
// between two prunes (~45 us of sync wake-up and launch latency on an idle GPU).
//
// overlap: all screens go, in order, to one stream, so two screens never share the chip and
// their event durations stay those of a kernel that has the matrix pipes to itself; verdict,
// refine, level buckets, ladder and result copy of prune r (eight small launches: ~110 us alone,
// up to 250 us beside a screen that holds every workgroup slot) go to stream r % kPruneLanes of
// three others and run beside the screens of prunes r+1 and r+2 -- with two lanes that chain,
// not the screen, set the pace (0.202 ms per prune at a 0.165 ms screen).  A workspace may
// therefore appear again only a multiple of kPruneLanes places later (same lane: ordered on that
// lane's stream); fc_prune_rmsd_many passes distinct ensembles, the bench hook cycles through an
// ensemble and its twins.
// The caller reads the slots with ladder_collect(work[r], r, ..., stride).
constexpr int kPruneLanes = 3;
static int prune_pipeline(fc_ensemble *const *work, int64_t n, double max_rmsd, double max_dev,
                          int64_t min_per_group, bool overlap, int64_t stride, double *screen_ms_sum,
                          double *total_ms) {
  Context &c = ctx();
  FC_TRY(timing_events(4 * n + 2 + kPruneLanes));
  std::vector<hipEvent_t> &ev = c.ev_pool;  // 4 per prune: around the screen kernel, counters reset, screen phase done
  hipEvent_t const ev_begin = ev[4 * n], ev_end = ev[4 * n + 1];
  std::vector<hipEvent_t> &dep = c.ev_dep_pool;  // 2 per prune: counters reset -> screen, screen -> rest of the prune
  while ((int64_t)dep.size() < 2 * n) {
    hipEvent_t e = nullptr;
    FC_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    dep.push_back(e);
  }
  FC_TRY(pinned_reserve((size_t)n * (size_t)stride * sizeof(uint64_t)));
  const int64_t stride_ev = bench_event_stride();
  hipStream_t const home = c.stream;
  StreamRestore restore{c, home};
  const bool lanes = overlap && n > 1;
  if (lanes) FC_TRY(side_streams());
  hipStream_t const s_screen = c.s_screen, s_lane[kPruneLanes] = {c.s_lane[0], c.s_lane[1], c.s_lane[2]};
  // everything enqueued here is ordered behind what the home stream already holds (also what
  // makes pool blocks released by earlier calls safe to reuse on the other streams)
  FC_HIP_TRY(hipEventRecord(ev_begin, home));
  if (lanes)
    for (hipStream_t s : {s_screen, s_lane[0], s_lane[1], s_lane[2]}) FC_HIP_TRY(hipStreamWaitEvent(s, ev_begin, 0));
  auto now_s = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_enqueue0 = now_s();
  for (int64_t r = 0; r < n; ++r) {
    fc_ensemble *e = work[r];
    hipStream_t const tail = lanes ? s_lane[r % kPruneLanes] : home, scr = lanes ? s_screen : home;
    c.stream = tail;
    FC_TRY(ensemble_shard(e, 0, 1, default_row_block()));
    FC_HIP_TRY(hipMemsetAsync(e->counters.p, 0, kCounters * sizeof(uint64_t), tail));
    if (lanes) {
      FC_HIP_TRY(hipEventRecord(dep[2 * r], tail));
      FC_HIP_TRY(hipStreamWaitEvent(scr, dep[2 * r], 0));
    }
    c.stream = scr;
    // timing events around the screen kernel of every `stride`-th prune only: the pair costs the
    // screen stream ~14 us (0.542 -> 0.528 ms per step when all 200 prunes carry it)
    e->lean = true;  // consumer: the one-launch pair ladder (a prune it declines is redone by the caller)
    const bool timed = screen_ms_sum != nullptr && r % stride_ev == 0;
    if (timed) FC_HIP_TRY(hipEventRecord(ev[4 * r], scr));
    c.mark_after_screen = timed ? ev[4 * r + 1] : nullptr;  // the launcher records it right behind the screen kernel
    // with lanes the launcher itself moves to the tail stream behind its main kernel: verdict and gated fp64 screen
    // run there (27 us between two screens on the screen stream otherwise: tools/attic/step_gaps.py)
    c.after_main_stream = lanes ? tail : nullptr;
    c.after_main_event = lanes ? dep[2 * r + 1] : nullptr;
    c.optimistic_screen = lanes;
    const int rc_screen = launch_simbits_screen(e, max_rmsd * max_rmsd + kScreenMargin);
    c.mark_after_screen = nullptr;
    c.after_main_stream = nullptr;
    c.after_main_event = nullptr;
    c.optimistic_screen = false;
    const bool moved = c.stream == tail;
    c.stream = scr;
    FC_TRY(rc_screen);
    if (lanes && !moved) {  // (a launch that ended before its main kernel: nothing to move)
      FC_HIP_TRY(hipEventRecord(dep[2 * r + 1], scr));
      FC_HIP_TRY(hipStreamWaitEvent(tail, dep[2 * r + 1], 0));
    }
    c.stream = tail;
    FC_TRY(launch_simbits_refine(e, max_rmsd, max_dev, nullptr, 0.0));
    e->bits_valid = true;
    LadderJob job;
    job.pairs_dev = e->simq.as<uint64_t>(), job.counters_zeroed = true, job.defer_slot = r, job.slot_stride = stride;
    FC_TRY(ladder_single(e, min_per_group, job));
  }
  c.stream = home;
  if (getenv("FC_DEBUG") && n > 8)
    fprintf(stderr, "[fc] prune_pipeline: %lld prunes enqueued in %.3f ms of host time (%.1f us each)\n", (long long)n,
            1e3 * (now_s() - t_enqueue0), 1e6 * (now_s() - t_enqueue0) / (double)n);
  if (lanes)  // the home stream ends behind the last prune of every lane
    for (int l = 0; l < kPruneLanes; ++l) {
      FC_HIP_TRY(hipEventRecord(ev[4 * n + 2 + l], s_lane[l]));
      FC_HIP_TRY(hipStreamWaitEvent(home, ev[4 * n + 2 + l], 0));
    }
  FC_HIP_TRY(hipEventRecord(ev_end, home));
  FC_HIP_TRY(hipEventSynchronize(ev_end));
  FC_TRY(elapsed_ms(ev_begin, ev_end, total_ms));
  if (screen_ms_sum) FC_TRY(mean_elapsed_ms(ev, n, 4, stride_ev, screen_ms_sum));  // mean over the timed prunes
  return FC_OK;
}

int fc_prune_rmsd_many(fc_ensemble *const *ens, int64_t n, double max_rmsd, double max_dev,
                       int64_t min_per_group, uint8_t *const *mask_out, int64_t *survivors_out) {
  FC_API_LOCK;
  FC_REQUIRE(n >= 0 && n <= 4096, "n=%lld outside 0..4096", (long long)n);
  if (n == 0) return FC_OK;
  FC_REQUIRE(ens && mask_out, "NULL pointer argument");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_REQUIRE(min_per_group >= 1, "min_per_group must be >= 1");
  FC_TRY(ensure_init());
  std::vector<fc_ensemble *> sorted(ens, ens + n);
  std::sort(sorted.begin(), sorted.end());
  for (int64_t r = 0; r < n; ++r) {
    FC_REQUIRE(sorted[r] != nullptr, "NULL ensemble in the list");
    FC_REQUIRE(r == 0 || sorted[r] != sorted[r - 1], "the same ensemble appears twice in the list");
    FC_REQUIRE(mask_out[r] != nullptr || ens[r]->N == 0, "mask_out[%lld] is NULL", (long long)r);
  }
  // in flight together: ensembles the one-launch ladder can take; the rest one by one behind them
  std::vector<fc_ensemble *> work;
  std::vector<int64_t> where;
  int64_t stride = 0;
  for (int64_t r = 0; r < n; ++r)
    if (ens[r]->N >= 2 && fits_pair_ladder(ens[r]->W)) {
      work.push_back(ens[r]);
      where.push_back(r);
      stride = std::max(stride, ens[r]->W + 16);
    }
  static const bool overlap = [] {
    const char *v = getenv("FC_PRUNE_LANES");
    return !(v && atoi(v) == 1);
  }();
  std::vector<char> done((size_t)n, 0);
  if (!work.empty()) {
    FC_TRY(prune_pipeline(work.data(), (int64_t)work.size(), max_rmsd, max_dev, min_per_group, overlap,
                          stride, nullptr, nullptr));
    for (size_t q = 0; q < work.size(); ++q) {
      int64_t levels = 0, alive = 0;
      const int64_t r = where[q];
      if (ladder_collect(work[q], (int64_t)q, mask_out[r], &levels, &alive, nullptr, stride)) {
        done[(size_t)r] = 1;
        if (survivors_out) survivors_out[r] = alive;
      }
    }
  }
  for (int64_t r = 0; r < n; ++r) {
    if (done[(size_t)r]) continue;
    int64_t st[6] = {0};
    if (ens[r]->N > 0) FC_TRY(fc_prune_rmsd(ens[r], max_rmsd, max_dev, nullptr, 0.0, min_per_group, mask_out[r], st));
    if (survivors_out) survivors_out[r] = st[5];
  }
  return FC_OK;
}

// ---- sharded prune over the ranks of the communicator (fc_comm.cpp), no host round trips -------
// Prune k works on workspace k&1 (the ensemble and its twin) and on lane k&1: counters reset,
// refine, export of the rank's similar-pair list, the all-gather (RCCL, on its own stream between
// two events) and the ladder replay; all screens go, in order, to the screen stream.  So the ~0.13 ms
// behind a screen run beside the next screen.  overlap = false: everything on the current stream.
static int sharded_pipeline(fc_ensemble *ens, int64_t steps, double max_rmsd, double max_dev,
                            int64_t min_per_group, int64_t row_block, bool overlap, double *screen_ms_mean,
                            double *total_ms) {
  Context &c = ctx();
  const int64_t rank = comm_rank(), world = comm_world();
  const int64_t cap = 1024 + 4 * ens->N / world;  // pairs a rank can send in the fixed-size message
  FC_TRY(side_streams());
  overlap = overlap && steps > 1;
  fc_ensemble *work[2] = {ens, ens};
  if (overlap) FC_TRY(ensemble_twin(ens, &work[1]));
  for (fc_ensemble *w : work) {  // every grow-only buffer reaches its size before the streams fork
    FC_TRY(ensemble_shard(w, rank, world, row_block));
    FC_TRY(w->msg_send.reserve((size_t)(cap + 1) * sizeof(uint64_t)));
    const size_t recv_bytes = (size_t)world * (size_t)(cap + 1) * sizeof(uint64_t);
    if (w->msg_recv.bytes < recv_bytes || !w->msg_recv.p) {  // a new block starts as "every rank sent an empty list"
      FC_TRY(w->msg_recv.reserve(recv_bytes));
      FC_HIP_TRY(hipMemsetAsync(w->msg_recv.p, 0, w->msg_recv.bytes, c.stream));
    }
    FC_TRY(w->gathered.reserve((size_t)std::max<int64_t>(world * cap, 1) * sizeof(uint64_t)));
  }
  FC_TRY(timing_events(2 * steps + 4));
  std::vector<hipEvent_t> &ev = c.ev_pool;
  const int64_t stride_ev = bench_event_stride();
  hipEvent_t const ev_begin = ev[2 * steps], ev_end = ev[2 * steps + 1];
  hipStream_t const home = c.stream;
  StreamRestore restore{c, home};
  FC_HIP_TRY(hipEventRecord(ev_begin, home));
  for (hipStream_t s : {c.s_screen, c.s_lane[0], c.s_lane[1], c.s_comm}) FC_HIP_TRY(hipStreamWaitEvent(s, ev_begin, 0));
  for (int64_t k = 0; k < steps; ++k) {
    fc_ensemble *e = work[k & 1];
    c.stream = overlap ? c.s_lane[k & 1] : home;
    const bool timed = k % stride_ev == 0;
    FC_TRY(begin_split(e, max_rmsd, max_dev, rank, world, row_block, overlap ? c.s_screen : c.stream,
                       timed ? ev[2 * k] : nullptr, timed ? ev[2 * k + 1] : nullptr));
    FC_TRY(fc_prune_export_pairs_dev(e, e->msg_send.as<uint64_t>(), cap));
    FC_TRY(comm_allgather_dev(e->msg_send.p, e->msg_recv.p, (size_t)(cap + 1) * sizeof(uint64_t), (int)(k & 1)));
    FC_TRY(fc_prune_from_gathered_dev_enqueue(e, e->msg_recv.as<uint64_t>(), world, cap, min_per_group, k, steps));
  }
  c.stream = home;
  if (overlap)
    for (hipStream_t s : {c.s_lane[0], c.s_lane[1], c.s_screen}) {
      FC_HIP_TRY(hipEventRecord(ev[2 * steps + 2], s));
      FC_HIP_TRY(hipStreamWaitEvent(home, ev[2 * steps + 2], 0));
    }
  FC_HIP_TRY(hipEventRecord(ev_end, home));
  FC_HIP_TRY(hipEventSynchronize(ev_end));
  FC_TRY(elapsed_ms(ev_begin, ev_end, total_ms));
  if (screen_ms_mean) FC_TRY(mean_elapsed_ms(ev, steps, 2, stride_ev, screen_ms_mean));
  return FC_OK;
}

// dense similarity (a rank's candidate queue overflowed or its list did not fit the message): one
// all-gather of the (N,) mask per ladder level; every rank takes this path together because every
// rank saw the same gathered headers
static int sharded_levels_fallback(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_per_group,
                                   int64_t row_block, uint8_t *mask_out, int64_t *stats) {
  const int64_t rank = comm_rank(), world = comm_world(), N = ens->N;
  int64_t st[6] = {0};
  FC_TRY(fc_prune_rmsd_begin(ens, max_rmsd, max_dev, nullptr, 0.0, rank, world, row_block, st));
  std::vector<uint8_t> mask((size_t)N, 1), mine((size_t)N), all((size_t)N * (size_t)world);
  for (int64_t k : kLadder) {
    int64_t alive = 0;
    for (uint8_t m : mask) alive += m;
    if (!(k == 1 || min_per_group * k < alive)) continue;
    FC_TRY(fc_prune_level(ens, k, mask.data(), mine.data()));
    FC_TRY(fc_allgather_mask(mine.data(), N, all.data()));
    for (int64_t i = 0; i < N; ++i) {
      uint8_t m = 1;
      for (int64_t r = 0; r < world; ++r) m = std::min(m, all[(size_t)r * N + i]);
      mask[(size_t)i] = m;
    }
  }
  int64_t alive = 0;
  for (int64_t i = 0; i < N; ++i) {
    mask_out[i] = mask[(size_t)i];
    alive += mask[(size_t)i];
  }
  if (stats) {
    for (int k = 0; k < 5; ++k) stats[k] = st[k];
    stats[5] = alive;
  }
  return FC_OK;
}

static int sharded_collect(fc_ensemble *ens, int64_t steps, uint8_t *mask_out, int64_t *stats, bool *all_ok,
                           int64_t *units = nullptr) {
  *all_ok = true;
  int64_t survivors = 0;
  for (int64_t k = 0; k < steps; ++k)
    if (!ladder_collect(ens, k, k == steps - 1 ? mask_out : nullptr, nullptr, &survivors, nullptr)) *all_ok = false;
  if (*all_ok && stats) fill_stats(stats, owned_pairs(ens), slot_local_counters(steps - 1, steps, ens->W), 0, survivors);
  if (*all_ok && units) {  // the subset stage of this rank's lean fp32 screen in the last prune (counters ride behind the mask words)
    const uint64_t *cnt_last = slot_counters(steps - 1, ens->W);
    units[0] = (int64_t)cnt_last[13];
    units[1] = (int64_t)cnt_last[15];
  }
  return FC_OK;
}

int fc_prune_rmsd_sharded(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t min_per_group,
                          int64_t row_block, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && mask_out, "NULL pointer argument");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0 && min_per_group >= 1, "bad arguments");
  FC_TRY(ensure_init());
  if (ens->N == 0) return FC_OK;
  if (row_block <= 0) row_block = default_row_block();
  bool ok = false;
  const int64_t world = comm_world();
  const int64_t cap = 1024 + 4 * ens->N / world;
  const bool device_path = (uint64_t)world * (uint64_t)cap <= kPairLadderCap && fits_pair_ladder(ens->W);
  if (device_path) {
    double ms = 0.0;
    FC_TRY(sharded_pipeline(ens, 1, max_rmsd, max_dev, min_per_group, row_block, false, &ms, nullptr));
    FC_TRY(sharded_collect(ens, 1, mask_out, stats, &ok));
    if (ok && stats) stats[4] = (int64_t)(ms * 1e6);
  }
  if (!ok) FC_TRY(sharded_levels_fallback(ens, max_rmsd, max_dev, min_per_group, row_block, mask_out, stats));
  return FC_OK;
}

int fc_bench_prune_rmsd_sharded(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t reps, int overlap,
                                double *ms_screen_kernel, double *ms_step, uint8_t *mask_out, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && reps >= 1 && reps <= 1024, "bad arguments");
  FC_REQUIRE(max_rmsd > 0.0 && max_dev > 0.0, "thresholds must be positive");
  FC_TRY(ensure_init());
  FC_REQUIRE(ens->N > 0, "empty ensemble");
  const int64_t row_block = default_row_block();
  double ms = 0.0, total = 0.0;
  FC_TRY(sharded_pipeline(ens, reps, max_rmsd, max_dev, 20, row_block, overlap != 0, &ms, &total));
  bool ok = false;
  std::vector<uint8_t> scratch;
  if (!mask_out) {
    scratch.resize((size_t)ens->N);
    mask_out = scratch.data();
  }
  if (stats) stats[6] = stats[7] = 0;  // EIGHT stats, as fc_bench_prune_rmsd
  FC_TRY(sharded_collect(ens, reps, mask_out, stats, &ok, stats ? stats + 6 : nullptr));
  if (!ok) FC_TRY(sharded_levels_fallback(ens, max_rmsd, max_dev, 20, row_block, mask_out, stats));
  if (ms_screen_kernel) *ms_screen_kernel = ms;
  if (ms_step) *ms_step = total / (double)reps;
  return FC_OK;
}

// ---- bench hook ----------------------------------------------------------------------
int fc_screen_last_kind(void) { return last_screen_kind(); }

int fc_prune_conventions(int drop_later) {
  FC_API_LOCK;
  prune_conventions_set(drop_later);
  return FC_OK;
}

int fc_debug_mfma_f16_model(int64_t trials, int64_t *flags_out, double *worst_out) {
  FC_API_LOCK;
  FC_REQUIRE(flags_out && worst_out && trials >= 0 && trials <= (1 << 24), "NULL output or trials outside 0..2^24");
  FC_TRY(ensure_init());
  return h2_model_report(trials, flags_out, worst_out);
}

int fc_debug_h2_covariance(fc_ensemble *ens, int64_t ib, int64_t jb, float *B_out, double *scale_out, double *entry_bound_out) {
  FC_API_LOCK;
  FC_REQUIRE(ens && B_out && scale_out && entry_bound_out, "NULL argument");
  FC_REQUIRE(ib >= 0 && jb >= 0 && ib % 16 == 0 && jb % 16 == 0 && ib + 16 <= ens->Npad && jb + 16 <= ens->Npad,
             "tile origin must be a multiple of 16 inside the padded ensemble");
  FC_TRY(ensure_init());
  FC_REQUIRE(ens->epoch == ctx().epoch, "ensemble belongs to a context that was shut down");
  double scale = 0.0;
  FC_TRY(ensure_h2_operands(ens, &scale));
  *scale_out = scale;
  const int64_t KS2 = (ens->A + 31) / 32;
  *entry_bound_out = kabsch_h2_entry_bound(KS2);
  if (scale == 0.0) return FC_OK;  // does not apply (more than 128 atoms, degenerate norms)
  DevBuf out;
  FC_TRY(out.reserve(256 * 9 * sizeof(float)));
  FC_TRY(launch_h2_cov_tile(ens, ib, jb, out.as<float>()));
  FC_TRY(d2h(B_out, out.p, 256 * 9 * sizeof(float)));
  return sync();
}

int fc_screen_select(int kind) {
  FC_API_LOCK;
  FC_REQUIRE(kind == 0 || kind == 16 || kind == 32 || kind == 64, "kind must be 0 (automatic), 16, 32 or 64");
  screen_select(kind);
  return FC_OK;
}

int fc_debug_screen_plan(int64_t N, int64_t A, int64_t row_block, int64_t lean, double g_max, double max_rmsd, int64_t h2_model_ok,
                         int64_t *plan_out) {
  FC_API_LOCK;
  FC_REQUIRE(plan_out && N >= 0 && N < (1ll << 31) && A >= 1 && row_block >= 1 && (h2_model_ok == 0 || h2_model_ok == 1),
             "NULL plan_out, N outside 0..2^31, A < 1, row_block < 1 or h2_model_ok not 0 / 1");
  return debug_screen_plan(N, A, row_block, lean != 0, g_max, max_rmsd, (int)h2_model_ok, plan_out);
}

int fc_bench_refine(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t reps, double *ms_refine,
                    int64_t *n_candidates) {
  FC_API_LOCK;
  FC_REQUIRE(ens && reps >= 1 && reps <= 4096, "bad arguments");
  FC_TRY(ensure_init());
  FC_TRY(ensemble_shard(ens, 0, 1, default_row_block()));
  Context &c = ctx();
  // one screen fills the candidate-pair queue; then the exact refine alone, `reps` times over that queue
  ens->lean = true;
  FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, kCounters * sizeof(uint64_t), c.stream));
  FC_TRY(launch_simbits_screen(ens, max_rmsd * max_rmsd + kScreenMargin));
  {  // the launcher chooses the long-queue kernels from what the host last saw of this ensemble's queue
    unsigned long long h0[8] = {0};
    FC_TRY(d2h(h0, ens->counters.p, sizeof h0));
    FC_TRY(sync());
    note_candidates(ens, h0[6], ens->last_similar < 0 ? 0 : (unsigned long long)ens->last_similar);
  }
  FC_TRY(timing_events(2 * reps));
  std::vector<hipEvent_t> &ev = c.ev_pool;
  auto *cnt = reinterpret_cast<unsigned long long *>(ens->counters.p);
  for (int64_t r = 0; r < reps; ++r) {
    FC_HIP_TRY(hipMemsetAsync(cnt + 1, 0, 3 * sizeof(uint64_t), c.stream));  // refined / similar / grey
    FC_HIP_TRY(hipEventRecord(ev[2 * r], c.stream));
    FC_TRY(launch_simbits_refine(ens, max_rmsd, max_dev, nullptr, 0.0));
    FC_HIP_TRY(hipEventRecord(ev[2 * r + 1], c.stream));
  }
  unsigned long long h[32] = {0};
  FC_TRY(d2h(h, ens->counters.p, sizeof h));
  FC_TRY(sync());
  if (getenv("FC_DEBUG") && h[22])  // (tuning build FC_RB_TIMELINE: sums over all launches since the counters were cleared)
    fprintf(stderr, "[fc] refine buckets: %llu wave-items, %llu with pairs; mean ticks (100 MHz) staging %.1f, compute %.1f\n", h[22], h[23],
            (double)h[20] / (double)h[22], (double)h[21] / (double)h[22]);
  if (getenv("FC_DEBUG") && h[27])
    fprintf(stderr, "[fc] refine buckets, wave 0 per item (%llu rounds): covariance pass %.1f ticks, polynomial + rotation %.1f, + deviation pass %.1f\n",
            h[27], (double)h[26] / (double)h[27], (double)h[24] / (double)h[27], (double)h[25] / (double)h[27]);
  if (ms_refine) FC_TRY(mean_elapsed_ms(ev, reps, 2, 1, ms_refine));
  if (n_candidates) *n_candidates = (int64_t)h[1];
  if (h[6] > (unsigned long long)ens->pairq_cap)
    return set_error(FC_E_LIMIT, "the candidate-pair queue overflowed (%llu > %lld): this probe times the pair refine only",
                     h[6], (long long)ens->pairq_cap);
  return FC_OK;
}

int fc_bench_prune_rmsd(fc_ensemble *ens, double max_rmsd, double max_dev, int64_t reps,
                        double *ms_simbits_kernel, double *ms_step, uint8_t *mask_out,
                        int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens && reps >= 1 && reps <= 4096, "bad arguments");
  FC_TRY(ensure_init());
  FC_TRY(ensemble_shard(ens, 0, 1, default_row_block()));
  // `reps` prunes of the same resident ensemble through prune_pipeline.  FC_BENCH_LANES=1:
  // strictly one after another; default: odd prunes use a second workspace (bit rows, queues,
  // counters, ladder words) over the same coordinates, so that the small kernels of one prune
  // can run beside the screen of the next.
  static const bool two_lanes = [] {
    const char *v = getenv("FC_BENCH_LANES");
    return !(v && atoi(v) == 1);
  }();
  const bool lanes = two_lanes && reps > 1;
  const int64_t stride = ens->W + 16;
  fc_ensemble *ws[kPruneLanes] = {ens, ens, ens};
  if (lanes) {
    const bool fresh = !ens->twin || !ens->twin->twin;
    for (int l = 1; l < kPruneLanes; ++l) FC_TRY(ensemble_twin(ws[l - 1], &ws[l]));  // a chain of twins over the same coordinates
    // one whole prune per workspace on the home stream: every grow-only buffer reaches its
    // size here, so no block changes hands while several streams are in flight
    if (fresh) FC_TRY(prune_pipeline(ws, kPruneLanes, max_rmsd, max_dev, 20, false, stride, nullptr, nullptr));
  }
  std::vector<fc_ensemble *> work((size_t)reps);
  for (int64_t r = 0; r < reps; ++r) work[(size_t)r] = ws[lanes ? r % kPruneLanes : 0];
  double t_kernel = 0.0, total = 0.0;
  FC_TRY(prune_pipeline(work.data(), reps, max_rmsd, max_dev, 20, lanes, stride, &t_kernel, &total));
  int64_t levels = 0, survivors = 0;
  unsigned long long cnt[8] = {0};
  bool redo = false;
  for (int64_t r = 0; r < reps; ++r)
    if (!ladder_collect(ens, r, mask_out, &levels, &survivors, cnt, stride)) redo = true;
  Context &c = ctx();
  if (redo) {  // dense similarity: the pair ladder declined; one synchronous prune through the bit matrix
    ens->lean = false;
    FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, kCounters * sizeof(uint64_t), c.stream));
    FC_TRY(launch_simbits_screen(ens, max_rmsd * max_rmsd + kScreenMargin));
    FC_TRY(launch_simbits_refine(ens, max_rmsd, max_dev, nullptr, 0.0));
    LadderJob job;
    job.bits_dev = ens->bits.as<uint64_t>(), job.pairs_dev = ens->simq.as<uint64_t>(), job.counters_zeroed = true;
    job.mask_out = mask_out, job.levels = &levels, job.survivors = &survivors, job.counters_out = cnt;
    FC_TRY(ladder_single(ens, 20, job));
  }
  if (getenv("FC_DEBUG")) {
    const uint64_t *cnt_host = slot_counters(reps - 1, ens->W, stride);
    fprintf(stderr, "[fc] bench prune: candidates %llu, similar %llu, screen units the subset stage queued: %llu\n",
            (unsigned long long)cnt_host[1], (unsigned long long)cnt_host[2], (unsigned long long)cnt_host[13]);
  }
  if (ms_simbits_kernel) *ms_simbits_kernel = t_kernel;  // mean over the timed prunes
  if (ms_step) *ms_step = total / (double)reps;
  if (stats) {
    fill_stats(stats, ens->N * (ens->N - 1) / 2, cnt, levels, survivors);
    // the subset stage of the lean fp32 screen in the last prune: units it queued for the full test
    // (0 with the single-stage kernels), and whether its sample found similarity dense
    const uint64_t *cnt_last = slot_counters(reps - 1, ens->W, stride);
    stats[6] = redo ? 0 : (int64_t)cnt_last[13];
    stats[7] = redo ? 0 : (int64_t)cnt_last[15];
  }
  return FC_OK;
}

}  // extern "C"
