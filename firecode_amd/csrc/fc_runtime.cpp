// fc_runtime.cpp -- what every entry point of libfc_hip.so stands on: error state, context, the caching pool behind
// DevBuf, staged copies, pinned staging, init / teardown, and the entry points for devices, streams and pinned memory.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>

#include "fc_internal.h"

namespace fc {

// ---- error state / context -----------------------------------------------------
std::string &last_error() {
  static thread_local std::string e;
  return e;
}

int set_error(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

Context &ctx() {
  static Context c;
  return c;
}

std::recursive_mutex &api_mutex() {
  static std::recursive_mutex *m = new std::recursive_mutex;  // never destroyed (see pool())
  return *m;
}

// ---- caching pool behind DevBuf (fc_common.h) ---------------------------------------------
namespace {
struct Pool {
  std::mutex mu;
  std::multimap<size_t, void *> free_blocks;  // capacity -> block
  size_t cached = 0;
  size_t limit = (size_t)8192 << 20;
  bool limit_read = false;
};
Pool &pool() {
  static Pool *p = new Pool;  // never destroyed: DevBufs with static storage may outlive it otherwise
  return *p;
}
size_t size_class(size_t n) {
  if (n <= 256) return 256;
  if (n <= ((size_t)1 << 20)) {
    size_t c = 256;
    while (c < n) c <<= 1;
    return c;
  }
  const size_t step = (size_t)2 << 20;
  return (n + step - 1) / step * step;
}
}  // namespace

void *pool_take(size_t n, size_t *capacity, bool any_larger) {
  Pool &P = pool();
  const size_t want = size_class(n);
  {
    std::lock_guard<std::mutex> lock(P.mu);
    if (!P.limit_read) {
      if (const char *v = getenv("FC_POOL_MB")) P.limit = (size_t)std::strtoull(v, nullptr, 10) << 20;
      P.limit_read = true;
    }
    auto it = P.free_blocks.lower_bound(want);
    if (it != P.free_blocks.end() && (any_larger || it->first <= 2 * want)) {  // never hand a huge block to a small LASTING request
      void *p = it->second;
      *capacity = it->first;
      P.cached -= it->first;
      P.free_blocks.erase(it);
      return p;
    }
  }
  void *p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) {
    (void)hipGetLastError();
    pool_trim();  // give the cached blocks back and try once more
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
  }
  *capacity = want;
  return p;
}

void pool_give(void *p, size_t capacity) {
  if (!p) return;
  Pool &P = pool();
  {
    std::lock_guard<std::mutex> lock(P.mu);
    if (ctx().ready && P.cached + capacity <= P.limit) {
      P.free_blocks.emplace(capacity, p);
      P.cached += capacity;
      return;
    }
  }
  (void)hipFree(p);
}

void pool_trim() {
  Pool &P = pool();
  std::multimap<size_t, void *> blocks;
  {
    std::lock_guard<std::mutex> lock(P.mu);
    blocks.swap(P.free_blocks);
    P.cached = 0;
  }
  for (auto &b : blocks) (void)hipFree(b.second);
}


// everything the context owns on its device: streams, events, pinned staging, cached blocks
static void context_teardown() {
  Context &c = ctx();
  if (!c.ready) return;
  (void)hipStreamSynchronize(c.stream);
  for (hipStream_t s : {c.s_screen, c.s_lane[0], c.s_lane[1], c.s_lane[2], c.s_comm})
    if (s) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
  c.s_screen = c.s_lane[0] = c.s_lane[1] = c.s_lane[2] = c.s_comm = nullptr;
  for (hipEvent_t e : c.ev_pool) (void)hipEventDestroy(e);
  c.ev_pool.clear();
  for (hipEvent_t e : c.ev_dep_pool) (void)hipEventDestroy(e);
  c.ev_dep_pool.clear();
  for (hipEvent_t *e : {&c.ev0, &c.ev1, &c.ev2, &c.ev3, &c.ev_reset, &c.ev_screened, &c.ev_comm[0], &c.ev_comm[1]})
    if (*e) {
      (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  pool_trim();  // cached blocks belong to the device being left
  (void)hipStreamDestroy(c.own_stream);
  c.stream = c.own_stream = nullptr;
  if (c.pinned) (void)hipHostFree(c.pinned);
  c.pinned = nullptr;
  if (c.pinned_word) (void)hipHostFree(c.pinned_word);
  c.pinned_word = nullptr;
  if (c.ladder_all) (void)hipFree(c.ladder_all);
  c.ladder_all = nullptr;
  c.pinned_bytes = 0;
  for (auto &set : c.stage)
    for (int b = 0; b < 2; ++b) {
      if (set.pin[b]) (void)hipHostFree(set.pin[b]);
      if (set.ev[b]) (void)hipEventDestroy(set.ev[b]);
      set.pin[b] = nullptr;
      set.ev[b] = nullptr;
      set.busy = false;
    }
  c.mark_after_screen = nullptr;
  c.ready = false;
}

static int do_init(int device) {
  Context &c = ctx();
  if (c.ready && c.device == device) return FC_OK;
  context_teardown();  // a device switch: nothing of the old context survives (ensembles are refused by epoch)
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return set_error(FC_E_NODEVICE, "no HIP device available (%s); libfc_hip has no CPU fallback",
                     e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device < 0 || device >= n)
    return set_error(FC_E_INVALID, "device %d out of range (have %d)", device, n);
  if (hipSetDevice(device) != hipSuccess)
    return set_error(FC_E_NODEVICE, "hipSetDevice(%d) failed", device);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    return set_error(FC_E_NODEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(FC_E_NODEVICE, "device %d is %s; this library is built for gfx950 only",
                     device, prop.gcnArchName);
  FC_HIP_TRY(hipStreamCreateWithFlags(&c.own_stream, hipStreamNonBlocking));
  c.stream = c.own_stream;
  FC_HIP_TRY(hipEventCreate(&c.ev0));
  FC_HIP_TRY(hipEventCreate(&c.ev1));
  FC_HIP_TRY(hipEventCreate(&c.ev2));
  FC_HIP_TRY(hipEventCreate(&c.ev3));
  c.device = device;
  c.n_cu = prop.multiProcessorCount;
  c.hbm = prop.totalGlobalMem;
  std::snprintf(c.name, sizeof c.name, "%s (%s)", prop.name, prop.gcnArchName);
  ++c.epoch;
  c.ready = true;
  return FC_OK;
}

int side_streams() {
  Context &c = ctx();
  if (c.s_screen) return FC_OK;
  // The screen fills every workgroup slot of the chip (three per CU): the small kernels of the
  // previous prune (and the collective behind them) get compute units only if the dispatcher
  // prefers them, so their streams have the highest priority and the screens' the lowest.
  // (Without: a refine launched beside a screen took 450 us instead of 45 and the prune after
  // next waited for it.)
  int least = 0, greatest = 0;
  FC_HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  FC_HIP_TRY(hipStreamCreateWithPriority(&c.s_screen, hipStreamNonBlocking, least));
  FC_HIP_TRY(hipStreamCreateWithPriority(&c.s_lane[0], hipStreamNonBlocking, greatest));
  FC_HIP_TRY(hipStreamCreateWithPriority(&c.s_lane[1], hipStreamNonBlocking, greatest));
  FC_HIP_TRY(hipStreamCreateWithPriority(&c.s_lane[2], hipStreamNonBlocking, greatest));
  FC_HIP_TRY(hipStreamCreateWithPriority(&c.s_comm, hipStreamNonBlocking, greatest));
  FC_HIP_TRY(hipEventCreateWithFlags(&c.ev_reset, hipEventDisableTiming));
  FC_HIP_TRY(hipEventCreateWithFlags(&c.ev_screened, hipEventDisableTiming));
  FC_HIP_TRY(hipEventCreateWithFlags(&c.ev_comm[0], hipEventDisableTiming));
  FC_HIP_TRY(hipEventCreateWithFlags(&c.ev_comm[1], hipEventDisableTiming));
  return FC_OK;
}

namespace {
constexpr size_t kStagePiece = (size_t)4 << 20;
struct StageLease {  // one set of pinned pieces for the duration of one staged copy
  Context::StageSet *set = nullptr;
  int acquire() {
    Context &c = ctx();
    {
      std::lock_guard<std::mutex> lock(c.stage_mu);
      for (auto &cand : c.stage)
        if (!cand.busy) {
          cand.busy = true;
          set = &cand;
          break;
        }
    }
    if (!set) return set_error(FC_E_LIMIT, "more than %d staged copies at once", Context::kStageSets);
    for (int b = 0; b < 2; ++b) {
      if (!set->pin[b] && hipHostMalloc(&set->pin[b], kStagePiece, hipHostMallocDefault) != hipSuccess)
        return set_error(FC_E_NOMEM, "pinned staging memory: hipHostMalloc failed");
    }
    for (int b = 0; b < 2; ++b)
      if (!set->ev[b] && hipEventCreateWithFlags(&set->ev[b], hipEventDisableTiming) != hipSuccess)
        return set_error(FC_E_HIP, "hipEventCreate failed");
    return FC_OK;
  }
  ~StageLease() {
    if (set) {
      std::lock_guard<std::mutex> lock(ctx().stage_mu);
      set->busy = false;
    }
  }
};
}  // namespace

bool staged_uploads() {
  static const bool on = [] {
    // measured (cfg3 search, ten runs per process, tools/attic/rescan_probe.py): with uploads on the runtime's own path one run
    // in three still lost 9-22 ms in the kernel behind the free of an uploaded array; with the pinned detour none did.
    // Price: memcpy + DMA instead of DMA from the caller's pages, +0.12 ms per 12 MB (FC_STAGED_UPLOADS=0: direct)
    const char *v = getenv("FC_STAGED_UPLOADS");
    return v ? atoi(v) != 0 : true;
  }();
  return on;
}

bool host_memory_is_pinned(const void *p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // an ordinary host pointer: not an error of ours
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

int d2h_staged(void *dst, const void *src_dev, size_t n, hipStream_t st) {
  if (n == 0) return FC_OK;
  StageLease lease;
  FC_TRY(lease.acquire());
  Context::StageSet &S = *lease.set;
  const char *src = static_cast<const char *>(src_dev);
  char *out = static_cast<char *>(dst);
  size_t issued = 0, copied = 0;
  while (copied < n) {
    // two pieces in flight: request the next one(s), then collect the oldest
    while (issued < n && issued - copied < 2 * kStagePiece) {
      const int b = (int)((issued / kStagePiece) & 1);
      const size_t len = std::min(kStagePiece, n - issued);
      FC_HIP_TRY(hipMemcpyAsync(S.pin[b], src + issued, len, hipMemcpyDeviceToHost, st));
      FC_HIP_TRY(hipEventRecord(S.ev[b], st));
      issued += len;
    }
    const int b = (int)((copied / kStagePiece) & 1);
    const size_t len = std::min(kStagePiece, n - copied);
    FC_HIP_TRY(hipEventSynchronize(S.ev[b]));
    std::memcpy(out + copied, S.pin[b], len);
    copied += len;
  }
  return FC_OK;
}

int h2d_staged(void *dst_dev, const void *src, size_t n, hipStream_t st) {
  if (n == 0) return FC_OK;
  StageLease lease;
  FC_TRY(lease.acquire());
  Context::StageSet &S = *lease.set;
  const char *in = static_cast<const char *>(src);
  char *dst = static_cast<char *>(dst_dev);
  size_t done = 0;
  int64_t piece = 0;
  bool used[2] = {false, false};
  while (done < n) {
    const int b = (int)(piece & 1);
    const size_t len = std::min(kStagePiece, n - done);
    if (used[b]) FC_HIP_TRY(hipEventSynchronize(S.ev[b]));  // the DMA out of this piece two turns ago
    std::memcpy(S.pin[b], in + done, len);
    FC_HIP_TRY(hipMemcpyAsync(dst + done, S.pin[b], len, hipMemcpyHostToDevice, st));
    FC_HIP_TRY(hipEventRecord(S.ev[b], st));
    used[b] = true;
    done += len;
    ++piece;
  }
  for (int b = 0; b < 2; ++b)
    if (used[b]) FC_HIP_TRY(hipEventSynchronize(S.ev[b]));  // the pieces go back to the pool idle
  return FC_OK;
}

int pinned_reserve(size_t bytes) {
  Context &c = ctx();
  if (bytes <= c.pinned_bytes) return FC_OK;
  if (c.pinned) (void)hipHostFree(c.pinned);
  c.pinned = nullptr;
  c.pinned_bytes = 0;
  const size_t want = std::max<size_t>(bytes, 1 << 20);
  FC_HIP_TRY(hipHostMalloc(&c.pinned, want, hipHostMallocDefault));
  c.pinned_bytes = want;
  return FC_OK;
}

int ensure_init() {
  if (ctx().ready) {
    // the calling thread may differ from the one that initialised
    if (hipSetDevice(ctx().device) != hipSuccess)
      return set_error(FC_E_NODEVICE, "hipSetDevice(%d) failed", ctx().device);
    return FC_OK;
  }
  return do_init(0);
}

}  // namespace fc

using namespace fc;

extern "C" {

int fc_abi_version(void) { return 1; }

int fc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fc_init(int device) {
  FC_API_LOCK;
  return do_init(device);
}

int fc_shutdown(void) {
  FC_API_LOCK;
  comm_teardown();
  context_teardown();
  return FC_OK;
}

const char *fc_last_error(void) { return last_error().c_str(); }

int fc_warmup(void) {
  FC_API_LOCK;
  FC_TRY(ensure_init());
  FC_TRY(warm_clash());
  FC_TRY(warm_embed());
  FC_TRY(warm_embed3());
  FC_TRY(warm_torsion());
  FC_TRY(warm_prune());
  FC_TRY(warm_h2_check());
  FC_TRY(warm_kabsch());
  FC_TRY(warm_tfd_ladder());
  FC_TRY(warm_diverse());
  FC_TRY(warm_clusters());
  FC_TRY(warm_symm());
  FC_TRY(warm_knn());
  FC_TRY(warm_medoid());
  FC_TRY(warm_silhouette());
  FC_TRY(warm_group_mean());
  FC_TRY(side_streams());  // the pipelines' streams and ordering events
  // the buffers a first large call would otherwise take from the runtime one by one (0.2 - 1 ms each): through the pool once
  {
    DevBuf warm[6];
    for (DevBuf &b : warm) FC_TRY(b.reserve((size_t)64 << 20));
  }
  return sync();
}

int fc_memory_trim(void) {
  FC_API_LOCK;
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
  pool_trim();
  return FC_OK;
}

int fc_host_alloc_pinned(int64_t bytes, void **out) {
  FC_API_LOCK;
  FC_REQUIRE(out != nullptr && bytes >= 0, "bad arguments");
  *out = nullptr;
  if (bytes == 0) return FC_OK;
  FC_TRY(ensure_init());
  void *p = nullptr;
  if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(FC_E_NOMEM, "hipHostMalloc of %lld bytes failed", (long long)bytes);
  }
  *out = p;
  return FC_OK;
}

int fc_host_free_pinned(void *p) {
  FC_API_LOCK;
  if (p == nullptr) return FC_OK;
  if (hipHostFree(p) != hipSuccess) return set_error(FC_E_HIP, "hipHostFree failed: %s", hipGetErrorString(hipGetLastError()));
  return FC_OK;
}

int fc_stream_set(void *hip_stream) {
  FC_API_LOCK;
  FC_TRY(ensure_init());
  Context &c = ctx();
  FC_HIP_TRY(hipStreamSynchronize(c.stream));  // nothing of ours may still be queued on the old one
  c.stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c.own_stream;
  return FC_OK;
}

int fc_stream_use(void *hip_stream) {
  FC_API_LOCK;
  FC_TRY(ensure_init());
  Context &c = ctx();
  c.stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c.own_stream;
  return FC_OK;
}

int fc_device_info(char *name, int64_t name_len, int64_t *n_cu, int64_t *hbm_bytes) {
  FC_API_LOCK;
  FC_TRY(ensure_init());
  if (name && name_len > 0) std::snprintf(name, (size_t)name_len, "%s", ctx().name);
  if (n_cu) *n_cu = ctx().n_cu;
  if (hbm_bytes) *hbm_bytes = (int64_t)ctx().hbm;
  return FC_OK;
}

}  // extern "C"
