// fc_api_ensemble.cpp -- the extern "C" surface (include/fc_hip.h) of the resident ensemble: building it from host or
// device coordinates, shaping its prune workspace (ensemble_shard, ensemble_twin), and the exact RMSD queries over it.
// Also what every file that takes a permutation table checks first (perm_table_check and its two companions).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>

#include "fc_internal.h"

namespace fc {

static int make_selection(const uint8_t *atom_mask, int64_t A_all, std::vector<int32_t> &sel) {
  sel.clear();
  for (int64_t a = 0; a < A_all; ++a)
    if (atom_mask == nullptr || atom_mask[a]) sel.push_back((int32_t)a);
  if (sel.empty()) return set_error(FC_E_INVALID, "atom_mask selects no atom");
  return FC_OK;
}

// prepared layout of N conformers taken from device-resident raw coordinates (all atoms, AoS):
// conformer n is raw[conf_idx[n]] (conf_idx_dev == nullptr: raw[n])
// defer_wait: return with the preparation kernel and the copy of the largest G still in flight -- the caller does host
// work that does not need them (fc_prune_rmsd_host: the prune's reserves and item table) and then calls
// ensemble_build_finish
int ensemble_build_finish(fc_ensemble *e) {
  if (!e->g_max_pending) return FC_OK;
  e->g_max_pending = false;
  FC_TRY(sync());
  std::memcpy(&e->g_max, ctx().pinned_word, sizeof(double));
  auto *gmax_dev = reinterpret_cast<unsigned long long *>(e->counters.p) + (kCounters - 1);
  FC_HIP_TRY(hipMemsetAsync(gmax_dev, 0, sizeof(unsigned long long), ctx().stream));
  return FC_OK;
}

// The largest G of a SMALL ensemble from the caller's array, on the host: the preparation kernel's arithmetic in its order
// (running sums over the selected atoms, the division, x*x + y*y + z*z per atom; nothing is fused on either side), so that
// fc_prune_rmsd_host needs no wait between the preparation and the prune -- at the sizes of FIRECODE's own runs (hundreds of
// conformers) the call is a chain of waits and launches, not of kernels (0.16 ms at 100 conformers).  Used a hair larger
// than computed: the band rule and the split-half scale are both conservative in a LARGER value.
double host_largest_g(const double *coords, int64_t N, int64_t A_all, const std::vector<int32_t> &sel, int center) {
  const int64_t A = (int64_t)sel.size();
  double gmax = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    const double *t = coords + n * A_all * 3;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (center) {
      for (int64_t a = 0; a < A; ++a) {
        const double *r = t + (int64_t)sel[(size_t)a] * 3;
        cx += r[0];
        cy += r[1];
        cz += r[2];
      }
      cx /= (double)A;
      cy /= (double)A;
      cz /= (double)A;
    }
    double g = 0.0;
    for (int64_t a = 0; a < A; ++a) {
      const double *r = t + (int64_t)sel[(size_t)a] * 3;
      const double x = r[0] - cx, y = r[1] - cy, z = r[2] - cz;
      g += x * x + y * y + z * z;
    }
    if (g == g && g > gmax) gmax = g;
  }
  return gmax;
}
// kHostGmaxDoubles (fc_internal.h), N * A * 3 up to which this pass beats the wait: measured at 50 atoms -- 100 conformers 0.148 against
// 0.161 ms per call, 300 conformers even, 1 000 conformers 0.247 against 0.228 (the pass is three dependent chains of additions per
// conformer)

// Two halves: what does not need the coordinates on the device (selection, reserves, the selection's upload, the reset of the
// largest-G word) and the preparation launch behind them -- ensemble_build issues the first half in FRONT of the upload, so
// that nothing but the launch itself stands between the last piece's DMA and the kernel (the trace of one
// prune_by_rmsd(host arrays) call showed 39 us there).
static int ensemble_build_prepare(int64_t N, int64_t A_all, const uint8_t *atom_mask, fc_ensemble *e, DevBuf &dsel) {
  std::vector<int32_t> &sel = e->sel_host;
  FC_TRY(make_selection(atom_mask, A_all, sel));
  e->N = N;
  e->A = (int64_t)sel.size();
  {  // (Context::hint_*: the last prune of an ensemble of this shape, scaled to this one's number of pairs)
    const Context &c = ctx();
    if (c.hint_A == e->A && c.hint_N >= 2 && N >= c.hint_N / 2 && N <= 2 * c.hint_N) {
      const double scale = ((double)N * (double)N) / ((double)c.hint_N * (double)c.hint_N);
      e->last_candidates = (int64_t)((double)c.hint_candidates * scale);
      e->last_similar = (int64_t)((double)c.hint_similar * scale);
    }
  }
  e->Npad = ceil_div(std::max<int64_t>(N, 1), 64) * 64;
  e->W = e->Npad / 64;
  FC_TRY(e->Xs.reserve((size_t)((e->A + 3) / 4 * 4) * 3 * e->Npad * sizeof(double)));
  FC_TRY(e->G.reserve((size_t)e->Npad * sizeof(double)));
  FC_TRY(e->Xa.reserve((size_t)std::max<int64_t>(N, 1) * e->A * 3 * sizeof(double)));
  FC_TRY(e->counters.reserve(kCounters * sizeof(uint64_t)));
  FC_TRY(upload(dsel, sel.data(), sel.size()));
  return launch_prep_begin(e);
}

static int ensemble_build_launch(const double *raw_dev, int64_t N, int64_t A_all, int center, const int32_t *conf_idx_dev,
                                 fc_ensemble *e, DevBuf &dsel, bool defer_wait, bool host_gmax = false) {
  FC_TRY(launch_prep_body(raw_dev, N, A_all, dsel.as<int32_t>(), e->A, center, e, conf_idx_dev));
  if (host_gmax) return FC_OK;  // (the caller computes the largest G from its array: fc_prune_rmsd_host on small ensembles)
  // the largest G (left by the prep kernel in the last counter word) comes back behind the same wait
  unsigned long long gmax_bits = 0;
  auto *gmax_dev = reinterpret_cast<unsigned long long *>(e->counters.p) + (kCounters - 1);
  if (defer_wait) {
    Context &c = ctx();
    if (!c.pinned_word && hipHostMalloc(&c.pinned_word, 64, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      c.pinned_word = nullptr;
    }
    if (c.pinned_word) {
      FC_HIP_TRY(hipMemcpyAsync(c.pinned_word, gmax_dev, sizeof gmax_bits, hipMemcpyDeviceToHost, c.stream));
      e->g_max_pending = true;
      return FC_OK;  // (dsel returns to the pool: its next user is ordered behind the kernel on this stream)
    }
  }
  FC_TRY(d2h(&gmax_bits, gmax_dev, sizeof gmax_bits));
  FC_TRY(sync());  // (also keeps `sel` / dsel alive until the kernel has read them)
  std::memcpy(&e->g_max, &gmax_bits, sizeof(double));
  FC_HIP_TRY(hipMemsetAsync(gmax_dev, 0, sizeof(unsigned long long), ctx().stream));
  return FC_OK;
}

int ensemble_build_dev(const double *raw_dev, int64_t N, int64_t A_all, const uint8_t *atom_mask,
                              int center, const int32_t *conf_idx_dev, fc_ensemble *e, bool defer_wait) {
  DevBuf dsel;
  FC_TRY(ensemble_build_prepare(N, A_all, atom_mask, e, dsel));
  return ensemble_build_launch(raw_dev, N, A_all, center, conf_idx_dev, e, dsel, defer_wait);
}

// Host arrays in (the drop-in call prune_by_rmsd(structures, ...)): the coordinates go through the pinned pieces like every
// large upload from pageable memory (h2d_staged; fc_common.h says why the caller's pages are not handed to the runtime,
// nor registered by the library for the duration of the copy).
// What that costs and what was tried against it (round 4; tools/attic/pin_probe.py, tools/hostin_breakdown.py; 12 MB):
// DMA from pinned memory 0.22 ms (54 GB/s), from the caller's pageable pages THE SAME 0.22 ms (the driver maps them; that
// mapping is what later stalls the queues when the caller frees the array), memmove into pinned memory 0.24 ms on one
// core -- piece by piece (3 x 4 MB, copy of piece k + 1 beside the DMA of piece k) 0.44 ms per ensemble with the
// preparation kernel.  Built and not kept: ~2 MB pieces of whole 64-conformer tiles, each followed by its own preparation
// launch -- on one stream every copy -> kernel -> copy hand-over between the copy engine and the compute queue costs
// ~25 us (0.67 ms); with the copies on a stream of their own every extra piece costs ~10 us and every event ~7 us
// (0.53 ms); the copy of each 4 MB piece split between this thread and a helper thread (0.41 ms: a thread per call
// for 0.03 ms).
int ensemble_build(const double *coords, int64_t N, int64_t A_all, const uint8_t *atom_mask,
                          int center, fc_ensemble *e, bool defer_wait, bool host_gmax) {
  DevBuf dsel, raw;
  FC_TRY(ensemble_build_prepare(N, A_all, atom_mask, e, dsel));
  FC_TRY(upload(raw, coords, (size_t)N * A_all * 3));
  return ensemble_build_launch(raw.as<double>(), N, A_all, center, nullptr, e, dsel, defer_wait, host_gmax);
}

// (re)shape the bit-matrix workspace for a given sharding
int ensemble_shard(fc_ensemble *e, int64_t rank, int64_t world, int64_t row_block) {
  FC_REQUIRE(e->epoch == 0 || e->epoch == ctx().epoch,
             "this ensemble was created before fc_shutdown / a device switch: create it again");
  FC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world %lld/%lld", (long long)rank,
             (long long)world);
  FC_REQUIRE(row_block >= 32 && row_block % 32 == 0 && row_block <= 4096,
             "row_block must be a multiple of 32 in [32, 4096]");
  e->rank = rank;
  e->world = world;
  e->row_block = row_block;
  const int64_t n_gblocks = ceil_div(e->N, row_block);
  const int64_t n_lblocks = local_block_count(n_gblocks, rank, world);
  e->rows_local = n_lblocks * row_block;
  if ((uint64_t)e->rows_local * (uint64_t)e->W >= (1ull << 32))
    return set_error(FC_E_LIMIT, "bit matrix of %lld x %lld words exceeds the 32-bit word index",
                     (long long)e->rows_local, (long long)e->W);
  FC_TRY(e->bits.reserve(std::max<size_t>((size_t)e->rows_local * e->W * sizeof(uint64_t), 8)));
  FC_TRY(e->cand.reserve(std::max<size_t>((size_t)e->rows_local * e->W * sizeof(uint32_t), 8)));
  // candidate-pair queue: 256 entries per conformer, 1M..64M entries
  e->pairq_cap = std::min<int64_t>(std::max<int64_t>(256 * e->N, 1 << 20), 1 << 26);
  if (const char *v = getenv("FC_PAIRQ_CAP")) {  // test knob: force the word-queue fallback
    const long long c = std::strtoll(v, nullptr, 10);
    if (c >= 1 && c <= (1ll << 26)) e->pairq_cap = c;
  }
  FC_TRY(e->pairq.reserve((size_t)e->pairq_cap * sizeof(uint64_t)));
  FC_TRY(e->simq.reserve((size_t)e->pairq_cap * sizeof(uint64_t)));
  {  // buckets of the long-queue refine: (row buckets of 1 024) x (column tiles of 64), numbered supertile by supertile
     // (8 column tiles of one row bucket; fc_kabsch.hip); sized here, before any pipeline forks
    const int64_t n_rb = ceil_div(e->N, (int64_t)kBucketRows), n_sc = ceil_div(e->Npad >> kBucketColShift, (int64_t)8);
    const int64_t n_st = n_rb * n_sc, nb = n_st * 8;
    e->bk_buckets = nb <= ((int64_t)1 << 22) ? nb : 0;  // one workgroup scans the counts; work items are bucket | piece << 24
    if (e->bk_buckets > 0) {
      FC_TRY(e->bk.reserve((size_t)(512 + 2 * nb + 1) * sizeof(int)));
      FC_TRY(e->bk_off.reserve((size_t)((nb + 1) + (n_st + 1) + 8 * ((n_st + 7) / 8 + 1)) * sizeof(int)));  // offsets | supertile starts | per-XCD prefixes
      FC_TRY(e->bk_list.reserve((size_t)(nb + e->pairq_cap / 256 + 1) * sizeof(int)));  // pieces of <= 512 pairs (256 in tuning builds)
      FC_TRY(e->sortq.reserve((size_t)e->pairq_cap * sizeof(uint64_t)));
    }
  }
  FC_TRY(e->maskA.reserve((size_t)e->Npad));
  FC_TRY(e->maskB.reserve((size_t)e->Npad));
  FC_TRY(e->mbits.reserve((size_t)e->W * sizeof(uint64_t)));
  e->bits_valid = false;
  return FC_OK;
}

// second prune workspace over the coordinates of `ens` (created once, destroyed with it)
int ensemble_twin(fc_ensemble *ens, fc_ensemble **out) {
  if (!ens->twin) {
    std::unique_ptr<fc_ensemble> t(new (std::nothrow) fc_ensemble);
    if (!t) return set_error(FC_E_NOMEM, "host allocation failed");
    t->epoch = ens->epoch;
    t->N = ens->N, t->A = ens->A, t->Npad = ens->Npad, t->W = ens->W;
    t->Xs.alias(ens->Xs), t->Xa.alias(ens->Xa), t->G.alias(ens->G);
    if (ens->xsf_valid) t->Xsf.alias(ens->Xsf), t->sub.alias(ens->sub), t->xsf_valid = true;
    if (ens->xt_valid) t->Xt.alias(ens->Xt), t->xt_valid = true;
    if (ens->xh_valid) t->Xh.alias(ens->Xh), t->xh_valid = true, t->xh_scale = ens->xh_scale;
    t->g_max = ens->g_max;
    t->head = ens->head ? ens->head : ens;
    t->last_candidates = ens->last_candidates, t->last_similar = ens->last_similar;
    FC_TRY(t->counters.reserve(kCounters * sizeof(uint64_t)));
    ens->twin = t.release();
  }
  *out = ens->twin;
  return FC_OK;
}

// pairs (i, j > i) whose row i lies in a row block dealt to `rank`
int64_t owned_pairs(int64_t N, int64_t row_block, int64_t rank, int64_t world) {
  int64_t n = 0;
  const int64_t nb = ceil_div(N, row_block);
  for (int64_t lb = 0, b; (b = global_block(lb, rank, world)) < nb; ++lb)
    for (int64_t i = b * row_block; i < std::min(N, (b + 1) * row_block); ++i) n += N - 1 - i;
  return n;
}

// at least n timing events in Context::ev_pool
int timing_events(int64_t n) {
  std::vector<hipEvent_t> &ev = ctx().ev_pool;
  while ((int64_t)ev.size() < n) {
    hipEvent_t e = nullptr;
    FC_HIP_TRY(hipEventCreate(&e));
    ev.push_back(e);
  }
  return FC_OK;
}

// milliseconds between two recorded events (out may be null: nothing is asked)
int elapsed_ms(hipEvent_t a, hipEvent_t b, double *out) {
  float ms = 0.f;
  if (out) FC_HIP_TRY(hipEventElapsedTime(&ms, a, b));
  if (out) *out = ms;
  return FC_OK;
}
// mean over the event pairs (ev[per * r], ev[per * r + 1]) of the prunes r = 0, step, 2 step, ... < n
int mean_elapsed_ms(const std::vector<hipEvent_t> &ev, int64_t n, int64_t per, int64_t step, double *out) {
  double sum = 0.0, ms = 0.0;
  int64_t n_timed = 0;
  for (int64_t r = 0; r < n; r += step, ++n_timed) {
    FC_TRY(elapsed_ms(ev[per * r], ev[per * r + 1], &ms));
    sum += ms;
  }
  *out = sum / (double)std::max<int64_t>(n_timed, 1);
  return FC_OK;
}

// every check the contract lists for the table, on the host; -> the table as the kernels take it (16-bit indices)
int perm_table_check(const int32_t *perms, int64_t K, int64_t A_sel, std::vector<uint16_t> &table) {
  FC_REQUIRE(perms != nullptr, "perms is NULL");
  FC_REQUIRE(K >= 1, "K=%lld: the table holds at least the identity", (long long)K);
  if (K > kPermMax)
    return set_error(FC_E_LIMIT, "K=%lld permutations exceed FC_PERM_MAX=%lld", (long long)K, (long long)kPermMax);
  FC_REQUIRE(A_sel >= 1 && A_sel <= 32767, "A_sel=%lld outside [1, 32767]", (long long)A_sel);
  const size_t A = (size_t)A_sel;
  std::vector<uint8_t> seen(A);
  for (int64_t k = 0; k < K; ++k) {
    std::fill(seen.begin(), seen.end(), (uint8_t)0);
    for (size_t a = 0; a < A; ++a) {
      const int32_t v = perms[(size_t)k * A + a];
      FC_REQUIRE(v >= 0 && v < A_sel && !seen[(size_t)v], "row %lld of perms is not a permutation of 0..%lld", (long long)k,
                 (long long)A_sel - 1);
      seen[(size_t)v] = 1;
    }
  }
  for (size_t a = 0; a < A; ++a) FC_REQUIRE(perms[a] == (int32_t)a, "row 0 of perms is not the identity");
  std::vector<int32_t> inv(A);
  for (int64_t k = 0; k < K; ++k) {
    const int32_t *row = perms + (size_t)k * A;
    for (size_t a = 0; a < A; ++a) inv[(size_t)row[a]] = (int32_t)a;
    bool found = false;
    for (int64_t l = 0; l < K && !found; ++l) found = std::equal(inv.begin(), inv.end(), perms + (size_t)l * A);
    FC_REQUIRE(found, "perms is not closed under inverse: the inverse of row %lld is not in the table", (long long)k);
  }
  table.resize((size_t)K * A);
  for (size_t t = 0; t < table.size(); ++t) table[t] = (uint16_t)perms[t];
  return FC_OK;
}

// the refusal of a table whose kernel would need more LDS than a workgroup has (per: " per tile", or nothing)
int perm_lds_check(size_t lds, int64_t A_sel, int64_t K, const char *per) {
  if (lds > kLdsLimit)
    return set_error(FC_E_LIMIT, "A_sel=%lld selected atoms with K=%lld permutations need %zu bytes of LDS%s (limit %zu)",
                     (long long)A_sel, (long long)K, lds, per, kLdsLimit);
  return FC_OK;
}

// what the table and the ensemble have to satisfy together, still before any device use
int perm_ensemble_check(const fc_ensemble *ens, int64_t K, int64_t A_sel, bool bit_matrix) {
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  FC_REQUIRE(A_sel == ens->A, "A_sel=%lld, the ensemble has %lld selected atoms", (long long)A_sel, (long long)ens->A);
  if (!bit_matrix) return FC_OK;
  FC_TRY(perm_lds_check(symm_lds_bytes(A_sel, K), A_sel, K, " per tile"));
  const int64_t rb = default_row_block();
  if ((uint64_t)(ceil_div(ens->N, rb) * rb) * (uint64_t)ens->W >= (1ull << 32))
    return set_error(FC_E_LIMIT, "N=%lld: the bit matrix exceeds the 32-bit word index", (long long)ens->N);
  return FC_OK;
}

}  // namespace fc

using namespace fc;

extern "C" {

// ---- ensemble ------------------------------------------------------------------
int fc_ensemble_create(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask,
                       int center, fc_ensemble **out) {
  FC_API_LOCK;
  FC_REQUIRE(out != nullptr, "out is NULL");
  *out = nullptr;
  FC_REQUIRE(coords != nullptr || N == 0, "coords is NULL");
  FC_REQUIRE(N >= 0 && A >= 1, "bad shape N=%lld A=%lld", (long long)N, (long long)A);
  FC_REQUIRE(A <= 32767, "A=%lld exceeds 32767 atoms", (long long)A);
  FC_TRY(ensure_init());
  std::unique_ptr<fc_ensemble> e(new (std::nothrow) fc_ensemble);
  if (!e) return set_error(FC_E_NOMEM, "host allocation failed");
  e->epoch = ctx().epoch;
  FC_TRY(ensemble_build(coords, N, A, atom_mask, center, e.get()));
  *out = e.release();
  return FC_OK;
}

int fc_ensemble_destroy(fc_ensemble *ens) {
  FC_API_LOCK;
  delete ens;
  return FC_OK;
}

int fc_ensemble_shape(const fc_ensemble *ens, int64_t *N, int64_t *A_selected) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  if (N) *N = ens->N;
  if (A_selected) *A_selected = ens->A;
  return FC_OK;
}

// ---- a4 ------------------------------------------------------------------------
static int ensemble_rmsd_pairs(fc_ensemble *ens, const int64_t *pair_i, const int64_t *pair_j, int64_t P, double *rmsd_out,
                               double *maxdev_out, bool inverted) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_REQUIRE(ens->epoch == ctx().epoch, "this ensemble was created before fc_shutdown / a device switch: create it again");
  FC_REQUIRE(P >= 0, "P < 0");
  if (P == 0) return FC_OK;
  FC_REQUIRE(pair_i && pair_j && rmsd_out && maxdev_out, "NULL pointer argument");
  for (int64_t k = 0; k < P; ++k)
    FC_REQUIRE(pair_i[k] >= 0 && pair_i[k] < ens->N && pair_j[k] >= 0 && pair_j[k] < ens->N,
               "pair %lld = (%lld, %lld) out of range [0, %lld)", (long long)k,
               (long long)pair_i[k], (long long)pair_j[k], (long long)ens->N);
  FC_TRY(ensure_init());
  DevBuf di, dj, dr, dm;
  FC_TRY(upload(di, pair_i, (size_t)P));
  FC_TRY(upload(dj, pair_j, (size_t)P));
  FC_TRY(dr.reserve((size_t)P * sizeof(double)));
  FC_TRY(dm.reserve((size_t)P * sizeof(double)));
  FC_TRY(launch_pairs_exact(ens, di.as<int64_t>(), dj.as<int64_t>(), P, dr.as<double>(),
                            dm.as<double>(), nullptr, inverted));
  FC_TRY(d2h(rmsd_out, dr.p, (size_t)P * sizeof(double)));
  FC_TRY(d2h(maxdev_out, dm.p, (size_t)P * sizeof(double)));
  return sync();
}
int fc_ensemble_rmsd_pairs(fc_ensemble *ens, const int64_t *pair_i, const int64_t *pair_j,
                           int64_t P, double *rmsd_out, double *maxdev_out) {
  return ensemble_rmsd_pairs(ens, pair_i, pair_j, P, rmsd_out, maxdev_out, false);
}
// the values of (X_i, -X_j): the partner inverted through the origin (include/fc_hip.h, "enantiomer-aware forms")
int fc_ensemble_rmsd_pairs_inv(fc_ensemble *ens, const int64_t *pair_i, const int64_t *pair_j, int64_t P, double *rmsd_out,
                               double *maxdev_out) {
  return ensemble_rmsd_pairs(ens, pair_i, pair_j, P, rmsd_out, maxdev_out, true);
}

static int kabsch_rmsd_pairs(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask, const int64_t *pair_i,
                             const int64_t *pair_j, int64_t P, int center, double *rmsd_out, double *maxdev_out,
                             bool inverted) {
  FC_API_LOCK;
  fc_ensemble *e = nullptr;
  FC_TRY(fc_ensemble_create(coords, N, A, atom_mask, center, &e));
  const int rc = ensemble_rmsd_pairs(e, pair_i, pair_j, P, rmsd_out, maxdev_out, inverted);
  fc_ensemble_destroy(e);
  return rc;
}
int fc_kabsch_rmsd_pairs(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask,
                         const int64_t *pair_i, const int64_t *pair_j, int64_t P, int center,
                         double *rmsd_out, double *maxdev_out) {
  return kabsch_rmsd_pairs(coords, N, A, atom_mask, pair_i, pair_j, P, center, rmsd_out, maxdev_out, false);
}
int fc_kabsch_rmsd_pairs_inv(const double *coords, int64_t N, int64_t A, const uint8_t *atom_mask, const int64_t *pair_i,
                             const int64_t *pair_j, int64_t P, int center, double *rmsd_out, double *maxdev_out) {
  return kabsch_rmsd_pairs(coords, N, A, atom_mask, pair_i, pair_j, P, center, rmsd_out, maxdev_out, true);
}

// all pairs, both outputs: covariance tiles on the fp64 matrix pipe, rotation + explicit rotated
// difference in the epilogue (k_simbits_screen_mfma<.., 2>); structures beyond the LDS column tile
// (A > 104) take the one-wave-per-row kernel.  Outputs may both be NULL (timing only).
static bool rmsd_and_max_tiled(const fc_ensemble *ens) {
  // (a 64-column tile up to 104 atoms, 32 columns up to 208, 16 up to 416: launch_rmsd_values picks)
  const size_t lds_m = ((size_t)(((ens->A + 3) / 4 + 1) / 2) * 384 + 16 + 128) * sizeof(double) + 1024;
  return lds_m <= kLdsLimit && (uint64_t)((ens->A + 3) / 4 * 4) * 3 * (uint64_t)ens->Npad < (1ull << 32);
}

static int rmsd_and_max_all(fc_ensemble *ens, double *rmsd_out, double *maxdev_out, double *ms_kernel) {
  FC_TRY(ensure_init());
  const int64_t N = ens->N;
  if (N == 0) return FC_OK;
  Context &c = ctx();
  DevBuf dr, dm;
  const size_t bytes = (size_t)N * N * sizeof(double);
  FC_TRY(dr.reserve(bytes));
  FC_TRY(dm.reserve(bytes));
  const bool tiled = rmsd_and_max_tiled(ens);
  unsigned long long cnt[16] = {0};
  if (tiled) {
    // the tiled kernel writes every (i, j >= i), exact zeros on the diagonal; the lower triangle is
    // mirrored on the device below: nothing to clear (2 x 800 MB of memset per call at 10^4 conformers)
    FC_TRY(ensemble_shard(ens, 0, 1, 256));  // sizes the pair queue of the fix-up
    FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, 16 * sizeof(uint64_t), c.stream));
  } else {
    FC_HIP_TRY(hipMemsetAsync(dr.p, 0, bytes, c.stream));
    FC_HIP_TRY(hipMemsetAsync(dm.p, 0, bytes, c.stream));
  }
  FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  if (tiled) FC_TRY(launch_rmsd_values(ens, 0.0, dr.as<double>(), dm.as<double>()));
  else FC_TRY(launch_matrix_exact(ens, dr.as<double>(), dm.as<double>()));
  FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  if (tiled) FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
  FC_TRY(sync());
  FC_TRY(elapsed_ms(c.ev0, c.ev1, ms_kernel));
  if (tiled && cnt[6] > (unsigned long long)ens->pairq_cap) {
    // more pairs for the fix-up than its queue holds.  Near-duplicates first (the eigenvalue form of the rmsd declines pairs
    // closer than ~1e-3 A): the same kernel with the running sum
    FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, 16 * sizeof(uint64_t), c.stream));
    FC_TRY(launch_rmsd_values(ens, 0.0, dr.as<double>(), dm.as<double>(), 0, 1, /*explicit_sum=*/true));
    FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
    FC_TRY(sync());
  }
  if (tiled && cnt[6] > (unsigned long long)ens->pairq_cap) {
    // more degenerate pairs than the fix-up queue holds (planar or collinear structures: every pair): the plain kernel
    // redoes the matrix
    FC_HIP_TRY(hipMemsetAsync(dr.p, 0, bytes, c.stream));
    FC_HIP_TRY(hipMemsetAsync(dm.p, 0, bytes, c.stream));
    FC_TRY(launch_matrix_exact(ens, dr.as<double>(), dm.as<double>()));
  }
  // both kernels write the upper triangle and the diagonal: the lower one is mirrored on the device, then the matrices
  // travel (the host's element loop took ~0.1 s per call at 10^4 conformers)
  if (rmsd_out) FC_TRY(launch_mirror_upper(dr.as<double>(), N));
  if (maxdev_out) FC_TRY(launch_mirror_upper(dm.as<double>(), N));
  if (rmsd_out) FC_TRY(d2h(rmsd_out, dr.p, bytes));
  if (maxdev_out) FC_TRY(d2h(maxdev_out, dm.p, bytes));
  return sync();
}

// bench hook: `reps` complete all-pairs alignment passes over the resident ensemble, enqueued back to
// back on the library's stream (outputs: two dense (N, N) matrices that stay in HBM), one host wait.
// ms_kernel_mean: HIP events around the dominant kernel (k_simbits_screen_mfma<., 2>) of every launch;
// ms_total: first launch to the end of the last fix-up kernel.  stats[0] = pairs per pass,
// stats[1] = pairs the last pass queued for the Jacobi fix-up, stats[2] = 1 when the tiled kernel ran, stats[3] = 16 x 16
// sub-tiles of the last pass that took the general form of the rotation (the caller's array holds FOUR words).
// sample_*: P elements (i, j) of the LAST pass's two output matrices, read back for the caller's checker
static int bench_rmsd_and_max_all(fc_ensemble *ens, int64_t reps, double *ms_kernel_mean, double *ms_total,
                                  int64_t *stats, const int64_t *sample_i = nullptr, const int64_t *sample_j = nullptr,
                                  int64_t P = 0, double *sample_rmsd = nullptr, double *sample_maxdev = nullptr) {
  FC_TRY(ensure_init());
  const int64_t N = ens->N;
  FC_REQUIRE(N >= 2, "needs at least two conformers");
  Context &c = ctx();
  DevBuf dr, dm;
  const size_t bytes = (size_t)N * N * sizeof(double);
  FC_TRY(dr.reserve(bytes));
  FC_TRY(dm.reserve(bytes));
  const bool tiled = rmsd_and_max_tiled(ens);
  // under a communicator (or the loopback hook) a rank computes the rows dealt to it: the units shard with
  // no exchange; every rank keeps its rows of the two matrices
  const int64_t rank = comm_rank(), world = comm_world();
  FC_REQUIRE(tiled || world == 1, "structures beyond the tiled kernel are not sharded");
  if (tiled) FC_TRY(ensemble_shard(ens, 0, 1, 256));
  FC_TRY(timing_events(2 * reps + 2));
  std::vector<hipEvent_t> &ev = c.ev_pool;
  FC_HIP_TRY(hipEventRecord(ev[2 * reps], c.stream));
  for (int64_t r = 0; r < reps; ++r) {
    if (tiled) {
      FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, 16 * sizeof(uint64_t), c.stream));
      FC_HIP_TRY(hipEventRecord(ev[2 * r], c.stream));
      c.mark_after_screen = ev[2 * r + 1];  // recorded right behind the tiled kernel, in front of the fix-up
      const int rc = launch_rmsd_values(ens, 0.0, dr.as<double>(), dm.as<double>(), rank, world);
      c.mark_after_screen = nullptr;
      FC_TRY(rc);
    } else {
      FC_HIP_TRY(hipEventRecord(ev[2 * r], c.stream));
      FC_TRY(launch_matrix_exact(ens, dr.as<double>(), dm.as<double>()));
      FC_HIP_TRY(hipEventRecord(ev[2 * r + 1], c.stream));
    }
  }
  FC_HIP_TRY(hipEventRecord(ev[2 * reps + 1], c.stream));
  unsigned long long cnt[16] = {0};
  if (tiled) FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
  FC_TRY(sync());
  double mean = 0.0;
  FC_TRY(mean_elapsed_ms(ev, reps, 2, 1, &mean));
  if (ms_kernel_mean) *ms_kernel_mean = mean;
  FC_TRY(elapsed_ms(ev[2 * reps], ev[2 * reps + 1], ms_total));
  if (stats) {
    stats[0] = owned_pairs(N, 128, rank, world);  // pairs this rank computed: rows of its blocks of 128, columns right of the diagonal
    stats[1] = (int64_t)cnt[6];
    stats[2] = tiled ? 1 : 0;
    stats[3] = (int64_t)cnt[kCntGeneralForm];  // 16 x 16 sub-tiles of the last pass that took the general form of the rotation
  }
  if (tiled && cnt[6] > (unsigned long long)ens->pairq_cap)
    return set_error(FC_E_LIMIT, "%llu degenerate pairs exceed the fix-up queue (%lld)", cnt[6], (long long)ens->pairq_cap);
  if (P > 0) {  // behind the timed passes and their events: what the last pass left in the two matrices
    DevBuf di, dj, sr, sm;
    FC_TRY(upload(di, sample_i, (size_t)P));
    FC_TRY(upload(dj, sample_j, (size_t)P));
    FC_TRY(sr.reserve((size_t)P * sizeof(double)));
    FC_TRY(sm.reserve((size_t)P * sizeof(double)));
    FC_TRY(launch_gather_matrix_pairs(dr.as<double>(), dm.as<double>(), N, di.as<int64_t>(), dj.as<int64_t>(), P,
                                      sr.as<double>(), sm.as<double>()));
    FC_TRY(d2h(sample_rmsd, sr.p, (size_t)P * sizeof(double)));
    FC_TRY(d2h(sample_maxdev, sm.p, (size_t)P * sizeof(double)));
    FC_TRY(sync());
  }
  return FC_OK;
}

int fc_ensemble_rmsd_matrix(fc_ensemble *ens, double *rmsd_out, double *maxdev_out) {
  FC_API_LOCK;
  FC_REQUIRE(ens && rmsd_out && maxdev_out, "NULL pointer argument");
  return rmsd_and_max_all(ens, rmsd_out, maxdev_out, nullptr);
}

int fc_ensemble_rmsd_and_max_all(fc_ensemble *ens, double *rmsd_out, double *maxdev_out, double *ms_kernel) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  return rmsd_and_max_all(ens, rmsd_out, maxdev_out, ms_kernel);
}

int fc_bench_rmsd_and_max_all(fc_ensemble *ens, int64_t reps, double *ms_kernel_mean, double *ms_total,
                              int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr && reps >= 1 && reps <= 4096, "bad arguments");
  return bench_rmsd_and_max_all(ens, reps, ms_kernel_mean, ms_total, stats);
}

int fc_bench_rmsd_and_max_all_sampled(fc_ensemble *ens, int64_t reps, const int64_t *pair_i, const int64_t *pair_j,
                                      int64_t P, double *rmsd_out, double *maxdev_out, double *ms_kernel_mean,
                                      double *ms_total, int64_t *stats) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr && reps >= 1 && reps <= 4096, "bad arguments");
  FC_REQUIRE(P >= 0 && (P == 0 || (pair_i && pair_j && rmsd_out && maxdev_out)), "NULL sample arrays");
  for (int64_t p = 0; p < P; ++p)
    FC_REQUIRE(pair_i[p] >= 0 && pair_i[p] < ens->N && pair_j[p] >= 0 && pair_j[p] < ens->N,
               "sample pair %lld out of range", (long long)p);
  return bench_rmsd_and_max_all(ens, reps, ms_kernel_mean, ms_total, stats, pair_i, pair_j, P, rmsd_out, maxdev_out);
}

int fc_ensemble_rmsd_values(fc_ensemble *ens, double *rmsd_out, double *ms_kernel) {
  FC_API_LOCK;
  FC_REQUIRE(ens != nullptr, "ens is NULL");
  FC_TRY(ensure_init());
  const int64_t N = ens->N;
  if (N == 0) return FC_OK;
  FC_TRY(ensemble_shard(ens, 0, 1, 256));  // sizes the pair queue
  Context &c = ctx();
  DevBuf dr;
  const size_t bytes = (size_t)N * N * sizeof(double);
  FC_TRY(dr.reserve(bytes));
  FC_HIP_TRY(hipMemsetAsync(dr.p, 0, bytes, c.stream));
  FC_HIP_TRY(hipMemsetAsync(ens->counters.p, 0, 16 * sizeof(uint64_t), c.stream));
  FC_HIP_TRY(hipEventRecord(c.ev0, c.stream));
  FC_TRY(launch_rmsd_values(ens, 0.02, dr.as<double>(), nullptr));
  FC_HIP_TRY(hipEventRecord(c.ev1, c.stream));
  unsigned long long cnt[16];
  FC_TRY(d2h(cnt, ens->counters.p, sizeof cnt));
  if (rmsd_out) {  // (the lower triangle mirrored on the device, then one copy)
    FC_TRY(launch_mirror_upper(dr.as<double>(), N));
    FC_TRY(d2h(rmsd_out, dr.p, bytes));
  }
  FC_TRY(sync());
  if (cnt[6] > (unsigned long long)ens->pairq_cap)
    return set_error(FC_E_LIMIT, "%llu pairs closer than 0.02 A or without a unique optimal rotation exceed the fix-up queue (%lld): "
                     "use fc_ensemble_rmsd_matrix", cnt[6], (long long)ens->pairq_cap);
  return elapsed_ms(c.ev0, c.ev1, ms_kernel);
}

int fc_ensemble_rmsd_pairs_perm(fc_ensemble *ens, const int32_t *perms, int64_t K, int64_t A_sel, const int64_t *pair_i,
                                const int64_t *pair_j, int64_t P, double *rmsd_out, double *maxdev_out) {
  FC_API_LOCK;
  std::vector<uint16_t> table;
  FC_TRY(perm_table_check(perms, K, A_sel, table));
  FC_TRY(perm_ensemble_check(ens, K, A_sel, false));
  FC_REQUIRE(P >= 0, "P < 0");
  if (P == 0) return FC_OK;
  FC_REQUIRE(pair_i && pair_j && rmsd_out && maxdev_out, "NULL pointer argument");
  for (int64_t k = 0; k < P; ++k)
    FC_REQUIRE(pair_i[k] >= 0 && pair_i[k] < ens->N && pair_j[k] >= 0 && pair_j[k] < ens->N,
               "pair %lld = (%lld, %lld) out of range [0, %lld)", (long long)k, (long long)pair_i[k], (long long)pair_j[k],
               (long long)ens->N);
  FC_TRY(ensure_init());
  DevBuf di, dj, dr, dm, dperm;
  const auto run = [&]() -> int {
    FC_TRY(upload(di, pair_i, (size_t)P));
    FC_TRY(upload(dj, pair_j, (size_t)P));
    FC_TRY(upload(dperm, table.data(), table.size()));
    FC_TRY(dr.reserve((size_t)P * K * sizeof(double)));
    FC_TRY(dm.reserve((size_t)P * K * sizeof(double)));
    FC_TRY(launch_symm_pairs(ens, dperm.as<uint16_t>(), K, di.as<int64_t>(), dj.as<int64_t>(), P, dr.as<double>(),
                             dm.as<double>()));
    FC_TRY(d2h(rmsd_out, dr.p, (size_t)P * K * sizeof(double)));
    FC_TRY(d2h(maxdev_out, dm.p, (size_t)P * K * sizeof(double)));
    return sync();
  };
  return drained(run());
}

int fc_ensemble_twin(fc_ensemble *ens, fc_ensemble **twin_out) {
  FC_API_LOCK;
  FC_REQUIRE(ens && twin_out, "NULL pointer argument");
  FC_TRY(ensure_init());
  return ensemble_twin(ens, twin_out);
}

}  // extern "C"
