// fc_api_torsion.cpp -- the extern "C" surface (include/fc_hip.h) of the torsion scan, fingerprints, TFD, the cartesian
// product and xyz files: argument checks, host<->HBM staging, kernel sequencing.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <thread>

#include "fc_internal.h"

namespace fc {

// rows of np.stack(np.meshgrid(*arrays), -1).reshape(-1, T) (firecode/utils.py:219-221): with the default
// 'xy' indexing array #2 varies slowest, then #1, then #3 ... #T (fastest).  Written row by row, once, on
// host threads: the NumPy expression makes T strided passes over the whole output (1.0-1.3 s for the
// 1 679 616 x 8 grid of cfg3 -- five times the GPU pipeline it feeds).
template <class V>
static void cartesian_rows(const V *values, const int64_t *counts, int64_t T, V *out) {
  std::vector<int64_t> first((size_t)T, 0);  // offset of array t in `values`
  for (int64_t t = 1; t < T; ++t) first[(size_t)t] = first[(size_t)t - 1] + counts[t - 1];
  // digit order, slowest first: 1, 0, 2, 3, ... (T == 1: just 0)
  std::vector<int64_t> ord;
  if (T >= 2) ord = {1, 0};
  else ord = {0};
  for (int64_t t = 2; t < T; ++t) ord.push_back(t);
  int64_t rows = 1;
  for (int64_t t = 0; t < T; ++t) rows *= counts[t];
  if (rows == 0) return;
  unsigned hw = std::thread::hardware_concurrency();
  if (hw == 0) hw = 1;
  const unsigned nthreads = (unsigned)std::min<int64_t>(std::min<unsigned>(hw, 16u), std::max<int64_t>(1, rows / 65536));
  auto fill = [&](int64_t r0, int64_t r1) {
    std::vector<int64_t> digit((size_t)T, 0);
    int64_t rem = r0;
    for (int64_t p = T - 1; p >= 0; --p) {  // mixed-radix digits of r0 in the order `ord`
      const int64_t t = ord[(size_t)p];
      digit[(size_t)t] = rem % counts[t];
      rem /= counts[t];
    }
    for (int64_t r = r0; r < r1; ++r) {
      V *row = out + r * T;
      for (int64_t t = 0; t < T; ++t) row[t] = values[first[(size_t)t] + digit[(size_t)t]];
      for (int64_t p = T - 1; p >= 0; --p) {  // + 1
        const int64_t t = ord[(size_t)p];
        if (++digit[(size_t)t] < counts[t]) break;
        digit[(size_t)t] = 0;
      }
    }
  };
  if (nthreads <= 1) {
    fill(0, rows);
    return;
  }
  std::vector<std::thread> pool;
  const int64_t per = (rows + nthreads - 1) / nthreads;
  for (unsigned k = 0; k < nthreads; ++k) {
    const int64_t r0 = (int64_t)k * per, r1 = std::min<int64_t>(rows, r0 + per);
    if (r0 < r1) pool.emplace_back(fill, r0, r1);
  }
  for (auto &th : pool) th.join();
}


// argument checks of fc_cartesian_product_i64 / _f64
template <class V>
static int cartesian_product(const V *values, const int64_t *counts, int64_t T, V *out) {
  FC_REQUIRE(T >= 1 && counts != nullptr, "at least one array");
  int64_t rows = 1, total = 0;
  for (int64_t t = 0; t < T; ++t) {
    FC_REQUIRE(counts[t] >= 0, "negative length");
    FC_REQUIRE(counts[t] == 0 || rows <= (int64_t)1 << 40, "product of the lengths too large");
    rows *= counts[t];
    total += counts[t];
  }
  if (rows == 0) return FC_OK;
  FC_REQUIRE(values != nullptr && out != nullptr && total > 0, "NULL pointer argument");
  cartesian_rows<V>(values, counts, T, out);
  return FC_OK;
}

}  // namespace fc

using namespace fc;

extern "C" {

// ---- a17-a20 -----------------------------------------------------------------------
// tfd_keep_out != nullptr (fc_torsion_scan_tfd): the fingerprints never leave the device -- the list
// [starting structure] + [scanned conformers with at least one rotated bond] is TFD-pruned at once.
static int torsion_scan_impl(const double *base, int64_t A, const int64_t *torsions, int64_t T,
                             const uint8_t *rotmasks, const int64_t *angles, int64_t S, double thresh,
                             int64_t backoff_deg, const int64_t *quads, int64_t Q, double *coords_out,
                             int64_t *rotated_bonds_out, double *tf_out, double tfd_thresh = 0.0,
                             uint8_t *tfd_keep_out = nullptr, const int64_t *grid_values = nullptr,
                             const int64_t *grid_counts = nullptr) {
  // grid_values / grid_counts (with angles == nullptr): the angle-sets are the rows of cartesian_product over the T
  // value lists, generated on the device (k_angle_grid)
  FC_REQUIRE(A >= 2 && T >= 1 && S >= 0 && Q >= 0, "bad shape");
  FC_REQUIRE(backoff_deg != 0, "backoff_deg must be non-zero");
  if (S == 0) return FC_OK;
  FC_REQUIRE(base && torsions && rotmasks && (angles || (grid_values && grid_counts)) && rotated_bonds_out, "NULL pointer argument");
  FC_REQUIRE(coords_out || tf_out || tfd_keep_out, "nothing to compute: coords_out and tf_out are both NULL");
  const bool want_tf = tf_out != nullptr || tfd_keep_out != nullptr;
  FC_REQUIRE(!want_tf || (quads != nullptr && Q >= 1), "fingerprints need quadruplets");
  if (want_tf)
    for (int64_t k = 0; k < Q * 4; ++k) FC_REQUIRE(quads[k] >= 0 && quads[k] < A, "quadruplet index out of range");
  if (tfd_keep_out && Q > 128) return set_error(FC_E_LIMIT, "Q=%lld fingerprints exceed 128 (NumPy's summation order changes there)", (long long)Q);
  if (4 * A * 24 > (int64_t)kLdsLimit || A > 32767)
    return set_error(FC_E_LIMIT, "A=%lld too large for the LDS slice", (long long)A);
  // moving / rest index lists per torsion (torsion_module.py:907-915)
  std::vector<int16_t> mv((size_t)T * A, 0), rs((size_t)T * A, 0);
  std::vector<int32_t> nmv((size_t)T, 0), nrs((size_t)T, 0);
  for (int64_t t = 0; t < T; ++t) {
    for (int k = 0; k < 4; ++k)
      FC_REQUIRE(torsions[t * 4 + k] >= 0 && torsions[t * 4 + k] < A, "torsion %lld index out of range", (long long)t);
    const int64_t i2 = torsions[t * 4 + 1], i3 = torsions[t * 4 + 2];
    for (int64_t a = 0; a < A; ++a) {
      if (rotmasks[t * A + a]) mv[(size_t)t * A + nmv[t]++] = (int16_t)a;
      else if (a != i2 && a != i3) rs[(size_t)t * A + nrs[t]++] = (int16_t)a;
    }
  }
  FC_TRY(ensure_init());
  static const bool dbg_laps = getenv("FC_DEBUG") != nullptr && getenv("FC_SCAN_LAPS") != nullptr;
  auto lap_t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!dbg_laps) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[fc]   scan S=%lld %s %.2f ms\n", (long long)S, what, std::chrono::duration<double, std::milli>(t - lap_t0).count());
    lap_t0 = t;
  };
  DevBuf db, dt, dmk, dmv, drs, dnm, dnr, da, dout, drot, dq, dtf;
  FC_TRY(upload(db, base, (size_t)A * 3));
  FC_TRY(upload(dt, torsions, (size_t)T * 4));
  FC_TRY(upload(dmk, rotmasks, (size_t)T * A));
  FC_TRY(upload(dmv, mv.data(), mv.size()));
  FC_TRY(upload(drs, rs.data(), rs.size()));
  FC_TRY(upload(dnm, nmv.data(), nmv.size()));
  FC_TRY(upload(dnr, nrs.data(), nrs.size()));
  if (angles) {
    FC_TRY(upload(da, angles, (size_t)S * T));
  } else {
    std::vector<int64_t> first((size_t)T, 0);
    for (int64_t t = 1; t < T; ++t) first[(size_t)t] = first[(size_t)t - 1] + grid_counts[t - 1];
    DevBuf dval, dfirst, dcnt;
    FC_TRY(upload(dval, grid_values, (size_t)(first[(size_t)T - 1] + grid_counts[T - 1])));
    FC_TRY(upload(dfirst, first.data(), (size_t)T));
    FC_TRY(upload(dcnt, grid_counts, (size_t)T));
    FC_TRY(da.reserve((size_t)S * T * sizeof(int64_t)));
    FC_TRY(launch_angle_grid(dval.as<int64_t>(), dfirst.as<int64_t>(), dcnt.as<int64_t>(), T, S, da.as<int64_t>()));
    FC_TRY(sync());  // (`first` and the three small buffers end here)
  }
  lap("uploads enqueued");
  if (coords_out) FC_TRY(dout.reserve((size_t)S * A * 3 * sizeof(double)));
  FC_TRY(drot.reserve((size_t)S * sizeof(int64_t)));
  lap("output buffers");
  if (want_tf) {
    FC_TRY(upload(dq, quads, (size_t)Q * 4));
    FC_TRY(dtf.reserve((size_t)S * Q * sizeof(double)));
  }
  FC_TRY(launch_torsion_scan(db.as<double>(), A, dt.as<int64_t>(), T, dmk.as<uint8_t>(),
                             dmv.as<int16_t>(), drs.as<int16_t>(), dnm.as<int32_t>(),
                             dnr.as<int32_t>(), da.as<int64_t>(), S, thresh, backoff_deg,
                             coords_out ? dout.as<double>() : nullptr, drot.as<int64_t>(),
                             want_tf ? dq.as<int64_t>() : nullptr, Q, want_tf ? dtf.as<double>() : nullptr));
  lap("scan launched");
  if (dbg_laps) {
    (void)hipStreamSynchronize(ctx().stream);
    lap("scan kernels done");
  }
  if (coords_out) FC_TRY(d2h(coords_out, dout.p, (size_t)S * A * 3 * sizeof(double)));
  lap("coords down");
  if (tf_out) FC_TRY(d2h(tf_out, dtf.p, (size_t)S * Q * sizeof(double)));
  if (!tfd_keep_out) {
    FC_TRY(d2h(rotated_bonds_out, drot.p, (size_t)S * sizeof(int64_t)));
    const int rc_sync = sync();
    lap("synchronised");
    return rc_sync;
  }
  // rows of the TFD problem: the starting structure, then the scanned conformers that rotated a bond -- selected on the
  // device (the counts are 13 MB at 1.7 M angle-sets: down, through a host loop and up again cost 6 ms in front of the
  // first-match kernels; now the counts travel down BESIDE those kernels, on another stream)
  DevBuf dtf0, didx, dT, dfm, dcount, dseltmp;
  FC_TRY(didx.reserve((size_t)S * sizeof(int64_t)));
  FC_TRY(dcount.reserve(sizeof(int64_t)));
  FC_TRY(launch_select_rotated(drot.as<int64_t>(), S, didx.as<int64_t>(), dcount.as<int64_t>(), dseltmp));
  int64_t M = 0;
  FC_TRY(d2h(&M, dcount.p, sizeof(int64_t)));
  FC_TRY(sync());  // (the scan is complete here)
  lap("scan done, rows selected");
  const int64_t N = M + 1, Npad = ceil_div(N, 64) * 64;
  FC_TRY(dtf0.reserve((size_t)Q * sizeof(double)));
  FC_TRY(launch_torsion_fingerprint(db.as<double>(), 1, A, dq.as<int64_t>(), Q, dtf0.as<double>()));
  FC_TRY(dT.reserve((size_t)Q * Npad * sizeof(double)));
  FC_TRY(launch_gather_transpose_pad(dtf.as<double>(), dtf0.as<double>(), didx.as<int64_t>(), M, Q, Npad, dT.as<double>()));
  FC_TRY(dfm.reserve((size_t)N * sizeof(int64_t)));
  DevBuf dtfF;
  FC_TRY(dtfF.reserve((size_t)std::min<int64_t>(Q, 8) * Npad * sizeof(float)));
  FC_TRY(launch_tfd_first_match(dT.as<double>(), N, Npad, Q, tfd_thresh, dfm.as<int64_t>(), dtfF.as<float>()));
  {  // the counts, while the first-match walk runs (the copy into the caller's pageable array keeps this thread busy for
     // 0.3 ms when the array's pages are in place and 1.3 ms when they are fresh from the kernel -- which of the two
     // depends on the caller's allocator, not on this library: a pre-faulting helper thread was built and brought
     // nothing measurable, FC_PREFAULT A/B over 4 x 10 searches)
    FC_TRY(side_streams());
    std::memset(tfd_keep_out, 0, (size_t)S + 1);
    FC_TRY(d2h_staged(rotated_bonds_out, drot.p, (size_t)S * sizeof(int64_t), ctx().s_comm));
  }
  lap("first match enqueued, counts down");
  std::vector<uint8_t> mask((size_t)N);
  FC_TRY(tfd_ladder_from_device(dfm.as<int64_t>(), N, mask.data()));
  lap("ladder");
  // keep flags: row r >= 1 of the TFD problem is the (r - 1)-th angle-set that rotated a bond, and the device still holds
  // that list (didx).  The survivors are few (thousands of 1.7 M): their rows go up, their angle-sets come down -- a
  // walk over all S counts on the host cost 0.7 ms
  tfd_keep_out[0] = mask[0];
  std::vector<int64_t> rows;
  {
    const uint8_t *mb = mask.data();
    int64_t r = 1;
    for (; r + 8 <= N; r += 8) {
      uint64_t w;
      std::memcpy(&w, mb + r, 8);
      if (!w) continue;
      for (int b = 0; b < 8; ++b)
        if (mb[r + b]) rows.push_back(r + b);
    }
    for (; r < N; ++r)
      if (mb[r]) rows.push_back(r);
  }
  if (!rows.empty()) {
    DevBuf drows, dsets;
    FC_TRY(upload(drows, rows.data(), rows.size()));
    FC_TRY(dsets.reserve(rows.size() * sizeof(int64_t)));
    FC_TRY(launch_rows_to_sets(didx.as<int64_t>(), drows.as<int64_t>(), (int64_t)rows.size(), dsets.as<int64_t>()));
    std::vector<int64_t> sets(rows.size());
    FC_TRY(d2h(sets.data(), dsets.p, rows.size() * sizeof(int64_t)));
    FC_TRY(sync());
    for (const int64_t sidx : sets) {
      if (sidx < 0 || sidx >= S) return set_error(FC_E_HIP, "internal: device selection returned angle-set %lld of %lld", (long long)sidx, (long long)S);
      tfd_keep_out[1 + sidx] = 1;
    }
  }
  lap("keep mask assembled");
  return FC_OK;
}

int fc_torsion_scan(const double *base, int64_t A, const int64_t *torsions, int64_t T,
                    const uint8_t *rotmasks, const int64_t *angles, int64_t S, double thresh,
                    int64_t backoff_deg, double *coords_out, int64_t *rotated_bonds_out) {
  FC_API_LOCK;
  FC_REQUIRE(S == 0 || coords_out != nullptr, "NULL pointer argument");
  return torsion_scan_impl(base, A, torsions, T, rotmasks, angles, S, thresh, backoff_deg, nullptr, 0, coords_out,
                           rotated_bonds_out, nullptr);
}

int fc_torsion_scan_fingerprints(const double *base, int64_t A, const int64_t *torsions, int64_t T,
                                 const uint8_t *rotmasks, const int64_t *angles, int64_t S, double thresh,
                                 int64_t backoff_deg, const int64_t *quads, int64_t Q, double *tf_out,
                                 int64_t *rotated_bonds_out, double *coords_out) {
  FC_API_LOCK;
  FC_REQUIRE(S == 0 || tf_out != nullptr, "NULL pointer argument");
  return torsion_scan_impl(base, A, torsions, T, rotmasks, angles, S, thresh, backoff_deg, quads, Q, coords_out,
                           rotated_bonds_out, tf_out);
}

int fc_torsion_scan_tfd(const double *base, int64_t A, const int64_t *torsions, int64_t T, const uint8_t *rotmasks,
                        const int64_t *angles, int64_t S, double thresh, int64_t backoff_deg, const int64_t *quads,
                        int64_t Q, double tfd_thresh, int64_t *rotated_bonds_out, uint8_t *keep_out) {
  FC_API_LOCK;
  FC_REQUIRE(keep_out != nullptr, "NULL pointer argument");
  if (S == 0) {  // the starting structure alone: nothing to compare it with
    keep_out[0] = 1;
    return FC_OK;
  }
  return torsion_scan_impl(base, A, torsions, T, rotmasks, angles, S, thresh, backoff_deg, quads, Q, nullptr,
                           rotated_bonds_out, nullptr, tfd_thresh, keep_out);
}

int fc_torsion_scan_tfd_grid(const double *base, int64_t A, const int64_t *torsions, int64_t T, const uint8_t *rotmasks,
                             const int64_t *values, const int64_t *counts, double thresh, int64_t backoff_deg,
                             const int64_t *quads, int64_t Q, double tfd_thresh, int64_t *rotated_bonds_out, uint8_t *keep_out) {
  FC_API_LOCK;
  FC_REQUIRE(keep_out != nullptr && counts != nullptr && values != nullptr && T >= 1, "NULL pointer argument");
  int64_t S = 1;
  for (int64_t t = 0; t < T; ++t) {
    FC_REQUIRE(counts[t] >= 0, "counts[%lld] is negative", (long long)t);
    FC_REQUIRE(counts[t] == 0 || S <= ((int64_t)1 << 40) / std::max<int64_t>(counts[t], 1), "the grid has more than 2^40 rows");
    S *= counts[t];
  }
  if (S == 0) {  // the starting structure alone: nothing to compare it with
    keep_out[0] = 1;
    return FC_OK;
  }
  return torsion_scan_impl(base, A, torsions, T, rotmasks, nullptr, S, thresh, backoff_deg, quads, Q, nullptr,
                           rotated_bonds_out, nullptr, tfd_thresh, keep_out, values, counts);
}

int fc_torsion_fingerprint(const double *coords, int64_t N, int64_t A, const int64_t *quads,
                           int64_t Q, double *tf_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && A >= 1 && Q >= 0, "bad shape");
  if (N == 0 || Q == 0) return FC_OK;
  FC_REQUIRE(coords && quads && tf_out, "NULL pointer argument");
  for (int64_t k = 0; k < Q * 4; ++k) FC_REQUIRE(quads[k] >= 0 && quads[k] < A, "quadruplet index out of range");
  FC_TRY(ensure_init());
  DevBuf dc, dq, dtf;
  FC_TRY(upload(dc, coords, (size_t)N * A * 3));
  FC_TRY(upload(dq, quads, (size_t)Q * 4));
  FC_TRY(dtf.reserve((size_t)N * Q * sizeof(double)));
  FC_TRY(launch_torsion_fingerprint(dc.as<double>(), N, A, dq.as<int64_t>(), Q, dtf.as<double>()));
  FC_TRY(d2h(tf_out, dtf.p, (size_t)N * Q * sizeof(double)));
  return sync();
}

int fc_tfd_simbits(const double *tf, int64_t N, int64_t Q, double thresh, int64_t row_begin,
                   int64_t row_end, uint64_t *bits_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && Q >= 0, "bad shape");
  FC_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= N, "bad row range");
  if (row_end == row_begin) return FC_OK;
  FC_REQUIRE(bits_out && (tf || Q == 0), "NULL pointer argument");
  if (Q > 128) return set_error(FC_E_LIMIT, "Q=%lld fingerprints exceed 128 (NumPy's summation order changes there)", (long long)Q);
  FC_TRY(ensure_init());
  const int64_t W = ceil_div(N, 64);
  DevBuf dtf, dbits;
  FC_TRY(upload(dtf, tf, (size_t)N * Q));
  const size_t bytes = (size_t)(row_end - row_begin) * W * sizeof(uint64_t);
  FC_TRY(dbits.reserve(bytes));
  FC_TRY(launch_tfd_simbits(dtf.as<double>(), N, Q, thresh, row_begin, row_end,
                            dbits.as<uint64_t>(), W));
  FC_TRY(d2h(bits_out, dbits.p, bytes));
  return sync();
}

int fc_tfd_first_match(const double *tf, int64_t N, int64_t Q, double thresh, int64_t *first_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && Q >= 0, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(first_out && (tf || Q == 0), "NULL pointer argument");
  if (Q > 128) return set_error(FC_E_LIMIT, "Q=%lld fingerprints exceed 128 (NumPy's summation order changes there)", (long long)Q);
  if (Q == 0) {  // NumPy's empty sum is 0: every structure is similar to its successor for thresh > 0, to none otherwise
    for (int64_t i = 0; i < N; ++i) first_out[i] = (thresh > 0.0 && i + 1 < N) ? i + 1 : -1;
    return FC_OK;  // (nothing to launch: there is no fingerprint to upload, and tf may be NULL)
  }
  FC_TRY(ensure_init());
  const int64_t Npad = ceil_div(N, 64) * 64;
  // fingerprint-major copy so that consecutive columns are contiguous: made on the device (on the
  // host the 13 M strided stores of a 1.7 M x 8 matrix cost more than the first-match kernel)
  DevBuf draw, dT, dfm;
  FC_TRY(upload(draw, tf, (size_t)N * (size_t)std::max<int64_t>(Q, 1)));
  FC_TRY(dT.reserve((size_t)std::max<int64_t>(Q, 1) * Npad * sizeof(double)));
  FC_TRY(launch_transpose_pad(draw.as<double>(), N, Q, Npad, dT.as<double>()));
  FC_TRY(dfm.reserve((size_t)N * sizeof(int64_t)));
  DevBuf dtfF;
  FC_TRY(dtfF.reserve((size_t)std::max<int64_t>(std::min<int64_t>(Q, 8), 1) * Npad * sizeof(float)));
  FC_TRY(launch_tfd_first_match(dT.as<double>(), N, Npad, Q, thresh, dfm.as<int64_t>(), dtfF.as<float>()));
  FC_TRY(d2h(first_out, dfm.p, (size_t)N * sizeof(int64_t)));
  return sync();
}

int fc_tfd_last_form(int64_t *n_open_out) { return tfd_last_form(n_open_out); }

int fc_tfd_ladder_from_first_match(const int64_t *first_match, int64_t N, uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(first_match && mask_out, "NULL pointer argument");
  const auto t0 = std::chrono::steady_clock::now();
  for (int64_t i = 0; i < N; ++i)
    FC_REQUIRE(first_match[i] == -1 || (first_match[i] > i && first_match[i] < N), "first_match[%lld] invalid", (long long)i);
  const auto t1 = std::chrono::steady_clock::now();
  // with a device at hand the ladder runs there (a pure host function otherwise: the CPU tests call it without a GPU)
  DevBuf dfm;
  const int64_t *fm_dev = nullptr;
  if (ctx().ready && N >= 20000) {
    FC_TRY(ensure_init());  // (the calling thread's current device: HIP keeps it per thread)
    FC_TRY(upload(dfm, first_match, (size_t)N));
    fm_dev = dfm.as<int64_t>();
  }
  const int rc = tfd_ladder_from_first_match(first_match, N, mask_out, fm_dev);
  if (getenv("FC_DEBUG"))
    fprintf(stderr, "[fc] fc_tfd_ladder_from_first_match: validation %.1f ms, ladder incl. tear-down %.1f ms\n",
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  return rc;
}

int fc_tfd_prune(const double *tf, int64_t N, int64_t Q, double thresh, uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0 && Q >= 0, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(mask_out != nullptr, "NULL pointer argument");
  std::vector<int64_t> fm((size_t)N);
  FC_TRY(fc_tfd_first_match(tf, N, Q, thresh, fm.data()));
  return fc_tfd_ladder_from_first_match(fm.data(), N, mask_out);
}

int fc_debug_pyset_order_ints(const int64_t *keys, int64_t n, int64_t *order_out, int64_t *n_out) {
  FC_API_LOCK;
  FC_REQUIRE(n >= 0 && (keys || n == 0) && order_out && n_out, "bad arguments");
  for (int64_t k = 0; k < n; ++k) FC_REQUIRE(keys[k] >= 0, "keys must be non-negative");
  std::vector<int64_t> o;
  pyset_order_ints(keys, n, o);
  for (size_t k = 0; k < o.size(); ++k) order_out[k] = o[k];
  *n_out = (int64_t)o.size();
  return FC_OK;
}

int fc_debug_tfd_ladder_emulate(const int64_t *first_match, int64_t N, uint8_t *mask_out) {
  FC_API_LOCK;
  FC_REQUIRE(N >= 0, "bad shape");
  if (N == 0) return FC_OK;
  FC_REQUIRE(first_match && mask_out, "NULL pointer argument");
  for (int64_t i = 0; i < N; ++i)
    FC_REQUIRE(first_match[i] == -1 || (first_match[i] > i && first_match[i] < N), "first_match[%lld] invalid", (long long)i);
  try {
    return tfd_ladder_emulate_device(first_match, N, mask_out);
  } catch (const std::bad_alloc &) {
    return set_error(FC_E_NOMEM, "out of host memory");
  }
}

int fc_debug_pyset_order_pairs_device(const int64_t *pairs, int64_t n, int64_t *order_out) {
  FC_API_LOCK;
  FC_REQUIRE(n >= 0 && (n == 0 || (pairs && order_out)), "bad arguments");
  FC_TRY(ensure_init());
  return pyset_order_pairs_device(pairs, n, order_out);
}

int fc_debug_pyset_order_pairs(const int64_t *pairs, int64_t n, int64_t *order_out, int64_t *n_out) {
  FC_API_LOCK;
  FC_REQUIRE(n >= 0 && (pairs || n == 0) && order_out && n_out, "bad arguments");
  std::vector<int64_t> o;
  pyset_order_pairs(pairs, n, o);
  for (size_t k = 0; k < o.size(); ++k) order_out[k] = o[k];
  *n_out = (int64_t)o.size();
  return FC_OK;
}

int fc_cartesian_product_i64(const int64_t *values, const int64_t *counts, int64_t T, int64_t *out) {
  return cartesian_product(values, counts, T, out);
}

int fc_cartesian_product_f64(const double *values, const int64_t *counts, int64_t T, double *out) {
  return cartesian_product(values, counts, T, out);
}

int fc_xyz_write(const char *path, const char *const *atoms, int64_t A, const double *coords,
                 int64_t N, const char *label, int mode) {
  FC_API_LOCK;
  FC_REQUIRE(path && atoms && label && (coords || N == 0), "NULL pointer argument");
  FC_REQUIRE(A >= 1 && N >= 0 && (mode == 0 || mode == 1), "bad arguments");
  for (int64_t a = 0; a < A; ++a) FC_REQUIRE(atoms[a] != nullptr, "atoms[%lld] is NULL", (long long)a);
  return xyz_write(path, atoms, A, coords, N, label, mode);
}

int fc_xyz_scan(const char *path, int64_t *N_out, int64_t *A_out) {
  FC_API_LOCK;
  FC_REQUIRE(path && N_out && A_out, "NULL pointer argument");
  return xyz_read(path, N_out, A_out, nullptr, nullptr);
}

int fc_xyz_read(const char *path, int64_t N, int64_t A, char *atoms_out, double *coords_out) {
  FC_API_LOCK;
  FC_REQUIRE(path && atoms_out && coords_out, "NULL pointer argument");
  FC_REQUIRE(N >= 0 && A >= 0, "bad shape");
  return xyz_read(path, &N, &A, atoms_out, coords_out);
}

}  // extern "C"
