"""firecode_amd/csrc/fc_kabsch_math.h itself, on the host, against the arbitrary-precision reference of
tests/kabsch_mp_ref.py on its fixed ladder of pairs (no GPU).

tools/kabsch_math_host.cpp runs every __host__ routine of the header on a file of records and writes every value, flag and
certificate; it is built with the ROCm compiler for the host only, as tests/test_qcp_col0_cpu.py builds its checker (FMA
contraction where the host has the instruction: the header's contract(fast) regions then fuse as they do on the device), and
a second time with -fsanitize=address,undefined, which runs on the whole ladder as a process of its own.  The bars are those
of tests/kabsch_math_bars.py, the same the device is held to (tests/test_gpu_kabsch_math.py).

The three NumPy restatements of the header that other tests lean on are tied to the header here, on the same ladder:
lambda_newton (test_knn_filter_bound_cpu.py), _lambda_newton (test_complete_eig_bound.py), poly / bounds
(test_fp32_screen_bounds.py).  NumPy sums the nine squares of |B|_F^2 in its own order and the header fuses where the host
has FMA, so the tie is "within 4 ulp of the quantity's scale" -- the sum of the magnitudes of its terms -- and for a root
of Newton's iteration that many ulp of P over the slope; kabsch_f32_bounds, where nothing fuses, is tied bit for bit.

What it found: kabsch_lambda_max ran out of its 64 steps on a covariance that vanishes against Gp + Gq (B = 0: P = x^4, a
factor 3/4 per step) and reported a healthy slope; kabsch_lambda_is_sharp then certified an rmsd that was 1.7e-8 A off.
The slope is now reported as 0 where the iteration has not settled (test_sharp_eigenvalue_carries_the_rmsd)."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kabsch_math_bars as kb
import test_complete_eig_bound as eig_copy
import test_fp32_screen_bounds as f32_copy
import test_knn_filter_bound_cpu as knn_copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = kb.EPS


def _host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def _build(tmp_path_factory, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is needed: fc_kabsch_math.h includes the HIP runtime header")
    out = str(tmp_path_factory.mktemp(name) / name)
    flags = ["-std=c++17", "--offload-host-only", "-ffp-contract=off", "-Wall", "-Werror"] + (["-mfma"] if _host_has_fma() else [])
    r = subprocess.run([hipcc] + flags + extra + ["-I", os.path.join(ROOT, "firecode_amd", "csrc"),
                                                  os.path.join(ROOT, "tools", "kabsch_math_host.cpp"), "-o", out],
                       capture_output=True, text=True)
    return out, r


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out, r = _build(tmp_path_factory, "kabsch_math_host", ["-O2"])
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(tool, mode, data, tmp_path, width):
    src, dst = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    np.ascontiguousarray(data, dtype=np.float64).tofile(src)
    r = subprocess.run([tool, mode, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return np.fromfile(dst, dtype=np.float64).reshape(-1, width)


@pytest.fixture(scope="module")
def rec():
    return kb.records()


@pytest.fixture(scope="module")
def out(tool, rec, tmp_path_factory):
    return _run(tool, "probe", rec.data, tmp_path_factory.mktemp("probe"), kb.slots()["kProbeOut"])


def test_sanitized_build_runs_the_whole_ladder_clean(rec, tmp_path_factory, out):
    """the same file under AddressSanitizer and UndefinedBehaviorSanitizer, a process of its own: status 0, no report, and
    the same decisions as the plain build"""
    exe, r = _build(tmp_path_factory, "kabsch_math_host_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                               "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitizer" in r.stderr.lower()):
        pytest.skip("this ROCm clang has no sanitizer runtime for the host: " + r.stderr.strip().splitlines()[-1][:200])
    assert r.returncode == 0, r.stderr[-4000:]
    got = _run(exe, "probe", rec.data, tmp_path_factory.mktemp("probe_san"), kb.slots()["kProbeOut"])
    s = kb.slots()
    for flag in ("kPrBelow", "kPrBelowEnant", "kPrSettled"):
        assert np.mean(got[:, s[flag]] == out[:, s[flag]]) > 0.99  # (-O1 fuses its own way: the flags at an edge may differ)
    _run(exe, "bounds", np.arange(0.0, 600.0, 4.0), tmp_path_factory.mktemp("bounds_san"), 7)


# ---- the bars --------------------------------------------------------------------------------------------------------------
def test_one_sided_eigenvalues_are_never_below_the_largest_root(out, rec):
    print(kb.bar_one_sided_eigenvalue(out, rec))


def test_sharp_eigenvalue_carries_the_rmsd(out, rec):
    print(kb.bar_sharp(out, rec))
    # the case that failed: an all-zero covariance under Gp + Gq > 0 is declined, not certified 1.7e-8 A off
    s = kb.slots()
    zero = [rec.first[k] for k, e in enumerate(rec.ladder) if e.claim.get("kind") == "zero-covariance"]
    assert len(zero) > 0 and np.all(out[zero, s["kPrSharp"]] == 0.0) and np.all(out[zero, s["kPrSlope"]] == 0.0)


def test_lean_eigenvalue_form(out, rec):
    print(kb.bar_lean_eigenvalue(out, rec))


def test_fp64_screen_never_drops_a_similar_pair_and_decides_clear_ones(out, rec):
    print(kb.bar_fp64_screen(out, rec))


def test_rotations_are_optimal_and_close_to_the_true_one(out, rec):
    print("oracle (LAPACK) ratios per family:", kb.oracle_rotation_ratios())
    print("c1, c2 per family:", kb.rotation_constants())
    for key, figures in sorted(kb.bar_rotations(out, rec).items()):
        print(key, figures)


def test_certificates_do_not_pass_by_declining(out, rec):
    print(kb.bar_certificates(out, rec))


# ---- the NumPy restatements, tied to the header -----------------------------------------------------------------------------
def _conditioned(rec):
    """one record per pair whose largest root is simple and clear: P'(lambda1) >= 1e-3 lambda1^3 (elsewhere two correct
    evaluations of the iteration end anywhere within sqrt(u) of the root: DESIGN.md section 18)"""
    keep = [rec.first[k] for k, e in enumerate(rec.ladder) if e.ref.lam[0] > 0 and e.ref.gap_product >= 1e-3 * e.ref.lam[0] ** 3]
    return np.array(keep)


def test_lambda_newton_of_the_knn_filter_test_is_the_header(out, rec):
    s, idx = kb.slots(), _conditioned(rec)
    assert len(idx) > 500
    B, gg = rec.data[idx, :9].reshape(-1, 3, 3), rec.data[idx, 9]
    lam, slope, step, n2 = knn_copy.lambda_newton(B, gg)
    S = 0.5 * gg
    noise = 9.0 * S ** 4 / out[idx, s["kPrSlope"]]  # a rounding of P (terms up to 9 x^4) moves a step and the root by this
    assert np.all(np.abs(n2 - out[idx, s["kPrNorm2"]]) <= 4 * EPS * n2)
    # (the slope is P' at the iterate before the last step: its own terms reach 9 x^3, and P'' <= 12 x^2 times the noise of x)
    assert np.all(np.abs(slope - out[idx, s["kPrSlope"]]) <= 4 * EPS * (9.0 * S ** 3 + 12.0 * S ** 2 * noise))
    assert np.all(np.abs(lam - out[idx, s["kPrLam"]]) <= 4 * EPS * (S + noise))
    assert np.all(np.abs(step - out[idx, s["kPrStep"]]) <= 4 * EPS * noise)
    settled = knn_copy.is_settled(lam, slope, step, n2)
    assert np.array_equal(settled, out[idx, s["kPrSettled"]] == 1.0) and settled.all()
    print(f"{len(idx)} pairs; identical bits: lambda {np.mean(lam == out[idx, s['kPrLam']]):.3f}, slope "
          f"{np.mean(slope == out[idx, s['kPrSlope']]):.3f}, |B|^2 {np.mean(n2 == out[idx, s['kPrNorm2']]):.3f}")
    # the copy on the whole ladder: every decision of its settled test is the header's wherever both iterations stopped
    B, gg = rec.data[rec.first, :9].reshape(-1, 3, 3), rec.data[rec.first, 9]
    lam, slope, step, n2 = knn_copy.lambda_newton(B, gg)
    both = knn_copy.is_settled(lam, slope, step, n2) & (out[rec.first, s["kPrSettled"]] == 1.0)
    assert np.all(np.abs(lam - out[rec.first, s["kPrLam"]])[both] <= 1.1e-11 * lam[both])


def test_lambda_newton_of_the_complete_eig_test_is_the_header(out, rec):
    s, idx = kb.slots(), _conditioned(rec)
    B, gg = rec.data[idx, :9].reshape(-1, 3, 3), rec.data[idx, 9]
    lam = eig_copy._lambda_newton(B, gg)
    S = 0.5 * gg
    noise = 9.0 * S ** 4 / out[idx, s["kPrSlope"]]
    assert np.all(out[idx, s["kPrLeanConverged"]] == 1.0)
    assert np.all(np.abs(lam - out[idx, s["kPrLeanLam"]]) <= 4 * EPS * (S + noise))
    print(f"{len(idx)} pairs; identical bits: {np.mean(lam == out[idx, s['kPrLeanLam']]):.3f}")


def test_poly_and_bounds_of_the_fp32_screen_test_are_the_header(tool, out, rec, tmp_path):
    s = kb.slots()
    counts = np.arange(0.0, 600.0, 4.0)
    got = _run(tool, "bounds", counts, tmp_path, 7)
    for n, row in zip(counts, got):
        want = np.array([np.float32(2.0 * v) for v in f32_copy.bounds(n)], dtype=np.float64)
        assert np.array_equal(row[:3], want), (n, row[:3], want)  # kabsch_f32_bounds: nothing fuses, bit for bit
        db = row[6] + f32_copy.U
        want = np.array([np.float32(2.0 * (45.0 * db + 172.0 * f32_copy.U)), np.float32(2.0 * (9.5 * db + 46.0 * f32_copy.U)),
                         np.float32(2.0 * (6.0 * db + 52.0 * f32_copy.U))], dtype=np.float64)
        assert np.array_equal(row[3:6], want)                     # kabsch_h2_bounds: the same polynomial part on its entry bound
    # the fp64 screen's three values against poly() in units of s (not-tiny records: 0.75 < l <= 1, |b|_F <= 1)
    sg = 0.5 * rec.data[:, 9]
    keep = (rec.A_thr2 < 0.5 * sg) & (sg > 0)
    B, sg, L = rec.data[keep, :9].reshape(-1, 3, 3), sg[keep], (sg - 0.5 * rec.A_thr2)[keep]
    P0, P1, P2 = f32_copy.poly(B, sg, L, np.float64)
    # scale of each quantity: the sum of the magnitudes of its terms with |b|_F <= 1, l <= 1, |det b| <= 0.2, e2 <= 1/3
    for name, mine, slot, power, scale in (("P0", P0, "kPrP0", 4, 1.0 + 4.0 / 3.0 + 1.6), ("P1", P1, "kPrP1", 3, 1.0 + 0.4),
                                           ("P2", P2, "kPrP2", 2, 3.0)):
        err = np.abs(mine - out[keep, s[slot]] / sg ** power)
        print(f"{name}: {keep.sum()} records, worst difference {err.max() / EPS:.2f} ulp of 1, allowed {4 * scale:.1f}")
        assert err.max() <= 4 * EPS * scale
    # and the verdict is those three values against the guard, nothing else
    verdict = ~((out[:, s["kPrP2"]] >= 0) & (out[:, s["kPrP1"]] >= 0) & (out[:, s["kPrP0"]] > 1e-12 * (0.5 * rec.data[:, 9]) ** 4))
    tiny = ~(rec.A_thr2 < 0.25 * rec.data[:, 9])
    assert np.array_equal(verdict | tiny, out[:, s["kPrBelow"]] == 1.0)


# ---- the device entry point refuses before it needs a device -----------------------------------------------------------------
def test_debug_entry_refuses_bad_arguments_before_any_device_use():
    from firecode_amd import _lib

    L = _lib.load()
    buf = np.zeros(94 * 2)
    p, null = _lib.pd(buf) if hasattr(_lib, "pd") else buf.ctypes.data_as(C.POINTER(C.c_double)), C.POINTER(C.c_double)()
    assert L.fc_debug_kabsch_math(0, null, 1, p) == _lib.FC_E_INVALID
    assert L.fc_debug_kabsch_math(0, p, 1, null) == _lib.FC_E_INVALID
    assert L.fc_debug_kabsch_math(0, p, -1, p) == _lib.FC_E_INVALID
    assert L.fc_debug_kabsch_math(0, p, (1 << 20) + 1, p) == _lib.FC_E_INVALID
    assert L.fc_debug_kabsch_math(3, p, 1, p) == _lib.FC_E_INVALID
    assert L.fc_debug_kabsch_math(-1, p, 1, p) == _lib.FC_E_INVALID
    bad = np.zeros(16)
    bad[11], bad[12] = 52.0, 2.0  # a kind that is neither kabsch_f32_bounds nor kabsch_h2_bounds
    assert L.fc_debug_kabsch_math(1, bad.ctypes.data_as(C.POINTER(C.c_double)), 1, p) == _lib.FC_E_INVALID
    bad[11], bad[12] = -4.0, 0.0
    assert L.fc_debug_kabsch_math(1, bad.ctypes.data_as(C.POINTER(C.c_double)), 1, p) == _lib.FC_E_INVALID
    for routine in (0, 1, 2):
        assert L.fc_debug_kabsch_math(routine, p, 0, p) == _lib.FC_OK  # an empty call needs no device
