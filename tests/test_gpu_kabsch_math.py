"""firecode_amd/csrc/fc_kabsch_math.h on the device, against the arbitrary-precision reference of tests/kabsch_mp_ref.py:
fc_debug_kabsch_math runs one lane per record, in whole wavefronts (a few thousand lanes per launch).

  routine 0  the probe of csrc/fc_kabsch_math_probe.h -- the text tools/kabsch_math_host.cpp runs on the host -- held to
             the bars of tests/kabsch_math_bars.py on the same ladder; here kabsch_quaternion_qcp and the lean family
             divide through v_rcp_f64, normalise through v_rsq_f64 and loop wave-uniformly
  routine 1  the fp32 screens, which exist on the device only: inputs made as tests/test_fp32_screen_bounds.py makes them
             (coordinates rounded to fp32, covariance accumulated in fp32 atom by atom, s kept as two rounded halves),
             under kabsch_f32_bounds(A4); and under kabsch_h2_bounds(KS2) with an entry error drawn uniformly inside
             kabsch_h2_entry_bound(KS2) s
  routine 2  fc_sqrt_nonneg within one ulp of the correctly rounded root, fc_rsqrt within four

The fp32 bars: never "cannot be similar" for a true msd below thr^2; always for a true msd >= thr^2 + 2 band,
band = 2 p0 s / A of the bounds in use ("the band rule", with the pair's own s) -- on the records where a
correct bounded test CAN decide: the exact P, P', P'' at L exceed 1.5 x the bounds (the bound, and the error it allows
for).  On atoms on a line, two atoms and a top against its image two bands away P(L) itself is below the bound (a
(nearly) double root: P(L) ~ (L - lambda1)^2): those records are counted and printed, they go to the exact path by
design."""

import os
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

import kabsch_math_bars as kb
from firecode_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _device(fc, routine, records, width):
    records = np.ascontiguousarray(records, dtype=np.float64)
    out = np.zeros((len(records), width), dtype=np.float64)
    _lib.call("fc_debug_kabsch_math", int(routine), _lib.pf(records), len(records), _lib.pf(out))
    return out


@pytest.fixture(scope="module")
def rec():
    return kb.records()


@pytest.fixture(scope="module")
def out(fc, rec):
    return _device(fc, 0, rec.data, kb.slots()["kProbeOut"])


# ---- routine 0: the bars of the host, on the device ----------------------------------------------------------------------------
def test_one_sided_eigenvalues_are_never_below_the_largest_root(out, rec):
    print(kb.bar_one_sided_eigenvalue(out, rec))


def test_sharp_eigenvalue_carries_the_rmsd(out, rec):
    print(kb.bar_sharp(out, rec))


def test_lean_eigenvalue_form(out, rec):
    print(kb.bar_lean_eigenvalue(out, rec))


def test_fp64_screen_never_drops_a_similar_pair_and_decides_clear_ones(out, rec):
    print(kb.bar_fp64_screen(out, rec))


def test_rotations_are_optimal_and_close_to_the_true_one(out, rec):
    print("c1, c2 per family:", kb.rotation_constants())
    for key, figures in sorted(kb.bar_rotations(out, rec).items()):
        print(key, figures)


def test_certificates_do_not_pass_by_declining(out, rec):
    print(kb.bar_certificates(out, rec))


def test_a_padded_wavefront_gives_the_full_launch_its_results(fc, out, rec):
    """n = 1, 63, 65: the last wavefront is padded with copies of the last record and every record's result is its own
    (wave-uniform loops run as long as the slowest lane: a fixed point moves by rounding at most, a flag not at all)"""
    s = kb.slots()
    flags = [s[k] for k in ("kPrSettled", "kPrSharp", "kPrBelow", "kPrBelowEnant", "kPrQcpOk", "kPrQuatOk", "kPrRawOk", "kPrCol0Ok")]
    exact = list(range(s["kPrLam"], s["kPrQuatIters"] + 1))  # nothing wave-wide up to the lean family
    for n in (1, 63, 65):
        part = _device(fc, 0, rec.data[:n], s["kProbeOut"])
        assert np.array_equal(part[:, exact], out[:n][:, exact], equal_nan=True)
        assert np.array_equal(part[:, flags], out[:n][:, flags])


def test_host_and_device_bit_differences_reported(out, rec, tmp_path):
    """reported, not asserted: how many outputs differ in any bit between the host build of the probe and the device,
    per routine (the routines without a device-only branch agree where the host fuses as the device does)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is needed for the host build of the probe")
    exe = str(tmp_path / "kabsch_math_host")
    fma = any(line.startswith("flags") and " fma " in line + " " for line in open("/proc/cpuinfo"))
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-host-only", "-ffp-contract=off"] + (["-mfma"] if fma else [])
                       + ["-I", os.path.join(ROOT, "firecode_amd", "csrc"), os.path.join(ROOT, "tools", "kabsch_math_host.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rec.data.tofile(str(tmp_path / "in"))
    assert subprocess.run([exe, "probe", str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True).returncode == 0
    host = np.fromfile(str(tmp_path / "out")).reshape(out.shape)
    s = kb.slots()
    names = sorted(s, key=s.get)
    for a, b in zip(names[:-1], names[1:]):
        cols = slice(s[a], s[b])
        differ = ~((host[:, cols] == out[:, cols]) | (np.isnan(host[:, cols]) & np.isnan(out[:, cols])))
        print(f"{a:18s} {int(differ.any(axis=1).sum()):5d} of {len(out)} records differ in some bit")


# ---- routine 1: the fp32 screens ---------------------------------------------------------------------------------------------
SCREEN_IN, SCREEN_OUT = 16, 16


def _fp32_inputs(e):
    """B accumulated in fp32 atom by atom from coordinates rounded to fp32, s as two rounded halves (test_fp32_screen_bounds)"""
    p, q = (e.p - e.p.mean(axis=0), e.q - e.q.mean(axis=0)) if e.center else (e.p, e.q)
    pf, qf = p.astype(f32), q.astype(f32)
    B = np.zeros((3, 3), dtype=f32)
    for a in range(e.A):
        B += pf[a, :, None] * qf[a, None, :]
    s = f32(f32(0.5 * (p * p).sum()) + f32(0.5 * (q * q).sum()))
    return B, s


@pytest.fixture(scope="module")
def screens(fc, rec):
    """-> (records (n, 16), out (n, 16), index of the probe record each belongs to, kind): every record of the ladder under
    kabsch_f32_bounds(A4), and those of at most 128 atoms again under kabsch_h2_bounds(KS2) with a drawn entry error"""
    rng = np.random.default_rng(77)
    # the entry bound of the split-half screen, from the bounds the library itself computes: p0 = 2 (45 (entry + u) + 172 u)
    U = 2.0 ** -24
    ks2 = sorted({(e.A + 31) // 32 for e in rec.ladder if e.A <= 128})
    probe = np.zeros((len(ks2), SCREEN_IN))
    probe[:, 9], probe[:, 11], probe[:, 12] = 1.0, ks2, 1.0
    entry = {k: (row[10] / 2.0 - 172.0 * U) / 45.0 - U for k, row in zip(ks2, _device(fc, 1, probe, SCREEN_OUT))}
    cache, rows, owner, kind = {}, [], [], []
    for i in range(len(rec.data)):
        k = rec.pair[i]
        e = rec.ladder[k]
        if k not in cache:
            cache[k] = _fp32_inputs(e)
        B, s = cache[k]
        half = f32(0.5 * rec.A_thr2[i])
        if not (np.isfinite(s) and float(s) > 0.0):
            continue
        base = [float(s), float(half), 0.0, 0.0, float(f32(4.0) * half), 0.0, 0.0]
        rows.append(np.concatenate([B.ravel().astype(np.float64), base]))
        rows[-1][11], rows[-1][12] = (e.A + 3) // 4 * 4, 0.0
        owner.append(i), kind.append(0)
        if e.A <= 128:
            K = (e.A + 31) // 32
            B64, _ = e.inputs
            Bh = (B64 + rng.uniform(-1.0, 1.0, size=(3, 3)) * 0.999 * entry[K] * float(s)).astype(f32)
            rows.append(np.concatenate([Bh.ravel().astype(np.float64), base]))
            rows[-1][11], rows[-1][12] = K, 1.0
            owner.append(i), kind.append(1)
    rows = np.array(rows)
    return rows, _device(fc, 1, rows, SCREEN_OUT), np.array(owner), np.array(kind)


def test_fp32_screens_never_drop_a_similar_pair_and_decide_beyond_the_band(screens, rec):
    rows, got, owner, kind = screens
    assert np.all((got[:, :10] == 0.0) | (got[:, :10] == 1.0))
    counts = {"must keep": 0, "must drop": 0, "beyond two bands but undecidable": 0}
    for j in range(len(rows)):
        i = owner[j]
        e = rec.ladder[rec.pair[i]]
        r = e.ref
        s = float(rows[j, 9])
        p0, p1, p2 = (float(v) for v in got[j, 10:13])
        tiny = not (rows[j, 13] < s)
        A_thr2 = mp.mpf(float(rec.A_thr2[i]))
        band = mp.mpf(2.0 * p0 * s / e.A)
        for enant, msd in ((0, r.msd), (1, min(r.msd, r.msd_m))):
            three, two, redo, wave, wave_redo = got[j, 5 * enant:5 * enant + 5]
            assert (two, redo) == (wave, wave_redo), (e.family, e.claim, "the wave form differs from the two-test form")
            if redo == 0.0:
                assert two == three, (e.family, e.claim, "two tests decide otherwise than three")
            else:
                assert two == 1.0  # (the conservative verdict until the three-test form has run)
            if e.A * msd < A_thr2:
                counts["must keep"] += 1
                assert three == 1.0 and two == 1.0, (e.family, e.claim, kind[j], enant, "a similar pair is dropped", float(msd))
            elif not tiny and e.A * msd >= A_thr2 + 2 * band * e.A:
                P0, P1, P2 = r.screen_values(r.S - A_thr2 / 2, enant=bool(enant))
                if P0 > 1.5 * p0 * r.S ** 4 and P1 > 1.5 * p1 * r.S ** 3 and P2 > 1.5 * p2 * r.S ** 2:
                    counts["must drop"] += 1
                    assert three == 0.0, (e.family, e.claim, kind[j], enant, "kept two bands beyond the threshold", float(msd))
                else:
                    counts["beyond two bands but undecidable"] += 1
    print(counts)
    assert counts["must keep"] > 2000 and counts["must drop"] > 1000


# ---- routine 2: the device's square roots -----------------------------------------------------------------------------------
def _root_inputs():
    rng = np.random.default_rng(5)
    tiny, dmin, dmax = np.nextafter(0.0, 1.0), np.finfo(np.float64).tiny, np.finfo(np.float64).max
    x = [0.0, tiny, np.nextafter(dmin, 0.0), dmin, dmax, 1e300, 1e-300]
    for k in range(-1022, 1024, 73):
        x += [2.0 ** k, np.nextafter(2.0 ** k, np.inf), np.nextafter(2.0 ** k, 0.0) if k > -1022 else 2.0 ** k]
    x += [float(n * n) for n in (1, 2, 3, 7, 10, 255, 4097, 94906265)] + [2.25, 6.25e-4 ** 2]
    x += list(np.ldexp(rng.uniform(0.5, 1.0, 4096), rng.integers(-1021, 1024, 4096)))
    return np.array(x, dtype=np.float64)


def _ulps(a, b):
    """distance in units in the last place between finite doubles of the same sign"""
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


def test_device_square_roots(fc):
    x = _root_inputs()
    got = _device(fc, 2, x[:, None], 2)
    root, inv = got[:, 0], got[:, 1]
    assert np.all(np.isfinite(root)) and root[0] == 0.0 and np.all(root[1:] > 0.0)
    d = _ulps(root, np.sqrt(x))  # np.sqrt is correctly rounded
    print(f"fc_sqrt_nonneg: {len(x)} inputs, {int((d == 0).sum())} correctly rounded, worst {int(d.max())} ulp")
    assert d.max() <= 1, (x[d.argmax()], root[d.argmax()])
    normal = x >= np.finfo(np.float64).tiny  # fc_rsqrt documents nothing for 0 and subnormals
    want = np.array([float(1 / mp.sqrt(mp.mpf(float(v)))) for v in x[normal]])
    d = _ulps(inv[normal], want)
    print(f"fc_rsqrt: {int(normal.sum())} inputs, {int((d == 0).sum())} correctly rounded, worst {int(d.max())} ulp")
    assert np.all(np.isfinite(inv[normal])) and d.max() <= 4, (x[normal][d.argmax()], inv[normal][d.argmax()])
