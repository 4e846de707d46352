"""Enantiomer-aware RMSD prune, the parts that need no device: the lemma the kernels rest on,
properties of the NumPy restatement (tests/enant_ref.py), and the boundary (symbols, keyword defaults, argument
validation, no CPU fallback)."""

import inspect
import os
import re

import numpy as np
import pytest

import enant_ref as er
from firecode_amd import _lib
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-9
NEW_SYMBOLS = ("fc_ensemble_rmsd_pairs_inv", "fc_kabsch_rmsd_pairs_inv", "fc_rmsd_simbits_enant", "fc_prune_rmsd_enant")


# ---- 1. the lemma ------------------------------------------------------------------------------------------------------
def _random_pairs(n_pairs, seed, planar_every=10):
    """centred pairs (P, Q) at all distances: q = p + noise with a log-uniform scale in [0.01, 3] A; half of the
    partners rotated, half of those reflected; every ``planar_every``-th pair exactly planar (z = 0 in both: det B = 0)"""
    rng = np.random.default_rng(seed)
    P, Q = [], []
    for k in range(n_pairs):
        A = int(rng.integers(4, 40))
        p = rng.normal(scale=1.5, size=(A, 3))
        q = p + rng.normal(size=(A, 3)) * 10.0 ** rng.uniform(-2.0, np.log10(3.0))
        planar = k % planar_every == 0
        if planar:
            p[:, 2] = 0.0
            q[:, 2] = 0.0
        if k % 2 == 1 and not planar:
            q = q @ syn.random_rotation(rng).T
            if k % 4 == 3:
                q[:, 0] *= -1.0
        P.append(p - p.mean(axis=0))
        Q.append(q - q.mean(axis=0))
    return P, Q


def _cov_terms(B):
    """n2 = |B|_F^2, det B and e2 = |cof B|_F^2 in the kernels' order of operations (B of any float dtype)"""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = B
    n2 = Sxx * Sxx + Sxy * Sxy + Sxz * Sxz + Syx * Syx + Syy * Syy + Syz * Syz + Szx * Szx + Szy * Szy + Szz * Szz
    c = [Syy * Szz - Syz * Szy, Syz * Szx - Syx * Szz, Syx * Szy - Syy * Szx,
         Sxz * Szy - Sxy * Szz, Sxx * Szz - Sxz * Szx, Sxy * Szx - Sxx * Szy,
         Sxy * Syz - Sxz * Syy, Sxz * Syx - Sxx * Syz, Sxx * Syy - Sxy * Syx]
    det = Sxx * c[0] + Sxy * c[1] + Sxz * c[2]
    e2 = c[0] * c[0]
    for x in c[1:]:
        e2 = e2 + x * x
    return n2, det, e2


def _may_f64(B, G, A_thr2, det_of):
    """kabsch_may_be_below (fp64, three sign tests) with det B replaced by det_of(det B)"""
    s = 0.5 * G
    L = s - 0.5 * A_thr2
    tiny = not (A_thr2 < 0.5 * s)
    n2, det, e2 = _cov_terms(B)
    d = det_of(det)
    L2 = L * L
    u = L2 - n2
    P2, P1, P0 = 2.0 * L2 + u, u * L - 2.0 * d, u * u - 4.0 * (e2 + 2.0 * L * d)
    eps = 1e-12 * (s * s) * (s * s)
    return bool(tiny or P2 < 0.0 or P1 < 0.0 or not P0 > eps)


def _may_f32_2t(B, G, A_thr2, p0, p2, det_of):
    """kabsch_may_be_below_f32_2t (fp32, two sign tests) with det B replaced by det_of(det B)"""
    f = np.float32
    B = np.asarray(B, dtype=f)
    s, h = f(0.5 * G), f(0.5 * A_thr2)
    L = f(s - h)
    tiny = not (f(4.0) * h < s)
    n2, det, e2 = _cov_terms(B)
    d = det_of(det)
    uu = f(L * L - n2)
    P0 = f(uu * uu - f(4.0) * f(e2 + f(2.0) * L * d))
    s2 = f(s * s)
    u_ok = uu > f(p2) * s2
    return bool(tiny or not u_ok or not P0 > f(p0) * f(s2 * s2))


def test_eigenvalue_form_of_the_inverted_pair():
    """lambda_max(-B) = s1 + s2 - sign(det B) s3, so r- = sqrt((G - 2 lambda_max(-B)) / A) = rmsd_and_max(p, -q)[0].
    Bar 1e-10: the difference carries a few ulp of G, i.e. d(r^2) ~ 1e-15 G / A ~ 1e-14 A^2 here, and
    dr = d(r^2) / (2 r) stays below 1e-12 for r >= 0.01 A, the closest pairs generated."""
    P, Q = _random_pairs(3000, seed=5)
    worst = 0.0
    for p, q in zip(P, Q):
        B = p.T @ q
        G = (p * p).sum() + (q * q).sum()
        sv = np.linalg.svd(B, compute_uv=False)
        for sign, qq in ((1.0, q), (-1.0, -q)):
            lam = sv[0] + sv[1] + sign * np.sign(np.linalg.det(B)) * sv[2]
            r = np.sqrt(max(G - 2.0 * lam, 0.0) / len(p))
            worst = max(worst, abs(r - o.rmsd_and_max(p, qq)[0]))
    assert worst < 1e-10, worst


def test_screen_tests_at_abs_det_are_the_or_of_both_handednesses():
    """the fp64 three-test and the fp32 two-test polynomial at |det B| == (test at +det B) or (test at -det B), as
    booleans, on every pair -- planar pairs (det B = 0) included -- at thresholds that put pairs on both sides"""
    P, Q = _random_pairs(3000, seed=6)
    n_may = n_not = n_planar = n_only_inverted = 0
    for k, (p, q) in enumerate(zip(P, Q)):
        B = p.T @ q
        G = (p * p).sum() + (q * q).sum()
        thr = (0.1, 0.5, 1.5)[k % 3]
        A_thr2 = len(p) * (thr * thr + 1e-6)
        n_planar += _cov_terms(B)[1] == 0.0
        for may in (lambda d: _may_f64(B, G, A_thr2, d), lambda d: _may_f32_2t(B, G, A_thr2, 1e-4, 2e-5, d)):
            at_abs, plus, minus = may(abs), may(lambda d: d), may(lambda d: -d)
            assert at_abs == (plus or minus), k
            n_may += at_abs
            n_not += not at_abs
            n_only_inverted += minus and not plus
    assert n_planar >= 300 and n_may > 500 and n_not > 500 and n_only_inverted > 50


# ---- 2. properties of the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
def test_restatement_properties(seed):
    N, A, thr = 60, 12, 0.5
    X, atoms, _ = syn.synthetic_ensemble(N, A, seed=seed)
    plain = er.similarity(X, atoms, thr)
    assert plain.min_gap > GAP, "choose another seed"
    # contains the default matrix, which is the oracle's
    assert np.array_equal(plain.S_default, o.rmsd_similarity_matrix(X, atoms, thr)[0])
    assert not (plain.S_default & ~plain.S).any()
    # random-walk skeletons are far from their own mirror images: nothing changes on an unreflected ensemble
    _, m_default = o.prune_by_rmsd(X, atoms, thr)
    _, m_enant, _ = er.prune_by_rmsd_enant(X, atoms, thr)
    assert np.array_equal(m_enant, m_default)
    _, m_pairwise, _ = er.prune_by_rmsd_enant(X, atoms, thr, from_matrix=False)
    assert np.array_equal(m_pairwise, m_enant)  # greedy_prune and greedy_prune_from_matrix agree on the predicate
    # reflecting ANY subset leaves the enantiomer-aware bits and mask alone and changes the default mask
    rng = np.random.default_rng(seed + 100)
    for trial in range(3):
        flip = rng.random(N) < (0.5, 0.2, 0.8)[trial]
        Y = er.reflect(X, flip, axis=trial)
        mats = er.similarity(Y, atoms, thr)
        assert mats.min_gap > GAP
        assert np.array_equal(mats.S, plain.S)
        assert np.array_equal(er.pack_bits(mats.S), er.pack_bits(plain.S))
        _, m_y, _ = er.prune_by_rmsd_enant(Y, atoms, thr)
        assert np.array_equal(m_y, m_enant)
        _, m_y_default = o.prune_by_rmsd(Y, atoms, thr)
        assert not np.array_equal(m_y_default, m_default) and m_y_default.sum() > m_default.sum()


def test_similar_enant_is_the_or_of_two_complete_tests():
    """not "the smaller rmsd, then its max deviation": a pair whose inverted rmsd passes and whose inverted max
    deviation fails is dissimilar even when r- < r+"""
    rng = np.random.default_rng(0)
    p = rng.normal(size=(30, 3))
    p -= p.mean(axis=0)
    q = -p.copy()
    q[0] += (0.0, 0.0, 1.2)  # one atom far off: r- = 1.2 / sqrt(30) = 0.22 < 0.5, m- = 1.2 > 1.0
    q -= q.mean(axis=0)
    r_m, m_m = o.rmsd_and_max(p, -q)
    r_p, _ = o.rmsd_and_max(p, q)
    assert r_m < 0.5 < r_p and m_m > 1.0
    assert not er.similar_enant(p, q, 0.5, 1.0)
    assert er.similar_enant(p, q, 0.5, 1.5)


# ---- 3. the boundary -------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fc_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/fc_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.fc_abi_version() == 1


def test_keyword_defaults():
    import firecode_amd as fc

    def default(fn, name):
        return inspect.signature(fn).parameters[name].default

    assert default(_lib.DeviceEnsemble.rmsd_pairs, "inverted") is False
    assert default(_lib.DeviceEnsemble.simbits, "prune_enantiomers") is False
    assert default(_lib.DeviceEnsemble.prune, "prune_enantiomers") is False
    assert default(fc.rmsd.rmsd_and_max, "inverted") is False
    assert default(fc.rmsd.rmsd_and_max_batch, "inverted") is False
    for fn in (fc.pruner.prune_by_rmsd, fc.pruner.prune_similarity, fc.pruner.prune,
               fc.ensemble.Ensemble.similarity_pruning, fc.refining.similarity_refining):
        assert default(fn, "prune_enantiomers") is False, fn
    assert default(fc.operators.gpu_prune_operator, "prune_enantiomers") is None
    # the positional signatures stay
    assert list(inspect.signature(fc.rmsd.rmsd_and_max).parameters)[:3] == ["p", "q", "center"]
    assert list(inspect.signature(fc.operators.gpu_prune_operator).parameters)[:5] == [
        "filename", "embedder", "moi", "rmsd", "rmsd_rot_corr"]


@pytest.mark.parametrize("bad", [1, 0, "yes", None, np.ones(2, dtype=bool)])
def test_non_bool_flags_are_input_errors_before_any_device_use(bad):
    import firecode_amd as fc

    X, atoms = np.zeros((3, 4, 3)), np.array(["C"] * 4)
    calls = [
        lambda: fc.rmsd.rmsd_and_max(X[0], X[1], inverted=bad),
        lambda: fc.rmsd.rmsd_and_max_batch(X, [0], [1], inverted=bad),
        lambda: fc.pruner.prune_by_rmsd(X, atoms, 0.5, prune_enantiomers=bad),
        lambda: fc.pruner.prune_similarity(X, atoms, prune_enantiomers=bad),
        lambda: fc.pruner.prune(X, atoms, prune_enantiomers=bad),
        lambda: fc.ensemble.Ensemble(atoms, X, logfunction=None).similarity_pruning(prune_enantiomers=bad),
        lambda: fc.refining.similarity_refining(X, atoms, prune_enantiomers=bad),
        # (the methods check the flag before they touch the handle)
        lambda: _lib.DeviceEnsemble.rmsd_pairs(object(), [0], [1], inverted=bad),
        lambda: _lib.DeviceEnsemble.simbits(object(), 0.5, 1.0, prune_enantiomers=bad),
        lambda: _lib.DeviceEnsemble.prune(object(), 0.5, 1.0, prune_enantiomers=bad),
    ]
    if bad is not None:  # None is the operator's "read the embedder's option"
        calls.append(lambda: fc.operators.gpu_prune_operator("x.xyz", object(), prune_enantiomers=bad))
    for call in calls:
        with pytest.raises(fc.FirecodeHipInputError):
            call()


def test_no_cpu_fallback_for_the_new_calls():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import firecode_amd as fc

    X, atoms = np.zeros((3, 4, 3)), np.array(["C"] * 4)
    for call in (lambda: fc.rmsd.rmsd_and_max(X[0], X[1] + 1.0, inverted=True),
                 lambda: fc.rmsd.rmsd_and_max_batch(X, [0], [1], center=True, inverted=True),
                 lambda: fc.pruner.prune_by_rmsd(X, atoms, 0.5, prune_enantiomers=True),
                 lambda: fc.pruner.prune_similarity(X, atoms, prune_enantiomers=True),
                 lambda: _lib.DeviceEnsemble(X).prune(0.5, 1.0, prune_enantiomers=True)):
        with pytest.raises(fc.FirecodeHipDeviceError):
            call()
