"""Enantiomer-aware RMSD prune on the GPU (fc_prune_rmsd_enant, fc_rmsd_simbits_enant, the inverted pair values and the
Python layers above them) against the NumPy restatement of the contract (tests/enant_ref.py on oracle.cpu_ref).

Bars: masks and similarity bits identical, values within 1e-10.  Every ensemble asserts ``min_gap > 1e-9`` from the
restatement first, so no pair is ever exempted."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import enant_ref as er
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
GAP = 1e-9
THR = 0.5
LANES_MIN = 1 << 17  # candidate queues longer than this take the one-lane-per-pair refine kernels


# ---- ensembles -----------------------------------------------------------------------------------------------------------
def clustered(N, A, seed, compact=False):
    """synthetic_ensemble with a random half of the conformers reflected in x"""
    X, atoms, assign = syn.synthetic_ensemble(N, A, seed=seed, compact=compact)
    flip = np.random.default_rng(seed + 100).random(N) < 0.5
    X[flip, :, 0] *= -1.0
    return X, atoms, assign, flip


def continuous(N, A, seed):
    """continuous_ensemble with a random half of the conformers reflected in z"""
    X = syn.continuous_ensemble(N, A, seed=seed)
    flip = np.random.default_rng(seed).random(N) < 0.5
    X[flip, :, 2] *= -1.0
    return X, np.array(["C"] * A)


def planar(N, A, seed, out_of_plane):
    """noisy copies of one flat structure (in-plane sigma 0.05, out-of-plane ``out_of_plane``), randomly rotated"""
    rng = np.random.default_rng(seed)
    base = np.zeros((A, 3))
    base[:, :2] = syn.compact_skeleton(A, rng)[:, :2] * 2.0
    X = base[None] + rng.normal(size=(N, A, 3)) * np.array([0.05, 0.05, out_of_plane])
    if out_of_plane > 0.0:
        X = np.stack([x @ syn.random_rotation(rng).T for x in X])
    return np.ascontiguousarray(X), np.array(["C"] * A)


@functools.lru_cache(maxsize=None)
def _named(name):
    """the ensembles of the parity cases by name (shared with the child processes) -> (X, atoms)"""
    kind, *args = name.split(":")
    if kind == "clustered":
        return clustered(int(args[0]), int(args[1]), int(args[2]), compact=len(args) > 3)[:2]
    if kind == "continuous":
        return continuous(int(args[0]), int(args[1]), int(args[2]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name, thr=THR):
    """the restatement of a named ensemble, computed once: (EnantMatrices, enantiomer-aware mask, default mask)"""
    X, atoms = _named(name)
    mats = er.similarity(X, atoms, thr)
    assert mats.min_gap > GAP, f"{name}: a decisive value within {mats.min_gap:.3g} of its threshold: choose another seed"
    return mats, o.greedy_prune_from_matrix(mats.S), o.greedy_prune_from_matrix(mats.S_default)


def _device_results(fc, X, thr=THR, twice=False):
    """default prune, enantiomer-aware bits and prune, then the default calls again, on ONE handle"""
    from firecode_amd import _lib

    out = {}
    iu, ju = np.triu_indices(len(X), 1)
    pick = np.random.default_rng(0).choice(len(iu), size=min(len(iu), 500), replace=False)
    with fc.DeviceEnsemble(X, center=True) as ens:
        out["mask_default_before"], out["stats_default"] = ens.prune(thr, 2 * thr)
        out["kind_default"] = _lib.screen_last_kind()
        bits, out["grey"] = ens.simbits(thr, 2 * thr, prune_enantiomers=True)
        out["kind_bits"] = _lib.screen_last_kind()
        out["bits"] = _lib.unpack_bits(bits, len(X))
        out["mask"], out["stats"] = ens.prune(thr, 2 * thr, prune_enantiomers=True)
        out["kind"] = _lib.screen_last_kind()
        if twice:  # the refine's form follows the LAST prune's queue length: the same prune again takes the other form
            out["mask_again"], out["stats_again"] = ens.prune(thr, 2 * thr, prune_enantiomers=True)
        # nothing moved: the default calls in the same process, on the same handle, after the enantiomer-aware ones
        out["mask_default"], _ = ens.prune(thr, 2 * thr)
        bits0, out["grey_default"] = ens.simbits(thr, 2 * thr)
        out["kind_bits_default"] = _lib.screen_last_kind()
        out["bits_default"] = _lib.unpack_bits(bits0, len(X))
        if len(pick):
            out["pairs"] = np.stack([iu[pick], ju[pick]])
            out["values_default"] = np.stack(ens.rmsd_pairs(iu[pick], ju[pick]))
            out["values_inverted"] = np.stack(ens.rmsd_pairs(iu[pick], ju[pick], inverted=True))
    return out


def _assert_parity(got, mats, mask_enant, mask_default, label=""):
    n = len(mask_enant)
    assert np.array_equal(got["bits"], np.triu(mats.S, 1)), label
    assert np.array_equal(got["mask"], mask_enant), label
    assert int(got["grey"]) == 0 and int(got["stats"][3]) == 0, label
    assert int(got["stats"][2]) == int(np.triu(mats.S, 1).sum()) and int(got["stats"][5]) == int(mask_enant.sum()), label
    assert int(got["stats"][0]) == n * (n - 1) // 2, label
    # the screen that runs is the default call's: prune against prune (lean launches), bits against bits (the 32-column
    # tiles exist for lean launches only, so the two may differ from each other)
    assert int(got["kind"]) == int(got["kind_default"]), label
    assert int(got["kind_bits"]) == int(got["kind_bits_default"]), label
    # nothing moved
    for key in ("mask_default_before", "mask_default"):
        assert np.array_equal(got[key], mask_default), (label, key)
    assert np.array_equal(got["bits_default"], np.triu(mats.S_default, 1)) and int(got["grey_default"]) == 0, label
    if "pairs" in got:
        i, j = got["pairs"]
        assert np.abs(got["values_default"][0] - mats.Rp[i, j]).max() < TOL, label
        assert np.abs(got["values_default"][1] - mats.Mp[i, j]).max() < TOL, label
        assert np.abs(got["values_inverted"][0] - mats.Rm[i, j]).max() < TOL, label
        assert np.abs(got["values_inverted"][1] - mats.Mm[i, j]).max() < TOL, label
    if "mask_again" in got:
        assert np.array_equal(got["mask_again"], mask_enant), label
        assert int(got["stats_again"][2]) == int(got["stats"][2]), label


# ---- 4. values -------------------------------------------------------------------------------------------------------
def _value_structures(kind, A, rng, K=24):
    if kind == "random":
        P, Q = rng.normal(scale=2.0, size=(K, A, 3)), rng.normal(scale=2.0, size=(K, A, 3))
    elif kind == "clustered":
        P = rng.normal(scale=2.0, size=(K, A, 3))
        Q = np.stack([p @ syn.random_rotation(rng).T for p in P]) + rng.normal(scale=0.05, size=(K, A, 3))
    elif kind == "reflected":  # r- ~ 0: a rotated mirror image of the partner (exact for the odd ones)
        P = rng.normal(scale=2.0, size=(K, A, 3))
        Q = np.stack([(p * np.array([1.0, 1.0, -1.0])) @ syn.random_rotation(rng).T for p in P])
        Q[::2] += rng.normal(scale=1e-3, size=Q[::2].shape)
    elif kind == "planar":
        P, Q = rng.normal(scale=2.0, size=(K, A, 3)), rng.normal(scale=2.0, size=(K, A, 3))
        P[:, :, 2] = 0.0
        Q[:, :, 2] = 0.0
    else:  # collinear
        P = rng.normal(scale=2.0, size=(K, A, 1)) * np.array([1.0, 0.0, 0.0])
        Q = rng.normal(scale=2.0, size=(K, A, 1)) * np.array([0.0, 1.0, 0.0])
    return P + rng.normal(scale=3.0, size=(K, 1, 3)), Q + rng.normal(scale=3.0, size=(K, 1, 3))


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("kind", ["random", "clustered", "reflected", "planar", "collinear"])
def test_inverted_values(fc, kind, center):
    """rmsd_and_max_batch(..., inverted=True) and rmsd_and_max(p, q, center, inverted=True) against the oracle on
    (P, -Q), 3 ... 200 atoms, with and without an atom mask; the default values on the same arrays beside them"""
    rng = np.random.default_rng(17)
    for A in (3, 4, 7, 30, 64, 200):
        P, Q = _value_structures(kind, A, rng)
        K = len(P)
        X = np.concatenate([P, Q])
        pi, pj = np.arange(K), np.arange(K) + K
        for am in (None, rng.random(A) < 0.7):
            if am is not None and am.sum() < 3:
                am[:3] = True
            sel = slice(None) if am is None else am
            r0, m0 = o.rmsd_and_max_batch(P[:, sel], -Q[:, sel], center)
            if center:  # centre first, then negate: the same numbers, said the way the contract says it
                Qc = Q[:, sel] - Q[:, sel].mean(axis=1, keepdims=True)
                r1, m1 = o.rmsd_and_max_batch(P[:, sel] - P[:, sel].mean(axis=1, keepdims=True), -Qc, False)
                assert np.abs(r1 - r0).max() < 1e-12 and np.abs(m1 - m0).max() < 1e-12
            r, m = fc.rmsd.rmsd_and_max_batch(X, pi, pj, center=center, atom_mask=am, inverted=True)
            assert np.abs(r - r0).max() < TOL and np.abs(m - m0).max() < TOL, (kind, A, center)
            rd, md = fc.rmsd.rmsd_and_max_batch(X, pi, pj, center=center, atom_mask=am)
            rd0, md0 = o.rmsd_and_max_batch(P[:, sel], Q[:, sel], center)
            assert np.abs(rd - rd0).max() < TOL and np.abs(md - md0).max() < TOL, (kind, A, center)
        for k in (0, 1):
            r, m = fc.rmsd.rmsd_and_max(P[k], Q[k], center, inverted=True)
            r0, m0 = o.rmsd_and_max(P[k], -Q[k], center)
            assert abs(r - r0) < TOL and abs(m - m0) < TOL, (kind, A, center)
    if kind == "reflected":
        r, _ = fc.rmsd.rmsd_and_max_batch(X, pi, pj, center=True, inverted=True)
        assert r[1::2].max() < 1e-10 and r[::2].max() < 1e-2  # the mirror image superposes


# ---- 5. / 6. / 11. prune parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,A,seed", [(1, 5, 1), (2, 5, 1), (64, 20, 7), (300, 30, 3), (400, 50, 2), (600, 80, 4),
                                      (300, 200, 5)])
def test_prune_parity_clustered(fc, N, A, seed):
    name = f"clustered:{N}:{A}:{seed}"
    X, atoms = _named(name)
    mats, mask_enant, mask_default = _reference(name)
    _assert_parity(_device_results(fc, X), mats, mask_enant, mask_default, name)
    assert np.array_equal(mask_default, o.prune_by_rmsd(X, atoms, THR)[1])
    _, _, assign, flip = clustered(N, A, seed)
    if N >= 64:  # survivors: one per cluster with the flag, one per (cluster, hand) without
        assert int(mask_enant.sum()) == len(np.unique(assign))
        assert int(mask_default.sum()) == len(set(zip(assign.tolist(), flip.tolist())))
    if (N, A, seed) == (300, 30, 3):
        assert (int(mask_enant.sum()), int(mask_default.sum())) == (60, 116)
    if (N, A, seed) == (400, 50, 2):
        assert (int(mask_enant.sum()), int(mask_default.sum())) == (80, 154)


@pytest.mark.parametrize("seed", [11, 12])
def test_prune_parity_continuous(fc, seed):
    """no cluster structure: the inverted max-deviation test decides pairs on its own and hundreds of pairs are similar
    only as mirror images"""
    name = f"continuous:500:50:{seed}"
    X, atoms = _named(name)
    mats, mask_enant, mask_default = _reference(name)
    only_mirror = int(np.triu(mats.S & ~mats.S_default, 1).sum())
    fails_on_m = int(np.triu((mats.Rm < THR) & ~(mats.Mm < 2 * THR), 1).sum())
    assert only_mirror > 500 and fails_on_m > 50, (only_mirror, fails_on_m)
    _assert_parity(_device_results(fc, X), mats, mask_enant, mask_default, name)
    assert mask_enant.sum() < mask_default.sum()


# ---- 7. both hands at once ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_of_plane", [0.15, 0.0])
def test_near_planar_and_planar(fc, out_of_plane):
    X, atoms = planar(200, 30, seed=21, out_of_plane=out_of_plane)
    mats = er.similarity(X, atoms, THR)
    assert mats.min_gap > GAP, "choose another seed"
    assert np.triu(mats.S_default, 1).sum() == 200 * 199 // 2  # every pair similar in the proper handedness ...
    assert ((mats.Rm < THR) & (mats.Mm < 2 * THR))[np.triu_indices(200, 1)].all()  # ... and in the inverted one
    got = _device_results(fc, X)
    _assert_parity(got, mats, o.greedy_prune_from_matrix(mats.S), o.greedy_prune_from_matrix(mats.S_default))
    assert got["mask"].sum() == 1 and got["bits"][np.triu_indices(200, 1)].all()


# ---- 8. every screen kind, every refine form ---------------------------------------------------------------------------
def _admitted_kinds(X, lean, thr=THR):
    """the kinds of 16 / 32 / 64 that the plan admits for this shape when forced (fc_debug_screen_plan)"""
    from firecode_amd import _lib

    Xp = er.prepared(X, np.array(["C"] * X.shape[1]))
    g_max = float((Xp * Xp).sum(axis=(1, 2)).max())
    kinds = []
    for kind in (16, 32, 64):
        out = np.zeros(5, dtype=np.int64)
        _lib.screen_select(kind)
        try:
            rc = _lib.load().fc_debug_screen_plan(X.shape[0], X.shape[1], 128, int(lean), g_max, thr, 1, _lib.pi(out))
        finally:
            _lib.screen_select(0)
        if rc == 0 and int(out[0]) == kind:
            kinds.append(kind)
    return kinds


@pytest.mark.parametrize("name", ["clustered:300:30:3", "continuous:500:50:11", "clustered:200:224:6:compact",
                                  "clustered:200:260:8:compact"])
def test_every_screen_kind(fc, monkeypatch, name):
    from firecode_amd import _lib

    X, atoms = _named(name)
    mats, mask_enant, mask_default = _reference(name)
    # kinds both launch forms admit (none at 224 / 260 atoms: no 64-column tile fits, the bit-matrix launch is VALU there)
    kinds = sorted(set(_admitted_kinds(X, lean=True)) & set(_admitted_kinds(X, lean=False)))
    assert _admitted_kinds(X, lean=True), "no matrix-pipe screen admitted for this shape"
    if X.shape[1] >= 224:
        assert set(_admitted_kinds(X, lean=True)) >= {16, 32}, "the 32-column tiles were meant to run here"
    monkeypatch.delenv("FC_SCREEN_F32", raising=False)
    for kind in kinds:
        _lib.screen_select(kind)
        try:
            got = _device_results(fc, X)
        finally:
            _lib.screen_select(0)
        assert got["kind"] == got["kind_bits"] == got["kind_default"] == got["kind_bits_default"] == kind, (name, kind)
        _assert_parity(got, mats, mask_enant, mask_default, (name, kind))
    # 32-column tiles exist for lean launches only: the prune alone, for the kinds only it admits
    for kind in sorted(set(_admitted_kinds(X, lean=True)) - set(kinds)):
        _lib.screen_select(kind)
        try:
            with fc.DeviceEnsemble(X, center=True) as ens:
                m0, _ = ens.prune(THR, 2 * THR)
                k0 = _lib.screen_last_kind()
                m1, st = ens.prune(THR, 2 * THR, prune_enantiomers=True)
                k1 = _lib.screen_last_kind()
        finally:
            _lib.screen_select(0)
        assert k0 == k1 == kind and np.array_equal(m0, mask_default) and np.array_equal(m1, mask_enant), (name, kind)
        assert int(st[2]) == int(np.triu(mats.S, 1).sum())
    # the VALU screen, and the speculative verdict behind the single-precision screens
    monkeypatch.setenv("FC_SCREEN_CFG", "valu")
    got = _device_results(fc, X)
    monkeypatch.delenv("FC_SCREEN_CFG")
    assert got["kind"] == got["kind_default"] == 1
    _assert_parity(got, mats, mask_enant, mask_default, (name, "valu"))
    monkeypatch.setenv("FC_SCREEN_F32", "3")
    got = _device_results(fc, X)
    monkeypatch.delenv("FC_SCREEN_F32")
    _assert_parity(got, mats, mask_enant, mask_default, (name, "speculative"))


def test_word_queue_fallback(fc, monkeypatch):
    """a candidate-pair queue too short for the candidates: the refine takes the word queue, which carries no polynomial
    verdict and evaluates both handednesses of every candidate"""
    monkeypatch.setenv("FC_PAIRQ_CAP", "64")
    for name in ("clustered:300:30:3", "continuous:500:50:12"):
        X, atoms = _named(name)
        _assert_parity(_device_results(fc, X), *_reference(name), label=name)


BIG = "continuous:2000:50:11"
BIG_THR = 0.7


def test_long_candidate_queue(fc):
    """a queue above 2^17 pairs: the first prune of a handle takes the straight walk (k_refine_pairs), the next one --
    the form follows the last prune's queue length -- the bucket refine"""
    X, atoms = _named(BIG)
    mats, mask_enant, mask_default = _reference(BIG, BIG_THR)
    assert np.triu(mats.S, 1).sum() > LANES_MIN
    got = _device_results(fc, X, thr=BIG_THR, twice=True)
    assert int(got["stats"][1]) > LANES_MIN and int(got["stats_again"][1]) > LANES_MIN
    assert int(got["stats_default"][1]) > 0
    _assert_parity(got, mats, mask_enant, mask_default, BIG)


def child_main(out_path, thr, *names):
    """(child process) the device results of the named ensembles -> one .npz"""
    import firecode_amd as fc

    fc.init(0)
    out = {}
    for name in names:
        for key, value in _device_results(fc, _named(name)[0], thr=float(thr), twice=True).items():
            out[f"{name}|{key}"] = np.asarray(value)
    np.savez(out_path, **out)


@pytest.mark.parametrize("knob", ["FC_SCREEN_STAGES=1", "FC_REFINE_LANES=0", "FC_REFINE_BUCKETS=0"])
def test_once_per_process_knobs(fc, tmp_path, knob):
    """the switches the library reads once per process, each in a fresh child: the single-stage fp32 launch, the refine
    without the one-lane-per-pair kernels (k_simbits_refine takes every queue) and without the bucket form (the
    straight walk takes the long queues)"""
    key, value = knob.split("=")
    runs = [(THR, ["clustered:400:50:2", "continuous:500:50:12"])]
    if key != "FC_SCREEN_STAGES":
        runs.append((BIG_THR, [BIG]))
    for thr, names in runs:
        out_path = str(tmp_path / f"{key}_{thr}.npz")
        code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_enant as t\nt.child_main(%r, %r, *%r)\n"
                % (ROOT, os.path.join(ROOT, "tests"), out_path, thr, names))
        env = dict(os.environ, **{key: value})
        env.pop("FC_SCREEN_F32", None)
        done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
        assert done.returncode == 0, done.stderr[-3000:]
        data = np.load(out_path)
        for name in names:
            got = {k.split("|", 1)[1]: data[k] for k in data.files if k.startswith(name + "|")}
            _assert_parity(got, *_reference(name, thr), label=(knob, name))
            if name == BIG:
                assert int(got["stats"][1]) > LANES_MIN


# ---- 9. energies and the other ladder rule -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clustered:300:30:3", "continuous:500:50:11"])
def test_energies_and_drop_later(fc, name):
    from firecode_amd import _lib

    X, atoms = _named(name)
    mats, _, _ = _reference(name)
    rng = np.random.default_rng(5)
    energies = rng.normal(scale=1.0, size=len(X))
    for max_dE in (0.3, 1.5):
        dE = np.abs(energies[:, None] - energies[None, :])[np.triu_indices(len(X), 1)]
        assert np.abs(dE - max_dE).min() > GAP
        _, ref_mask, _ = er.prune_by_rmsd_enant(X, atoms, THR, energies=energies, max_dE=max_dE)
        _, mask = fc.pruner.prune_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE, prune_enantiomers=True)
        assert np.array_equal(mask, ref_mask), (name, max_dE)
        with fc.DeviceEnsemble(X, center=True) as ens:
            bits, grey = ens.simbits(THR, 2 * THR, energies=energies, max_dE=max_dE, prune_enantiomers=True)
        ref_bits = _lib.unpack_bits(er.pack_bits(mats.S, energies, max_dE), len(X))
        assert np.array_equal(_lib.unpack_bits(bits, len(X)), ref_bits) and grey == 0
        _, mask0 = fc.pruner.prune_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE)
        assert np.array_equal(mask0, o.prune_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE)[1])
    # the mirror rule of the ladder (fc_prune_conventions(1)), served by the pair ladder
    fc.pruner.CONVENTIONS["drop"] = "later"
    try:
        _, mask = fc.pruner.prune_by_rmsd(X, atoms, THR, prune_enantiomers=True)
        _, mask_e = fc.pruner.prune_by_rmsd(X, atoms, THR, energies=energies, max_dE=1.5, prune_enantiomers=True)
    finally:
        fc.pruner.CONVENTIONS["drop"] = "earlier"
        _lib.call("fc_prune_conventions", 0)
    assert np.array_equal(mask, o.greedy_prune_from_matrix(mats.S, drop="later"))
    assert np.array_equal(mask_e, er.prune_by_rmsd_enant(X, atoms, THR, energies=energies, max_dE=1.5, drop="later")[1])


# ---- 10. the drivers -------------------------------------------------------------------------------------------------
class _Options:
    rmsd = THR


class _Mol:
    def __init__(self, atoms, coords, basename):
        self.atoms, self.coords, self.basename, self.graph = atoms, coords, basename, None


class _Embedder:
    def __init__(self, mol, **options):
        self.mols = {"mol.xyz": mol}
        self.options = _Options()
        for key, value in options.items():
            setattr(self.options, key, value)
        self.lines = []

    def log(self, msg=""):
        self.lines.append(msg)


def test_drivers(fc, tmp_path, monkeypatch):
    name = "clustered:300:30:3"
    X, atoms = _named(name)
    mats, mask_enant, mask_default = _reference(name)
    # prune_similarity / prune: MOI stage unchanged, then the enantiomer-aware RMSD stage on its survivors
    m_moi0, m_both0, counts0 = fc.pruner.prune_similarity(X, atoms, max_rmsd=THR)
    m_moi, m_both, counts = fc.pruner.prune_similarity(X, atoms, max_rmsd=THR, prune_enantiomers=True)
    assert np.array_equal(m_moi, m_moi0) and counts[0] == counts0[0] and counts[1] == counts0[1]
    keep = np.flatnonzero(m_moi)
    sub = er.similarity(X[keep], atoms, THR)
    assert sub.min_gap > GAP
    expect = np.zeros(len(X), dtype=bool)
    expect[keep[o.greedy_prune_from_matrix(sub.S)]] = True
    assert np.array_equal(m_both, expect) and tuple(counts) == (len(X), len(keep), int(expect.sum()))
    _, m_rmsd_only, counts_r = fc.pruner.prune_similarity(X, atoms, moi=False, max_rmsd=THR, prune_enantiomers=True)
    assert np.array_equal(m_rmsd_only, mask_enant) and tuple(counts_r) == (len(X), len(X), int(mask_enant.sum()))
    _, m_moi_only, _ = fc.pruner.prune_similarity(X, atoms, rmsd=False, max_rmsd=THR, prune_enantiomers=True)
    assert np.array_equal(m_moi_only, m_moi0)
    assert np.array_equal(fc.pruner.prune(X, atoms, max_rmsd=THR, prune_enantiomers=True)[1], expect)
    assert np.array_equal(fc.pruner.prune(X, atoms, max_rmsd=THR)[1], m_both0)
    debug = []
    _, m = fc.pruner.prune_by_rmsd(X, atoms, THR, prune_enantiomers=True, debugfunction=debug.append)
    assert np.array_equal(m, mask_enant) and "mirror images included" in debug[0]
    debug = []
    _, m = fc.pruner.prune_by_rmsd(X, atoms, THR, debugfunction=debug.append)
    assert np.array_equal(m, mask_default) and "mirror" not in debug[0]

    # Ensemble.similarity_pruning and similarity_refining: the flag reaches the RMSD stage only; the log says so
    for moi in (False, True):
        want = {False: m_both0 if moi else mask_default, True: expect if moi else mask_enant}
        for flag in (False, True):
            log = []
            ens = fc.ensemble.Ensemble(atoms, X.copy(), logfunction=log.append)
            ens.similarity_pruning(moi=moi, rmsd=True, max_rmsd=THR, prune_enantiomers=flag)
            assert np.array_equal(ens.coords, X[want[flag]]), (moi, flag)
            rmsd_lines = [line for line in log if "RMSD similarity" in line]
            assert len(rmsd_lines) == 1 and ("RMSD similarity (mirror images included)" in rmsd_lines[0]) == flag
            log = []
            mask = fc.refining.similarity_refining(X, atoms, rmsd_thr=THR, moi=moi, logfunction=log.append,
                                                   prune_enantiomers=flag)
            assert np.array_equal(mask, want[flag]), (moi, flag)
            rmsd_lines = [line for line in log if "RMSD similarity" in line]
            assert len(rmsd_lines) == 1 and ("RMSD similarity (mirror images included)" in rmsd_lines[0]) == flag
            assert all("mirror" not in line for line in log if "MOI" in line)

    # the operator: None reads options.keep_enantiomers; an embedder without it behaves as before
    monkeypatch.chdir(tmp_path)
    for options, argument, want_mask in (({}, None, m_both0), ({"keep_enantiomers": True}, None, m_both0),
                                         ({"keep_enantiomers": False}, None, expect),
                                         ({"keep_enantiomers": True}, True, expect),
                                         ({"keep_enantiomers": False}, False, m_both0)):
        emb = _Embedder(_Mol(atoms, X, str(tmp_path / "mol")), **options)
        outname = fc.operators.gpu_prune_operator("mol.xyz", emb, prune_enantiomers=argument)
        _, kept = fc._lib.xyz_read(outname)
        assert len(kept) == int(want_mask.sum()), (options, argument)
        assert np.abs(kept - X[want_mask]).max() < 1e-5, (options, argument)
