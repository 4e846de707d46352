"""Nearest neighbours across two ensembles on the GPU (fc_ensemble_knn_cross and the Python layers above it) against
the NumPy restatement of its contract (tests/knn_cross_ref.py) on the oracle's Kabsch RMSD.

Bars, those of test_gpu_knn.py: indices identical (-1 padding included), distances within 1e-10 (+inf where padded) --
on cases whose every decision the restatement recorded with a gap above 1e-9 (consecutive sorted distances of a row
among positions 1 ... k + 1; with a cap, every pair's distance to the cap), asserted first, so that rounding cannot
flip one.  No row is left out of any comparison."""

import ctypes as C

import numpy as np
import pytest

import knn_cross_ref as xr
from firecode_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9

SHAPES = [(1, 1, 5), (3, 2, 5), (5, 64, 20), (65, 257, 7), (257, 65, 50), (16, 600, 80), (40, 300, 200), (5, 70, 300)]
CAP_SHAPES = [(65, 257, 7), (16, 600, 80), (5, 70, 300)]

_CASES = {}  # (kind, Nq, Nr, A) -> (queries, references, atoms, oracle rows), made once and shared, never written to


def _case(kind, Nq, Nr, A):
    key = (kind, Nq, Nr, A)
    if key not in _CASES:
        seed = Nq + Nr + A
        if kind == "clusters":
            X, atoms, _ = syn.synthetic_ensemble(Nq + Nr, A, seed=seed)
        else:
            X, atoms = syn.continuous_ensemble(Nq + Nr, A, seed=seed), np.array(["C"] * A)
        p = np.random.default_rng(seed).permutation(Nq + Nr)
        Q, R = np.ascontiguousarray(X[p[:Nq]]), np.ascontiguousarray(X[p[Nq:]])
        D = xr.distance_rows(xr.prepared(Q, atoms), xr.prepared(R, atoms))
        for a in (Q, R, D):
            a.setflags(write=False)
        _CASES[key] = (Q, R, atoms, D)
    return _CASES[key]


def _middle_cap(D):
    """the midpoint of the two middle values of all sorted pair distances: about half of the pairs are within it"""
    v = np.sort(D.reshape(-1))
    m = (len(v) - 1) // 2
    return 0.5 * (v[m] + v[m + 1])


def _tight_cap(D):
    """a cap of the test's own, between two of the smallest pair distances (the 2 % quantile): most lists end in padding
    and some queries have no reference within it"""
    v = np.sort(D.reshape(-1))
    m = len(v) // 50
    return 0.5 * (v[m] + v[m + 1])


def _check(got, ref, Nq, k, what=""):
    idx, dist = got
    assert ref.min_gap > GAP, f"the case has a near-tie ({ref.min_gap:.3g}): choose another"
    assert idx.dtype == np.int32 and idx.shape == (Nq, k) and dist.dtype == np.float64 and dist.shape == (Nq, k)
    assert np.array_equal(idx, ref.indices)
    pad = ref.indices < 0
    assert np.all(np.isposinf(dist[pad])) and np.all(np.isfinite(dist[~pad]))
    err = np.abs(dist[~pad] - ref.distances[~pad]).max(initial=0.0)
    print(f"{what} Nq={Nq} k={k} gap={ref.min_gap:.3g} padded={int(pad.sum())} max|d - ref|={err:.3g}")
    assert err < TOL


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("kind", ["clusters", "continuous"])
@pytest.mark.parametrize("Nq,Nr,A", SHAPES)
def test_knn_cross_parity(fc, kind, Nq, Nr, A, k):
    """lists longer than the reference set, Nq and Nr that are no multiple of 16 and 64 in both orders (so that the two
    paddings differ), one query tile against many strips, and 300 atoms, beyond the LDS stage"""
    Q, R, atoms, D = _case(kind, Nq, Nr, A)
    nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k)
    _check((nb.indices, nb.distances), xr.knn_from_rows(D, k), Nq, k, f"{kind} Nr={Nr} A={A}")


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("kind", ["clusters", "continuous"])
@pytest.mark.parametrize("Nq,Nr,A", CAP_SHAPES)
def test_knn_cross_cap(fc, kind, Nq, Nr, A, k):
    """the cap at the middle of all pair distances: the capped lists against the restatement, and as the uncapped device
    lists with the entries d >= max_rmsd replaced by -1 / +inf; novelty and coverage against the restatement"""
    Q, R, atoms, D = _case(kind, Nq, Nr, A)
    cap = _middle_cap(D)
    assert np.abs(D - cap).min() > GAP
    ref = xr.knn_from_rows(D, k, cap)
    nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap)
    _check((nb.indices, nb.distances), ref, Nq, k, f"{kind} Nr={Nr} A={A} cap={cap:.4f}")
    plain = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k)
    far = plain.distances >= cap
    assert np.array_equal(nb.indices, np.where(far, -1, plain.indices))
    assert np.array_equal(nb.distances, np.where(far, np.inf, plain.distances))
    assert np.array_equal(nb.novel(cap), xr.novel(D, cap))
    if k == 1:
        novel = fc.pruner.novel_conformers(Q, R, atoms, cap)
        assert novel.dtype == np.bool_ and np.array_equal(novel, xr.novel(D, cap))
        # coverage: the roles swapped -- the restatement on the oracle's rows of the references against the queries
        Dsw = xr.distance_rows(xr.prepared(R, atoms), xr.prepared(Q, atoms))
        assert xr.knn_from_rows(Dsw, 1, cap).min_gap > GAP
        cov = fc.pruner.ensemble_coverage(Q, R, atoms, cap)
        covered, fraction, nearest, dist = xr.coverage(Dsw, cap)
        assert np.array_equal(cov.covered, covered) and cov.fraction == fraction
        assert cov.nearest.dtype == np.int32 and np.array_equal(cov.nearest, nearest)
        assert np.abs(cov.distances - dist).max() < TOL


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("Nq,Nr,A", CAP_SHAPES)
def test_knn_cross_tight_cap(fc, Nq, Nr, A, k):
    """a cap among the smallest pair distances: lists that the cap cuts short or empties, queries that are novel and
    queries that are not -- the filter starts every row at tau = max_rmsd and rules out most chunks at once.  (The
    continuous ensembles only: in the clustered ones every query has cluster mates among the references, closer than
    any such cap.)"""
    kind = "continuous"
    Q, R, atoms, D = _case(kind, Nq, Nr, A)
    cap = _tight_cap(D)
    ref = xr.knn_from_rows(D, k, cap)
    nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap)
    _check((nb.indices, nb.distances), ref, Nq, k, f"{kind} Nr={Nr} A={A} cap={cap:.4f}")
    assert (ref.indices[:, -1] < 0).any() and (ref.indices >= 0).any()  # the cap cuts lists short
    novel = xr.novel(D, cap)
    assert novel.any() and not novel.all()
    assert np.array_equal(nb.novel(cap), novel) and np.array_equal(fc.pruner.novel_conformers(Q, R, atoms, cap), novel)


def test_knn_cross_shares_the_arithmetic_of_the_self_form(fc):
    """an ensemble against a bitwise copy of itself: every row lists itself first, at ~1e-15, and then the neighbours of
    the self form with the same distance bits -- through two handles and through one"""
    N, A = 130, 20
    X, atoms = syn.continuous_ensemble(N, A, seed=150), np.array(["C"] * A)
    own = fc.pruner.knn_by_rmsd(X, atoms, 8)
    mask = np.ones(A, dtype=bool)
    with fc.DeviceEnsemble(X, atom_mask=mask, center=True) as q, fc.DeviceEnsemble(X.copy(), atom_mask=mask, center=True) as r:
        two = q.knn_against(r, 9)
        one = q.knn_against(q, 9)
    for idx, dist in (two, one):
        assert np.array_equal(idx[:, 0], np.arange(N)) and np.all(dist[:, 0] >= 0.0) and np.all(dist[:, 0] < TOL)
        assert np.array_equal(idx[:, 1:], own.indices)
        assert np.array_equal(dist[:, 1:], own.distances)  # the same bits
    assert own.distances.min() > 1e-3  # (the self form's lists hold no near-duplicate that could trade places with column 0)


def test_knn_cross_duplicates(fc, monkeypatch):
    """the references doubled bitwise, the queries their first half: a query's first two entries are its two copies at
    ~1e-15, every later pair of copies at bit-equal distances, the lower index first -- and kept at the cut"""
    M, A = 40, 20
    X0 = syn.continuous_ensemble(M, A, seed=60)
    R, atoms = np.concatenate([X0, X0]), np.array(["C"] * A)
    monkeypatch.setenv("FC_KNN_STRIPS", "2")  # the copies in different strips
    k = 7
    nb = fc.pruner.knn_by_rmsd_against(X0, R, atoms, k)
    idx, dist = nb.indices.astype(np.int64), nb.distances
    for i in range(M):
        assert idx[i, 0] == i and idx[i, 1] == i + M and dist[i, 0] == dist[i, 1] and 0.0 <= dist[i, 0] < TOL, (i, idx[i], dist[i])
        for p in range(2, k, 2):
            assert idx[i, p] < M, (i, idx[i])
            if p + 1 < k:
                assert idx[i, p + 1] == idx[i, p] + M and dist[i, p + 1] == dist[i, p], (i, idx[i], dist[i])
        assert len(set(idx[i].tolist())) == k  # (k = 7: the list ends inside the fourth pair, on its lower index)
    first = fc.pruner.knn_by_rmsd_against(X0, R, atoms, 1)
    assert np.array_equal(first.indices[:, 0], np.arange(M)) and np.array_equal(first.distances[:, 0], dist[:, 0])
    # against the restatement, pair by pair (its copies are equal only within rounding), the pairs ordered with a margin
    D = xr.distance_rows(X0, X0)
    ref = xr.knn_from_rows(D, 4)
    assert ref.min_gap > GAP
    assert np.array_equal(idx[:, 0::2], ref.indices) and np.abs(dist[:, 0::2] - ref.distances).max() < TOL


@pytest.mark.parametrize("capped", [False, True])
@pytest.mark.parametrize("Nq,Nr,A", [(16, 600, 80), (257, 65, 50)])
def test_knn_cross_independent_of_the_launch_shape(fc, monkeypatch, Nq, Nr, A, capped):
    """the same bits for every strip count and with the explicit pass for every pair"""
    Q, R, atoms, D = _case("continuous", Nq, Nr, A)
    k, cap = 8, (_middle_cap(D) if capped else None)
    runs = []
    for strips, flt in (("1", None), ("3", None), ("7", None), (None, None), (None, "0"), ("3", "0")):
        for name, value in (("FC_KNN_STRIPS", strips), ("FC_KNN_FILTER", flt)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)
        runs.append(fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap))
    for nb in runs[1:]:
        assert np.array_equal(nb.indices, runs[0].indices) and np.array_equal(nb.distances, runs[0].distances)
    _check((runs[0].indices, runs[0].distances), xr.knn_from_rows(D, k, cap), Nq, k, f"Nr={Nr} capped={capped}")


@pytest.mark.parametrize("heavy_atoms_only", [True, False])
def test_knn_cross_layers_agree(fc, heavy_atoms_only):
    """DeviceEnsemble.knn_against, pruner.knn_by_rmsd_against and Ensemble.nearest_in, with hydrogens present"""
    from firecode_amd.ensemble import Ensemble

    Nq, Nr, A, k = 33, 70, 30, 5
    X = syn.continuous_ensemble(Nq + Nr, A, seed=94)
    atoms = np.array(["C"] * A)
    atoms[2::3] = "H"
    Q, R = X[:Nq], X[Nq:]
    Qsel, Rsel = xr.prepared(Q, atoms, heavy_atoms_only), xr.prepared(R, atoms, heavy_atoms_only)
    assert Qsel.shape[1] == (20 if heavy_atoms_only else 30)
    D = xr.distance_rows(Qsel, Rsel)
    cap = _tight_cap(D)
    for max_rmsd in (None, cap):
        nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=max_rmsd, heavy_atoms_only=heavy_atoms_only)
        _check((nb.indices, nb.distances), xr.knn_from_rows(D, k, max_rmsd), Nq, k, f"heavy={heavy_atoms_only}")
        mask = atoms != "H" if heavy_atoms_only else np.ones(A, dtype=bool)
        with fc.DeviceEnsemble(Q, atom_mask=mask, center=True) as q, fc.DeviceEnsemble(R, atom_mask=mask, center=True) as r:
            idx, dist = q.knn_against(r, k, max_rmsd=max_rmsd)
            dev_ms, host_ms, strips = q.bench_knn_against(r, k, max_rmsd=max_rmsd, reps=2)
        assert np.array_equal(idx, nb.indices) and np.array_equal(dist, nb.distances)
        assert dev_ms > 0.0 and host_ms > 0.0 and strips >= 1
        a = Ensemble(atoms=atoms, coords=Q.copy(), logfunction=None)
        b = Ensemble(atoms=atoms, coords=R.copy(), logfunction=None)
        top = a.nearest_in(b, k=k, max_rmsd=max_rmsd, heavy_atoms_only=heavy_atoms_only)
        assert np.array_equal(top.indices, nb.indices) and np.array_equal(top.distances, nb.distances)
    novel = a.novel_against(b, cap, heavy_atoms_only=heavy_atoms_only)
    assert np.array_equal(novel, xr.novel(D, cap)) and novel.any() and not novel.all()


def test_knn_cross_refusals_leave_the_ensembles_usable(fc):
    L = fc._lib
    Q, R, atoms, D = _case("continuous", 5, 64, 20)
    out_i, out_d = np.zeros(5 * 64, dtype=np.int32), np.zeros(5 * 64)
    with fc.DeviceEnsemble(Q, atom_mask=atoms != "H", center=True) as q, \
            fc.DeviceEnsemble(R, atom_mask=atoms != "H", center=True) as r, \
            fc.DeviceEnsemble(R[:, :19], center=True) as other, fc.DeviceEnsemble(R[:0], center=True) as none:
        with pytest.raises(fc.FirecodeHipInputError):  # the Python layer: not the same atom selection
            q.knn_against(other, 2)
        with pytest.raises(fc.FirecodeHipInputError) as err:  # the library's own check of A
            L.call("fc_ensemble_knn_cross", q.handle, other.handle, 2, float("inf"), L.ptr(out_i, C.c_int32), L.pf(out_d))
        assert err.value.code == L.FC_E_INVALID
        with pytest.raises(fc.FirecodeHipError) as err:
            q.knn_against(r, 65)
        assert err.value.code == L.FC_E_LIMIT
        for bad in (dict(k=0), dict(k=2, max_rmsd=0.0), dict(k=2, max_rmsd=float("nan"))):
            with pytest.raises(fc.FirecodeHipInputError):
                q.knn_against(r, **bad)
        for bad_k, bad_cap in ((0, 1.0), (2, float("nan")), (2, -1.0)):
            with pytest.raises(fc.FirecodeHipInputError) as err:  # the library's own checks
                L.call("fc_ensemble_knn_cross", q.handle, r.handle, bad_k, bad_cap, L.ptr(out_i, C.c_int32), L.pf(out_d))
            assert err.value.code == L.FC_E_INVALID
        assert not out_i.any() and not out_d.any()  # a refusal writes nothing
        # an empty reference set: every slot empty; an empty query set: nothing
        idx, dist = q.knn_against(none, 3)
        assert idx.shape == (5, 3) and np.all(idx == -1) and np.all(np.isposinf(dist))
        assert none.knn_against(r, 3)[0].shape == (0, 3)
        # both ensembles still answer, in both directions
        _check(q.knn_against(r, 8), xr.knn_from_rows(D, 8), 5, 8)
        _check(r.knn_against(q, 1), xr.knn_from_rows(np.ascontiguousarray(D.T), 1), 64, 1)
        idx, dist = other.knn_against(other, 1)
        assert np.array_equal(idx[:, 0], np.arange(64)) and np.all(dist < TOL)
