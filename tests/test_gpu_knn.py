"""k nearest neighbours under the RMSD on the GPU (fc_ensemble_knn and the Python layers above it) against the NumPy
restatement of its contract (tests/knn_ref.py) on the oracle's Kabsch RMSD.

Bars: indices identical (-1 padding included), distances within 1e-10 (+inf where padded) -- on ensembles whose every
ordering decision (consecutive sorted distances of a row among positions 1 ... k + 1) the restatement recorded with a
gap above 1e-9, so that rounding cannot flip one.  No row is left out of any comparison."""

import ctypes as C

import numpy as np
import pytest

import dbscan_ref as dr
import knn_ref
from firecode_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9

_ROWS = {}  # the oracle's rows of an ensemble, computed once and shared by the cases that need them


def _ensemble(kind, N, A, seed):
    if kind == "clusters":
        X, atoms, _ = syn.synthetic_ensemble(N, A, seed=seed)
        return X, atoms
    return syn.continuous_ensemble(N, A, seed=seed), np.array(["C"] * A)


def _rows(key, Xsel):
    if key not in _ROWS:
        D = knn_ref.distance_rows(Xsel)
        D.setflags(write=False)
        _ROWS[key] = D
    return _ROWS[key]


def _check(got, ref, N, k):
    idx, dist = got
    assert ref.min_gap > GAP, f"the ensemble has a near-tie ({ref.min_gap:.3g}): choose another"
    assert idx.dtype == np.int32 and idx.shape == (N, k) and dist.dtype == np.float64 and dist.shape == (N, k)
    assert np.array_equal(idx, ref.indices)
    pad = ref.indices < 0
    assert np.all(np.isposinf(dist[pad])) and np.all(np.isfinite(dist[~pad]))
    print(f"N={N} k={k} gap={ref.min_gap:.3g} max|d - ref|={np.abs(dist[~pad] - ref.distances[~pad]).max(initial=0.0):.3g}")
    assert np.abs(dist[~pad] - ref.distances[~pad]).max(initial=0.0) < TOL


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("kind", ["clusters", "continuous"])
@pytest.mark.parametrize("N,A", [(1, 5), (2, 5), (3, 5), (64, 20), (65, 7), (257, 50), (600, 80), (300, 200)])
def test_knn_parity(fc, kind, N, A, k):
    """lists longer than the ensemble (N = 1, 2, 3; k = 64 at N = 64), N that is no multiple of the wavefront or the
    row tile (65, 257), 7 atoms, and 200 atoms (beyond the tiled regimes of the other RMSD kernels)"""
    X, atoms = _ensemble(kind, N, A, seed=N + A)
    ref = knn_ref.knn_from_rows(_rows((kind, N, A), knn_ref.prepared(X, atoms)), k)
    nb = fc.pruner.knn_by_rmsd(X, atoms, k)
    _check((nb.indices, nb.distances), ref, N, k)


def test_knn_ties_and_duplicates(fc, monkeypatch):
    """every conformer twice, bitwise: the twin first (the self-pair is left out by index, not by value; the explicit
    form, not the eigenvalue form, which gives ~1e-8 here), then the other conformers in twin pairs (m, m + 40) at
    bit-equal distances with the lower index first -- and the lower index kept where the list ends inside a pair"""
    X0 = syn.continuous_ensemble(40, 20, seed=60)
    X = np.concatenate([X0, X0])
    atoms = np.array(["C"] * 20)
    k = 8
    monkeypatch.setenv("FC_KNN_STRIPS", "3")  # twins in different strips
    nb = fc.pruner.knn_by_rmsd(X, atoms, k)
    ref = knn_ref.knn_from_rows(_rows("twins", X), k)
    idx, dist = nb.indices.astype(np.int64), nb.distances
    assert idx.shape == (80, k)
    for i in range(80):
        assert idx[i, 0] == (i + 40) % 80 and 0.0 <= dist[i, 0] < TOL, (i, idx[i], dist[i])
        rest_j, rest_d = idx[i, 1:], dist[i, 1:]
        assert rest_d.min() > 0.2  # (the nearest conformer that is not the twin: >= 0.21 A)
        for p in range(0, k - 1, 2):
            m = rest_j[p]
            assert m < 40, (i, idx[i])                      # the lower index of a pair first
            if p + 1 < k - 1:
                assert rest_j[p + 1] == m + 40 and rest_d[p + 1] == rest_d[p], (i, idx[i], dist[i])
            # (k - 1 = 7 entries: the list ends inside the fourth pair, and the entry kept is m)
        assert len(set(idx[i].tolist())) == k and i not in idx[i]
        # the restatement's order of the pairs (its twins are equal only within rounding: compare by pair)
        assert np.array_equal(rest_j % 40, ref.indices[i, 1:] % 40), (i, idx[i], ref.indices[i])
        assert np.abs(rest_d - ref.distances[i, 1:]).max() < TOL
    # the pairs of the restatement are ordered with a margin of their own
    pair_d = np.sort(np.where(np.eye(40, dtype=bool), np.inf, _rows("twins", X)[:40, :40]), axis=1)[:, :5]
    assert np.diff(pair_d, axis=1).min() > GAP


def test_knn_independent_of_the_launch_shape(fc, monkeypatch):
    X, atoms = _ensemble("continuous", 600, 80, seed=680)
    runs = []
    for strips in ("1", "3", "7", None):
        if strips is None:
            monkeypatch.delenv("FC_KNN_STRIPS", raising=False)
        else:
            monkeypatch.setenv("FC_KNN_STRIPS", strips)
        runs.append(fc.pruner.knn_by_rmsd(X, atoms, 8))
    for nb in runs[1:]:
        assert np.array_equal(nb.indices, runs[0].indices) and np.array_equal(nb.distances, runs[0].distances)
    _check((runs[0].indices, runs[0].distances), knn_ref.knn_from_rows(_rows(("continuous", 600, 80), X), 8), 600, 8)


def test_knn_independent_of_the_filter(fc, monkeypatch):
    """FC_KNN_FILTER=0 (the explicit pass for every pair) against the default (skipped where the eigenvalue rules a
    whole chunk of columns out of a row's list): the same bits, on the ensemble with the smallest gaps and on twins"""
    X0 = syn.continuous_ensemble(40, 20, seed=60)
    cases = [(_ensemble("continuous", 600, 80, seed=680), 64), ((np.concatenate([X0, X0]), np.array(["C"] * 20)), 8)]
    for (X, atoms), k in cases:
        monkeypatch.setenv("FC_KNN_FILTER", "0")
        plain = fc.pruner.knn_by_rmsd(X, atoms, k)
        monkeypatch.delenv("FC_KNN_FILTER")
        nb = fc.pruner.knn_by_rmsd(X, atoms, k)
        assert np.array_equal(nb.indices, plain.indices) and np.array_equal(nb.distances, plain.distances)


@pytest.mark.parametrize("heavy_atoms_only", [True, False])
def test_knn_atom_selection(fc, heavy_atoms_only):
    X = syn.continuous_ensemble(64, 30, seed=94)
    atoms = np.array(["C"] * 30)
    atoms[2::3] = "H"
    Xsel = knn_ref.prepared(X, atoms, heavy_atoms_only)
    assert Xsel.shape[1] == (20 if heavy_atoms_only else 30)
    nb = fc.pruner.knn_by_rmsd(X, atoms, 8, heavy_atoms_only=heavy_atoms_only)
    _check((nb.indices, nb.distances), knn_ref.knn(Xsel, 8), 64, 8)


def test_knn_beyond_the_lds_stage(fc):
    """2 100 selected atoms: the row conformers no longer fit the kernel's LDS stage and are read from HBM"""
    rng = np.random.default_rng(7)
    X = rng.normal(scale=4.0, size=(1, 2100, 3)) + rng.normal(scale=0.3, size=(40, 2100, 3))
    nb = fc.pruner.knn_by_rmsd(X, np.array(["C"] * 2100), 3)
    _check((nb.indices, nb.distances), knn_ref.knn(X, 3), 40, 3)


def test_knn_layers_agree(fc):
    from firecode_amd.ensemble import Ensemble

    N, A, k = 257, 50, 8
    X, atoms = _ensemble("continuous", N, A, seed=N + A)
    nb = fc.pruner.knn_by_rmsd(X, atoms, k)
    with fc.DeviceEnsemble(X, atom_mask=atoms != "H", center=True) as ens:
        idx, dist = ens.knn(k)
        R, _ = ens.rmsd_matrix()
    assert np.array_equal(idx, nb.indices) and np.array_equal(dist, nb.distances)
    top = Ensemble(atoms=atoms, coords=X.copy(), logfunction=None).nearest_neighbours(k)
    assert np.array_equal(top.indices, nb.indices) and np.array_equal(top.distances, nb.distances)
    # k_distances(4): the distance to the fourth neighbour -- the fifth-smallest entry of the matrix's row, whose
    # smallest is the diagonal's 0 -- sorted in descending order
    np.fill_diagonal(R, -1.0)
    fourth = np.sort(R, axis=1)[:, 4]
    assert np.all(fourth > 0.0)
    curve = nb.k_distances(4)
    assert np.all(np.diff(curve) <= 0.0) and np.abs(curve - np.sort(fourth)[::-1]).max() < TOL
    assert np.array_equal(nb.k_distances(), np.sort(nb.distances[:, -1])[::-1])
    # the k-NN graph through the density-based clusters
    for mutual, min_samples in ((False, k + 1), (True, 4)):
        e = nb.pairs(mutual=mutual)
        assert np.array_equal(e, knn_ref.pairs(nb.indices, mutual))
        got = fc.pruner.dbscan_from_pairs(e, N, min_samples)
        ref = dr.dbscan(N, e[:, 0], e[:, 1], min_samples)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)


def test_knn_refusals_leave_the_ensemble_usable(fc):
    L = fc._lib
    X, atoms = _ensemble("continuous", 64, 20, seed=84)
    with fc.DeviceEnsemble(X, atom_mask=atoms != "H", center=True) as ens:
        with pytest.raises(fc.FirecodeHipError) as err:
            ens.knn(65)
        assert err.value.code == L.FC_E_LIMIT
        with pytest.raises(fc.FirecodeHipInputError):
            ens.knn(0)
        with pytest.raises(fc.FirecodeHipInputError) as err:  # the library's own check of k < 1
            L.call("fc_ensemble_knn", ens.handle, 0, L.ptr(np.zeros(64, dtype=np.int32), C.c_int32),
                   L.pf(np.zeros(64)))
        assert err.value.code == L.FC_E_INVALID
        idx, dist = ens.knn(1)
        ref = knn_ref.knn_from_rows(_rows(("continuous", 64, 20), X), 1)
        _check((idx, dist), ref, 64, 1)
        dev_ms, host_ms, strips = ens.bench_knn(1, reps=2)
        assert dev_ms > 0.0 and host_ms > 0.0 and strips >= 1
