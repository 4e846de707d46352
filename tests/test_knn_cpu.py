"""Nearest neighbours under the RMSD without a device: the NumPy restatement of the contract (tests/knn_ref.py)
against a brute-force argsort and its padding rules, the host-side methods of ``RmsdNeighbours`` on hand-made arrays,
argument refusals before any device use, and the new C symbols."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import cluster_ref as cr
import dbscan_ref as dr
import firecode_amd as fc
import knn_ref
from firecode_amd import _lib as L
from firecode_amd import synthetic as syn
from firecode_amd.pruner import RmsdNeighbours, knn_by_rmsd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _symmetric_rows(n, seed):
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.1, 3.0, size=(n, n))
    D = 0.5 * (D + D.T)
    np.fill_diagonal(D, 0.0)
    return D


@pytest.mark.parametrize("n,k", [(9, 1), (9, 4), (9, 8), (30, 7)])
def test_restatement_against_brute_force(n, k):
    D = _symmetric_rows(n, seed=n + k)
    ref = knn_ref.knn_from_rows(D, k)
    M = D.copy()
    np.fill_diagonal(M, np.inf)
    order = np.argsort(M, axis=1, kind="stable")[:, :k]
    assert ref.indices.dtype == np.int32 and np.array_equal(ref.indices, order)
    assert np.array_equal(ref.distances, np.take_along_axis(D, order, axis=1))
    assert np.all(np.diff(ref.distances, axis=1) >= 0.0)
    assert not (ref.indices == np.arange(n)[:, None]).any()
    # the recorded gap: consecutive sorted off-diagonal distances among positions 1 ... k + 1
    head = np.sort(M, axis=1)[:, :k + 1]
    head = head[:, np.isfinite(head).all(axis=0)]
    assert ref.min_gap == np.diff(head, axis=1).min()


def test_restatement_on_the_oracle():
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=3)
    Xsel = knn_ref.prepared(X, atoms)
    ref = knn_ref.knn(Xsel, 3)
    D = knn_ref.distance_rows(Xsel)
    for i in range(12):
        assert np.array_equal(D[i], knn_ref.rmsd_row(Xsel, i))
        assert set(ref.indices[i].tolist()) == set(np.argsort(np.where(np.arange(12) == i, np.inf, D[i]))[:3].tolist())
    assert ref.min_gap > 0.0


def test_restatement_ties_and_self_by_index():
    """equal distances: the lower index first, inside the list and at its cut; a zero distance to ANOTHER conformer stays"""
    D = np.array([[0.0, 1.0, 1.0, 0.0, 1.0],
                  [1.0, 0.0, 2.0, 2.0, 2.0],
                  [1.0, 2.0, 0.0, 0.5, 0.5],
                  [0.0, 2.0, 0.5, 0.0, 3.0],
                  [1.0, 2.0, 0.5, 3.0, 0.0]])
    ref = knn_ref.knn_from_rows(D, 2)
    assert ref.indices.tolist() == [[3, 1], [0, 2], [3, 4], [0, 2], [2, 0]]
    assert ref.distances.tolist() == [[0.0, 1.0], [1.0, 2.0], [0.5, 0.5], [0.0, 0.5], [0.5, 1.0]]
    assert ref.min_gap == 0.0


def test_restatement_padding():
    D = _symmetric_rows(3, seed=1)
    ref = knn_ref.knn_from_rows(D, 5)
    assert ref.indices.shape == (3, 5) and np.all(ref.indices[:, 2:] == -1) and np.all(np.isposinf(ref.distances[:, 2:]))
    assert np.all(ref.indices[:, :2] >= 0) and np.all(np.isfinite(ref.distances[:, :2]))
    one = knn_ref.knn_from_rows(np.zeros((1, 1)), 4)
    assert one.indices.tolist() == [[-1] * 4] and np.all(np.isposinf(one.distances)) and one.min_gap == np.inf
    none = knn_ref.knn_from_rows(np.zeros((0, 0)), 4)
    assert none.indices.shape == (0, 4) and none.distances.shape == (0, 4)


# ---- RmsdNeighbours: host-side NumPy on the outputs
IDX = np.array([[1, 2], [0, 3], [3, 1], [2, -1], [-1, -1]], dtype=np.int32)
DST = np.array([[0.1, 0.4], [0.1, 0.7], [0.2, 0.9], [0.2, np.inf], [np.inf, np.inf]])


def test_k_distances():
    nb = RmsdNeighbours(IDX, DST)
    assert np.array_equal(nb.k_distances(), np.array([np.inf, np.inf, 0.9, 0.7, 0.4]))
    assert np.array_equal(nb.k_distances(2), nb.k_distances())
    assert np.array_equal(nb.k_distances(1), np.array([np.inf, 0.2, 0.2, 0.1, 0.1]))
    for bad in (0, 3, 1.5, True):
        with pytest.raises(fc.FirecodeHipInputError):
            nb.k_distances(bad)


def test_pairs_plain_mutual_and_padding():
    nb = RmsdNeighbours(IDX, DST)
    plain = nb.pairs()
    assert plain.dtype == np.int64 and plain.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    assert nb.pairs(mutual=True).tolist() == [[0, 1], [2, 3]]
    assert np.array_equal(plain, knn_ref.pairs(IDX)) and np.array_equal(nb.pairs(mutual=True), knn_ref.pairs(IDX, True))
    with pytest.raises(fc.FirecodeHipInputError):
        nb.pairs(mutual=1)
    empty = RmsdNeighbours(np.full((2, 3), -1, dtype=np.int32), np.full((2, 3), np.inf))
    assert empty.pairs().shape == (0, 2) and empty.pairs().dtype == np.int64
    assert RmsdNeighbours(np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3))).pairs().shape == (0, 2)


@pytest.mark.parametrize("seed", range(3))
def test_pairs_of_random_lists_feed_the_graph_references(seed):
    n, k = 40, 3
    ref = knn_ref.knn_from_rows(_symmetric_rows(n, seed), k)
    nb = RmsdNeighbours(ref.indices, ref.distances)
    for mutual in (False, True):
        e = nb.pairs(mutual=mutual)
        assert np.array_equal(e, knn_ref.pairs(ref.indices, mutual))
        assert np.all(e[:, 0] < e[:, 1]) and len(np.unique(e, axis=0)) == len(e)
        comp = cr.components(n, e[:, 0], e[:, 1])
        assert comp.sizes.sum() == n
        db = dr.dbscan(n, e[:, 0], e[:, 1], k + 1)
        assert np.array_equal(db.degrees, np.bincount(e.reshape(-1), minlength=n))
        if not mutual:  # every vertex names k neighbours: degree >= k, all core, the clusters are the components
            assert db.core.all() and cr.same_partition(db.labels, comp.labels)


# ---- refusals before any device use
@pytest.mark.parametrize("kwargs", [
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=0),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=-2),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=65),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=2.0),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=2.5),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=True),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, k=None),
    dict(structures=np.zeros((4, 5, 2)), atoms=["C"] * 5, k=2),      # not (N, A, 3)
    dict(structures=np.zeros((4, 5)), atoms=["C"] * 5, k=2),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 4, k=2),      # len(atoms)
    dict(structures=np.zeros((4, 5, 3)), atoms=["H"] * 5, k=2),      # no heavy atom to align
])
def test_bad_arguments_raise_before_device_use(kwargs):
    with pytest.raises(fc.FirecodeHipInputError):
        knn_by_rmsd(**kwargs)


def test_limit_code_and_empty_ensemble():
    with pytest.raises(fc.FirecodeHipError) as err:
        knn_by_rmsd(np.zeros((4, 5, 3)), ["C"] * 5, 65)
    assert err.value.code == L.FC_E_LIMIT
    nb = knn_by_rmsd(np.zeros((0, 5, 3)), ["C"] * 5, 3)  # no device needed
    assert nb.indices.shape == (0, 3) and nb.indices.dtype == np.int32 and nb.distances.shape == (0, 3)
    assert nb.pairs().shape == (0, 2) and nb.k_distances().shape == (0,)


def test_c_entry_points_refuse_before_device_use():
    idx, dist = np.zeros(8, dtype=np.int32), np.zeros(8)
    pi32, ms = idx.ctypes.data_as(C.POINTER(C.c_int32)), C.c_double(0)
    lib = L.load()
    assert lib.fc_ensemble_knn(None, 2, pi32, L.pf(dist)) == L.FC_E_INVALID
    assert lib.fc_bench_knn(None, 2, 1, C.byref(ms), C.byref(ms), None) == L.FC_E_INVALID
    assert lib.fc_bench_knn(None, 2, 0, C.byref(ms), C.byref(ms), None) == L.FC_E_INVALID


def test_no_cpu_fallback():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=1)
    with pytest.raises(fc.FirecodeHipDeviceError):
        knn_by_rmsd(X, atoms, 3)


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "fc_hip.h")).read()
    assert re.search(r"#define\s+FC_KNN_MAX\s+64\b", text) and L.KNN_MAX == 64
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    for name in ("fc_ensemble_knn", "fc_bench_knn"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/fc_hip.h"
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert lib.fc_abi_version() == 1
    for layer, name in ((fc.DeviceEnsemble, "knn"), (fc.DeviceEnsemble, "bench_knn"), (fc.pruner, "knn_by_rmsd"),
                        (fc.ensemble.Ensemble, "nearest_neighbours")):
        assert callable(getattr(layer, name))
