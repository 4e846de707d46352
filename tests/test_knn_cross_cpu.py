"""Nearest neighbours across two ensembles without a device: the NumPy restatement of the contract
(tests/knn_cross_ref.py) against a brute-force argsort on hand-made rows (ties, the cap, padding, empty sets), the
host-side methods of ``RmsdCrossNeighbours`` and ``EnsembleCoverage`` on hand-made arrays, every refusal before any
device use through ctypes and through the Python layers, and the new C symbols."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import firecode_amd as fc
import knn_cross_ref as xr
from firecode_amd import _lib as L
from firecode_amd import synthetic as syn
from firecode_amd.ensemble import Ensemble
from firecode_amd.pruner import (EnsembleCoverage, RmsdCrossNeighbours, ensemble_coverage, knn_by_rmsd_against,
                                 novel_conformers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(nq, nr, seed):
    return np.random.default_rng(seed).uniform(0.1, 3.0, size=(nq, nr))


# ---- the restatement
@pytest.mark.parametrize("nq,nr,k", [(5, 9, 1), (5, 9, 4), (9, 5, 5), (7, 30, 8)])
def test_restatement_against_brute_force(nq, nr, k):
    D = _rows(nq, nr, seed=nq + nr + k)
    ref = xr.knn_from_rows(D, k)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    assert ref.indices.dtype == np.int32 and np.array_equal(ref.indices, order)
    assert np.array_equal(ref.distances, np.take_along_axis(D, order, axis=1))
    assert np.all(np.diff(ref.distances, axis=1) >= 0.0)
    assert ref.min_gap == np.diff(np.sort(D, axis=1)[:, :k + 1], axis=1).min()


def test_restatement_nothing_left_out_and_ties():
    """no pair is left out by index (a zero on the "diagonal" is listed); equal distances: the lower index first, inside
    the list and at its cut"""
    D = np.array([[0.0, 1.0, 1.0, 0.5],
                  [2.0, 0.0, 2.0, 2.0],
                  [1.0, 1.0, 1.0, 1.0]])
    ref = xr.knn_from_rows(D, 2)
    assert ref.indices.tolist() == [[0, 3], [1, 0], [0, 1]]
    assert ref.distances.tolist() == [[0.0, 0.5], [0.0, 2.0], [1.0, 1.0]]
    assert ref.min_gap == 0.0


def test_restatement_cap_is_strict_and_pads():
    D = np.array([[0.2, 0.5, 0.9, 0.1],
                  [0.5, 0.6, 0.7, 0.8],
                  [0.49, 0.3, 0.5, 0.4]])
    ref = xr.knn_from_rows(D, 3, max_rmsd=0.5)
    assert ref.indices.tolist() == [[3, 0, -1], [-1, -1, -1], [1, 3, 0]]
    assert ref.distances.tolist() == [[0.1, 0.2, np.inf], [np.inf] * 3, [0.3, 0.4, 0.49]]
    assert ref.min_gap == 0.0  # (d == max_rmsd occurs: the strict comparison leaves it out)
    # the capped lists are the uncapped ones with the entries d >= max_rmsd replaced
    plain = xr.knn_from_rows(D, 3)
    far = plain.distances >= 0.5
    assert np.array_equal(np.where(far, -1, plain.indices), ref.indices)
    assert np.array_equal(np.where(far, np.inf, plain.distances), ref.distances)
    # the recorded gap with a cap: the smaller of the ordering gap and the distance of any pair to the cap
    loose = xr.knn_from_rows(D, 1, max_rmsd=0.55)
    assert loose.min_gap == pytest.approx(0.05) and xr.knn_from_rows(D, 1).min_gap == pytest.approx(0.1)
    assert xr.knn_from_rows(D, 1, max_rmsd=0.605).min_gap == pytest.approx(0.005)
    assert np.array_equal(xr.novel(D, 0.5), [False, True, False])


def test_restatement_padding_and_empty_sets():
    D = _rows(3, 2, seed=1)
    ref = xr.knn_from_rows(D, 5)  # k > Nr
    assert ref.indices.shape == (3, 5) and np.all(ref.indices[:, 2:] == -1) and np.all(np.isposinf(ref.distances[:, 2:]))
    assert np.all(ref.indices[:, :2] >= 0) and np.all(np.isfinite(ref.distances[:, :2]))
    none = xr.knn_from_rows(np.zeros((4, 0)), 3, max_rmsd=0.5)  # Nr = 0
    assert none.indices.tolist() == [[-1] * 3] * 4 and np.all(np.isposinf(none.distances)) and none.min_gap == np.inf
    empty = xr.knn_from_rows(np.zeros((0, 6)), 3)  # Nq = 0
    assert empty.indices.shape == (0, 3) and empty.indices.dtype == np.int32 and empty.distances.shape == (0, 3)
    one = xr.knn_from_rows(np.array([[0.25]]), 1)
    assert one.indices.tolist() == [[0]] and one.distances.tolist() == [[0.25]] and one.min_gap == np.inf


def test_restatement_on_the_oracle():
    X, atoms, _ = syn.synthetic_ensemble(14, 6, seed=3)
    Xsel = xr.prepared(X, atoms)
    Q, R = Xsel[:5], Xsel[5:]
    D = xr.distance_rows(Q, R)
    assert D.shape == (5, 9)
    from oracle import cpu_ref as o
    for i in range(5):
        for j in range(9):
            assert D[i, j] == pytest.approx(o.rmsd_and_max(Q[i], R[j], center=True)[0], abs=1e-12)
    ref = xr.knn(Q, R, 3)
    assert np.array_equal(ref.indices, np.argsort(D, axis=1, kind="stable")[:, :3]) and ref.min_gap > 0.0
    # a query that is a copy of a reference lists it first, at ~0
    same = xr.knn(R[2:4], R, 1)
    assert same.indices[:, 0].tolist() == [2, 3] and np.all(same.distances[:, 0] < 1e-7)
    assert xr.distance_rows(Q, R[:0]).shape == (5, 0)


# ---- RmsdCrossNeighbours, EnsembleCoverage: host-side NumPy on the outputs
IDX = np.array([[4, 2], [0, -1], [-1, -1], [3, 1]], dtype=np.int32)
DST = np.array([[0.1, 0.4], [0.3, np.inf], [np.inf, np.inf], [0.5, 0.9]])


def test_nearest_and_novel():
    nb = RmsdCrossNeighbours(IDX, DST)
    near_j, near_d = nb.nearest()
    assert near_j.tolist() == [4, 0, -1, 3] and np.array_equal(near_d, [0.1, 0.3, np.inf, 0.5])
    assert nb.novel(0.3).tolist() == [False, True, True, True]      # strict: d = 0.3 is not within 0.3
    assert nb.novel(0.31).tolist() == [False, False, True, True]
    assert nb.novel(0.5).tolist() == [False, False, True, True]
    assert nb.novel(5.0).tolist() == [False, False, True, False]
    for bad in (0.0, -1.0, float("nan"), "0.5", True):
        with pytest.raises(fc.FirecodeHipInputError):
            nb.novel(bad)
    empty = RmsdCrossNeighbours(np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2)))
    assert empty.novel(0.5).shape == (0,) and empty.nearest()[0].shape == (0,)
    assert not hasattr(nb, "pairs") and not hasattr(nb, "k_distances")  # not an RmsdNeighbours: two different sets


def test_coverage_bookkeeping():
    cov = EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(IDX, DST), 0.5)
    assert cov.covered.tolist() == [True, True, False, False] and cov.fraction == 0.5
    assert cov.nearest.tolist() == [4, 0, -1, 3] and np.array_equal(cov.distances, [0.1, 0.3, np.inf, 0.5])
    assert EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(IDX, DST), 0.51).fraction == 0.75
    none = EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(np.zeros((0, 1), dtype=np.int32), np.zeros((0, 1))), 0.5)
    assert none.covered.shape == (0,) and np.isnan(none.fraction)
    # against the restatement on hand-made rows (references x structures)
    D = np.array([[0.7, 0.2, 0.2], [0.6, 0.9, 0.8], [0.1, 0.3, 0.05]])
    ref = xr.knn_from_rows(D, 1)
    got = EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(ref.indices, ref.distances), 0.5)
    want = xr.coverage(D, 0.5)
    assert want[0].tolist() == [True, False, True] and want[2].tolist() == [1, 0, 2]
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert got.fraction == pytest.approx(2 / 3)
    with pytest.raises(fc.FirecodeHipInputError):
        EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(IDX, DST), -0.5)


# ---- empty sets: correctly shaped results without a device
def test_empty_sets_need_no_device():
    atoms = ["C"] * 5
    nb = knn_by_rmsd_against(np.zeros((0, 5, 3)), np.zeros((4, 5, 3)), atoms, 3)
    assert isinstance(nb, RmsdCrossNeighbours)
    assert nb.indices.shape == (0, 3) and nb.indices.dtype == np.int32 and nb.distances.shape == (0, 3)
    nb = knn_by_rmsd_against(np.zeros((4, 5, 3)), np.zeros((0, 5, 3)), atoms, 3, max_rmsd=0.5)
    assert nb.indices.shape == (4, 3) and nb.indices.dtype == np.int32 and np.all(nb.indices == -1)
    assert nb.distances.dtype == np.float64 and np.all(np.isposinf(nb.distances)) and nb.novel(0.5).all()
    assert novel_conformers(np.zeros((4, 5, 3)), np.zeros((0, 5, 3)), atoms, 0.5).tolist() == [True] * 4
    assert novel_conformers(np.zeros((0, 5, 3)), np.zeros((4, 5, 3)), atoms, 0.5).shape == (0,)
    cov = ensemble_coverage(np.zeros((0, 5, 3)), np.zeros((4, 5, 3)), atoms, 0.5)  # nothing generated: nothing covered
    assert cov.covered.tolist() == [False] * 4 and cov.fraction == 0.0 and cov.nearest.tolist() == [-1] * 4
    assert np.all(np.isposinf(cov.distances))
    cov = ensemble_coverage(np.zeros((4, 5, 3)), np.zeros((0, 5, 3)), atoms, 0.5)  # no reference
    assert cov.covered.shape == (0,) and np.isnan(cov.fraction) and cov.nearest.dtype == np.int32
    a = Ensemble(atoms=np.array(atoms), coords=np.zeros((4, 5, 3)), logfunction=None)
    b = Ensemble(atoms=np.array(atoms), coords=np.zeros((0, 5, 3)), logfunction=None)
    assert a.nearest_in(b, k=2).indices.tolist() == [[-1, -1]] * 4 and a.novel_against(b, 0.5).all()
    assert b.nearest_in(a).indices.shape == (0, 1)


# ---- refusals before any device use
Q, R, AT = np.zeros((4, 5, 3)), np.zeros((6, 5, 3)), ["C"] * 5


@pytest.mark.parametrize("kwargs", [
    dict(structures=Q, references=R, atoms=AT, k=0),
    dict(structures=Q, references=R, atoms=AT, k=-2),
    dict(structures=Q, references=R, atoms=AT, k=65),
    dict(structures=Q, references=R, atoms=AT, k=2.0),
    dict(structures=Q, references=R, atoms=AT, k=True),
    dict(structures=Q, references=R, atoms=AT, k=None),
    dict(structures=Q, references=R, atoms=AT, k=2, max_rmsd=0.0),
    dict(structures=Q, references=R, atoms=AT, k=2, max_rmsd=-0.5),
    dict(structures=Q, references=R, atoms=AT, k=2, max_rmsd=float("nan")),
    dict(structures=Q, references=R, atoms=AT, k=2, max_rmsd="0.5"),
    dict(structures=Q, references=R, atoms=AT, k=2, max_rmsd=True),
    dict(structures=np.zeros((4, 5, 2)), references=R, atoms=AT, k=2),       # not (N, A, 3)
    dict(structures=np.zeros((4, 5)), references=R, atoms=AT, k=2),
    dict(structures=Q, references=np.zeros((6, 4, 3)), atoms=AT, k=2),       # another atom count
    dict(structures=Q, references=np.zeros((6, 5, 2)), atoms=AT, k=2),
    dict(structures=Q, references=np.zeros((6, 5)), atoms=AT, k=2),
    dict(structures=Q, references=R, atoms=["C"] * 4, k=2),                  # len(atoms)
    dict(structures=Q, references=R, atoms=["H"] * 5, k=2),                  # no heavy atom to align
    dict(structures=np.zeros((0, 5, 3)), references=R, atoms=AT, k=0),       # an empty set excuses nothing
    dict(structures=Q, references=np.zeros((0, 5, 3)), atoms=AT, k=2, max_rmsd=-1.0),
])
def test_bad_arguments_raise_before_device_use(kwargs):
    with pytest.raises(fc.FirecodeHipInputError):
        knn_by_rmsd_against(**kwargs)


@pytest.mark.parametrize("max_rmsd", [None, 0.0, -0.25, float("nan"), "0.5"])
def test_novelty_and_coverage_need_a_positive_radius(max_rmsd):
    with pytest.raises(fc.FirecodeHipInputError):
        novel_conformers(Q, R, AT, max_rmsd)
    with pytest.raises(fc.FirecodeHipInputError):
        ensemble_coverage(Q, R, AT, max_rmsd)
    with pytest.raises(fc.FirecodeHipInputError):
        novel_conformers(Q, np.zeros((6, 4, 3)), AT, 0.5)
    with pytest.raises(fc.FirecodeHipInputError):
        ensemble_coverage(Q, np.zeros((6, 4, 3)), AT, 0.5)


def test_limit_code():
    with pytest.raises(fc.FirecodeHipError) as err:
        knn_by_rmsd_against(Q, R, AT, 65)
    assert err.value.code == L.FC_E_LIMIT
    with pytest.raises(fc.FirecodeHipError) as err:
        knn_by_rmsd_against(Q, R, AT, 0)
    assert err.value.code == L.FC_E_INVALID


def test_ensemble_layer_refuses_other_atoms():
    a = Ensemble(atoms=np.array(["C"] * 5), coords=np.zeros((4, 5, 3)), logfunction=None)
    for other_atoms, n in ((["C", "C", "C", "C", "N"], 5), (["C"] * 4, 4)):
        b = Ensemble(atoms=np.array(other_atoms), coords=np.zeros((3, n, 3)), logfunction=None)
        with pytest.raises(fc.FirecodeHipInputError):
            a.nearest_in(b)
        with pytest.raises(fc.FirecodeHipInputError):
            a.novel_against(b, 0.5)
    with pytest.raises(fc.FirecodeHipInputError):
        a.nearest_in(np.zeros((3, 5, 3)))
    same = Ensemble(atoms=np.array(["C"] * 5), coords=np.zeros((3, 5, 3)), logfunction=None)
    for bad in (dict(k=0), dict(k=65), dict(max_rmsd=0.0), dict(max_rmsd=float("nan"))):
        with pytest.raises(fc.FirecodeHipInputError):
            a.nearest_in(same, **bad)
    with pytest.raises(fc.FirecodeHipInputError):
        a.novel_against(same, -1.0)


def test_c_entry_points_refuse_before_device_use():
    idx, dist = np.zeros(8, dtype=np.int32), np.zeros(8)
    pi32, ms = idx.ctypes.data_as(C.POINTER(C.c_int32)), C.c_double(0)
    inf = float("inf")
    lib = L.load()
    # NULL handles and outputs
    assert lib.fc_ensemble_knn_cross(None, None, 2, inf, pi32, L.pf(dist)) == L.FC_E_INVALID
    assert lib.fc_ensemble_knn_cross(None, None, 2, 0.5, None, None) == L.FC_E_INVALID
    # k and max_rmsd are judged first: the codes do not depend on the handles
    assert lib.fc_ensemble_knn_cross(None, None, 0, inf, pi32, L.pf(dist)) == L.FC_E_INVALID
    assert lib.fc_ensemble_knn_cross(None, None, -3, inf, pi32, L.pf(dist)) == L.FC_E_INVALID
    assert lib.fc_ensemble_knn_cross(None, None, 65, inf, pi32, L.pf(dist)) == L.FC_E_LIMIT
    assert lib.fc_ensemble_knn_cross(None, None, 64, inf, pi32, L.pf(dist)) == L.FC_E_INVALID  # (the NULL handles)
    for bad in (float("nan"), 0.0, -0.5, -inf):
        assert lib.fc_ensemble_knn_cross(None, None, 2, bad, pi32, L.pf(dist)) == L.FC_E_INVALID
        assert b"max_rmsd" in lib.fc_last_error()
    assert lib.fc_bench_knn_cross(None, None, 2, inf, 1, C.byref(ms), C.byref(ms), None) == L.FC_E_INVALID
    assert lib.fc_bench_knn_cross(None, None, 2, inf, 0, C.byref(ms), C.byref(ms), None) == L.FC_E_INVALID
    assert lib.fc_bench_knn_cross(None, None, 65, inf, 1, C.byref(ms), C.byref(ms), None) == L.FC_E_LIMIT
    assert lib.fc_bench_knn_cross(None, None, 0, inf, 1, C.byref(ms), C.byref(ms), None) == L.FC_E_INVALID
    assert not idx.any() and not dist.any()  # nothing was written


def test_no_cpu_fallback():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=1)
    with pytest.raises(fc.FirecodeHipDeviceError):
        knn_by_rmsd_against(X[:4], X[4:], atoms, 3)
    with pytest.raises(fc.FirecodeHipDeviceError):
        novel_conformers(X[:4], X[4:], atoms, 0.5)


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "fc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    for name in ("fc_ensemble_knn_cross", "fc_bench_knn_cross"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/fc_hip.h"
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert lib.fc_abi_version() == 1
    for layer, name in ((fc.DeviceEnsemble, "knn_against"), (fc.DeviceEnsemble, "bench_knn_against"),
                        (fc.pruner, "knn_by_rmsd_against"), (fc.pruner, "novel_conformers"),
                        (fc.pruner, "ensemble_coverage"), (Ensemble, "nearest_in"), (Ensemble, "novel_against")):
        assert callable(getattr(layer, name))
    # the self form's header block no longer lists the cross form as missing
    block = text[text.index("k nearest neighbours of every conformer"):text.index("#define FC_KNN_MAX")]
    assert "fc_ensemble_knn_cross" in block
