"""Symmetry- and mirror-aware nearest neighbours under the RMSD without a device: the restatement of d_sym across two
ensembles (tests/knn_sym_ref.py) and every refusal the contract lists (include/fc_hip.h, fc_ensemble_knn_perm and
fc_ensemble_knn_cross_perm), each raised before any device use -- through the Python layers and on the C entry points
themselves with NULL handles."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import diverse_sym_ref as ds
import enant_ref as er
import knn_cross_ref as xr
import knn_sym_ref as ks
import symm_ref as sr
from firecode_amd import _lib
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,A", [("path", 9), ("blocks", 13), ("swaps64", 14)])
@pytest.mark.parametrize("mirror", [False, True])
def test_d_sym_is_symmetric_and_below_d(kind, A, mirror):
    """tables closed under inverse: d_sym(i, j) = d_sym(j, i), also across two sets; the identity is in the table:
    d_sym <= d"""
    X, _, table, _ = ds.ensemble("clusters", 24, A, kind, mirror)
    M = ks.self_rows(X, table, mirror)
    assert np.abs(M - M.T).max() < 1e-12
    assert np.abs(M - ds.matrix(X, table, mirror)).max() < 1e-12  # (the rows of the diverse selection's restatement)
    Q, R = X[:7], X[7:]
    D, Dt = ks.distance_rows(Q, R, table, mirror), ks.distance_rows(R, Q, table, mirror)
    assert D.shape == (7, 17) and np.abs(D - Dt.T).max() < 1e-12 and np.abs(D - M[:7, 7:]).max() < 1e-12
    D0 = xr.distance_rows(Q, R)
    assert np.all(D <= D0 + 1e-12) and (D < D0 - 0.1).any()  # (the relabelled / reflected copies are much closer)


def test_hand_made_square():
    """four atoms near a square (a chiral arrangement), a copy with two labels exchanged and a mirror image"""
    sq = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, -1.0, 0]])
    bent = sq + np.array([[0.3, 0, 0.2], [0, 0, 0], [0, 0.1, 0], [0, 0, -0.4]])
    swap = np.array([[0, 1, 2, 3], [2, 1, 0, 3]])  # atoms 0 and 2 exchanged
    X = np.stack([bent, bent[swap[1]], bent * np.array([1.0, 1.0, -1.0])])
    plain = ks.self_rows(X, swap[:1])
    assert plain[0, 1] > 0.1 and plain[0, 2] > 0.1
    sym = ks.self_rows(X, swap)
    assert sym[0, 1] < 1e-12 and sym[0, 2] > 0.1  # the table does not undo a reflection
    both = ks.self_rows(X, swap, mirror=True)
    assert both[0, 1] < 1e-12 and both[0, 2] < 1e-12 and both[1, 2] < 1e-12
    assert np.all(both <= sym + 1e-12) and np.all(sym <= plain + 1e-12)


@pytest.mark.parametrize("kind,A", [("path", 7), ("blocks", 13), ("swaps64", 20)])
def test_copies_are_at_distance_zero(kind, A):
    """a conformer against its relabelled copy, and with the flag against its reflected copy"""
    X = syn.continuous_ensemble(6, A, seed=4)
    table = ds.table(kind, A)
    for row in table[1:4]:
        Y = X[:, row]
        assert np.diag(ks.distance_rows(X, Y, table)).max() < 1e-12
        assert np.diag(xr.distance_rows(X, Y)).min() > 1e-3
        Z = er.reflect(Y, np.arange(len(Y)), axis=2)
        assert np.diag(ks.distance_rows(X, Z, table, mirror=True)).max() < 1e-12
        assert np.diag(ks.distance_rows(X, Z, table)).min() > 1e-3


def test_lists_under_d_sym_name_the_copies():
    """the issue's observation at a small size: under d the relabelled copy is somewhere in the list, under d_sym first"""
    X = syn.continuous_ensemble(12, 9, seed=8)
    table = sr.path_table(9)
    Y = np.concatenate([X, X[:, table[1]]])
    nb = ks.knn_from_rows(ks.self_rows(Y, table), 1)
    assert np.array_equal(nb.indices[:, 0], np.concatenate([np.arange(12) + 12, np.arange(12)]))
    assert nb.distances.max() < 1e-12
    plain = ks.knn_from_rows(ks.self_rows(Y, table[:1]), 1)
    assert not np.array_equal(plain.indices, nb.indices)
    cross = ks.knn_cross_from_rows(ks.distance_rows(X, Y, table), 2)
    assert np.array_equal(np.sort(cross.indices, axis=1), np.stack([np.arange(12), np.arange(12) + 12], axis=1))


def test_mean_distance():
    from firecode_amd.pruner import EnsembleCoverage, RmsdCrossNeighbours

    inf = np.inf
    nb = RmsdCrossNeighbours(np.array([[0], [2], [-1], [1]], dtype=np.int32), np.array([[0.25], [0.75], [inf], [1.5]]))
    cov = EnsembleCoverage.from_neighbours(nb, 1.0)
    assert cov.covered.tolist() == [True, True, False, False] and cov.fraction == 0.5
    assert cov.mean_distance() == pytest.approx((0.25 + 0.75 + 1.5) / 3) == ks.mean_distance(cov.distances)
    none = EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(np.full((3, 1), -1, dtype=np.int32), np.full((3, 1), inf)), 1.0)
    assert np.isnan(none.mean_distance()) and none.fraction == 0.0
    empty = EnsembleCoverage.from_neighbours(RmsdCrossNeighbours(np.zeros((0, 1), dtype=np.int32), np.zeros((0, 1))), 1.0)
    assert np.isnan(empty.mean_distance()) and np.isnan(empty.fraction)
    one = EnsembleCoverage(np.array([True]), 1.0, np.array([0], dtype=np.int32), np.array([0.125]))
    assert one.mean_distance() == 0.125


# ---- 2. the boundary ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fc_ensemble_knn_perm", "fc_ensemble_knn_cross_perm", "fc_bench_knn_perm", "fc_bench_knn_cross_perm")


def test_new_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "fc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared in include/fc_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.fc_abi_version() == 1
    # neither header block lists the aware forms as missing any more
    for start, end in (("k nearest neighbours of every conformer", "#define FC_KNN_MAX"),
                       ("The same lists across two ensembles", "int fc_ensemble_knn_cross(")):
        block = text[text.index(start):text.index(end)]
        assert "fc_ensemble_knn_perm" in block or "fc_ensemble_knn_cross_perm" in block


def _callables():
    import firecode_amd as fc

    E = fc.ensemble.Ensemble
    return (_lib.DeviceEnsemble.knn, _lib.DeviceEnsemble.knn_against, _lib.DeviceEnsemble.bench_knn,
            _lib.DeviceEnsemble.bench_knn_against, fc.pruner.knn_by_rmsd, fc.pruner.knn_by_rmsd_against,
            fc.pruner.novel_conformers, fc.pruner.ensemble_coverage, E.nearest_neighbours, E.nearest_in, E.novel_against)


def test_keyword_defaults():
    fns = _callables()
    assert len(fns) == 11
    for fn in fns:
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["symmetry", "prune_enantiomers"], fn
        assert params["symmetry"].default is None and params["prune_enantiomers"].default is False


def _handle_less_ensemble(N, A):
    """a DeviceEnsemble that has no handle: whatever raises on it raised before the device was asked for anything"""
    ens = _lib.DeviceEnsemble.__new__(_lib.DeviceEnsemble)
    ens.N, ens.A_all, ens.W, ens._atom_mask, ens._h = N, A, 1, None, None
    return ens


def _python_calls(X, atoms, k=2, max_rmsd=0.5, **kw):
    """every Python entry of the three layers, on objects that own no device handle"""
    import firecode_amd as fc

    E = fc.ensemble.Ensemble
    ens = lambda: _handle_less_ensemble(len(X), len(atoms))  # noqa: E731
    return [
        lambda: ens().knn(k, **kw),
        lambda: ens().bench_knn(k, **kw),
        lambda: ens().knn_against(ens(), k, max_rmsd=max_rmsd, **kw),
        lambda: ens().bench_knn_against(ens(), k, max_rmsd=max_rmsd, **kw),
        lambda: fc.pruner.knn_by_rmsd(X, atoms, k, **kw),
        lambda: fc.pruner.knn_by_rmsd_against(X, X, atoms, k, max_rmsd=max_rmsd, **kw),
        lambda: fc.pruner.novel_conformers(X, X, atoms, max_rmsd, **kw),
        lambda: fc.pruner.ensemble_coverage(X, X, atoms, max_rmsd, **kw),
        lambda: E(atoms, X, logfunction=None).nearest_neighbours(k, **kw),
        lambda: E(atoms, X, logfunction=None).nearest_in(E(atoms, X, logfunction=None), k=k, max_rmsd=max_rmsd, **kw),
        lambda: E(atoms, X, logfunction=None).novel_against(E(atoms, X, logfunction=None), max_rmsd, **kw),
    ]


def _c_calls(table, A_sel, mirror=0, k=2, max_rmsd=float("inf")):
    """the four C entry points with NULL handles -> [(return code, message)]"""
    lib = _lib.load()
    t32 = None if table is None else np.ascontiguousarray(table, dtype=np.int32)
    tp, K = (None, 2) if t32 is None else (_lib.ptr(t32, C.c_int32), len(t32))
    idx, dist = np.zeros(8, dtype=np.int32), np.zeros(8)
    pi32, ms = idx.ctypes.data_as(C.POINTER(C.c_int32)), C.c_double(0)
    out = []
    for call in (lambda: lib.fc_ensemble_knn_perm(None, tp, K, A_sel, mirror, k, pi32, _lib.pf(dist)),
                 lambda: lib.fc_ensemble_knn_cross_perm(None, None, tp, K, A_sel, mirror, k, max_rmsd, pi32, _lib.pf(dist)),
                 lambda: lib.fc_bench_knn_perm(None, tp, K, A_sel, mirror, k, 1, C.byref(ms), C.byref(ms), None, None),
                 lambda: lib.fc_bench_knn_cross_perm(None, None, tp, K, A_sel, mirror, k, max_rmsd, 1, C.byref(ms),
                                                     C.byref(ms), None, None)):
        out.append((call(), lib.fc_last_error().decode()))
    assert not idx.any() and not dist.any()  # a refusal writes nothing
    return out


def _bad_tables(A):
    ident = np.arange(A)
    not_perm = ident.copy()
    not_perm[1] = 0
    return {
        "too many": (np.stack([ident] * 65), _lib.FC_E_LIMIT, "FC_PERM_MAX"),
        "not a permutation": (np.stack([ident, not_perm]), _lib.FC_E_INVALID, "not a permutation"),
        "out of range": (np.stack([ident, ident + 1]), _lib.FC_E_INVALID, "not a permutation"),
        "no identity": (np.stack([ident[::-1], ident]), _lib.FC_E_INVALID, "identity"),
        "not closed": (np.stack([ident, np.roll(ident, 1)]), _lib.FC_E_INVALID, "closed under inverse"),
    }


@pytest.mark.parametrize("what", ["too many", "not a permutation", "out of range", "no identity", "not closed"])
def test_bad_tables_are_refused_before_any_device_use(what):
    import firecode_amd as fc

    A = 6
    table, code, text = _bad_tables(A)[what]
    X, atoms = np.zeros((3, A, 3)), np.array(["C"] * A)
    for flag in (False, True):
        for call in _python_calls(X, atoms, symmetry=table, prune_enantiomers=flag):
            with pytest.raises(fc.FirecodeHipInputError, match=text) as err:
                call()
            assert err.value.code == code
    for rc, msg in _c_calls(table, A):
        assert rc == code and text in msg
    # the table speaks before anything else that is wrong with the call
    for rc, msg in _c_calls(table, A, mirror=2, k=0, max_rmsd=-1.0):
        assert rc == code and text in msg


def test_good_table_then_the_other_checks():
    """the table is looked at first, then the flag, then the handles, then the sibling's own checks"""
    t = sr.path_table(6)
    for rc, msg in _c_calls(t, 6, mirror=2, k=0):
        assert rc == _lib.FC_E_INVALID and "mirror" in msg
    for rc, msg in _c_calls(t, 6, mirror=-1):
        assert rc == _lib.FC_E_INVALID and "mirror" in msg
    for mirror in (0, 1):
        for k, cap in ((2, float("inf")), (0, float("inf")), (65, float("inf")), (2, -1.0), (2, float("nan"))):
            for rc, msg in _c_calls(t, 6, mirror=mirror, k=k, max_rmsd=cap):  # (the handle's A_sel comes before k and the cap)
                assert rc == _lib.FC_E_INVALID and "NULL" in msg
    for rc, msg in _c_calls(None, 6):
        assert rc == _lib.FC_E_INVALID and "perms is NULL" in msg
    for rc, _ in _c_calls(t[:0], 6):
        assert rc == _lib.FC_E_INVALID
    for rc, _ in _c_calls(t, 0):
        assert rc == _lib.FC_E_INVALID
    lib, ms = _lib.load(), C.c_double(0)
    t32 = np.ascontiguousarray(t, dtype=np.int32)
    assert lib.fc_bench_knn_perm(None, _lib.ptr(t32, C.c_int32), 2, 6, 0, 2, 0, C.byref(ms), C.byref(ms), None, None) == _lib.FC_E_INVALID
    assert lib.fc_bench_knn_cross_perm(None, None, _lib.ptr(t32, C.c_int32), 2, 6, 0, 2, 1.0, 5000, C.byref(ms), C.byref(ms),
                                       None, None) == _lib.FC_E_INVALID


def test_python_layers_refuse_the_rest_before_any_device_use():
    """a table of another width (the A_sel mismatch of the Python layers), k = 0 and 65, a bad cap -- with a good table
    and with the flag alone"""
    import firecode_amd as fc

    A = 6
    X, atoms, t = np.zeros((3, A, 3)), np.array(["C"] * A), sr.path_table(A)
    for call in _python_calls(X, atoms, symmetry=sr.path_table(A - 1)):
        with pytest.raises(fc.FirecodeHipInputError, match=r"\(K, 6\) integer table") as err:
            call()
        assert err.value.code == _lib.FC_E_INVALID
    for kw in (dict(symmetry=t), dict(prune_enantiomers=True), dict(symmetry=t, prune_enantiomers=True)):
        for bad in (dict(k=0), dict(k=65), dict(max_rmsd=0.0), dict(max_rmsd=float("nan")), dict(max_rmsd=-1.0)):
            calls = _python_calls(X, atoms, **bad, **kw)
            if "max_rmsd" in bad:  # (the calls that take a cap)
                calls = [calls[2], calls[3], calls[5], calls[6], calls[7], calls[9], calls[10]]
            else:                   # (the calls that take k)
                calls = [calls[0], calls[1], calls[2], calls[3], calls[4], calls[5], calls[8], calls[9]]
            for call in calls:
                with pytest.raises(fc.FirecodeHipInputError):
                    call()
        with pytest.raises(fc.FirecodeHipError) as err:
            fc.pruner.knn_by_rmsd(X, atoms, 65, **kw)
        assert err.value.code == _lib.FC_E_LIMIT
        with pytest.raises(fc.FirecodeHipError) as err:
            fc.pruner.knn_by_rmsd_against(X, X, atoms, 65, **kw)
        assert err.value.code == _lib.FC_E_LIMIT
    # a permutation that leaves the atom selection
    atoms_h = np.array(["C", "C", "C", "C", "C", "H"])
    leaves = np.array([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 5, 4]])  # C4 <-> H5
    for call in (lambda: fc.pruner.knn_by_rmsd(X, atoms_h, 2, symmetry=leaves),
                 lambda: fc.pruner.ensemble_coverage(X, X, atoms_h, 0.5, symmetry=leaves)):
        with pytest.raises(fc.FirecodeHipInputError, match="outside the atom selection"):
            call()


def test_non_bool_flag_is_refused():
    import firecode_amd as fc

    X, atoms = np.zeros((3, 6, 3)), np.array(["C"] * 6)
    for bad in (1, 0, "yes", None, np.ones(2, bool)):
        for call in _python_calls(X, atoms, prune_enantiomers=bad):
            with pytest.raises(fc.FirecodeHipInputError, match="prune_enantiomers must be a bool"):
                call()


@pytest.mark.parametrize("K", [2, 64])
def test_lds_limit(K):
    """the documented formula: 16 x 24 A_sel + (2 K A_sel rounded up to 8) bytes within 160 KiB; one atom more is refused"""
    import firecode_amd as fc

    limit = 160 * 1024
    need = lambda a: 16 * 24 * a + ((2 * K * a + 7) // 8) * 8  # noqa: E731
    A = max(a for a in range(1, 1000) if need(a) <= limit)
    assert A == {2: 422, 64: 320}[K] == S.knn_max_selected(K) and need(A + 1) > limit
    assert S.knn_lds_bytes(K, A) == need(A) and S.knn_lds_bytes(K, A + 1) == need(A + 1)
    make = lambda a: sr.path_table(a) if K == 2 else sr.transposition_table(a, 6)  # noqa: E731
    for rc, msg in _c_calls(make(A), A):
        assert rc == _lib.FC_E_INVALID and "NULL" in msg  # (admitted: the next check speaks)
    for rc, msg in _c_calls(make(A + 1), A + 1, mirror=2):  # (the LDS limit belongs to the table: before the flag)
        assert rc == _lib.FC_E_LIMIT and "LDS" in msg
    S.knn_lds_check(K, A)
    with pytest.raises(fc.FirecodeHipInputError, match="LDS") as err:
        S.knn_lds_check(K, A + 1)
    assert err.value.code == _lib.FC_E_LIMIT
    X, atoms = np.zeros((2, A + 1, 3)), np.array(["C"] * (A + 1))
    for call in _python_calls(X, atoms, symmetry=make(A + 1)):
        with pytest.raises(fc.FirecodeHipInputError, match="LDS") as err:
            call()
        assert err.value.code == _lib.FC_E_LIMIT
    # the table over all atoms may be wider: the limit is on the selected atoms
    atoms_h = np.array(["C"] * A + ["H"] * 3)
    t = S.knn_table(S.resolve(np.arange(A + 3)[None], atoms_h), True, atoms_h != "H", A + 3)
    assert t.shape == (1, A) and t.dtype == np.int32
    assert S.knn_table(None, False, atoms_h != "H", A + 3) is None


def test_empty_sets_need_no_device():
    import firecode_amd as fc

    A = 6
    atoms, t = np.array(["C"] * A), sr.path_table(A)
    some, none = np.zeros((4, A, 3)), np.zeros((0, A, 3))
    for kw in (dict(symmetry=t), dict(prune_enantiomers=True), dict(symmetry=t, prune_enantiomers=True)):
        nb = fc.pruner.knn_by_rmsd(none, atoms, 3, **kw)
        assert nb.indices.shape == (0, 3) and nb.indices.dtype == np.int32
        nb = fc.pruner.knn_by_rmsd_against(some, none, atoms, 3, **kw)
        assert nb.indices.shape == (4, 3) and np.all(nb.indices == -1) and np.all(np.isposinf(nb.distances))
        assert fc.pruner.knn_by_rmsd_against(none, some, atoms, 3, **kw).indices.shape == (0, 3)
        assert fc.pruner.novel_conformers(some, none, atoms, 0.5, **kw).tolist() == [True] * 4
        cov = fc.pruner.ensemble_coverage(none, some, atoms, 0.5, **kw)
        assert cov.fraction == 0.0 and np.isnan(cov.mean_distance())
        # ... and excuse nothing
        with pytest.raises(fc.FirecodeHipInputError, match="closed under inverse"):
            fc.pruner.knn_by_rmsd(none, atoms, 3, symmetry=np.stack([np.arange(A), np.roll(np.arange(A), 1)]))


def test_a_graph_is_perceived():
    import networkx as nx

    import firecode_amd as fc

    g = nx.path_graph(6)
    with pytest.raises(fc.FirecodeHipInputError, match="element symbols"):
        _handle_less_ensemble(3, 6).knn(2, symmetry=g)
    atoms = np.array(["C"] * 6)
    table = S.resolve(g, atoms)
    assert np.array_equal(table, sr.path_table(6))
    assert fc.pruner.knn_by_rmsd(np.zeros((0, 6, 3)), atoms, 2, symmetry=g).indices.shape == (0, 2)


def test_no_cpu_fallback_for_the_new_calls():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import firecode_amd as fc

    X, atoms = syn.continuous_ensemble(5, 6, seed=1), np.array(["C"] * 6)
    for kw in ({"symmetry": sr.path_table(6)}, {"prune_enantiomers": True}):
        with pytest.raises(fc.FirecodeHipDeviceError):
            fc.pruner.knn_by_rmsd(X, atoms, 3, **kw)
        with pytest.raises(fc.FirecodeHipDeviceError):
            fc.pruner.ensemble_coverage(X, X, atoms, 0.5, **kw)
