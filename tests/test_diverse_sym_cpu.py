"""Symmetry- and mirror-aware RMSD-diverse selection without a device: the restatement of d_sym (tests/diverse_sym_ref.py)
and every refusal the contract lists (include/fc_hip.h, fc_ensemble_select_diverse_perm), each raised before any device
use -- through the Python layers and on the C entry point itself with a NULL handle."""

import ctypes as C
import inspect
import os
import re

import networkx as nx
import numpy as np
import pytest

import diverse_ref as dr
import diverse_sym_ref as ds
import enant_ref as er
import symm_ref as sr
from firecode_amd import _lib
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,A", [("path", 9), ("blocks", 13), ("swaps64", 14)])
@pytest.mark.parametrize("mirror", [False, True])
def test_d_sym_is_symmetric_and_below_d(kind, A, mirror):
    """tables closed under inverse: d_sym(i, j) = d_sym(j, i); the identity is in the table: d_sym <= d"""
    X, _, table, _ = ds.ensemble("clusters", 24, A, kind, mirror)
    M = ds.matrix(X, table, mirror)
    assert np.abs(M - M.T).max() < 1e-12
    M0 = np.stack([dr.rmsd_row(X, s) for s in range(len(X))])
    assert np.all(M <= M0 + 1e-12) and (M < M0 - 0.1).any()  # (the relabelled / reflected copies are much closer)


def test_identity_without_mirror_is_the_default_row():
    X, _, _ = syn.synthetic_ensemble(30, 11, seed=5)
    row = ds.sym_row(ds.table("identity", 11), mirror=False)
    for s in (0, 7, 29):
        assert np.abs(row(X, s) - dr.rmsd_row(X, s)).max() < 1e-12
    ref = dr.select_diverse(X, 12, start=2)
    got = dr.select_diverse(X, 12, start=2, row=row)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.abs(got[2] - ref[2]).max() < 1e-12


def test_mirror_distance_to_the_own_reflection_is_zero():
    X = syn.continuous_ensemble(12, 17, seed=2)
    Y = np.concatenate([X, er.reflect(X, np.arange(12), axis=1)])
    M = ds.matrix(Y, ds.table("identity", 17), mirror=True)
    assert np.abs(M[np.arange(12), 12 + np.arange(12)]).max() < 1e-12
    M0 = ds.matrix(Y, ds.table("identity", 17), mirror=False)
    assert M0[np.arange(12), 12 + np.arange(12)].min() > 0.1  # (without the flag they are far apart)


def test_cover_is_one_per_cluster_under_d_sym_only():
    """the issue's observation at a small size: relabelled and reflected copies make the default cover pick duplicates"""
    X, _, table, cid = ds.ensemble("clusters", 60, 13, "blocks", True)
    sym = dr.select_diverse(X, len(X), stop_rmsd=0.5, row=ds.sym_row(table, True))
    plain = dr.select_diverse(X, len(X), stop_rmsd=0.5)
    assert sorted(cid[sym[0]].tolist()) == list(range(12)) and len(plain[0]) > len(sym[0])
    assert np.array_equal(cid[sym[0]][sym[1]], cid)


def test_recorded_cover_is_the_restatement_s():
    """tests/golden/diverse_sym_v1.npz against the functions that wrote it: the ensemble's generator still gives the
    coordinates the record belongs to -- the rows of three of its picks, recomputed, are the recorded distances where
    those picks are the representative and nowhere below them"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "diverse_sym_v1.npz"), allow_pickle=False)
    X, _, table, cid = ds.ensemble("clusters", 600, 80, "path", True)
    idx, lab, dist = g["cover_indices"], g["cover_labels"], g["cover_distances"]
    assert len(idx) == 120 and sorted(cid[idx].tolist()) == list(range(120)) and float(g["cover_min_gap"]) > 1e-9
    assert g["prune_mask"].shape == (600,) and g["prune_mask"].sum() > 120
    row = ds.sym_row(table, True)
    for k in (0, 57, 119):
        r = row(X, int(idx[k]))
        mine = (lab == k) & (np.arange(600) != idx[k])
        assert mine.sum() == 4 and np.abs(r[mine] - dist[mine]).max() < 1e-12 and np.all(r >= dist - 1e-12)
    assert np.all(dist[idx] == 0.0) and abs(g["cover_radii"][1] - row(X, int(idx[0]))[idx[1]]) < 1e-12


# ---- 2. the boundary ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fc_ensemble_select_diverse_perm", "fc_bench_select_diverse_perm")


def test_new_symbols_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fc_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/fc_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.fc_abi_version() == 1


def test_keyword_defaults():
    import firecode_amd as fc

    for fn in (_lib.DeviceEnsemble.select_diverse, fc.pruner.select_diverse, fc.ensemble.Ensemble.diversity_selection,
               fc.torsion_module.most_diverse_conformers, fc.torsion_module.clustered_csearch_core,
               fc.torsion_module.clustered_csearch):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["symmetry", "prune_enantiomers"], fn
        assert inspect.signature(fn).parameters["symmetry"].default is None
        assert inspect.signature(fn).parameters["prune_enantiomers"].default is False


def _graph(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


def _handle_less_ensemble(N, A):
    """a DeviceEnsemble that has no handle: whatever raises on it raised before the device was asked for anything"""
    ens = _lib.DeviceEnsemble.__new__(_lib.DeviceEnsemble)
    ens.N, ens.A_all, ens.W, ens._atom_mask, ens._h = N, A, 1, None, None
    return ens


def _python_calls(X, atoms, **kw):
    import firecode_amd as fc

    return [
        lambda: _handle_less_ensemble(len(X), len(atoms)).select_diverse(3, **kw),
        lambda: fc.pruner.select_diverse(X, atoms, n=3, **kw),
        lambda: fc.ensemble.Ensemble(atoms, X, logfunction=None).diversity_selection(n=3, **kw),
        lambda: fc.torsion_module.most_diverse_conformers(2, list(X), method="rmsd", atoms=atoms, **kw),
    ]


def _c_call(table, A_sel, mirror=0, handle=None):
    lib = _lib.load()
    t32 = np.ascontiguousarray(table, dtype=np.int32)
    n = C.c_int64(0)
    idx = np.zeros(4, dtype=np.int64)
    rc = lib.fc_ensemble_select_diverse_perm(handle, _lib.ptr(t32, C.c_int32), len(t32), A_sel, mirror, 3, 0, -1.0,
                                             _lib.pi(idx), None, None, None, C.byref(n))
    return rc, lib.fc_last_error().decode()


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
    for call in _python_calls(X, atoms, symmetry=table):
        with pytest.raises(fc.FirecodeHipInputError, match=text) as err:
            call()
        assert err.value.code == code
    rc, msg = _c_call(table, A)
    assert rc == code and text in msg


def test_good_table_then_the_other_checks():
    """the table is looked at first, then the LDS, then the flag, then the handle"""
    t = sr.path_table(6)
    rc, msg = _c_call(t, 6, mirror=2)
    assert rc == _lib.FC_E_INVALID and "mirror" in msg
    for mirror in (0, 1):
        rc, msg = _c_call(t, 6, mirror=mirror)
        assert rc == _lib.FC_E_INVALID and "ens is NULL" in msg
    lib = _lib.load()
    n = C.c_int64(0)
    assert lib.fc_ensemble_select_diverse_perm(None, None, 2, 6, 0, 3, 0, -1.0, None, None, None, None, C.byref(n)) == _lib.FC_E_INVALID
    rc, _ = _c_call(t[:0], 6)
    assert rc == _lib.FC_E_INVALID


@pytest.mark.parametrize("K", [2, 64])
def test_lds_limit(K):
    """the documented formula: 24 A_sel + (2 K A_sel rounded up to 8) + 64 bytes within 160 KiB; one atom more is refused"""
    import firecode_amd as fc

    limit = 160 * 1024
    need = lambda a: 24 * a + ((2 * K * a + 7) // 8) * 8 + 64  # noqa: E731
    A = max(a for a in range(1, 8000) if need(a) <= limit)
    assert A == {2: 5849, 64: 1077}[K] == S.diverse_max_selected(K) and need(A + 1) > limit
    make = lambda a: sr.path_table(a) if K == 2 else sr.transposition_table(a, 6)  # noqa: E731
    rc, msg = _c_call(make(A), A)
    assert rc == _lib.FC_E_INVALID and "ens is NULL" in msg  # (admitted: the next check speaks)
    rc, msg = _c_call(make(A + 1), A + 1)
    assert rc == _lib.FC_E_LIMIT and "LDS" in msg
    X, atoms = np.zeros((2, A + 1, 3)), np.array(["C"] * (A + 1))
    for call in _python_calls(X, atoms, symmetry=make(A + 1)):
        with pytest.raises(fc.FirecodeHipInputError, match="LDS") as err:
            call()
        assert err.value.code == _lib.FC_E_LIMIT
    S.diverse_lds_check(K, A)


def test_non_bool_flag_is_refused():
    import firecode_amd as fc

    X, atoms = np.zeros((3, 6, 3)), np.array(["C"] * 6)
    for bad in (1, 0, "yes", None, np.ones(2, bool)):
        for call in _python_calls(X, atoms, prune_enantiomers=bad) + [
                lambda: fc.torsion_module.clustered_csearch_core(X[0], [], [], diversity="rmsd", prune_enantiomers=bad)]:
            with pytest.raises(fc.FirecodeHipInputError, match="prune_enantiomers must be a bool"):
                call()


def test_random_draw_takes_neither_keyword():
    import firecode_amd as fc

    X, t = np.zeros((5, 6, 3)), sr.path_table(6)
    for kw in ({"symmetry": t}, {"prune_enantiomers": True}, {"symmetry": t, "prune_enantiomers": True}):
        with pytest.raises(fc.FirecodeHipInputError, match="method='rmsd'"):
            fc.torsion_module.most_diverse_conformers(2, list(X), **kw)
        with pytest.raises(fc.FirecodeHipInputError, match="diversity='rmsd'"):
            fc.torsion_module.clustered_csearch_core(X[0], [], [], **kw)
    assert len(fc.torsion_module.most_diverse_conformers(2, list(X), seed=1)) == 2  # (the draw itself is as it was)


def test_a_graph_needs_the_element_symbols():
    import firecode_amd as fc

    g = _graph(6, [(a, a + 1) for a in range(5)])
    with pytest.raises(fc.FirecodeHipInputError, match="element symbols"):
        _handle_less_ensemble(3, 6).select_diverse(3, symmetry=g)
    with pytest.raises(fc.FirecodeHipInputError, match="element symbols"):
        fc.torsion_module.most_diverse_conformers(2, list(np.zeros((5, 6, 3))), method="rmsd", symmetry=g)
    # where the symbols are known the graph is perceived: the path's reversal, checked like a table
    atoms = np.array(["C", "C", "C", "C", "C", "H"])
    with pytest.raises(fc.FirecodeHipInputError, match=r"\(K, 6\) integer table"):
        fc.pruner.select_diverse(np.zeros((3, 6, 3)), atoms, n=2, symmetry=np.zeros((2, 5), dtype=int))
    leaves = np.array([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 5, 4]])  # C4 <-> H5
    with pytest.raises(fc.FirecodeHipInputError, match="outside the atom selection"):
        fc.pruner.select_diverse(np.zeros((3, 6, 3)), atoms, n=2, symmetry=leaves)


def test_twin_workspace_is_refused():
    import firecode_amd as fc

    view = _lib._EnsembleView.__new__(_lib._EnsembleView)
    view.N, view.A_all, view.W = 3, 6, 1
    for kw in ({"symmetry": sr.path_table(6)}, {"prune_enantiomers": True}):
        with pytest.raises(fc.FirecodeHipInputError, match="twin workspace"):
            view.select_diverse(3, **kw)


def test_the_prune_still_refuses_the_combination():
    import firecode_amd as fc

    A = 6
    X, atoms, table = np.zeros((3, A, 3)), np.array(["C"] * A), sr.path_table(A)
    for call in (lambda: fc.pruner.prune_by_rmsd(X, atoms, 0.5, prune_enantiomers=True, symmetry=table),
                 lambda: fc.pruner.cluster_by_rmsd(X, atoms, 0.5, prune_enantiomers=True, symmetry=table),
                 lambda: fc.ensemble.Ensemble(atoms, X, logfunction=None).similarity_pruning(
                     prune_enantiomers=True, symmetry=table),
                 lambda: fc.rmsd.rmsd_and_max_batch(X, [0], [1], inverted=True, symmetry=table)):
        with pytest.raises(fc.FirecodeHipInputError, match="cannot be combined"):
            call()


def test_no_cpu_fallback_for_the_new_calls():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import firecode_amd as fc

    X, atoms = syn.continuous_ensemble(5, 6, seed=1), np.array(["C"] * 6)
    for kw in ({"symmetry": sr.path_table(6)}, {"prune_enantiomers": True}):
        with pytest.raises(fc.FirecodeHipDeviceError):
            fc.pruner.select_diverse(X, atoms, n=3, **kw)
