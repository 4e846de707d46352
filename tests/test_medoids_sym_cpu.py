"""Symmetry- and mirror-aware medoids, k-medoids and silhouettes without a device: the restatement's glue
(tests/medoid_sym_ref.py) against a brute-force loop, what d_sym does to the sums, and every refusal the contract lists
(include/fc_hip.h, fc_ensemble_medoids_perm / fc_ensemble_kmedoids_perm / fc_ensemble_silhouette_perm), each raised
before any device use -- through the Python layers and on the C entry points themselves with a NULL handle."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import diverse_sym_ref as ds
import medoid_ref as mr
import medoid_sym_ref as ms
import silhouette_ref as sil
import symm_ref as sr
from firecode_amd import _lib
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 2.0 ** 32


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
def _brute_rows(X, table, mirror):
    """d_sym pair by pair, one oracle call per (i, j, p, h)"""
    Xc = X - X.mean(axis=1, keepdims=True)
    N = len(Xc)
    D = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            D[i, j] = min(o.rmsd_and_max_batch(Xc[i][None], h * Xc[j][perm][None])[0][0]
                          for perm in table for h in ((1.0, -1.0) if mirror else (1.0,)))
    return D


@pytest.mark.parametrize("kind,A,mirror", [("path", 7, False), ("blocks", 13, True)])
def test_glue_against_a_brute_force_loop(kind, A, mirror):
    X, atoms, table, _ = ds.ensemble("continuous", 12, A, kind, mirror)
    D = ms.rows(X, atoms, table, mirror)
    B = _brute_rows(X, table, mirror)
    assert np.abs(D - B).max() < 1e-12
    labels = np.arange(12) % 3
    # medoids: the upper triangle serves both partners
    ref = ms.medoids(D, labels)
    for c in range(3):
        mem = np.flatnonzero(labels == c)
        tri = lambda M, i, j: int(np.rint(M[min(i, j), max(i, j)] * Q))  # noqa: E731
        assert [int(v) for v in ref.sums_q32[mem]] == [sum(tri(D, i, j) for j in mem if j != i) for i in mem]
        brute = [sum(tri(B, i, j) for j in mem if j != i) for i in mem]
        assert max(abs(int(v) - w) for v, w in zip(ref.sums_q32[mem], brute)) <= 64  # (1e-12 A per distance)
        assert ref.medoids[c] == mem[int(np.argmin(ref.sums_q32[mem]))]
    # silhouettes: every ordered pair, a and b from the brute rows
    got = ms.silhouette(D, labels)
    s_txt, a_txt, b_txt = sil.textbook_from_matrix(B, labels)
    assert np.abs(got.intra - a_txt).max() < 1e-9 and np.abs(got.nearest_mean - b_txt).max() < 1e-9
    assert np.abs(got.values - s_txt).max() < 1e-8
    # k-medoids: the loop on the same rows ends at a local minimum of the brute cost
    km = ms.kmedoids(D, 3)
    cost = sum(0.0 if j in km.medoids else min(B[j, m] for m in km.medoids) for j in range(12))
    assert abs(km.cost_q32 / Q - cost) < 1e-8 and km.cost_q32 <= km.cost0_q32


def test_sums_under_d_sym_never_exceed_the_plain_ones():
    X, atoms, table, cid = ds.ensemble("clusters", 40, 13, "blocks", True)
    Xs = ms.prepared(X, atoms)
    D, D0 = ms.rows(X, atoms, table, True), mr.distance_rows(Xs)
    assert np.all(D <= D0 + 1e-12)
    for labels in (None, cid, np.arange(40) % 4):
        a, b = ms.medoids(D, labels), mr.medoids_from_rows(D0, labels)
        assert np.all(a.sums_q32 <= b.sums_q32 + np.uint64(64)) and np.all(a.eccentricity <= b.eccentricity + 1e-12)
        assert np.array_equal(a.sizes, b.sizes)
        sa, sb = ms.silhouette(D, labels), sil.silhouette_from_rows(D0, labels)
        assert np.all(sa.intra <= sb.intra + 1e-10)
        if labels is not None:
            assert np.all(sa.nearest_mean <= sb.nearest_mean + 1e-10)
    assert ms.kmedoids(D, 5).cost_q32 < mr.kmedoids_from_rows(D0, 5).cost_q32


def test_identity_table_without_the_flag_is_the_plain_restatement():
    X, atoms, table, cid = ds.ensemble("clusters", 30, 7, "path", True)
    Xs = ms.prepared(X, atoms)
    D, D0 = ms.rows(X, atoms, table[:1], False), mr.distance_rows(Xs)
    assert np.array_equal(D, D0)
    for a, b in ((ms.medoids(D, cid), mr.medoids_from_rows(D0, cid)), (ms.silhouette(D, cid), sil.silhouette_from_rows(D0, cid)),
                 (ms.kmedoids(D, 4), mr.kmedoids_from_rows(D0, 4))):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)


def test_the_labelling_judged_under_the_wrong_distance():
    """the figures of the issue: the clustered ensemble with relabelled and reflected halves under its own 20 labels"""
    X, atoms, table, cid = ds.ensemble("clusters", 100, 13, "blocks", True)
    D, D0 = ms.rows(X, atoms, table, True), mr.distance_rows(ms.prepared(X, atoms))
    good, bad = ms.silhouette(D, cid), sil.silhouette_from_rows(D0, cid)
    print(f"score under d_sym {good.score:.4f}, under d {bad.score:.4f}")
    assert good.score > 0.9 and bad.score < 0.0
    ma, mb = ms.medoids(D, cid), mr.medoids_from_rows(D0, cid)
    assert (ma.medoids != mb.medoids).sum() >= 5 and (good.nearest != bad.nearest).sum() > 50
    assert ms.kmedoids(D, 5).cost_q32 < mr.kmedoids_from_rows(D0, 5).cost_q32


# ---- 2. the boundary ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fc_ensemble_medoids_perm", "fc_ensemble_kmedoids_perm", "fc_ensemble_silhouette_perm")


def test_new_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "fc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared in include/fc_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
        n_args = len(re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1).split(","))
        assert len(_lib._SIGNATURES[name]) == n_args, name
    assert lib.fc_abi_version() == 1
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "No symmetry- or mirror-aware form" not in readme and "medoids_by_rmsd_sym" in readme


def _callables():
    import firecode_amd as fc

    E, D = fc.ensemble.Ensemble, _lib.DeviceEnsemble
    return (D.medoids_sym, D.kmedoids_sym, D.silhouette_sym, fc.pruner.medoids_by_rmsd_sym, fc.pruner.kmedoids_by_rmsd_sym,
            fc.pruner.silhouette_by_rmsd_sym, fc.pruner.silhouette_scan_sym, E.medoids_sym, E.silhouette_sym,
            E.kmedoids_selection_sym)


def test_keywords_and_the_plain_signatures():
    import firecode_amd as fc

    for fn in _callables():
        params = inspect.signature(fn).parameters
        assert params["symmetry"].default is None and params["prune_enantiomers"].default is False, fn
    # the new callables are the plain ones plus the two keywords
    for plain, aware in ((fc.pruner.medoids_by_rmsd, fc.pruner.medoids_by_rmsd_sym),
                         (fc.pruner.kmedoids_by_rmsd, fc.pruner.kmedoids_by_rmsd_sym),
                         (fc.pruner.silhouette_by_rmsd, fc.pruner.silhouette_by_rmsd_sym),
                         (fc.pruner.silhouette_scan, fc.pruner.silhouette_scan_sym)):
        assert list(inspect.signature(aware).parameters) == list(inspect.signature(plain).parameters) + ["symmetry", "prune_enantiomers"]
    # ... and the plain ones keep theirs
    for plain in (fc.pruner.medoids_by_rmsd, fc.pruner.silhouette_by_rmsd, _lib.DeviceEnsemble.medoids, _lib.DeviceEnsemble.silhouette):
        assert "symmetry" not in inspect.signature(plain).parameters


def _handle_less_ensemble(N, A):
    """a DeviceEnsemble that has no handle: whatever raises on it raised before the device was asked for anything"""
    ens = _lib.DeviceEnsemble.__new__(_lib.DeviceEnsemble)
    ens.N, ens.A_all, ens.W, ens._atom_mask, ens._h = N, A, 1, None, None
    return ens


def _python_calls(X, atoms, labels=None, n=2, **kw):
    """every Python entry of the three layers, on objects that own no device handle"""
    import firecode_amd as fc

    E = fc.ensemble.Ensemble
    ens = lambda: _handle_less_ensemble(len(X), len(atoms))  # noqa: E731
    return [
        lambda: ens().medoids_sym(labels, **kw),
        lambda: ens().kmedoids_sym(n, **kw),
        lambda: ens().silhouette_sym(labels, **kw),
        lambda: fc.pruner.medoids_by_rmsd_sym(X, atoms, labels, **kw),
        lambda: fc.pruner.kmedoids_by_rmsd_sym(X, atoms, n, **kw),
        lambda: fc.pruner.silhouette_by_rmsd_sym(X, atoms, labels, **kw),
        lambda: E(atoms, X, logfunction=None).medoids_sym(labels, **kw),
        lambda: E(atoms, X, logfunction=None).silhouette_sym(labels, **kw),
        lambda: E(atoms, X, logfunction=None).kmedoids_selection_sym(n, **kw),
        lambda: fc.torsion_module.most_diverse_conformers(n, list(X), method="kmedoids_sym", atoms=atoms, **kw),
    ]


def _c_calls(table, A_sel, mirror=0, n_groups=1, n=1):
    """the three C entry points with a NULL handle -> [(return code, message)]"""
    lib = _lib.load()
    t32 = None if table is None else np.ascontiguousarray(table, dtype=np.int32)
    tp, K = (None, 2) if t32 is None else (_lib.ptr(t32, C.c_int32), len(t32))
    i64, f64, i32 = np.zeros(8, dtype=np.int64), np.zeros(8), np.zeros(8, dtype=np.int32)
    u64, score, n_iter = C.c_uint64(0), C.c_double(0), C.c_int64(0)
    pi, pf, p32 = _lib.pi(i64), _lib.pf(f64), _lib.ptr(i32, C.c_int32)
    out = []
    for call in (lambda: lib.fc_ensemble_medoids_perm(None, tp, K, A_sel, mirror, None, n_groups, pi, pi, pf, pf, None, None, None, None),
                 lambda: lib.fc_ensemble_kmedoids_perm(None, tp, K, A_sel, mirror, None, n, 5, pi, p32, pf, C.byref(u64), C.byref(n_iter)),
                 lambda: lib.fc_ensemble_silhouette_perm(None, tp, K, A_sel, mirror, None, n_groups, pf, pf, pf, p32, pf, pi,
                                                         C.byref(score), None, None)):
        out.append((call(), lib.fc_last_error().decode()))
    assert not i64.any() and not f64.any() and not i32.any()  # a refusal writes nothing
    return out


def _bad_tables(A):
    ident = np.arange(A)
    not_perm = ident.copy()
    not_perm[1] = 0
    return {
        "too many": (np.stack([ident] * 65), _lib.FC_E_LIMIT, "FC_PERM_MAX"),
        "not a permutation": (np.stack([ident, not_perm]), _lib.FC_E_INVALID, "not a permutation"),
        "no identity": (np.stack([ident[::-1], ident]), _lib.FC_E_INVALID, "identity"),
        "not closed": (np.stack([ident, np.roll(ident, 1)]), _lib.FC_E_INVALID, "closed under inverse"),
    }


@pytest.mark.parametrize("what", ["too many", "not a permutation", "no identity", "not closed"])
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
        with pytest.raises(fc.FirecodeHipInputError):
            fc.pruner.silhouette_scan_sym(X, atoms, [0.5], symmetry=table)
    for rc, msg in _c_calls(table, A):
        assert rc == code and text in msg
    # the table speaks before anything else that is wrong with the call
    for rc, msg in _c_calls(table, A, mirror=2, n_groups=0, n=0):
        assert rc == code and text in msg


def test_good_table_then_the_other_checks():
    """the table, its LDS, the flag, the handle -- where fc_ensemble_knn_perm has them -- then the plain twin's checks"""
    t = sr.path_table(6)
    for rc, msg in _c_calls(t, 6, mirror=2, n_groups=0, n=0):
        assert rc == _lib.FC_E_INVALID and "mirror" in msg
    for rc, msg in _c_calls(t, 6, mirror=-1):
        assert rc == _lib.FC_E_INVALID and "mirror" in msg
    for mirror in (0, 1):
        for rc, msg in _c_calls(t, 6, mirror=mirror, n_groups=0, n=0):
            assert rc == _lib.FC_E_INVALID and "ens is NULL" in msg
    for rc, msg in _c_calls(None, 6):
        assert rc == _lib.FC_E_INVALID and "perms is NULL" in msg
    for rc, _ in _c_calls(t[:0], 6):
        assert rc == _lib.FC_E_INVALID
    for rc, _ in _c_calls(t, 0):
        assert rc == _lib.FC_E_INVALID


def test_labels_and_counts_are_judged_as_the_plain_twins_judge_them():
    """behind a good table (and with the flag alone): the label, n_groups, n, max_iter and init errors of the plain
    callables, with their texts, before any device use; a bad table speaks first"""
    import firecode_amd as fc

    A = 6
    X, atoms, t = np.zeros((5, A, 3)), np.array(["C"] * A), sr.path_table(A)
    for kw in (dict(symmetry=t), dict(prune_enantiomers=True), dict(symmetry=t, prune_enantiomers=True), dict()):
        ens = lambda: _handle_less_ensemble(5, A)  # noqa: E731
        for bad, text in ((dict(labels=np.zeros(4, dtype=int)), "one entry per conformer"), (dict(labels=np.zeros(5)), "integers"),
                          (dict(labels=np.full(5, 3), n_groups=3), "not below n_groups"), (dict(n_groups=0), "n_groups")):
            for fn in ("medoids_sym", "silhouette_sym"):
                with pytest.raises(fc.FirecodeHipInputError, match=text):
                    getattr(ens(), fn)(**bad, **kw)
        for bad in (dict(n=0), dict(n=6), dict(n=2, max_iter=-1), dict(n=2, init=[0, 5]), dict(n=2, init=[4, 4]), dict(n=2, init=[1])):
            with pytest.raises(fc.FirecodeHipInputError):
                ens().kmedoids_sym(**bad, **kw)
            with pytest.raises(fc.FirecodeHipInputError):
                fc.pruner.kmedoids_by_rmsd_sym(X, atoms, bad["n"], init=bad.get("init"), max_iter=bad.get("max_iter", 50), **kw)
        for fn in (fc.pruner.medoids_by_rmsd_sym, fc.pruner.silhouette_by_rmsd_sym):
            with pytest.raises(fc.FirecodeHipInputError, match="one entry per conformer"):
                fn(X, atoms, np.zeros(4, dtype=int), **kw)
        with pytest.raises(fc.FirecodeHipInputError, match="method="):
            fc.pruner.silhouette_scan_sym(X, atoms, [0.5], method="kmeans", **kw)
        with pytest.raises(fc.FirecodeHipInputError):
            fc.pruner.silhouette_scan_sym(X, atoms, [[0.5]], **{k: v for k, v in kw.items() if len(kw) < 2})
    bad_table = np.stack([np.arange(A), np.roll(np.arange(A), 1)])
    with pytest.raises(fc.FirecodeHipInputError, match="closed under inverse"):
        fc.pruner.medoids_by_rmsd_sym(X, atoms, np.zeros(4, dtype=int), symmetry=bad_table)
    with pytest.raises(fc.FirecodeHipInputError, match="closed under inverse"):
        _handle_less_ensemble(5, A).silhouette_sym(np.zeros(4, dtype=int), symmetry=bad_table)
    # a twin workspace refuses as the other symmetry= forms do
    view = _lib._EnsembleView.__new__(_lib._EnsembleView)
    view.N, view.A_all, view._atom_mask = 5, A, None
    for call in (lambda: view.medoids_sym(symmetry=t), lambda: view.kmedoids_sym(2, prune_enantiomers=True),
                 lambda: view.silhouette_sym(symmetry=t)):
        with pytest.raises(fc.FirecodeHipInputError, match="twin workspace"):
            call()


def test_the_scan_refuses_the_combination_up_front():
    import firecode_amd as fc

    A = 6
    X, atoms, t = np.zeros((3, A, 3)), np.array(["C"] * A), sr.path_table(A)
    with pytest.raises(fc.FirecodeHipInputError, match="cannot be combined with symmetry=") as err:
        fc.pruner.silhouette_scan_sym(X, atoms, [0.5], symmetry=t, prune_enantiomers=True)
    assert err.value.code == _lib.FC_E_INVALID
    with pytest.raises(fc.FirecodeHipInputError) as same:  # the clusterers' own error
        S.refuse_with_enantiomers(t, True)
    assert str(same.value) == str(err.value)


def test_the_plain_methods_of_most_diverse_conformers_are_unchanged():
    import firecode_amd as fc

    X, atoms = np.zeros((3, 6, 3)), np.array(["C"] * 6)
    with pytest.raises(fc.FirecodeHipInputError, match="k-medoids has no such form"):
        fc.torsion_module.most_diverse_conformers(2, list(X), method="kmedoids", atoms=atoms, symmetry=sr.path_table(6))
    with pytest.raises(fc.FirecodeHipInputError, match="kmedoids_sym"):
        fc.torsion_module.most_diverse_conformers(2, list(X), method="pam")
    assert fc.torsion_module.most_diverse_conformers(2, [], method="kmedoids_sym", prune_enantiomers=True) == []


def test_non_bool_flag_is_refused():
    import firecode_amd as fc

    X, atoms = np.zeros((3, 6, 3)), np.array(["C"] * 6)
    for bad in (1, 0, "yes", None):
        for call in _python_calls(X, atoms, prune_enantiomers=bad):
            with pytest.raises(fc.FirecodeHipInputError, match="prune_enantiomers must be a bool"):
                call()


@pytest.mark.parametrize("K", [2, 64])
def test_lds_limit(K):
    """the formula of the nearest-neighbour tiles, no static LDS on top: 16 x 24 A_sel + (2 K A_sel rounded up to 8) bytes
    within 160 KiB -- 422 selected atoms at K = 2, 320 at K = 64; one atom more is refused"""
    import firecode_amd as fc

    limit = 160 * 1024
    need = lambda a: 16 * 24 * a + ((2 * K * a + 7) // 8) * 8  # noqa: E731
    A = {2: 422, 64: 320}[K]
    assert need(A) <= limit < need(A + 1) and S.medoid_max_selected(K) == A
    assert S.medoid_lds_bytes(K, A) == need(A) and S.medoid_lds_bytes(K, A + 1) == need(A + 1)
    make = lambda a: sr.path_table(a) if K == 2 else sr.transposition_table(a, 6)  # noqa: E731
    for rc, msg in _c_calls(make(A), A):
        assert rc == _lib.FC_E_INVALID and "NULL" in msg  # (admitted: the next check speaks)
    for rc, msg in _c_calls(make(A + 1), A + 1, mirror=2):  # (the LDS limit belongs to the table: before the flag)
        assert rc == _lib.FC_E_LIMIT and "LDS" in msg
    S.medoid_lds_check(K, A)
    with pytest.raises(fc.FirecodeHipInputError, match="LDS") as err:
        S.medoid_lds_check(K, A + 1)
    assert err.value.code == _lib.FC_E_LIMIT
    X, atoms = np.zeros((2, A + 1, 3)), np.array(["C"] * (A + 1))
    for call in _python_calls(X, atoms, symmetry=make(A + 1)):
        with pytest.raises(fc.FirecodeHipInputError, match="LDS") as err:
            call()
        assert err.value.code == _lib.FC_E_LIMIT
    with pytest.raises(fc.FirecodeHipInputError, match="LDS"):
        fc.pruner.silhouette_scan_sym(X, atoms, [0.5], symmetry=make(A + 1))


def test_empty_ensembles_need_no_device():
    import firecode_amd as fc

    A = 6
    atoms, t = np.array(["C"] * A), sr.path_table(A)
    none = np.zeros((0, A, 3))
    for kw in (dict(symmetry=t), dict(prune_enantiomers=True), dict(symmetry=t, prune_enantiomers=True)):
        m = fc.pruner.medoids_by_rmsd_sym(none, atoms, **kw)
        assert isinstance(m, fc.pruner.RmsdMedoids) and m.medoids.tolist() == [-1] and m.sums.shape == (0,)
        k = fc.pruner.kmedoids_by_rmsd_sym(none, atoms, 3, **kw)
        assert isinstance(k, fc.pruner.RmsdKMedoids) and k.medoids.shape == (0,) and k.cost == 0.0 and k.n_iter == 0
        s = fc.pruner.silhouette_by_rmsd_sym(none, atoms, None, **kw)
        assert isinstance(s, fc.pruner.RmsdSilhouette) and s.values.shape == (0,) and np.isnan(s.score)
        if len(kw) == 1:
            recs = fc.pruner.silhouette_scan_sym(none, atoms, [0.3, 0.5], **kw)
            assert [r.max_rmsd for r in recs] == [0.3, 0.5] and all(np.isnan(r.score) for r in recs)
        # ... and excuse nothing
        with pytest.raises(fc.FirecodeHipInputError, match="closed under inverse"):
            fc.pruner.medoids_by_rmsd_sym(none, atoms, symmetry=np.stack([np.arange(A), np.roll(np.arange(A), 1)]))


def test_a_graph_is_perceived():
    import networkx as nx

    import firecode_amd as fc

    atoms = np.array(["C"] * 6)
    g = nx.path_graph(6)
    assert fc.pruner.medoids_by_rmsd_sym(np.zeros((0, 6, 3)), atoms, symmetry=g).medoids.tolist() == [-1]
    with pytest.raises(fc.FirecodeHipInputError, match="element symbols"):
        _handle_less_ensemble(3, 6).medoids_sym(symmetry=g)


def test_no_cpu_fallback_for_the_new_calls():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import firecode_amd as fc

    X, atoms = syn.continuous_ensemble(5, 6, seed=1), np.array(["C"] * 6)
    for kw in ({"symmetry": sr.path_table(6)}, {"prune_enantiomers": True}):
        for call in (lambda: fc.pruner.medoids_by_rmsd_sym(X, atoms, **kw), lambda: fc.pruner.kmedoids_by_rmsd_sym(X, atoms, 2, **kw),
                     lambda: fc.pruner.silhouette_by_rmsd_sym(X, atoms, np.arange(5) % 2, **kw),
                     lambda: fc.pruner.silhouette_scan_sym(X, atoms, [0.5], **kw)):
            with pytest.raises(fc.FirecodeHipDeviceError):
                call()
