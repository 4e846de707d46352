"""Symmetry- and mirror-aware nearest neighbours under the RMSD on the GPU (fc_ensemble_knn_perm,
fc_ensemble_knn_cross_perm and the Python layers above them) against the NumPy restatement of d_sym (tests/knn_sym_ref.py)
on the oracle's Kabsch RMSD.

Bars, those of test_gpu_knn.py and test_gpu_knn_cross.py: indices identical (-1 padding included), distances within 1e-10
(+inf where padded) -- on cases whose every decision the restatement recorded with a gap above 1e-9 (consecutive sorted
distances of a row among positions 1 ... k + 1; with a cap, every pair's distance to the cap), asserted first, so that
rounding cannot flip one.  The ensembles are those of tests/diverse_sym_ref.py: a random half relabelled by a row of
the table, a random half reflected where the flag is tested.

FC_KNN_STRIPS and FC_KNN_FILTER are read at every call, so the launch-shape tests switch them in this process, as
test_gpu_knn.py and test_gpu_knn_cross.py do."""

import numpy as np
import pytest

import diverse_sym_ref as ds
import enant_ref as er
import knn_cross_ref as xr
import knn_ref
import knn_sym_ref as ks
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9

# (kind, N, A, table, mirror)
SELF_CASES = [
    ("clusters", 5, 3, "blocks", True),
    ("continuous", 33, 5, "path", False),
    ("clusters", 65, 7, "path", True),
    ("continuous", 130, 20, "path", True),
    ("clusters", 100, 13, "blocks", True),
    ("continuous", 70, 50, "blocks", False),
    ("clusters", 40, 80, "swaps64", False),
    ("continuous", 24, 20, "swaps64", True),
]
# (kind, Nq, Nr, A, table, mirror)
CROSS_CASES = [
    ("continuous", 65, 257, 7, "path", False),
    ("clusters", 257, 65, 13, "blocks", True),
    ("continuous", 16, 300, 50, "blocks", True),
    ("clusters", 5, 70, 20, "swaps64", False),
]
NOVEL_AT_THE_TIGHT_CAP = {("continuous", 65, 257, 7, "path", False): 12, ("clusters", 257, 65, 13, "blocks", True): 69}

_CASES = {}  # made once and shared, never written to


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _self_case(kind, N, A, table, mirror):
    key = ("self", kind, N, A, table, mirror)
    if key not in _CASES:
        X, atoms, t, _ = ds.ensemble(kind, N, A, table, mirror)
        D = ks.self_rows(ks.prepared(X, atoms), t, mirror)
        _CASES[key] = _frozen(X, atoms, np.ascontiguousarray(t), D)
    return _CASES[key]


def _cross_case(kind, Nq, Nr, A, table, mirror):
    key = ("cross", kind, Nq, Nr, A, table, mirror)
    if key not in _CASES:
        X, atoms, t, _ = ds.ensemble(kind, Nq + Nr, A, table, mirror)
        p = np.random.default_rng(9).permutation(Nq + Nr)
        Q, R = np.ascontiguousarray(X[p[:Nq]]), np.ascontiguousarray(X[p[Nq:]])
        D = ks.distance_rows(ks.prepared(Q, atoms), ks.prepared(R, atoms), t, mirror)
        _CASES[key] = _frozen(Q, R, atoms, np.ascontiguousarray(t), D)
    return _CASES[key]


def _swapped_rows(case):
    """the rows of the references against the queries (the coverage's direction), made once"""
    key = ("swapped",) + case
    if key not in _CASES:
        Q, R, atoms, t, _ = _cross_case(*case)
        _CASES[key] = _frozen(ks.distance_rows(ks.prepared(R, atoms), ks.prepared(Q, atoms), t, case[-1]))[0]
    return _CASES[key]


def _middle_cap(D):
    """the midpoint of the two middle values of all sorted pair distances: about half of the pairs are within it"""
    v = np.sort(D.reshape(-1))
    m = (len(v) - 1) // 2
    return 0.5 * (v[m] + v[m + 1])


def _tight_cap(D):
    """between two of the smallest pair distances (the 2 % quantile): most lists end in padding"""
    v = np.sort(D.reshape(-1))
    m = len(v) // 50
    return 0.5 * (v[m] + v[m + 1])


def _check(got, ref, rows, k, what=""):
    idx, dist = got
    assert ref.min_gap > GAP, f"the case has a near-tie ({ref.min_gap:.3g}): choose another"
    assert idx.dtype == np.int32 and idx.shape == (rows, k) and dist.dtype == np.float64 and dist.shape == (rows, k)
    assert np.array_equal(idx, ref.indices)
    pad = ref.indices < 0
    assert np.all(np.isposinf(dist[pad])) and np.all(np.isfinite(dist[~pad]))
    err = np.abs(dist[~pad] - ref.distances[~pad]).max(initial=0.0)
    print(f"{what} rows={rows} k={k} gap={ref.min_gap:.3g} padded={int(pad.sum())} max|d - ref|={err:.3g}")
    assert err < TOL


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # indices, and the distances bit for bit


# ---- parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: "-".join(map(str, c)))
def test_knn_sym_parity(fc, case, k):
    """3 atoms and a list longer than the ensemble, N that is no multiple of the wavefront or the row tile, more than one
    tile and chunk, K = 2, 6 and 64, with and without the flag"""
    X, atoms, t, D = _self_case(*case)
    nb = fc.pruner.knn_by_rmsd(X, atoms, k, symmetry=t, prune_enantiomers=case[-1])
    _check((nb.indices, nb.distances), ks.knn_from_rows(D, k), len(X), k, str(case))


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("case", CROSS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_knn_cross_sym_parity(fc, case, k):
    Q, R, atoms, t, D = _cross_case(*case)
    nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, symmetry=t, prune_enantiomers=case[-1])
    _check((nb.indices, nb.distances), ks.knn_cross_from_rows(D, k), len(Q), k, str(case))


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("case", CROSS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_knn_cross_sym_cap(fc, case, tight, k):
    """the cap at the middle of all pair distances and among the smallest: the capped lists against the restatement, and
    as the uncapped device lists with the entries d >= max_rmsd replaced by -1 / +inf; novelty against the restatement"""
    Q, R, atoms, t, D = _cross_case(*case)
    kw = dict(symmetry=t, prune_enantiomers=case[-1])
    cap = _tight_cap(D) if tight else _middle_cap(D)
    assert np.abs(D - cap).min() > GAP
    ref = ks.knn_cross_from_rows(D, k, cap)
    nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap, **kw)
    _check((nb.indices, nb.distances), ref, len(Q), k, f"{case} cap={cap:.4f}")
    plain = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, **kw)
    far = plain.distances >= cap
    assert np.array_equal(nb.indices, np.where(far, -1, plain.indices))
    assert np.array_equal(nb.distances, np.where(far, np.inf, plain.distances))
    novel = ks.novel(D, cap)
    assert np.array_equal(nb.novel(cap), novel)
    if tight and case in NOVEL_AT_THE_TIGHT_CAP:  # empty rows beside filled ones
        assert int(novel.sum()) == NOVEL_AT_THE_TIGHT_CAP[case] and (ref.indices[:, 0] < 0).any() and (ref.indices >= 0).any()
    if k == 1:
        got = fc.pruner.novel_conformers(Q, R, atoms, cap, **kw)
        assert got.dtype == np.bool_ and np.array_equal(got, novel)


@pytest.mark.parametrize("case", CROSS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_coverage_under_d_sym(fc, case):
    """ensemble_coverage (the references are the rows) and its mean distance against the restatement, at the middle cap
    and at 0.5 A"""
    Q, R, atoms, t, _ = _cross_case(*case)
    Dsw = _swapped_rows(case)
    kw = dict(symmetry=t, prune_enantiomers=case[-1])
    for cap in (_middle_cap(Dsw), 0.5):
        assert ks.knn_cross_from_rows(Dsw, 1, cap).min_gap > GAP
        cov = fc.pruner.ensemble_coverage(Q, R, atoms, cap, **kw)
        covered, fraction, nearest, dist = ks.coverage(Dsw, cap)
        assert np.array_equal(cov.covered, covered) and cov.fraction == fraction
        assert cov.nearest.dtype == np.int32 and np.array_equal(cov.nearest, nearest)
        assert np.abs(cov.distances - dist).max() < TOL
        assert abs(cov.mean_distance() - ks.mean_distance(dist)) < TOL
    if case == ("clusters", 257, 65, 13, "blocks", True):  # the figure the default distance under-reports
        plain = fc.pruner.ensemble_coverage(Q, R, atoms, 0.5)
        print(f"coverage at 0.5 A: d_sym {cov.fraction:.3f}, default {plain.fraction:.3f}")
        assert cov.fraction == 1.0 and plain.fraction < 1.0 and cov.mean_distance() < plain.mean_distance()


# ---- copies --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True])
def test_copies_are_first_neighbours(fc, mirror):
    """exact relabelled copies and, with the flag, reflected copies appended to an ensemble: each is its original's
    first neighbour (and the original the copy's), at ~1e-15 -- in the self form and across two sets"""
    N, A = 37, 13
    X, atoms, t = syn.continuous_ensemble(N, A, seed=12), np.array(["C"] * A), ds.table("blocks", A)
    rows = np.random.default_rng(5).integers(1, len(t), size=N)
    Y = np.stack([X[n][t[rows[n]]] for n in range(N)])
    if mirror:
        Y = er.reflect(Y, np.arange(N), axis=1)
    both = np.concatenate([X, Y])
    nb = fc.pruner.knn_by_rmsd(both, atoms, 2, symmetry=t, prune_enantiomers=mirror)
    assert np.array_equal(nb.indices[:, 0], np.concatenate([np.arange(N) + N, np.arange(N)]))
    assert np.all(nb.distances[:, 0] >= 0.0) and np.all(nb.distances[:, 0] < TOL) and nb.distances[:, 1].min() > 1e-3
    cross = fc.pruner.knn_by_rmsd_against(Y, X, atoms, 1, symmetry=t, prune_enantiomers=mirror)
    assert np.array_equal(cross.indices[:, 0], np.arange(N)) and np.all(cross.distances < TOL)
    assert not fc.pruner.novel_conformers(Y, X, atoms, 1e-6, symmetry=t, prune_enantiomers=mirror).any()
    # without the table (and the flag) they are new
    assert fc.pruner.novel_conformers(Y, X, atoms, 1e-6).all()
    if mirror:
        assert fc.pruner.novel_conformers(Y, X, atoms, 1e-6, symmetry=t).all()
        # the flag alone undoes the reflection, not the relabelling: the reflected ensemble itself is not new
        Z = er.reflect(X, np.arange(N), axis=2)
        assert not fc.pruner.novel_conformers(Z, X, atoms, 1e-6, prune_enantiomers=True).any()
        assert fc.pruner.novel_conformers(Z, X, atoms, 1e-6).all()


def test_cross_form_shares_the_arithmetic_of_the_self_form(fc):
    """an ensemble against a bitwise copy of itself: every row lists itself first, at ~1e-15, and then the neighbours of
    the self form with the same distance bits -- through two handles and through one"""
    case = ("continuous", 130, 20, "path", True)
    X, atoms, t, _ = _self_case(*case)
    kw = dict(symmetry=t, prune_enantiomers=True)
    own = fc.pruner.knn_by_rmsd(X, atoms, 8, **kw)
    mask = np.ones(20, dtype=bool)
    with fc.DeviceEnsemble(X, atom_mask=mask, center=True) as q, fc.DeviceEnsemble(X.copy(), atom_mask=mask, center=True) as r:
        two = q.knn_against(r, 9, **kw)
        one = q.knn_against(q, 9, **kw)
    for idx, dist in (two, one):
        assert np.array_equal(idx[:, 0], np.arange(130)) and np.all(dist[:, 0] >= 0.0) and np.all(dist[:, 0] < TOL)
        assert np.array_equal(idx[:, 1:], own.indices)
        assert np.array_equal(dist[:, 1:], own.distances)  # the same bits
    assert own.distances.min() > 1e-3  # (no near-duplicate that could trade places with column 0)


def test_identity_table_without_the_flag_is_the_default(fc):
    """K = 1, mirror = 0: the default's entry points, bit for bit"""
    Q, R, atoms, _, _ = _cross_case(*CROSS_CASES[0])
    ident = np.arange(len(atoms))[None]
    for k in (1, 8):
        a, b = fc.pruner.knn_by_rmsd(R, atoms, k, symmetry=ident), fc.pruner.knn_by_rmsd(R, atoms, k)
        assert _same(a, b)
        for cap in (None, 1.0):
            a = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap, symmetry=ident)
            assert _same(a, fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap))


# ---- determinism -----------------------------------------------------------------------------------------------------------
_SHAPES = (("1", None), ("3", None), ("7", None), (None, None), (None, "0"), ("3", "0"))


def _under(monkeypatch, strips, flt):
    for name, value in (("FC_KNN_STRIPS", strips), ("FC_KNN_FILTER", flt)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


@pytest.mark.parametrize("capped", [False, True])
@pytest.mark.parametrize("case", [CROSS_CASES[2], CROSS_CASES[1]], ids=lambda c: "-".join(map(str, c)))
def test_cross_form_independent_of_the_launch_shape(fc, monkeypatch, case, capped):
    """the same bits for every strip count and with the explicit pass for every (pair, p, h)"""
    Q, R, atoms, t, D = _cross_case(*case)
    k, cap = 8, (_middle_cap(D) if capped else None)
    runs = []
    for strips, flt in _SHAPES:
        _under(monkeypatch, strips, flt)
        runs.append(fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=cap, symmetry=t, prune_enantiomers=case[-1]))
    for nb in runs[1:]:
        assert _same(nb, runs[0])
    _check((runs[0].indices, runs[0].distances), ks.knn_cross_from_rows(D, k, cap), len(Q), k, f"{case} capped={capped}")


@pytest.mark.parametrize("k", [1, 8])
def test_self_form_independent_of_the_launch_shape(fc, monkeypatch, k):
    case = ("continuous", 130, 20, "path", True)
    X, atoms, t, D = _self_case(*case)
    runs = []
    for strips, flt in _SHAPES:
        _under(monkeypatch, strips, flt)
        runs.append(fc.pruner.knn_by_rmsd(X, atoms, k, symmetry=t, prune_enantiomers=True))
    for nb in runs[1:]:
        assert _same(nb, runs[0])
    _check((runs[0].indices, runs[0].distances), ks.knn_from_rows(D, k), len(X), k, str(case))


# ---- limits, perception, layers ----------------------------------------------------------------------------------------------
def test_largest_atom_count_of_64_permutations(fc):
    """320 selected atoms with K = 64: rows and table fill the 160 KiB of LDS exactly"""
    A = S.knn_max_selected(64)
    assert A == 320 and S.knn_lds_bytes(64, A) == 160 * 1024
    case = ("continuous", 20, 70, A, "swaps64", False)
    Q, R, atoms, t, D = _cross_case(*case)
    assert t.shape == (64, A)
    nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, 8, symmetry=t)
    _check((nb.indices, nb.distances), ks.knn_cross_from_rows(D, 8), 20, 8, str(case))
    with pytest.raises(fc.FirecodeHipInputError, match="LDS"):
        fc.pruner.knn_by_rmsd_against(np.zeros((2, A + 1, 3)), np.zeros((2, A + 1, 3)), ["C"] * (A + 1), 1,
                                      symmetry=ds.table("swaps64", A + 1))


@pytest.mark.parametrize("heavy_atoms_only", [True, False])
def test_perceived_graph_and_the_three_layers(fc, heavy_atoms_only):
    """a chain of 7 carbons with three hydrogens: the graph as symmetry= is its perceived table; DeviceEnsemble, pruner
    and Ensemble give the same lists, in the self form and across two sets"""
    import networkx as nx

    from firecode_amd.ensemble import Ensemble

    atoms = np.array(["C"] * 7 + ["H"] * 3)
    g = nx.path_graph(7)
    g.add_edges_from([(0, 7), (6, 8), (3, 9)])
    table = S.graph_automorphisms(g, atoms, heavy_atoms_only)
    assert table.shape == (2, 10) and np.array_equal(table[1, :7], np.arange(7)[::-1])
    assert np.array_equal(table[1, 7:], [7, 8, 9] if heavy_atoms_only else [8, 7, 9])
    N, Nq, k = 60, 21, 5
    X0 = syn.continuous_ensemble(N, 10, seed=31)
    flip = np.random.default_rng(2).random(N) < 0.5
    X = np.where(flip[:, None, None], X0[:, table[1]], X0)
    X = er.reflect(X, np.random.default_rng(3).random(N) < 0.5)
    mask = atoms != "H" if heavy_atoms_only else np.ones(10, dtype=bool)
    tsel = S.selected_table(table, mask)
    Xsel = ks.prepared(X, atoms, heavy_atoms_only)
    assert Xsel.shape[1] == (7 if heavy_atoms_only else 10) == tsel.shape[1]
    kw = dict(heavy_atoms_only=heavy_atoms_only, prune_enantiomers=True)
    # the self form
    nb = fc.pruner.knn_by_rmsd(X, atoms, k, symmetry=g, **kw)
    _check((nb.indices, nb.distances), ks.knn_from_rows(ks.self_rows(Xsel, tsel, True), k), N, k, f"heavy={heavy_atoms_only}")
    assert _same(nb, fc.pruner.knn_by_rmsd(X, atoms, k, symmetry=table, **kw))
    assert _same(nb, Ensemble(atoms=atoms, coords=X.copy(), logfunction=None).nearest_neighbours(k, symmetry=g, **kw))
    # across two sets
    Q, R = X[:Nq], X[Nq:]
    D = ks.distance_rows(Xsel[:Nq], Xsel[Nq:], tsel, True)
    cap = _tight_cap(D)
    a, b = Ensemble(atoms=atoms, coords=Q.copy(), logfunction=None), Ensemble(atoms=atoms, coords=R.copy(), logfunction=None)
    with fc.DeviceEnsemble(X, atom_mask=mask, center=True) as ens, fc.DeviceEnsemble(Q, atom_mask=mask, center=True) as q, \
            fc.DeviceEnsemble(R, atom_mask=mask, center=True) as r:
        assert _same(nb, ens.knn(k, symmetry=table, prune_enantiomers=True))
        dev_ms, host_ms, strips, (formed, explicit) = ens.bench_knn(k, reps=2, symmetry=table, prune_enantiomers=True)
        assert dev_ms > 0.0 and host_ms > 0.0 and strips >= 1 and formed == N * (N - 1) * 4 and 0 < explicit <= formed
        for max_rmsd in (None, cap):
            xb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k, max_rmsd=max_rmsd, symmetry=g, **kw)
            _check((xb.indices, xb.distances), ks.knn_cross_from_rows(D, k, max_rmsd), Nq, k, f"heavy={heavy_atoms_only}")
            assert _same(xb, q.knn_against(r, k, max_rmsd=max_rmsd, symmetry=table, prune_enantiomers=True))
            assert _same(xb, a.nearest_in(b, k=k, max_rmsd=max_rmsd, symmetry=table, **kw))
            stats = q.bench_knn_against(r, k, max_rmsd=max_rmsd, reps=1, symmetry=table, prune_enantiomers=True)
            assert stats[0] > 0.0 and stats[3][0] == Nq * (N - Nq) * 4 and 0 < stats[3][1] <= stats[3][0]
    novel = a.novel_against(b, cap, symmetry=g, **kw)
    assert np.array_equal(novel, ks.novel(D, cap)) and novel.any() and not novel.all()


def test_default_forms_are_untouched_by_the_aware_calls(fc):
    """after every symmetry-aware call on two handles, the default lists of the same handles still match their references"""
    case = ("clusters", 257, 65, 13, "blocks", True)
    Q, R, atoms, t, D = _cross_case(*case)
    Qsel, Rsel = ks.prepared(Q, atoms), ks.prepared(R, atoms)
    k = 8
    ref_self = knn_ref.knn(Rsel, k)
    ref_cross = xr.knn(Qsel, Rsel, k)
    ref_sym_self = ks.knn_from_rows(ks.self_rows(Rsel, t, True), k)
    mask = np.ones(len(atoms), dtype=bool)
    with fc.DeviceEnsemble(Q, atom_mask=mask, center=True) as q, fc.DeviceEnsemble(R, atom_mask=mask, center=True) as r:
        def defaults():
            _check(r.knn(k), ref_self, len(R), k, "default self")
            _check(q.knn_against(r, k), ref_cross, len(Q), k, "default cross")

        defaults()
        _check(r.knn(k, symmetry=t, prune_enantiomers=True), ref_sym_self, len(R), k, "aware self")
        defaults()
        _check(q.knn_against(r, k, symmetry=t, prune_enantiomers=True), ks.knn_cross_from_rows(D, k), len(Q), k, "aware cross")
        defaults()
        cap = _middle_cap(D)
        _check(q.knn_against(r, k, max_rmsd=cap, symmetry=t, prune_enantiomers=True), ks.knn_cross_from_rows(D, k, cap), len(Q),
               k, "aware cross, capped")
        defaults()
        # a refusal in between leaves both usable as well
        with pytest.raises(fc.FirecodeHipError):
            q.knn_against(r, 65, symmetry=t)
        with pytest.raises(fc.FirecodeHipInputError):
            q.knn_against(r, 2, max_rmsd=-1.0, prune_enantiomers=True)
        defaults()
        only_table = r.knn(k, symmetry=t)
        only_flag = r.knn(k, prune_enantiomers=True)
        assert np.all(only_table[1] >= r.knn(k, symmetry=t, prune_enantiomers=True)[1] - TOL)
        assert np.all(only_flag[1] <= r.knn(k)[1] + TOL)
        defaults()
