"""Density-based RMSD clusters on the GPU (fc_rmsd_dbscan, fc_rmsd_dbscan_enant, fc_rmsd_dbscan_perm,
fc_dbscan_from_pairs, fc_dbscan_from_bits and the Python layers above them) against the NumPy / SciPy restatement
(tests/dbscan_ref.py).

No tolerance anywhere: labels, representatives, sizes, core flags, degrees and counts are integers and must match
exactly.  Every RMSD ensemble asserts ``min_gap > 1e-9`` from the restatement first, so no pair is ever exempted."""

import functools
import re

import numpy as np
import pytest

import cluster_ref as cr
import dbscan_ref as dr
import enant_ref as er
import symm_ref as sr
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

GAP = 1e-9
THR = 0.5


def _assert_same(got, ref, label=""):
    assert got.labels.dtype == np.int32 and got.representatives.dtype == np.int64 and got.sizes.dtype == np.int64, label
    assert got.core.dtype == np.bool_ and got.degrees.dtype == np.int32, label
    assert np.array_equal(got.degrees, ref.degrees), label
    assert np.array_equal(got.core, ref.core), label
    assert np.array_equal(got.sizes, ref.sizes), label
    assert np.array_equal(got.representatives, ref.representatives), label
    assert np.array_equal(got.labels, ref.labels), label


def _assert_same_clusters(got, ref, label=""):
    for a, b in zip(got[:3], ref[:3]):
        assert np.array_equal(a, b), label


# ---- graph cases ---------------------------------------------------------------------------------------------------------
def _distinct_edges(n, m, seed):
    rng = np.random.default_rng(seed)
    ei, ej = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keep = ei != ej
    lo, hi = np.unique(np.stack([np.minimum(ei, ej)[keep], np.maximum(ei, ej)[keep]]), axis=1)
    perm = rng.permutation(len(lo))
    swap = rng.random(len(lo)) < 0.5
    return np.where(swap, hi, lo)[perm], np.where(swap, lo, hi)[perm]


@functools.lru_cache(maxsize=None)
def _graph(name):
    """-> (n, ei, ej, the values of min_samples): the graphs of the issue by name, every unordered pair once"""
    rng = np.random.default_rng(3)
    none = np.zeros(0, np.int64)
    if name == "single":
        return 1, none, none, (1, 2)
    if name == "no_edge":
        return 5, none, none, (1, 2)
    if name == "path_70000":  # a path under a random relabelling, the list shuffled
        n = 70000
        relabel = rng.permutation(n)
        perm = rng.permutation(n - 1)
        return n, relabel[:-1][perm], relabel[1:][perm], (1, 3, 4)
    if name == "star_centre_last":  # the hub's atomic path: 4 096 adds to one degree word, 4 096 leaves attached to one core
        n = 4097
        return n, np.full(n - 1, n - 1), rng.permutation(n - 1), (1, 2, 3)
    if name == "star_centre_first":
        n = 4097
        return n, 1 + rng.permutation(n - 1), np.zeros(n - 1, np.int64), (1, 2, 3)
    if name == "complete_300":
        iu, ju = np.triu_indices(300, 1)
        return 300, iu, ju, (1, 300, 301)
    if name == "random_100000":
        return (100000,) + _distinct_edges(100000, 150000, 11) + ((1, 4),)
    if name.startswith("edge_"):  # word and workgroup edges of the degree, flag and numbering passes
        n = int(name.split("_")[1])
        return (n,) + _distinct_edges(n, 2 * n, n) + ((1, 2, 4, 6),)
    raise KeyError(name)


GRAPHS = ["single", "no_edge", "path_70000", "star_centre_last", "star_centre_first", "complete_300", "random_100000",
          "edge_63", "edge_64", "edge_65", "edge_1023", "edge_1024", "edge_1025"]


@pytest.mark.parametrize("name", GRAPHS)
def test_graph_cases(fc, name):
    n, ei, ej, ms = _graph(name)
    pairs = cr.pack_pairs(ei, ej)
    with_bits = n <= 5000
    if with_bits:
        bits = cr.pack_bits(n, ei, ej)
        W = bits.shape[1]
        low = np.zeros((n, W * 64), dtype=bool)  # bits at and below the diagonal are not read: set them all
        low[:, :n] = np.tril(np.ones((n, n), dtype=bool))
        noisy = bits | np.packbits(low.reshape(n, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, W)
    for m in ms:
        ref = dr.dbscan(n, ei, ej, m)
        label = (name, m)
        if name == "path_70000" and m == 3:
            assert ref.sizes.tolist() == [n] and int(ref.core.sum()) == n - 2 and ref.degrees[~ref.core].tolist() == [1, 1]
        if name == "path_70000" and m == 4 or name == "complete_300" and m == 301:
            assert len(ref.sizes) == 0 and (ref.labels == -1).all()
        if name.startswith("star") and m == 3:
            centre = 0 if name.endswith("first") else n - 1
            assert np.flatnonzero(ref.core).tolist() == [centre] and ref.sizes.tolist() == [n] and ref.degrees[centre] == n - 1
            assert ref.representatives.tolist() == [centre]
        if name.startswith("star") and m == 2 or name == "complete_300" and m == 300:
            assert ref.sizes.tolist() == [n] and ref.core.all()
        _assert_same(fc.pruner.dbscan_from_pairs(pairs, n, m, assume_unique=True), ref, label)
        _assert_same(fc.pruner.dbscan_from_pairs(np.stack([ej, ei], axis=1).reshape(-1, 2), n, m), ref, label)  # (P, 2), swapped
        if with_bits:
            _assert_same(fc.pruner.dbscan_from_bits(bits, n, m), ref, label)
            _assert_same(fc.pruner.dbscan_from_bits(noisy, n, m), ref, label)
        if m == 1:  # the components, exactly
            _assert_same_clusters(ref, fc.pruner.clusters_from_pairs(pairs, n), label)
            if with_bits:
                _assert_same_clusters(ref, fc.pruner.clusters_from_bits(bits, n), label)


def test_graph_result_is_a_function_of_the_graph(fc):
    """one graph as five differently shuffled lists with swapped ends: identical output; with duplicates appended, the
    wrapper removes them, and assume_unique=True counts them"""
    n, ei, ej, _ = _graph("random_100000")
    ref = dr.dbscan(n, ei, ej, 4)
    assert 0 < len(ref.sizes) and 0 < (ref.labels < 0).sum() and (~ref.core & (ref.labels >= 0)).any()
    rng = np.random.default_rng(1)
    for _ in range(5):
        perm = rng.permutation(len(ei))
        swap = rng.random(len(ei)) < 0.5
        a, b = np.where(swap, ej, ei)[perm], np.where(swap, ei, ej)[perm]
        _assert_same(fc.pruner.dbscan_from_pairs(cr.pack_pairs(a, b), n, 4, assume_unique=True), ref)
    dup = cr.pack_pairs(np.r_[a, b[:999]], np.r_[b, a[:999]])
    _assert_same(fc.pruner.dbscan_from_pairs(dup, n, 4), ref)
    _assert_same(fc.pruner.dbscan_from_pairs(dup, n, 4, assume_unique=True), dr.dbscan_from_pairs(dup, n, 4, unique=False))


def test_long_list_is_hooked_in_phases(fc):
    """more entries than the short-list bound (2^16), so the seed / coarse / fine launches all act and the borders are
    attached by the seed launch: 3 000 vertices, 120 000 distinct edges"""
    n = 3000
    ei, ej = _distinct_edges(n, 125000, 21)
    assert len(ei) > 1 << 16
    deg = np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)
    m = int(np.sort(deg)[n // 2]) + 1  # about half of the vertices are core
    ref = dr.dbscan(n, ei, ej, m)
    assert 0.3 * n < ref.core.sum() < 0.7 * n and (~ref.core & (ref.labels >= 0)).any()
    _assert_same(fc.pruner.dbscan_from_pairs(cr.pack_pairs(ei, ej), n, m, assume_unique=True), ref)
    _assert_same(fc.pruner.dbscan_from_bits(cr.pack_bits(n, ei, ej), n, m), ref)


def test_tie_graph_follows_the_smaller_index(fc):
    """two 4-cliques of core vertices and one vertex adjacent to one core of each: it joins the cluster of its
    smaller-index core neighbour, under both relabellings"""
    k4 = [(a, b) for q in (0, 4) for a in range(q, q + 4) for b in range(a + 1, q + 4)]
    for relabel in (np.arange(9), np.array([4, 5, 6, 7, 0, 1, 2, 3, 8]), np.arange(9)[::-1].copy()):
        e = np.array(k4 + [(8, 3), (8, 4)])
        ei, ej = relabel[e[:, 0]], relabel[e[:, 1]]
        ref = dr.dbscan(9, ei, ej, 4)
        v, a, b = relabel[8], relabel[3], relabel[4]
        assert not ref.core[v] and ref.core[a] and ref.core[b] and ref.labels[a] != ref.labels[b]
        assert ref.labels[v] == ref.labels[min(a, b)] and sorted(ref.sizes.tolist()) == [4, 5]
        _assert_same(fc.pruner.dbscan_from_pairs(cr.pack_pairs(ei, ej), 9, 4), ref, relabel)
        _assert_same(fc.pruner.dbscan_from_bits(cr.pack_bits(9, ei, ej), 9, 4), ref, relabel)


def test_empty_graph_calls(fc):
    for got in (fc.pruner.dbscan_from_pairs(np.zeros(0, np.uint64), 0, 2), fc.pruner.dbscan_from_bits(np.zeros((0, 0), np.uint64), 0, 2)):
        assert all(arr.shape == (0,) for arr in got)


# ---- RMSD cases ----------------------------------------------------------------------------------------------------------
def _identical(n, A, seed):
    rng = np.random.default_rng(seed)
    base = syn.synthetic_ensemble(1, A, seed=2)[0][0]
    X = np.stack([base @ syn.random_rotation(rng).T + rng.normal(scale=5.0, size=3) for _ in range(n)])
    return np.ascontiguousarray(X), np.array(["C"] * A)


@functools.lru_cache(maxsize=None)
def _ensemble(name):
    """-> (X, atoms, extra) by name; extra: cluster assignment / path positions / None"""
    kind, *args = name.split(":")
    if kind == "clustered":
        return syn.synthetic_ensemble(int(args[0]), int(args[1]), seed=int(args[2]))
    if kind == "reflected":
        X, atoms, assign = syn.synthetic_ensemble(333, 30, seed=4)
        return er.reflect(X, np.random.default_rng(0).random(333) < 0.5), atoms, assign
    if kind == "continuous":
        return syn.continuous_ensemble(300, 30), np.array(["C"] * 30), None
    if kind == "identical":
        return _identical(200, 20, 9) + (None,)
    if kind == "path":
        return cr.path_ensemble(1100, 20, cuts=(400, 401, 900))
    if kind == "dumbbell":
        return dr.line_ensemble(dr.DUMBBELL_T) + (None,)
    if kind == "tie":
        return dr.line_ensemble(dr.TIE_T) + (None,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _similarity(name, enant=False):
    """the restatement's similarity matrix of a named ensemble, computed once -> S (gap asserted)"""
    X, atoms, _ = _ensemble(name)
    if enant or name == "reflected":
        mats = er.similarity(X, atoms, THR)
        assert mats.min_gap > GAP, f"{name}: a decisive value within {mats.min_gap:.3g} of its threshold"
        return mats.S if enant else mats.S_default
    S, gap = cr.default_similarity(X, atoms, THR)
    assert gap > GAP, f"{name}: a decisive value within {gap:.3g} of its threshold"
    return S


def _resident(fc, X, S, S_default, ms, enant=False, symmetry=None, expect_bits=0):
    """dbscan for every m on ONE resident handle, each against the restatement; then the default prune, simbits and
    clusters on the same handle against their oracles: nothing leaked -> {m: (RmsdDbscan, stats)}"""
    from firecode_amd import _lib

    n = len(X)
    out = {}
    with fc.DeviceEnsemble(X, center=True) as ens:
        for m in ms:
            *res, stats = ens.dbscan(THR, 2 * THR, m, prune_enantiomers=enant, symmetry=symmetry)
            out[m] = (fc.pruner.RmsdDbscan(*res), stats)
        mask, _ = ens.prune(THR, 2 * THR)
        bits, grey = ens.simbits(THR, 2 * THR)
        cl = ens.clusters(THR, 2 * THR)
        again = ens.dbscan(THR, 2 * THR, ms[-1], prune_enantiomers=enant, symmetry=symmetry)
    assert np.array_equal(mask, o.greedy_prune_from_matrix(S_default))
    assert np.array_equal(_lib.unpack_bits(bits, n), np.triu(S_default, 1)) and grey == 0
    _assert_same_clusters(cl, cr.clusters_from_matrix(S_default))
    for a, b in zip(again, tuple(out[ms[-1]][0]) + (out[ms[-1]][1],)):
        assert np.array_equal(a, b)
    for m in ms:
        got, stats = out[m]
        ref = dr.dbscan_from_matrix(S, m)
        _assert_same(got, ref, (m,))
        assert stats.tolist()[2:] == [int(np.triu(S, 1).sum()), 0, expect_bits, len(ref.sizes), int(ref.core.sum()),
                                      int((ref.labels < 0).sum())], (m, stats)
        assert int(stats[0]) == n * (n - 1) // 2
        if m == 1:
            _assert_same_clusters(got, cr.clusters_from_matrix(S), "m = 1")
    return out


def _check(fc, name, ms, enant=False, expect_bits=0):
    X, atoms, _ = _ensemble(name)
    S = _similarity(name, enant)
    out = _resident(fc, X, S, _similarity(name, False), ms, enant, expect_bits=expect_bits)
    got = fc.pruner.dbscan_by_rmsd(X, atoms, THR, min_samples=ms[-1], prune_enantiomers=enant)
    _assert_same(got, dr.dbscan_from_matrix(S, ms[-1]), name)
    if 1 in ms:  # m = 1 reproduces cluster_by_rmsd bit for bit
        _assert_same_clusters(out[1][0], fc.pruner.cluster_by_rmsd(X, atoms, THR, prune_enantiomers=enant), name)
    return {m: out[m][0] for m in ms}


def test_dumbbell_separates_where_the_components_weld(fc):
    name = "dumbbell"
    S = _similarity(name)
    assert int(np.triu(S, 1).sum()) == 934 and cr.clusters_from_matrix(S).sizes.tolist() == [65]
    got = _check(fc, name, (1, 4, 17, 31, 32, 33))
    assert got[1].sizes.tolist() == [65]
    for m in (4, 17, 31, 32):
        assert got[m].sizes.tolist() == [32, 32] and got[m].labels[30:35].tolist() == [0, 0, -1, 1, 1], m
        assert (got[m].labels[:30] == 0).all() and (got[m].labels[35:] == 1).all()
    assert np.flatnonzero(got[32].core).tolist() == [30, 34] and got[32].representatives.tolist() == [30, 34]
    assert int(got[31].core.sum()) == 62
    assert (got[33].labels == -1).all() and len(got[33].sizes) == 0 and not got[33].core.any()


def test_tie_joins_the_earlier_cluster(fc):
    name = "tie"
    X, atoms, _ = _ensemble(name)
    S = _similarity(name)
    got = _check(fc, name, (5,))[5]
    assert got.degrees.tolist() == [4, 4, 4, 4, 5, 2, 5, 4, 4, 4, 4] and not got.core[5] and got.core[[4, 6]].all()
    assert got.labels.tolist() == [0] * 6 + [1] * 5 and got.sizes.tolist() == [6, 5]
    rev = fc.pruner.dbscan_by_rmsd(np.ascontiguousarray(X[::-1]), atoms, THR, min_samples=5)
    _assert_same(rev, dr.dbscan_from_matrix(S[::-1, ::-1], 5))
    assert rev.labels.tolist() == [0] * 6 + [1] * 5       # reversed: the middle conformer again joins the earlier cluster
    energies = np.linspace(1.0, 0.0, 11)                    # energies that flip the order: it joins the other one
    flipped = fc.pruner.dbscan_by_rmsd(X, atoms, THR, min_samples=5, energies=energies, max_dE=100.0)
    _assert_same(flipped, dr.dbscan_from_matrix(S, 5, energies, 100.0))
    assert flipped.labels.tolist() == [1] * 5 + [0] * 6 and flipped.representatives.tolist() == [10, 4]


def test_path_ensemble(fc):
    got = _check(fc, "path", (1, 3))[3]
    k = _ensemble("path")[2]
    assert sorted(got.sizes.tolist()) == [199, 400, 498] and int((~got.core).sum()) == 6 and (got.labels >= 0).all()
    assert cr.same_partition(got.labels, np.digitize(k, [400, 900]))
    assert sorted(k[~got.core].tolist()) == [0, 399, 402, 899, 901, 1099]  # the ends of the three pieces are the borders


def test_continuous_both_paths(fc, monkeypatch):
    """no cluster structure: once from the pair list, once -- the candidate queue cut to four entries -- from the bit
    matrix.  Identical outputs, and the figures of the restatement."""
    ms = (1, 2, 3, 4, 5, 8)
    S = _similarity("continuous")
    assert int(np.triu(S, 1).sum()) == 729 and int(S.sum(axis=1).max()) == 26
    from_list = _check(fc, "continuous", ms)
    assert [len(from_list[m].sizes) for m in ms] == [62, 6, 1, 1, 2, 1]
    assert [int((from_list[m].labels < 0).sum()) for m in ms] == [0, 56, 66, 81, 95, 129]
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")
    from_bits = _check(fc, "continuous", ms, expect_bits=1)
    monkeypatch.delenv("FC_PAIRQ_CAP")
    for m in ms:
        _assert_same(from_bits[m], from_list[m], m)


@pytest.mark.parametrize("N,A,seed", [(1, 5, 1), (2, 5, 1), (65, 12, 3)])
def test_clustered(fc, N, A, seed):
    name = f"clustered:{N}:{A}:{seed}"
    got = _check(fc, name, (1, 5, 6) if N == 65 else (1, 2))
    if N == 65:
        assign = _ensemble(name)[2]
        assert cr.same_partition(got[5].labels, assign) and got[5].core.all() and (got[5].degrees == 4).all()
        assert (got[6].labels == -1).all() and len(got[6].sizes) == 0
    if N == 1:
        assert got[1].labels.tolist() == [0] and got[2].labels.tolist() == [-1] and got[2].degrees.tolist() == [0]


def test_identical_copies_dense(fc, monkeypatch):
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")
    got = _check(fc, "identical", (1, 200, 201), expect_bits=1)
    _check(fc, "identical", (200,), enant=True, expect_bits=1)
    monkeypatch.delenv("FC_PAIRQ_CAP")
    assert got[200].sizes.tolist() == [200] and (got[200].degrees == 199).all() and (got[201].labels == -1).all()
    _check(fc, "identical", (1, 200, 201))


def test_reflected_half(fc):
    """mirror images: the default form keeps the hands apart (no conformer reaches five), the enantiomer-aware form
    pairs them (every generator cluster of five is dense)"""
    default = _check(fc, "reflected", (1, 3, 5))
    enant = _check(fc, "reflected", (1, 3, 5), enant=True)
    assign = _ensemble("reflected")[2]
    inside = enant[5].labels >= 0
    assert inside.sum() >= 330 and cr.same_partition(enant[5].labels[inside], assign[inside])
    assert (default[5].labels < 0).sum() > (enant[5].labels < 0).sum()


def test_symmetry_table(fc):
    """K = 2 atom permutations (the reversal of a path), a random half of the conformers relabelled"""
    table = sr.path_table(9)
    X, atoms, assign = syn.synthetic_ensemble(150, 9, seed=1)
    Y, _ = sr.relabel_half(X, table, 1)
    mats = sr.similarity(Y, atoms, table, THR)
    assert mats.min_gap > GAP and len(table) == 2
    out = _resident(fc, Y, mats.S, mats.S_default, (1, 5, 6), symmetry=table)
    assert cr.same_partition(out[5][0].labels, assign) and (out[6][0].labels == -1).all()
    ref_default = dr.dbscan_from_matrix(mats.S_default, 5)
    assert (ref_default.labels < 0).sum() > 0                                   # without the table the clusters thin out
    lines = []
    got = fc.pruner.dbscan_by_rmsd(Y, atoms, THR, min_samples=5, symmetry=table, debugfunction=lines.append)
    _assert_same(got, dr.dbscan_from_matrix(mats.S, 5))
    assert lines[0].startswith("DEBUG: dbscan_by_rmsd [gfx950, 2 atom permutations] - 11175 pairs screened, ")
    _assert_same(fc.pruner.dbscan_by_rmsd(Y, atoms, THR, min_samples=5), ref_default)


def test_energies_window_and_order(fc):
    name = "clustered:60:12:5"
    X, atoms, assign = _ensemble(name)
    S = _similarity(name)
    rng = np.random.default_rng(2)
    # two members of every cluster of five lie 5 above the other three: the window (1.0) splits every cluster in two
    rank = np.zeros(60, dtype=np.int64)
    for c in np.unique(assign):
        members = np.flatnonzero(assign == c)
        rank[members] = rng.permutation(len(members))
    energies = rng.random(60) * 0.3 + np.where(rank >= 3, 5.0, 0.0)
    max_dE = 1.0
    dE = np.abs(energies[:, None] - energies[None, :])[np.triu_indices(60, 1)]
    assert np.abs(dE - max_dE).min() > GAP and len(np.unique(energies)) == 60
    ref = dr.dbscan_from_matrix(S, 3, energies, max_dE)
    assert len(ref.sizes) == len(np.unique(assign)) and set(ref.sizes.tolist()) == {3} and int((ref.labels < 0).sum()) == 24
    got = fc.pruner.dbscan_by_rmsd(X, atoms, THR, min_samples=3, energies=energies, max_dE=max_dE)
    _assert_same(got, ref)
    assert np.all(np.diff(energies[got.representatives]) > 0)  # cluster order follows energy
    for c, r in enumerate(got.representatives):              # the representative is the lowest-energy core member
        members = np.flatnonzero((got.labels == c) & got.core)
        assert r == members[np.argmin(energies[members])]
    # a window that cuts nothing: the partition of the plain call, ordered by energy
    wide = fc.pruner.dbscan_by_rmsd(X, atoms, THR, min_samples=5, energies=energies, max_dE=100.0)
    _assert_same(wide, dr.dbscan_from_matrix(S, 5, energies, 100.0))
    assert cr.same_partition(wide.labels, assign)
    # energies of the wrong length are not usable: index order, no window
    _assert_same(fc.pruner.dbscan_by_rmsd(X, atoms, THR, min_samples=5, energies=energies[:10], max_dE=max_dE),
                 dr.dbscan_from_matrix(S, 5))


def test_ensemble_method_and_debug_line(fc):
    name = "clustered:60:12:5"
    X, atoms, assign = _ensemble(name)
    S025, gap = cr.default_similarity(X, atoms, 0.25)  # Ensemble passes no threshold: the pruner's default
    assert gap > GAP
    energies = np.random.default_rng(4).random(60) * 0.5
    log = []
    ens = fc.ensemble.Ensemble(atoms, X.copy(), energies=energies.copy(), logfunction=log.append)
    got = ens.dbscan_by_rmsd(min_samples=4)
    ref = dr.dbscan_from_matrix(S025, 4, energies, 1.0)
    _assert_same(got, ref)
    assert len(ens.coords) == 60 and len(ens.energies) == 60  # not masked
    line = [ln for ln in log if "dbscan_by_rmsd" in ln]
    assert len(line) == 1
    m = re.fullmatch(r"DEBUG: dbscan_by_rmsd \[gfx950\] - (\d+) pairs screened, (\d+) similar, min_samples 4: (\d+) clusters, "
                     r"(\d+) core, (\d+) border, (\d+) noise, in \d+\.\d{3} s", line[0])
    assert m, line[0]
    n_core, n_noise = int(ref.core.sum()), int((ref.labels < 0).sum())
    assert [int(v) for v in m.groups()] == [60 * 59 // 2, int(np.triu(S025, 1).sum()), len(ref.sizes), n_core,
                                            60 - n_core - n_noise, n_noise]
    log.clear()
    quiet = fc.ensemble.Ensemble(atoms, X.copy(), logfunction=log.append)  # no energies: index order, no window
    _assert_same(quiet.dbscan_by_rmsd(max_rmsd=THR, verbose=False), dr.dbscan_from_matrix(_similarity(name), 5))
    assert log == []
    debug = []
    fc.pruner.dbscan_by_rmsd(X, atoms, THR, prune_enantiomers=True, debugfunction=debug.append)
    assert debug[0].startswith("DEBUG: dbscan_by_rmsd [gfx950, mirror images included] - ")
