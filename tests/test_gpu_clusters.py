"""RMSD similarity clusters on the GPU (fc_rmsd_clusters, fc_rmsd_clusters_enant, fc_clusters_from_pairs,
fc_clusters_from_bits and the Python layers above them) against the NumPy / SciPy restatement (tests/cluster_ref.py).

No tolerance anywhere: labels, representatives, sizes and counts are integers and must match exactly.  Every RMSD
ensemble asserts ``min_gap > 1e-9`` from the restatement first, so no pair is ever exempted."""

import functools
import re

import numpy as np
import pytest

import cluster_ref as cr
import enant_ref as er
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

GAP = 1e-9
THR = 0.5


def _assert_same(got, ref, label=""):
    assert got.labels.dtype == np.int32 and got.representatives.dtype == np.int64 and got.sizes.dtype == np.int64, label
    assert np.array_equal(got.sizes, ref.sizes), label
    assert np.array_equal(got.representatives, ref.representatives), label
    assert np.array_equal(got.labels, ref.labels), label


# ---- graph cases ---------------------------------------------------------------------------------------------------------
def _random_edges(n, m, seed):
    rng = np.random.default_rng(seed)
    ei, ej = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keep = ei != ej
    return ei[keep], ej[keep]


def _random_tree(lo, hi, rng):
    """a random recursive tree on the vertices lo .. hi-1, its edges shuffled"""
    v = np.arange(lo + 1, hi)
    parent = lo + (rng.random(len(v)) * (v - lo)).astype(np.int64)
    perm = rng.permutation(len(v))
    return v[perm], parent[perm]


@functools.lru_cache(maxsize=None)
def _graph(name):
    """-> (n, ei, ej): the graphs of the issue by name"""
    rng = np.random.default_rng(3)
    if name == "single":
        return 1, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if name == "no_edge":
        return 5, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if name == "one_edge_reversed":
        return 5, np.array([3]), np.array([1])
    if name == "duplicates":
        ei, ej = np.array([0, 4, 0, 4, 2, 0]), np.array([4, 0, 4, 0, 6, 4])
        return 9, ei, ej
    if name == "path_70000":  # find depth and path halving: a path under a random relabelling, the list shuffled
        n = 70000
        relabel = rng.permutation(n)
        perm = rng.permutation(n - 1)
        return n, relabel[:-1][perm], relabel[1:][perm]
    if name == "star_centre_last":  # every union moves one root; contention on one word
        n = 4097
        return n, np.full(n - 1, n - 1), rng.permutation(n - 1)
    if name == "star_centre_first":
        n = 4097
        return n, 1 + rng.permutation(n - 1), np.zeros(n - 1, np.int64)
    if name == "complete_300":
        iu, ju = np.triu_indices(300, 1)
        return 300, iu, ju
    if name == "random_100000":
        return (100000,) + _random_edges(100000, 150000, 11)
    if name == "joined_by_last_pair":
        a, b = _random_tree(0, 50000, rng), _random_tree(50000, 100000, rng)
        ei, ej = np.r_[a[0], b[0]], np.r_[a[1], b[1]]
        perm = rng.permutation(len(ei))
        return 100000, np.r_[ei[perm], 99999], np.r_[ej[perm], 17]
    if name.startswith("edge_"):  # word and workgroup edges of the numbering pass
        n = int(name.split("_")[1])
        return (n,) + _random_edges(n, n // 2, n)
    raise KeyError(name)


GRAPHS = ["single", "no_edge", "one_edge_reversed", "duplicates", "path_70000", "star_centre_last", "star_centre_first",
          "complete_300", "random_100000", "joined_by_last_pair", "edge_63", "edge_64", "edge_65", "edge_1023",
          "edge_1024", "edge_1025"]


@pytest.mark.parametrize("name", GRAPHS)
def test_graph_cases(fc, name):
    n, ei, ej = _graph(name)
    ref = cr.components(n, ei, ej)
    if name == "joined_by_last_pair":
        assert ref.sizes.tolist() == [100000]
        assert cr.components(n, ei[:-1], ej[:-1]).sizes.tolist() == [50000, 50000]
    if name.startswith("star") or name in ("path_70000", "complete_300"):
        assert ref.sizes.tolist() == [n] and ref.representatives.tolist() == [0]
    _assert_same(fc.pruner.clusters_from_pairs(cr.pack_pairs(ei, ej), n), ref, name)
    _assert_same(fc.pruner.clusters_from_pairs(np.stack([ej, ei], axis=1).reshape(-1, 2), n), ref, name)  # (P, 2), swapped
    if n <= 2048:
        bits = cr.pack_bits(n, ei, ej)
        _assert_same(fc.pruner.clusters_from_bits(bits, n), ref, name)
        # bits at and below the diagonal are not read: set them all
        W = bits.shape[1]
        low = np.zeros((n, W * 64), dtype=bool)
        low[:, :n] = np.tril(np.ones((n, n), dtype=bool))
        noisy = bits | np.packbits(low.reshape(n, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, W)
        _assert_same(fc.pruner.clusters_from_bits(noisy, n), ref, name)


def test_graph_result_is_a_function_of_the_graph(fc):
    """the same graph as a shuffled list with duplicates and swapped ends, five times over: identical output"""
    n, ei, ej = _graph("random_100000")
    ref = cr.components(n, ei, ej)
    rng = np.random.default_rng(1)
    for _ in range(5):
        perm = rng.permutation(len(ei))
        swap = rng.random(len(ei)) < 0.5
        a, b = np.where(swap, ej, ei)[perm], np.where(swap, ei, ej)[perm]
        _assert_same(fc.pruner.clusters_from_pairs(cr.pack_pairs(np.r_[a, a[:999]], np.r_[b, b[:999]]), n), ref)


def test_empty_graph_calls(fc):
    for got in (fc.pruner.clusters_from_pairs(np.zeros(0, np.uint64), 0), fc.pruner.clusters_from_bits(np.zeros((0, 0), np.uint64), 0)):
        assert got.labels.shape == got.representatives.shape == got.sizes.shape == (0,)


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


def _resident(fc, X, S_default, enant=False):
    """clusters on a resident handle, then the default prune and simbits on the SAME handle: nothing leaked, `enant`
    cleared -> (RmsdClusters, stats)"""
    from firecode_amd import _lib

    with fc.DeviceEnsemble(X, center=True) as ens:
        labels, reps, sizes, stats = ens.clusters(THR, 2 * THR, prune_enantiomers=enant)
        mask, _ = ens.prune(THR, 2 * THR)
        bits, grey = ens.simbits(THR, 2 * THR)
        again = ens.clusters(THR, 2 * THR, prune_enantiomers=enant)
    assert np.array_equal(mask, o.greedy_prune_from_matrix(S_default))
    assert np.array_equal(_lib.unpack_bits(bits, len(X)), np.triu(S_default, 1)) and grey == 0
    for a, b in zip(again, (labels, reps, sizes, stats)):
        assert np.array_equal(a, b)
    return fc.pruner.RmsdClusters(labels, reps, sizes), stats


def _check(fc, name, enant=False, expect_bits=0):
    X, atoms, _ = _ensemble(name)
    n = len(X)
    S = _similarity(name, enant)
    S_default = _similarity(name, False)
    ref = cr.clusters_from_matrix(S)
    got, stats = _resident(fc, X, S_default, enant)
    _assert_same(got, ref, name)
    assert stats.tolist()[2:] == [int(np.triu(S, 1).sum()), 0, expect_bits, len(ref.sizes)], (name, stats)
    assert int(stats[0]) == n * (n - 1) // 2
    _assert_same(fc.pruner.cluster_by_rmsd(X, atoms, THR, prune_enantiomers=enant), ref, name)
    _, mask = fc.pruner.prune_by_rmsd(X, atoms, THR, prune_enantiomers=enant)
    assert len(ref.sizes) <= int(mask.sum()), name  # the highest-index member of a component is never removed by the ladder
    return ref, mask


@pytest.mark.parametrize("N,A,seed", [(1, 5, 1), (2, 5, 1), (65, 12, 3), (60, 12, 5)])
def test_clustered(fc, N, A, seed):
    name = f"clustered:{N}:{A}:{seed}"
    ref, mask = _check(fc, name)
    assign = _ensemble(name)[2]
    assert cr.same_partition(ref.labels, assign)
    assert len(ref.sizes) == int(mask.sum())


def test_reflected_half(fc):
    """mirror images: the default form keeps the hands apart, the enantiomer-aware form pairs them"""
    ref_default, _ = _check(fc, "reflected")
    ref_enant, _ = _check(fc, "reflected", enant=True)
    assert len(ref_enant.sizes) < len(ref_default.sizes)
    assert cr.same_partition(ref_enant.labels, _ensemble("reflected")[2])


def test_continuous_both_paths(fc, monkeypatch):
    """no cluster structure: chains of similar pairs; once from the pair list, once -- the candidate queue cut to four
    entries -- from the bit matrix.  Identical outputs."""
    from firecode_amd import _lib

    ref, _ = _check(fc, "continuous")
    assert len(ref.sizes) > 1 and ref.sizes.max() > 100
    X = _ensemble("continuous")[0]
    with fc.DeviceEnsemble(X, center=True) as ens:
        from_list = ens.clusters(THR, 2 * THR)
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")
    ref_bits, _ = _check(fc, "continuous", expect_bits=1)
    with fc.DeviceEnsemble(X, center=True) as ens:
        from_bits = ens.clusters(THR, 2 * THR)
    monkeypatch.delenv("FC_PAIRQ_CAP")
    assert int(from_list[3][4]) == 0 and int(from_bits[3][4]) == 1
    for a, b in zip(from_list[:3], from_bits[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(from_list[3][[0, 2, 3, 5]], from_bits[3][[0, 2, 3, 5]])


def test_identical_copies_dense(fc, monkeypatch):
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")
    ref, _ = _check(fc, "identical", expect_bits=1)
    assert ref.sizes.tolist() == [200] and ref.representatives.tolist() == [0]
    ref, _ = _check(fc, "identical", enant=True, expect_bits=1)
    assert ref.sizes.tolist() == [200]
    monkeypatch.delenv("FC_PAIRQ_CAP")
    _check(fc, "identical")


def test_path_ensemble_and_its_reverse(fc):
    """a similarity graph that is exactly a path broken at the cuts: three clusters of known sizes, one long chain each;
    with the input reversed the partition is the same and the representatives are again by index"""
    ref, _ = _check(fc, "path")
    X, atoms, k = _ensemble("path")
    assert sorted(ref.sizes.tolist()) == [199, 400, 498]
    assert cr.same_partition(ref.labels, np.digitize(k, [400, 900]))
    S = _similarity("path")
    ref_rev = cr.clusters_from_matrix(S[::-1, ::-1])
    got_rev = fc.pruner.cluster_by_rmsd(np.ascontiguousarray(X[::-1]), atoms, THR)
    _assert_same(got_rev, ref_rev)
    assert cr.same_partition(got_rev.labels[::-1], ref.labels)
    assert all(r == np.flatnonzero(got_rev.labels == c).min() for c, r in enumerate(got_rev.representatives))


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
    ref = cr.clusters_from_matrix(S, energies, max_dE)
    assert len(ref.sizes) == 2 * len(np.unique(assign)) and sorted(set(ref.sizes.tolist())) == [2, 3]
    got = fc.pruner.cluster_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE)
    _assert_same(got, ref)
    assert cr.same_partition(got.labels, assign * 2 + (rank >= 3))
    assert np.all(np.diff(energies[got.representatives]) > 0)  # cluster order follows energy
    for c, r in enumerate(got.representatives):              # the representative is the lowest-energy member
        members = np.flatnonzero(got.labels == c)
        assert r == members[np.argmin(energies[members])]
    _, mask = fc.pruner.prune_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE)
    assert len(got.sizes) <= int(mask.sum())
    assert np.array_equal(mask, o.prune_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE)[1])
    # a window that cuts nothing: the clusters of the plain call, ordered by energy
    wide = fc.pruner.cluster_by_rmsd(X, atoms, THR, energies=energies, max_dE=100.0)
    _assert_same(wide, cr.clusters_from_matrix(S, energies, 100.0))
    assert cr.same_partition(wide.labels, assign)
    # energies of the wrong length are not usable: index order, no window (as prune_by_rmsd treats them)
    _assert_same(fc.pruner.cluster_by_rmsd(X, atoms, THR, energies=energies[:10], max_dE=max_dE), cr.clusters_from_matrix(S))


def test_ensemble_method_and_debug_line(fc):
    name = "clustered:60:12:5"
    X, atoms, assign = _ensemble(name)
    S025, gap = cr.default_similarity(X, atoms, 0.25)  # Ensemble passes no threshold: the pruner's default
    assert gap > GAP
    energies = np.random.default_rng(4).random(60) * 0.5
    log = []
    ens = fc.ensemble.Ensemble(atoms, X.copy(), energies=energies.copy(), logfunction=log.append)
    got = ens.cluster_by_rmsd()
    _assert_same(got, cr.clusters_from_matrix(S025, energies, 1.0))
    assert len(ens.coords) == 60 and len(ens.energies) == 60  # not masked
    line = [ln for ln in log if "cluster_by_rmsd" in ln]
    assert len(line) == 1
    m = re.fullmatch(r"DEBUG: cluster_by_rmsd \[gfx950\] - (\d+) pairs screened, (\d+) similar, (\d+) clusters, "
                     r"largest (\d+), in \d+\.\d{3} s", line[0])
    assert m, line[0]
    assert [int(v) for v in m.groups()] == [60 * 59 // 2, int(np.triu(S025, 1).sum()), len(got.sizes), int(got.sizes.max())]
    log.clear()
    quiet = fc.ensemble.Ensemble(atoms, X.copy(), logfunction=log.append)  # no energies: index order, no window
    _assert_same(quiet.cluster_by_rmsd(max_rmsd=THR, verbose=False), cr.clusters_from_matrix(_similarity(name)))
    assert log == []
    debug = []
    fc.pruner.cluster_by_rmsd(X, atoms, THR, prune_enantiomers=True, debugfunction=debug.append)
    assert debug[0].startswith("DEBUG: cluster_by_rmsd [gfx950, mirror images included] - ")
