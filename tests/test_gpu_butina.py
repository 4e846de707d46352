"""Sphere-exclusion (Butina) RMSD clusters on the GPU (fc_rmsd_butina, fc_rmsd_butina_enant, fc_rmsd_butina_perm,
fc_butina_from_pairs, fc_butina_from_bits and the Python layers above them) against the NumPy restatement
(tests/butina_ref.py): the literal walk, and the independent checker on every result.

No tolerance anywhere: labels, centroids, sizes, degrees and counts are integers and must match exactly.  Every RMSD
ensemble asserts ``min_gap > 1e-6`` from the restatement first, so no pair is ever exempted."""

import functools
import re

import numpy as np
import pytest

import butina_ref as br
import cluster_ref as cr
import dbscan_ref as dr
import enant_ref as er
import symm_ref as sr
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

GAP = 1e-6
THR = 0.5
ROUNDS = (None, "0", "1")  # FC_BUTINA_ROUNDS: the default, everything to the finish, one round ahead of it


def _assert_same(got, ref, label=""):
    assert got.labels.dtype == np.int32 and got.centroids.dtype == np.int64 and got.sizes.dtype == np.int64, label
    assert got.degrees.dtype == np.int32, label
    assert np.array_equal(got.degrees, ref.degrees), label
    assert np.array_equal(got.sizes, ref.sizes), label
    assert np.array_equal(got.centroids, ref.centroids), label
    assert np.array_equal(got.labels, ref.labels), label


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (n, ei, ej, the walk's result), computed once and not modified"""
    n, ei, ej = br.graph(name)
    return n, ei, ej, br.walk(n, ei, ej)


def _both_forms(fc, n, ei, ej, ref, label=""):
    """pairs form and bits form: each against the walk and the checker, and hence equal to each other"""
    got_p = fc.pruner.butina_from_pairs(cr.pack_pairs(ei, ej), n, assume_unique=True)
    got_b = fc.pruner.butina_from_bits(cr.pack_bits(n, ei, ej), n)
    for got in (got_p, got_b):
        _assert_same(got, ref, label)
        br.check(n, ei, ej, *got)
    return got_p


def _set_rounds(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("FC_BUTINA_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("FC_BUTINA_ROUNDS", value)


# ---- a caller's graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.SMALL_GRAPHS)
def test_graph_cases(fc, monkeypatch, name):
    n, ei, ej, ref = _case(name)
    for rounds in ROUNDS:
        _set_rounds(monkeypatch, rounds)
        _both_forms(fc, n, ei, ej, ref, (name, rounds))
    _set_rounds(monkeypatch, None)
    if name == "late_claim":
        assert ref.labels[4] == ref.labels[2] != ref.labels[3] and ref.depth == 4
    if n <= 130:  # (P, 2) indices with swapped ends and every pair twice: the wrapper brings the list to a set
        twice = np.stack([np.r_[ej, ei], np.r_[ei, ej]], axis=1).reshape(-1, 2)
        _assert_same(fc.pruner.butina_from_pairs(twice, n), ref, name)
        low = np.zeros((n, (n + 63) // 64 * 64), dtype=bool)  # bits at and below the diagonal are not read: set them all
        low[:, :n] = np.tril(np.ones((n, n), dtype=bool))
        W = low.shape[1] // 64
        noisy = cr.pack_bits(n, ei, ej) | np.packbits(low.reshape(n, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, W)
        _assert_same(fc.pruner.butina_from_bits(noisy, n), ref, name)


def test_disjoint_cliques_equal_the_components(fc):
    n, ei, ej, ref = _case("cliques")
    got = _both_forms(fc, n, ei, ej, ref)
    comp = fc.pruner.clusters_from_pairs(cr.pack_pairs(ei, ej), n)
    assert np.array_equal(got.labels, comp.labels) and np.array_equal(got.centroids, comp.representatives)
    assert np.array_equal(got.sizes, comp.sizes)


@pytest.mark.parametrize("name", ["path_3000", "thick_3000"])
def test_deep_graphs_for_every_round_count(fc, monkeypatch, name):
    """the depth worst cases: identical outputs whatever share of the rounds the one-workgroup finish takes; with the
    live-edge list cut to 16 entries the finish walks the graph itself (the caller's list, the bit matrix)"""
    n, ei, ej, ref = _case(name)
    assert ref.depth > 100
    for rounds in ROUNDS:
        _set_rounds(monkeypatch, rounds)
        _both_forms(fc, n, ei, ej, ref, (name, rounds))
    _set_rounds(monkeypatch, None)
    monkeypatch.setenv("FC_BUTINA_LIVE_CAP", "16")
    _both_forms(fc, n, ei, ej, ref, (name, "live list overflows"))
    monkeypatch.delenv("FC_BUTINA_LIVE_CAP")


def test_random_graph_beyond_one_grid(fc):
    """G(2 000, 0.3): about 6e5 entries, more than one grid's worth, so the stride loops run; then the same list shuffled
    with the ends flipped at random"""
    n, ei, ej, ref = _case("gnp_2000_0.3")
    assert 5.5e5 < len(ei) < 6.5e5
    got = _both_forms(fc, n, ei, ej, ref)
    rng = np.random.default_rng(1)
    perm, swap = rng.permutation(len(ei)), rng.random(len(ei)) < 0.5
    a, b = np.where(swap, ej, ei)[perm], np.where(swap, ei, ej)[perm]
    again = fc.pruner.butina_from_pairs(cr.pack_pairs(a, b), n, assume_unique=True)
    _assert_same(again, got)
    _assert_same(fc.pruner.butina_from_pairs(cr.pack_pairs(a, b), n), got)


def test_empty_graph_calls(fc):
    for got in (fc.pruner.butina_from_pairs(np.zeros(0, np.uint64), 0), fc.pruner.butina_from_bits(np.zeros((0, 0), np.uint64), 0)):
        assert isinstance(got, fc.pruner.RmsdButina) and all(arr.shape == (0,) for arr in got)
    got = fc.pruner.butina_from_pairs(np.zeros(0, np.uint64), 5)  # no edges: five singletons
    assert got.labels.tolist() == [0, 1, 2, 3, 4] and got.sizes.tolist() == [1] * 5 and got.degrees.tolist() == [0] * 5


# ---- the resident depth cases: stats[6] and stats[7] -----------------------------------------------------------------------
def _line(n, step):
    return dr.line_ensemble(step * np.arange(n))


def _line_band_is_clear(X, atoms, band, stride=15):
    """the oracle on a sample of the pairs that decide the band: (k, k + band) similar, (k, k + band + 1) not, both
    more than GAP from the thresholds"""
    for k in range(0, len(X) - band - 1, stride):
        for d, want in ((band, True), (band + 1, False)):
            r, m = o.rmsd_and_max(X[k], X[k + d], center=True)
            assert (r < THR and m < 2 * THR) == want and abs(r - THR) > GAP and (r >= THR or abs(m - 2 * THR) > GAP), (k, d, r, m)


@pytest.mark.parametrize("name,step,band", [("path_3000", 0.3, 1), ("thick_3000", 0.0475, 10)])
def test_resident_deep_graphs_reach_the_finish(fc, monkeypatch, name, step, band):
    """3 000 conformers on a line in index order: the similarity graph is the path (the band of 10).  The grid-wide
    rounds leave most of it (stats[7] > 0), one workgroup finishes it, and the rounds needed (stats[6]) are the depth of
    the walk whatever the knob says."""
    n, ei, ej, ref = _case(name)
    X, atoms = _line(n, step)
    _line_band_is_clear(X, atoms, band)
    seen = []
    with fc.DeviceEnsemble(X, center=True) as ens:
        for rounds in ROUNDS:
            _set_rounds(monkeypatch, rounds)
            *res, stats = ens.butina(THR, 2 * THR)
            got = fc.pruner.RmsdButina(*res)
            assert int(stats[2]) == len(ei) and int(stats[3]) == 0, (rounds, stats)  # the graph is the one the case names
            _assert_same(got, ref, (name, rounds))
            assert int(stats[5]) == len(ref.centroids) and int(stats[6]) == ref.depth, (rounds, stats)
            seen.append(int(stats[7]))
    _set_rounds(monkeypatch, None)
    assert seen[0] > 0 and seen[1] > seen[0] and seen[1] >= seen[2] > 0, seen  # (default, 0, 1): the finish really ran
    br.check(n, ei, ej, *got)


def test_cliques_never_reach_the_finish(fc):
    """identical copies: one clique, two rounds, nothing left for the finish"""
    X, atoms = _identical(130, 12, 3)
    with fc.DeviceEnsemble(X, center=True) as ens:
        *res, stats = ens.butina(THR, 2 * THR)
    assert res[1].tolist() == [0] and res[2].tolist() == [130] and stats.tolist()[2:] == [130 * 129 // 2, 0, 0, 1, 2, 0]


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
        X, atoms, assign = syn.synthetic_ensemble(200, 30, seed=4)
        return er.reflect(X, np.random.default_rng(0).random(200) < 0.5), atoms, assign
    if kind == "continuous":
        return syn.continuous_ensemble(300, 30), np.array(["C"] * 30), None
    if kind == "identical":
        return _identical(200, 20, 9) + (None,)
    if kind == "path":
        return cr.path_ensemble(400, 20, cuts=(150, 151, 300))
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


def _resident(fc, X, S, S_default, enant=False, symmetry=None, expect_bits=0):
    """butina on a resident handle against the walk and the checker; then the default prune, the clusters and the
    density-based clusters on the same handle against their restatements, and butina again: nothing leaked"""
    n = len(X)
    with fc.DeviceEnsemble(X, center=True) as ens:
        *res, stats = ens.butina(THR, 2 * THR, prune_enantiomers=enant, symmetry=symmetry)
        mask, _ = ens.prune(THR, 2 * THR)
        cl = ens.clusters(THR, 2 * THR)
        db = ens.dbscan(THR, 2 * THR, 3)
        again = ens.butina(THR, 2 * THR, prune_enantiomers=enant, symmetry=symmetry)
    got = fc.pruner.RmsdButina(*res)
    ref = br.walk_from_matrix(S)
    _assert_same(got, ref)
    br.check(n, *cr.edges(S), *got)
    assert stats.tolist()[2:7] == [int(np.triu(S, 1).sum()), 0, expect_bits, len(ref.centroids), ref.depth], stats
    assert int(stats[0]) == n * (n - 1) // 2 and 0 <= int(stats[7]) < n
    assert np.array_equal(mask, o.greedy_prune_from_matrix(S_default))
    for a, b in zip(cl[:3], cr.clusters_from_matrix(S_default)):
        assert np.array_equal(a, b)
    for a, b in zip(db[:5], dr.dbscan_from_matrix(S_default, 3)):
        assert np.array_equal(a, b)
    for a, b in zip(again, tuple(got) + (stats,)):
        assert np.array_equal(a, b)
    return got, stats


def _check(fc, name, enant=False, expect_bits=0):
    X, atoms, _ = _ensemble(name)
    S = _similarity(name, enant)
    got, stats = _resident(fc, X, S, _similarity(name, False), enant, expect_bits=expect_bits)
    _assert_same(fc.pruner.butina_by_rmsd(X, atoms, THR, prune_enantiomers=enant), got, name)
    return got, stats


@pytest.mark.parametrize("N,A,seed", [(1, 5, 1), (2, 5, 1), (65, 12, 3), (300, 12, 3)])
def test_clustered(fc, N, A, seed):
    name = f"clustered:{N}:{A}:{seed}"
    got, stats = _check(fc, name)
    assign = _ensemble(name)[2]
    if N >= 65:  # the generator's clusters of five are cliques: one centroid each, its first member
        assert cr.same_partition(got.labels, assign) and (got.degrees == 4).all() and int(stats[6]) == 2
        assert got.centroids.tolist() == [int(np.flatnonzero(assign == c).min()) for c in assign[got.centroids]]
        assert got.members(3).tolist() == np.flatnonzero(assign == assign[got.centroids[3]]).tolist()
    if N == 1:
        assert got.labels.tolist() == [0] and got.centroids.tolist() == [0] and got.degrees.tolist() == [0]


def test_continuous_both_paths(fc, monkeypatch):
    """no cluster structure: once from the pair list, once -- the candidate queue cut to four entries -- from the bit
    matrix.  Identical outputs; members within the threshold of their centroid where the components weld everything."""
    S = _similarity("continuous")
    assert int(np.triu(S, 1).sum()) == 729
    from_list, _ = _check(fc, "continuous")
    assert len(from_list.centroids) > len(cr.clusters_from_matrix(S).sizes)
    own = from_list.centroids[from_list.labels]
    member = own != np.arange(len(S))
    assert S[own[member], np.flatnonzero(member)].all()
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")
    from_bits, stats = _check(fc, "continuous", expect_bits=1)
    monkeypatch.delenv("FC_PAIRQ_CAP")
    assert int(stats[4]) == 1
    _assert_same(from_bits, from_list)


def test_path_ensemble(fc):
    """a path under a random relabelling, broken at three cuts: every cluster is a centroid with one or two neighbours"""
    got, _ = _check(fc, "path")
    assert set(got.sizes.tolist()) <= {1, 2, 3} and (got.degrees <= 2).all()


def test_identical_copies_dense(fc, monkeypatch):
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")
    got, stats = _check(fc, "identical", expect_bits=1)
    _check(fc, "identical", enant=True, expect_bits=1)
    monkeypatch.delenv("FC_PAIRQ_CAP")
    assert int(stats[4]) == 1 and int(stats[7]) == 0
    assert got.sizes.tolist() == [200] and got.centroids.tolist() == [0] and (got.degrees == 199).all()
    _assert_same(_check(fc, "identical")[0], got)


def test_reflected_half(fc):
    """mirror images: the default form keeps the hands apart, the enantiomer-aware form pairs them (every generator
    cluster of five is one sphere)"""
    default, _ = _check(fc, "reflected")
    enant, _ = _check(fc, "reflected", enant=True)
    assign = _ensemble("reflected")[2]
    assert cr.same_partition(enant.labels, assign) and len(default.centroids) > len(enant.centroids)


def test_symmetry_table(fc):
    """K = 2 atom permutations (the reversal of a path), a random half of the conformers relabelled"""
    table = sr.path_table(9)
    X, atoms, assign = syn.synthetic_ensemble(150, 9, seed=1)
    Y, _ = sr.relabel_half(X, table, 1)
    mats = sr.similarity(Y, atoms, table, THR)
    assert mats.min_gap > GAP and len(table) == 2
    got, _ = _resident(fc, Y, mats.S, mats.S_default, symmetry=table)
    assert cr.same_partition(got.labels, assign)
    ref_default = br.walk_from_matrix(mats.S_default)
    assert len(ref_default.centroids) > len(got.centroids)                     # without the table the clusters split
    lines = []
    _assert_same(fc.pruner.butina_by_rmsd(Y, atoms, THR, symmetry=table, debugfunction=lines.append), got)
    assert lines[0].startswith("DEBUG: butina_by_rmsd [gfx950, 2 atom permutations] - 11175 pairs screened, ")
    _assert_same(fc.pruner.butina_by_rmsd(Y, atoms, THR), ref_default)


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
    ref = br.walk_from_matrix(S, energies, max_dE)
    assert sorted(set(ref.sizes.tolist())) == [2, 3] and len(ref.sizes) == 2 * len(np.unique(assign))
    got = fc.pruner.butina_by_rmsd(X, atoms, THR, energies=energies, max_dE=max_dE)
    _assert_same(got, ref)
    order, ei, ej = br.sorted_edges(S, energies, max_dE)               # the checker, in processing order
    inv = np.empty(60, dtype=np.int64)
    inv[order] = np.arange(60)
    br.check(60, ei, ej, got.labels[order], inv[got.centroids], got.sizes, got.degrees[order])
    assert np.all(np.diff(energies[got.centroids]) > 0)                # cluster order follows energy ...
    for c, r in enumerate(got.centroids):                              # ... and within a clique the lowest energy leads
        assert r == got.members(c)[np.argmin(energies[got.members(c)])]
    wide = fc.pruner.butina_by_rmsd(X, atoms, THR, energies=energies, max_dE=100.0)
    _assert_same(wide, br.walk_from_matrix(S, energies, 100.0))
    assert cr.same_partition(wide.labels, assign)
    # energies of the wrong length are not usable: index order, no window
    _assert_same(fc.pruner.butina_by_rmsd(X, atoms, THR, energies=energies[:10], max_dE=max_dE), br.walk_from_matrix(S))


def test_ensemble_method_and_debug_line(fc):
    name = "clustered:60:12:5"
    X, atoms, assign = _ensemble(name)
    S025, gap = cr.default_similarity(X, atoms, 0.25)  # Ensemble passes no threshold: the pruner's default
    assert gap > GAP
    energies = np.random.default_rng(4).random(60) * 0.5
    log = []
    ens = fc.ensemble.Ensemble(atoms, X.copy(), energies=energies.copy(), logfunction=log.append)
    got = ens.butina_by_rmsd()
    ref = br.walk_from_matrix(S025, energies, 1.0)
    _assert_same(got, ref)
    assert len(ens.coords) == 60 and len(ens.energies) == 60  # not masked
    line = [ln for ln in log if "butina_by_rmsd" in ln]
    assert len(line) == 1
    m = re.fullmatch(r"DEBUG: butina_by_rmsd \[gfx950\] - (\d+) pairs screened, (\d+) similar: (\d+) clusters, largest (\d+), "
                     r"(\d+) singletons, (\d+) rounds, in \d+\.\d{3} s", line[0])
    assert m, line[0]
    assert [int(v) for v in m.groups()] == [60 * 59 // 2, int(np.triu(S025, 1).sum()), len(ref.sizes), int(ref.sizes.max()),
                                            int((ref.sizes == 1).sum()), ref.depth]
    log.clear()
    quiet = fc.ensemble.Ensemble(atoms, X.copy(), logfunction=log.append)  # no energies: index order, no window
    _assert_same(quiet.butina_by_rmsd(max_rmsd=THR, verbose=False), br.walk_from_matrix(_similarity(name)))
    assert log == []
    debug = []
    fc.pruner.butina_by_rmsd(X, atoms, THR, prune_enantiomers=True, debugfunction=debug.append)
    assert debug[0].startswith("DEBUG: butina_by_rmsd [gfx950, mirror images included] - ")


def test_empty_ensemble(fc):
    out = fc.pruner.butina_by_rmsd(np.zeros((0, 4, 3)), np.array(["C"] * 4), THR)
    assert isinstance(out, fc.pruner.RmsdButina) and all(arr.shape == (0,) for arr in out)
