"""The threshold consumers of the RMSD -- the prune in every screen mode (kabsch_may_be_below, the bounded fp32 tests, the
split-half test), the enantiomer- and the symmetry-aware prune (k_symm_simbits), the four forms of the refine, the graph
consumers (clusters, DBSCAN, Butina) and the medoids (k_group_sums) -- on the rank-deficient and edge geometries of
tests/degenerate_ref.py, and on pairs put at a known distance on either side of a threshold.

Bars, those of test_gpu_degenerate_neighbours.py and test_gpu_enant.py: bits, masks, labels, representatives, centroids
and counts identical to the reference, grey count 0, distances, means and radii within TOL = 1e-10 -- on cases whose
every decision the reference alone puts more than GAP = 1e-9 from its threshold (asserted before the device is touched).

(a) every degenerate kind (one atom, two atoms, atoms on a line, in a plane, symmetric tops and their mirror images) at
    three sizes: closed forms where the kind has one, the oracle's rows elsewhere.
(b) the knife-edge: one base structure at many scales (degenerate_ref.scaled_family), so that every (conformer,
    reference) pair lies 1e-8 ... 3e-5 A inside or outside the threshold of the RMSD test or of the max-deviation test,
    with the RMSD, the max deviation and hence every bit known in closed form for a base of any rank.  At a cap of
    0.25 A the mean square deviation falls short of the threshold's by 5e-9 ... 1.5e-5 A^2: on both sides of the
    screens' margin (kScreenMargin, 1e-6 A^2).  Every run prints how many edge pairs it lost or admitted.
(c) k-medoids on the scaled family: a metric on a line with two tight clumps.

What was measured: DESIGN.md section 18.1."""

import functools

import numpy as np
import pytest

import butina_ref as br
import cluster_ref as cr
import dbscan_ref as dbr
import degenerate_ref as dg
import diverse_ref as dr
import enant_ref as er
import medoid_ref as mr
import symm_ref as sr
from oracle import cpu_ref as o
from test_gpu_degenerate_neighbours import CASES, KINDS, _case, _ids, _middle_cap

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-9
LANES_MIN = 1 << 17  # kRefineLanesMin: candidate queues longer than this take the one-lane-per-pair refine kernels
# FC_SCREEN_F32 = 0 / 2 / 3 (no single-precision screen / one whatever the band / the same with the verdict behind it),
# fc_screen_select(16) / (32) (each single-precision kernel by name), FC_SCREEN_CFG=valu8x4 (the VALU screen)
MODES = ("0", "2", "3", "k16", "k32", "valu8x4")
SINGLE = (16, 32)


# ---- the screen modes ------------------------------------------------------------------------------------------------------
def _in_mode(fc, monkeypatch, mode, call):
    """``call()`` under one screen mode -> its result, or None where the launcher refuses the forced kind for the shape"""
    from firecode_amd import _lib

    monkeypatch.delenv("FC_SCREEN_F32", raising=False)
    monkeypatch.delenv("FC_SCREEN_CFG", raising=False)
    if mode.startswith("k"):
        _lib.screen_select(int(mode[1:]))
    elif mode.startswith("valu"):
        monkeypatch.setenv("FC_SCREEN_CFG", mode)
    else:
        monkeypatch.setenv("FC_SCREEN_F32", mode)
    try:
        return call()
    except fc.FirecodeHipError as err:
        if mode.startswith("k") and err.code in (_lib.FC_E_INVALID, _lib.FC_E_LIMIT) and "screen" in str(err):
            return None
        raise
    finally:
        _lib.screen_select(0)
        monkeypatch.delenv("FC_SCREEN_F32", raising=False)
        monkeypatch.delenv("FC_SCREEN_CFG", raising=False)


def _bits_and_mask(fc, X, thr, dev, twice=False, **kw):
    """similarity bits and the prune on one fresh handle (``twice``: both again -- the refine's form follows the last
    queue's length) -> a list of (bits (N, N) bool, grey, kind of the bit launch, mask, stats, kind of the lean launch)"""
    from firecode_amd import _lib

    out = []
    with fc.DeviceEnsemble(X, center=True) as ens:
        for _ in range(2 if twice else 1):
            bits, grey = ens.simbits(thr, dev, **kw)
            kind_bits = _lib.screen_last_kind()
            mask, stats = ens.prune(thr, dev, **kw)
            out.append((_lib.unpack_bits(bits, len(X)), int(grey), kind_bits, mask, stats, _lib.screen_last_kind()))
    return out


def _assert_run(run, S, mask, what):
    bits, grey, _, got_mask, stats, _ = run
    n = len(S)
    assert np.array_equal(bits, np.triu(S, 1)), f"{what}: similarity bits"
    assert grey == 0 and int(stats[3]) == 0, f"{what}: grey pairs"
    assert np.array_equal(got_mask, mask), f"{what}: mask"
    assert int(stats[2]) == int(np.triu(S, 1).sum()), f"{what}: similar-pair count"
    assert int(stats[0]) == n * (n - 1) // 2 and int(stats[5]) == int(mask.sum()), f"{what}: stats"


def _gap(r, m, thr, dev):
    """distance of the decisive values from their thresholds: r always, m where r passes (enant_ref's rule)"""
    g = np.abs(r - thr)
    g = np.where(r < thr, np.minimum(g, np.abs(m - dev)), g)
    return float(g.min()) if g.size else float("inf")


# ---- (a) parity on each degenerate kind ------------------------------------------------------------------------------------
class Ref:
    """what the reference alone says about a case: the threshold, the three similarity matrices with their gaps, the masks"""

    def __init__(self, kind, N):
        c = _case(kind, N)
        self.c = c
        atoms, iu = c.atoms, np.triu_indices(N, 1)
        R = c.rows("self")
        self.thr = 0.5 if kind == "one_atom" else float(_middle_cap(R[iu], ties=c.image_of is not None))
        self.dev = 2.0 * self.thr
        _, R0, M0 = o.rmsd_similarity_matrix(c.X, atoms, self.thr)
        self.S = (R < self.thr) & (M0 < self.dev) & ~np.eye(N, dtype=bool)
        self.S = self.S | self.S.T  # (the rows of the tops and the planar kind are the oracle's, one per ordered pair)
        self.gap = min(_gap(R[iu], M0[iu], self.thr, self.dev), _gap(R.T[iu], M0[iu], self.thr, self.dev))
        enant = er.similarity(c.X, atoms, self.thr)
        self.S_enant, self.gap_enant = enant.S, enant.min_gap
        self.same_as_oracle = np.array_equal(enant.S_default, self.S)
        self.table = sr.path_table(c.A) if c.A >= 3 else None
        if self.table is not None:
            sym = sr.similarity(c.X, atoms, self.table, self.thr)
            self.S_sym, self.gap_sym = sym.S, sym.min_gap
        for name in ("S", "S_enant", "S_sym"):
            if hasattr(self, name):
                getattr(self, name).setflags(write=False)
                setattr(self, "mask" + name[1:], o.greedy_prune_from_matrix(getattr(self, name)))

    def assert_gaps(self):
        what = f"{self.c.kind}-N{self.c.N}"
        assert self.gap > GAP, f"{what}: a pair within {self.gap:.3g} of a threshold: choose another seed"
        assert self.gap_enant > GAP, f"{what}, mirror flag: a pair within {self.gap_enant:.3g} of a threshold"
        assert self.table is None or self.gap_sym > GAP, f"{what}, reversal: a pair within {self.gap_sym:.3g} of a threshold"
        assert self.same_as_oracle, f"{what}: the closed form's bits are not the oracle's"


@functools.lru_cache(maxsize=None)
def _ref(kind, N):
    return Ref(kind, N)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_plain_prune_in_every_screen_mode(fc, monkeypatch, case):
    """DeviceEnsemble.simbits and .prune under each screen mode, and the one-call host path"""
    ref = _ref(*case)
    ref.assert_gaps()
    c = ref.c
    ran = {}
    for mode in MODES:
        runs = _in_mode(fc, monkeypatch, mode, lambda: _bits_and_mask(fc, c.X, ref.thr, ref.dev))
        if runs is None:
            ran[mode] = None
            continue
        _assert_run(runs[0], ref.S, ref.mask, f"{case} mode={mode}")
        ran[mode] = (runs[0][2], runs[0][5])
    print(f"{case} thr={ref.thr:.6g} gap={ref.gap:.3g} similar={int(np.triu(ref.S, 1).sum())} kinds (bits, prune) by mode: {ran}")
    kinds = {k for pair in ran.values() if pair is not None for k in pair}
    assert ran["0"] is not None and not set(ran["0"]) & set(SINGLE) and ran["valu8x4"] == (1, 1)
    for mode in ("k16", "k32"):
        assert ran[mode] is None or ran[mode] == (int(mode[1:]),) * 2, f"{case}: forced {mode} ran {ran[mode]}"
    if c.A >= 3:
        assert 64 in kinds and kinds & set(SINGLE), f"{case}: the fp64 screen and a single-precision screen were to run: {ran}"
        assert set(ran["2"]) <= set(SINGLE) and set(ran["3"]) <= set(SINGLE), f"{case}: {ran}"
    _, mask = fc.pruner.prune_by_rmsd(c.X, c.atoms, ref.thr)
    assert np.array_equal(mask, ref.mask), f"{case}: prune_by_rmsd"
    if c.kind == "one_atom":  # every pair is similar: the greedy ladder on the complete graph
        assert np.triu(ref.S, 1).sum() == c.N * (c.N - 1) // 2
        assert np.array_equal(mask, o.greedy_prune_from_matrix(~np.eye(c.N, dtype=bool)))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_aware_prunes(fc, case):
    """prune_enantiomers=True on every kind, symmetry=path_table(A) from three atoms on"""
    ref = _ref(*case)
    ref.assert_gaps()
    c = ref.c
    run = _bits_and_mask(fc, c.X, ref.thr, ref.dev, prune_enantiomers=True)[0]
    _assert_run(run, ref.S_enant, ref.mask_enant, f"{case} mirror flag")
    _, mask = fc.pruner.prune_by_rmsd(c.X, c.atoms, ref.thr, prune_enantiomers=True)
    assert np.array_equal(mask, ref.mask_enant)
    if c.kind.startswith("planar") or c.kind.startswith("collinear") or c.A <= 2:
        # the mirror image of a structure in a plane is reached by a proper rotation: the flag changes no bit
        assert np.array_equal(ref.S_enant, ref.S) and np.array_equal(run[0], np.triu(ref.S, 1))
    if c.image_of is not None:  # tops: every structure and its image are similar, at distance 0
        has = np.flatnonzero(c.image_of >= 0)
        lo, hi = np.minimum(has, c.image_of[has]), np.maximum(has, c.image_of[has])
        assert run[0][lo, hi].all()
        with fc.DeviceEnsemble(c.X, center=True) as ens:
            r, m = ens.rmsd_pairs(lo, hi, inverted=True)
        assert r.max() < TOL and m.max() < TOL
    if ref.table is not None:
        run = _bits_and_mask(fc, c.X, ref.thr, ref.dev, symmetry=ref.table)[0]
        _assert_run(run, ref.S_sym, ref.mask_sym, f"{case} reversal")
        _, mask = fc.pruner.prune_by_rmsd(c.X, c.atoms, ref.thr, symmetry=ref.table)
        assert np.array_equal(mask, ref.mask_sym)
    print(f"{case} thr={ref.thr:.6g} gaps: mirror {ref.gap_enant:.3g}" + ("" if ref.table is None else f", reversal {ref.gap_sym:.3g}")
          + f"; similar: plain {int(np.triu(ref.S, 1).sum())}, mirror {int(np.triu(ref.S_enant, 1).sum())}"
          + ("" if ref.table is None else f", reversal {int(np.triu(ref.S_sym, 1).sum())}"))


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("kind", KINDS)
def test_graph_consumers(fc, kind, mirror):
    """clusters, DBSCAN (min_samples 3) and Butina on the graph of a degenerate ensemble: the resident path serves them
    the bits of the prune"""
    ref = _ref(kind, 65)
    ref.assert_gaps()
    c, S = ref.c, (ref.S_enant if mirror else ref.S)
    kw = dict(prune_enantiomers=mirror)
    got, want = fc.pruner.cluster_by_rmsd(c.X, c.atoms, ref.thr, **kw), cr.clusters_from_matrix(S)
    for name in ("labels", "representatives", "sizes"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), f"{kind} clusters: {name}"
    got, want = fc.pruner.dbscan_by_rmsd(c.X, c.atoms, ref.thr, min_samples=3, **kw), dbr.dbscan_from_matrix(S, 3)
    for name in ("labels", "representatives", "sizes", "core", "degrees"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), f"{kind} dbscan: {name}"
    got, want = fc.pruner.butina_by_rmsd(c.X, c.atoms, ref.thr, **kw), br.walk_from_matrix(S)
    for name in ("labels", "centroids", "sizes", "degrees"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), f"{kind} butina: {name}"
    print(f"{kind} mirror={mirror}: {len(want.sizes)} Butina clusters, largest {int(want.sizes.max())}, "
          f"{int(np.triu(S, 1).sum())} edges")


# ---- medoids and k-medoids -------------------------------------------------------------------------------------------------
def _odd_groups(labels):
    """a copy with the last member of every group of even size taken out (label -1)"""
    labels = np.array(labels, dtype=np.int64)
    for g in np.unique(labels[labels >= 0]):
        mem = np.flatnonzero(labels == g)
        if len(mem) % 2 == 0:
            labels[mem[-1]] = -1
    return labels


def _groupings(c):
    """one group and i mod 7 -- without the exact ties two kinds have by construction: two atoms (a metric on a line: a
    group of even size has two medians with equal sums) gets groups of odd size, the tops (a top and its image have equal
    sums where both are in a group) get originals and images in groups of their own"""
    N = c.N
    one, mod7 = np.zeros(N, dtype=np.int64), np.arange(N) % 7
    if c.kind == "two_atoms":
        one, mod7 = _odd_groups(one), _odd_groups(mod7)
    if c.image_of is not None:
        image = np.arange(N) >= (N + 1) // 2
        one, mod7 = image.astype(np.int64), np.where(image, 7 + mod7, mod7)
    return (("one", one), ("mod7", mod7))


def _assert_medoids(got, ref, what):
    print(f"{what}: groups={len(ref.sizes)} largest={int(ref.sizes.max(initial=0))} gap={ref.min_gap:.3g} "
          f"max|E - ref|={np.abs(got.eccentricity - ref.eccentricity).max(initial=0.0):.3g}")
    assert np.array_equal(got.medoids, ref.medoids) and np.array_equal(got.sizes, ref.sizes), what
    live = ref.sizes > 0
    assert np.all(np.isnan(got.mean_distance[~live])) and np.all(np.isnan(got.radius[~live])), what
    assert np.abs(got.mean_distance[live] - ref.mean_distance[live]).max(initial=0.0) < TOL, what
    assert np.abs(got.radius[live] - ref.radius[live]).max(initial=0.0) < TOL, what
    assert np.abs(got.eccentricity - ref.eccentricity).max(initial=0.0) < TOL, what


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_medoids_parity(fc, case):
    c = _case(*case)
    D = c.rows("self")
    for name, labels in _groupings(c):
        n_groups = int(labels.max()) + 1
        ref = mr.medoids_from_rows(D, labels, n_groups)
        if c.kind != "one_atom":
            assert ref.min_gap > GAP, f"{case} {name}: two sums within {ref.min_gap:.3g}: choose another grouping"
        got = fc.pruner.medoids_by_rmsd(c.X, c.atoms, labels)
        _assert_medoids(got, ref, f"{case} {name}")
        if c.kind == "one_atom":  # every sum ties at 0: the lowest index of each group, mean and radius exactly 0
            first = np.array([np.flatnonzero(labels == g)[0] if (labels == g).any() else -1 for g in range(n_groups)])
            live = first >= 0
            assert np.array_equal(got.medoids, first) and np.all(got.sums == 0.0) and np.all(got.eccentricity == 0.0)
            assert np.all(got.mean_distance[live] == 0.0) and np.all(got.radius[live] == 0.0)


@functools.lru_cache(maxsize=None)
def _kmedoids_reference(kind, N, n, max_iter=50, tries=64):
    """the restatement on the whole ensemble (the tops: without their images, which tie with them) or, where its trajectory
    has a tie, on the first seeded draw of all but one to three conformers that has none.  Ties are common here: under the
    metric on a line of the two-atom kind a cluster of even size has two medians with equal sums, and a cluster of two
    moves to its lower index at no change of the cost -> (indices used, reference)"""
    c = _case(kind, N)
    D, size = c.rows("self"), (N if c.image_of is None else (N + 1) // 2)
    for s in range(tries):
        idx = np.arange(size)
        if s > 0:
            idx = np.sort(np.random.default_rng(s).choice(size, size=size - 1 - s % 3, replace=False))
        if len(idx) < n:
            continue
        ref = mr.kmedoids_from_rows(D[np.ix_(idx, idx)], n, max_iter=max_iter)
        if ref.min_gap > GAP:
            return idx, ref
    return idx, ref


def _assert_kmedoids(got, ref, what):
    print(f"{what}: gap={ref.min_gap:.3g} n_iter={ref.n_iter} cost {ref.cost0_q32 / mr.Q:.6f} -> {ref.cost_q32 / mr.Q:.6f}")
    assert np.array_equal(got.medoids, ref.medoids) and np.array_equal(got.labels, ref.labels) and got.n_iter == ref.n_iter, what
    assert np.abs(got.distances - ref.distances).max() < TOL, what
    assert got.cost == int(mr.q32(got.distances).astype(object).sum()) / mr.Q, what


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kmedoids_parity(fc, case):
    """n = 5 (the whole ensemble where it has fewer); the tops without their images, which tie with them"""
    c = _case(*case)
    D = c.rows("self")
    N = c.N if c.image_of is None else (c.N + 1) // 2
    n = min(5, N)
    if c.kind == "one_atom":  # every distance 0, every decision a tie that goes to the lowest index: the initial picks, cost 0
        got = fc.pruner.kmedoids_by_rmsd(c.X, c.atoms, n)
        picks = fc.pruner.select_diverse(c.X, c.atoms, n=n, start=0).indices
        ref = mr.kmedoids_from_rows(D, n)
        assert np.array_equal(got.medoids, picks) and picks.tolist() == list(range(n)) == ref.medoids.tolist()
        assert got.cost == 0.0 and np.all(got.distances == 0.0) and got.n_iter == ref.n_iter == 1
        assert np.array_equal(got.labels, ref.labels) and np.all(got.labels[n:] == 0)
        return
    # two atoms: a metric on a line, where every cluster of even size has two medians with equal sums -- a trajectory free
    # of ties needs five odd clusters at every move (none in 400 draws).  There the assignment to the initial picks alone;
    # the sums of this kind are test_medoids_parity's, on groups of odd size
    max_iter = 0 if c.kind == "two_atoms" and N > n else 50
    idx, ref = _kmedoids_reference(*case, n, max_iter)
    assert ref.min_gap > GAP, f"{case}: every trajectory tried has a near-tie ({ref.min_gap:.3g}): choose another seed"
    got = fc.pruner.kmedoids_by_rmsd(np.ascontiguousarray(c.X[idx]), c.atoms, n, max_iter=max_iter)
    _assert_kmedoids(got, ref, f"{case} n={n} on {len(idx)} conformers")


# ---- (b) the knife-edge ----------------------------------------------------------------------------------------------------
# (base, queries): 128 -- with the reference 129 conformers, the small-ensemble route of the one-call host path; 448 -- the
# whole pair matrix fits the short candidate queue; 1024 -- two clumps of about 512: 2.6e5 similar pairs, above
# kRefineLanesMin, so the first prune of a handle walks the queue as it lies and the second orders it by bucket
KNIFE = [(name, nq) for name in ("full", "planar", "line") for nq in (128, 448, 1024)] + [("full224", 128), ("full224", 256)]


@functools.lru_cache(maxsize=None)
def _knife(name, cap, nq):
    b = dg.scaled_base(name)
    X, a = dg.scaled_family(b, dg.knife_offsets(cap, nq), seed=len(b) + nq)
    R, M = dg.scaled_rmsd(b, a), dg.scaled_maxdev(b, a)
    for arr in (X, R, M):
        arr.setflags(write=False)
    return b, X, np.array(["C"] * len(b)), R, M


@functools.lru_cache(maxsize=None)
def _knife_ref(name, cap, nq, edge):
    """-> (max_rmsd, max_dev, S, gap, mask, signed distance of every (query, reference) pair from the edge)"""
    b, X, atoms, R, M = _knife(name, cap, nq)
    thr, dev = dg.knife_thresholds(b, cap, edge)
    S = (R < thr) & (M < dev) & ~np.eye(len(X), dtype=bool)
    iu = np.triu_indices(len(X), 1)
    off = R[:-1, -1] - thr if edge == "rmsd" else M[:-1, -1] - dev
    S.setflags(write=False)
    return thr, dev, S, _gap(R[iu], M[iu], thr, dev), o.greedy_prune_from_matrix(S), off


def _edge_report(what, bits, S, off):
    """how many (query, reference) pairs inside the threshold the run lost, how many outside it admitted, the closest"""
    got, want = bits[:-1, -1], S[:-1, -1]
    lost, admitted = want & ~got, ~want & got
    wrong = lost | admitted
    print(f"{what}: {int(lost.sum())} of {int(want.sum())} pairs inside the threshold lost, {int(admitted.sum())} of "
          f"{int((~want).sum())} outside admitted; the closest {np.abs(off[wrong]).min(initial=np.inf):.3g} A from it")


def _expected_kinds(mode, A):
    """(of the bit launch, of the lean launch).  Up to 40 atoms every 64-column tile fits; at 224 none does: the bit launch
    is VALU, the lean launch has the 32-column single-precision tiles (plan_screen rows 2 and 3) and no fp64 tile"""
    lean = {"0": (64,) if A <= 40 else (1,), "2": SINGLE, "3": SINGLE, "k16": (16,), "k32": (32,), "valu8x4": (1,)}[mode]
    return (lean if A <= 40 else (1,)), lean


@pytest.mark.parametrize("edge", ["rmsd", "dev"])
@pytest.mark.parametrize("cap", [0.05, 0.25])
@pytest.mark.parametrize("base", KNIFE, ids=lambda b: f"{b[0]}-{b[1]}")
def test_knife_edge(fc, monkeypatch, base, cap, edge):
    """edge="rmsd": max_rmsd = cap, max_dev = 4 cap; edge="dev": max_rmsd = 1.5 cap, max_dev = (max|b| / rms b) cap -- the
    RMSD of every (query, reference) pair is clear and its max deviation at the edge.  Bits in every screen mode, with
    the mirror flag and under the reversal table; mask and similar-pair count, once more through the word queue"""
    name, nq = base
    b, X, atoms, R, M = _knife(name, cap, nq)
    thr, dev, S, gap, mask, off = _knife_ref(name, cap, nq, edge)
    A, N, n_similar = len(b), nq + 1, int(np.triu(S, 1).sum())
    what = f"{name}-{nq} cap={cap} {edge} edge"
    assert gap > GAP, f"{what}: a pair within {gap:.3g} of a threshold: choose another seed"
    # the first half of the queries inside, the second outside, the closest of each 1e-8 ... 2e-8 A from the threshold
    assert np.array_equal(S[:-1, -1], np.arange(nq) < nq // 2) and np.abs(off).max() < 1e-4
    assert GAP < np.abs(off[:nq // 2]).min() < 2e-8 and GAP < np.abs(off[nq // 2:]).min() < 2e-8
    if edge == "rmsd":  # the closed form of the whole square against the oracle on a few rows
        spot = np.arange(0, N, 97)
        assert max(np.abs(dr.rmsd_row(X, int(n)) - R[n]).max() for n in spot) < 1e-12
    long_queue = nq == 1024
    assert (n_similar > LANES_MIN) == long_queue
    print(f"{what}: thr={thr:.6g} dev={dev:.6g} gap={gap:.3g} similar={n_similar} survivors={int(mask.sum())}")

    def check(runs, S_ref, mask_ref, label):
        for k, run in enumerate(runs):
            _edge_report(f"{what} {label} call {k}: kinds {run[2]}, {run[5]}; refined {int(run[4][1])}", run[0], S_ref, off)
        for k, run in enumerate(runs):
            _assert_run(run, S_ref, mask_ref, f"{what} {label} call {k}")
            if long_queue:  # the straight walk (k_refine_pairs), then the bucket form (k_refine_buckets)
                assert int(run[4][1]) > LANES_MIN, f"{what} {label} call {k}: a queue of {int(run[4][1])}"

    for mode in MODES:
        runs = _in_mode(fc, monkeypatch, mode, lambda: _bits_and_mask(fc, X, thr, dev, twice=long_queue))
        assert runs is not None, f"{what}: the launcher refused mode {mode}"
        check(runs, S, mask, f"mode={mode}")
        kinds_bits, kinds_lean = _expected_kinds(mode, A)
        for run in runs:
            assert run[2] in kinds_bits and run[5] in kinds_lean, f"{what} mode={mode}: kinds {run[2]}, {run[5]}"
    # the aware forms: neither the inverted nor the reversed alignment is ever better, the same bits
    check(_bits_and_mask(fc, X, thr, dev, twice=long_queue, prune_enantiomers=True), S, mask, "mirror flag")
    if A <= 40:  # (the same-side blocks make k_symm_simbits drain its queue with edge pairs inside)
        check(_bits_and_mask(fc, X, thr, dev, symmetry=sr.path_table(A)), S, mask, "reversal")
    monkeypatch.setenv("FC_PAIRQ_CAP", "4")  # the word-queue fallback of the refine
    try:
        check(_bits_and_mask(fc, X, thr, dev), S, mask, "word queue")
    finally:
        monkeypatch.delenv("FC_PAIRQ_CAP")
    _, got = fc.pruner.prune_by_rmsd(X, atoms, thr, dev)  # the one-call host path
    assert np.array_equal(got, mask), f"{what}: prune_by_rmsd"


# ---- (c) k-medoids on the scaled family ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_clumps(name, seeds=16):
    """the family at a cap of 0.25 A, from the first seed whose trajectory the restatement records without a near-tie: the
    sums are made of distances rounded to 2^-32 A (2.3e-10), a few of those apart within a clump, and a clump of even size
    has two medians with equal sums -- 128 queries, or one less -> (X, closed-form rows, queries, reference)"""
    b = dg.scaled_base(name)
    for seed in range(seeds):
        X, a = dg.scaled_family(b, dg.knife_offsets(0.25, 128), seed=4000 + seed)
        R = dg.scaled_rmsd(b, a)
        for q in (128, 127):
            keep = np.append(np.arange(q), 128)
            ref = mr.kmedoids_from_rows(R[np.ix_(keep, keep)], 2)
            if ref.min_gap > GAP:
                return np.ascontiguousarray(X[keep]), R[np.ix_(keep, keep)], q, ref
    return np.ascontiguousarray(X[keep]), R[np.ix_(keep, keep)], q, ref


@pytest.mark.parametrize("name", ["full", "planar", "line"])
def test_kmedoids_on_two_clumps(fc, name):
    """128 queries at 0.25 A on either side of the reference: n = 2 returns one medoid per clump and the clumps' labels"""
    X, R, q, ref = _two_clumps(name)
    assert ref.min_gap > GAP, f"{name}: every trajectory has a near-tie ({ref.min_gap:.3g}): choose other seeds"
    got = fc.pruner.kmedoids_by_rmsd(X, np.array(["C"] * X.shape[1]), 2)
    _assert_kmedoids(got, ref, f"{name} on {q} queries and the reference")
    # the clumps: queries 2 cap apart are on opposite sides of the reference
    far = R[:q, 0] > 0.25
    assert 0 < far.sum() < q and far[got.medoids[0]] != far[got.medoids[1]] and got.medoids.max() < q
    assert np.array_equal(got.labels[:q] != got.labels[0], far)
    assert got.cost < 0.25 + q * 1e-4  # the reference is 0.25 A from its medoid, every query a few 1e-5 A from its own
