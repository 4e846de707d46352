"""Symmetry- and mirror-aware medoids, k-medoids and silhouettes on the GPU (fc_ensemble_medoids_perm,
fc_ensemble_kmedoids_perm, fc_ensemble_silhouette_perm and the Python layers above them) against the NumPy restatement
of their contract (tests/medoid_sym_ref.py) on the oracle's Kabsch RMSD.

The bars are those of test_gpu_medoids.py and test_gpu_silhouette.py, unchanged: BAR = 2.5e-10 A per distance (the
project's 1e-10 plus 2^-33 of quantisation) -- |S - S_ref| <= (s - 1) BAR for a group of s, |E - E_ref| < 1e-10,
|a - a_ref| <= BAR, |b - b_ref| <= BAR, |s - s_ref| <= 4 BAR / max(a, b); medoids, nearest, labels, sizes and n_iter
identical.  Every comparison sits behind the assertion that the restatement's smallest gap exceeds the bar (2 s BAR for
the sums of a group of s, 2 BAR for b, 1e-9 for an assignment), so that rounding cannot flip a decision.  The ensembles
are those of tests/diverse_sym_ref.py: a random half relabelled by a row of the table, a random half reflected where
the flag is tested.  The sums are integers: every "same bits" below is an array_equal.

FC_MEDOID_STRIPS and FC_SILHOUETTE_STRIPS (the plain forms' knobs, which the symmetry-aware kernels reuse) and
FC_MEDOID_SYM_FILTER are read at every call, so the launch-shape tests switch them in this process."""

import ctypes as C

import numpy as np
import pytest

import diverse_sym_ref as ds
import enant_ref as er
import medoid_ref as mr
import medoid_sym_ref as ms
import silhouette_ref as sil
import symm_ref as sr
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 2.5e-10
TOL = 1e-10
GAP = 1e-9
Q = 2.0 ** 32

# (kind, N, A, table, mirror, labels)
CASES = [
    ("clusters", 5, 3, "blocks", True, "one"),
    ("clusters", 40, 5, "path", True, "own"),
    ("continuous", 65, 7, "path", False, "mod7"),
    ("clusters", 100, 13, "blocks", True, "own"),
    ("continuous", 130, 20, "path", True, "mod2"),
    ("continuous", 70, 50, "blocks", False, "mod7"),
    ("clusters", 40, 80, "swaps64", False, "own"),
    ("continuous", 195, 20, "blocks", True, "sizes"),
    ("continuous", 257, 50, "path", True, "mod7"),
]
IDS = ["-".join(map(str, c)) for c in CASES]
THE_CASE = CASES[3]  # the one of the issue's table: 100 x 13, K = 6 with the flag, under its own 20 cluster labels

_CASES = {}  # made once and shared, never written to


def _labels(kind, N, own):
    if kind == "one":
        return None
    if kind == "own":
        return np.asarray(own)
    if kind == "sizes":  # groups of 1, 2, 63, 64 and 65 members, scattered over the ensemble
        return np.repeat(np.arange(5), [1, 2, 63, 64, 65])[np.random.default_rng(3).permutation(195)]
    return np.arange(N) % int(kind[3:])


def _case(kind, N, A, table, mirror, labels="one"):
    key = (kind, N, A, table, mirror)
    if key not in _CASES:
        X, atoms, t, own = ds.ensemble(kind, N, A, table, mirror)
        D = ms.rows(X, atoms, t, mirror)
        for a in (X, D):
            a.setflags(write=False)
        _CASES[key] = (X, atoms, np.ascontiguousarray(t), own, D)
    X, atoms, t, own, D = _CASES[key]
    return X, atoms, t, _labels(labels, N, own), D, dict(symmetry=t, prune_enantiomers=mirror)


def _check_medoids(got, ref, labels, what=""):
    """got: RmsdMedoids (sums in A); ref: the restatement on the same labels (test_gpu_medoids.py's check)"""
    N = len(got.sums)
    labels = np.zeros(N, dtype=np.int64) if labels is None else np.asarray(labels)
    smax = int(ref.sizes.max(initial=1))
    print(f"{what} N={N} groups={len(ref.sizes)} largest={smax} gap={ref.min_gap:.3g} "
          f"max|S - ref|={np.abs(got.sums - ref.sums_q32 / Q).max(initial=0.0):.3g} "
          f"max|E - ref|={np.abs(got.eccentricity - ref.eccentricity).max(initial=0.0):.3g}")
    assert ref.min_gap > 2 * smax * BAR, f"the ensemble has a near-tie ({ref.min_gap:.3g}): choose another"
    assert got.medoids.dtype == np.int64 and got.sizes.dtype == np.int64 and got.sums.dtype == np.float64
    assert np.array_equal(got.medoids, ref.medoids) and np.array_equal(got.sizes, ref.sizes)
    s = np.where(labels >= 0, ref.sizes[np.maximum(labels, 0)], 1)  # each conformer's group size
    assert np.all(np.abs(got.sums - ref.sums_q32 / Q) <= (s - 1) * BAR)
    assert np.all(np.abs(got.eccentricity - ref.eccentricity) < TOL)
    assert np.all(got.sums[s == 1] == 0.0) and np.all(got.eccentricity[s == 1] == 0.0)
    empty = ref.sizes == 0
    assert np.all(np.isnan(got.mean_distance[empty])) and np.all(np.isnan(got.radius[empty]))
    assert np.all(np.abs(got.mean_distance[~empty] - ref.mean_distance[~empty]) <= BAR)
    assert np.all(np.abs(got.radius[~empty] - ref.radius[~empty]) < TOL)
    live = np.flatnonzero(~empty)
    assert np.array_equal(got.radius[live], got.eccentricity[got.medoids[live]])


def _check_silhouette(got, ref, what=""):
    """got: RmsdSilhouette; ref: the restatement on the same labels (test_gpu_silhouette.py's check)"""
    a0, b0, s0 = ref.intra, ref.nearest_mean, ref.values
    lab = ~np.isnan(a0)
    top = np.fmax(a0, b0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s_bar = np.where(top > 0.0, 4 * BAR / top, 0.0)
    both = lab & ~np.isnan(b0)
    print(f"{what} N={len(a0)} groups={len(ref.sizes)} gap={ref.min_gap:.3g} score={ref.score:.6f} "
          f"max|a - ref|={np.abs(got.intra - a0)[lab].max(initial=0.0):.3g} "
          f"max|b - ref|={np.abs(got.nearest_mean - b0)[both].max(initial=0.0):.3g} "
          f"max|s - ref|={np.abs(got.values - s0)[both].max(initial=0.0):.3g} (bar up to {s_bar[both].max(initial=0.0):.3g})")
    assert ref.min_gap > 2 * BAR, f"the ensemble has a near-tie ({ref.min_gap:.3g}): choose another"
    assert got.nearest.dtype == np.int32 and got.sizes.dtype == np.int64 and isinstance(got.score, float)
    assert np.array_equal(got.nearest, ref.nearest) and np.array_equal(got.sizes, ref.sizes)
    for g, r in ((got.intra, a0), (got.nearest_mean, b0), (got.values, s0), (got.cluster_means, ref.cluster_means)):
        assert np.array_equal(np.isnan(g), np.isnan(r))
    assert np.all(np.abs(got.intra - a0)[lab] <= BAR)
    assert np.all(np.abs(got.nearest_mean - b0)[both] <= BAR)
    assert np.all(np.abs(got.values - s0)[both] <= s_bar[both])
    assert np.all(np.abs(got.values[both]) <= 1.0)
    worst = s_bar[both].max(initial=0.0)
    live = ~np.isnan(ref.cluster_means)
    assert np.all(np.abs(got.cluster_means - ref.cluster_means)[live] <= worst)
    assert np.isnan(got.score) if np.isnan(ref.score) else abs(got.score - ref.score) <= worst


def _check_kmedoids(fc, X, atoms, kw, n, got, ref, what=""):
    N = len(X)
    print(f"{what} N={N} n={n} gap={ref.min_gap:.3g} n_iter={ref.n_iter} cost {ref.cost0_q32 / Q:.6f} -> {ref.cost_q32 / Q:.6f}")
    assert ref.min_gap > max(2 * N * BAR, GAP), f"the trajectory has a near-tie ({ref.min_gap:.3g}): choose another"
    assert np.array_equal(got.medoids, ref.medoids) and np.array_equal(got.labels, ref.labels) and got.n_iter == ref.n_iter
    assert got.labels.dtype == np.int32 and got.medoids.dtype == np.int64
    assert np.abs(got.distances - ref.distances).max() < TOL
    # the distances: the k = 1 list of the symmetry-aware cross form against the medoids, bit for bit
    nb = fc.pruner.knn_by_rmsd_against(X, X[got.medoids], atoms, 1, **kw)
    others = np.ones(N, dtype=bool)
    others[got.medoids] = False
    assert np.array_equal(got.distances[others], nb.distances[others, 0]) and np.array_equal(got.labels[others], nb.indices[others, 0])
    assert np.all(got.distances[got.medoids] == 0.0) and np.array_equal(got.labels[got.medoids], np.arange(n))
    cost = int(np.rint(got.distances * Q).astype(np.uint64).astype(object).sum())
    assert got.cost == cost / Q and abs(cost - ref.cost_q32) <= N * BAR * Q
    assert got.cost <= ref.cost0_q32 / Q + N * BAR


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_medoids_sym_parity(fc, case):
    """3 atoms, N that is no multiple of the wavefront or the row tile, more than one tile and chunk, K = 2, 6 and 64,
    with and without the flag; under the case's labels and as one group"""
    X, atoms, t, labels, D, kw = _case(*case)
    for lab in ((labels, None) if labels is not None else (None,)):
        got = fc.pruner.medoids_by_rmsd_sym(X, atoms, lab, **kw)
        _check_medoids(got, ms.medoids(D, lab), lab, str(case))
    if case == THE_CASE:  # the feature does something: the plain call picks other medoids
        plain = fc.pruner.medoids_by_rmsd(X, atoms, labels)
        got = fc.pruner.medoids_by_rmsd_sym(X, atoms, labels, **kw)
        print(f"medoids that differ from the plain call's: {int((plain.medoids != got.medoids).sum())} of {len(got.medoids)}")
        assert (plain.medoids != got.medoids).sum() >= 5 and np.all(got.sums <= plain.sums + 100 * BAR)
        assert got.mean_distance.max() < 0.2 < plain.mean_distance.max()


@pytest.mark.parametrize("case", [c for c in CASES if c[5] != "one"], ids=[i for i, c in zip(IDS, CASES) if c[5] != "one"])
def test_silhouette_sym_parity(fc, case):
    X, atoms, t, labels, D, kw = _case(*case)
    got = fc.pruner.silhouette_by_rmsd_sym(X, atoms, labels, **kw)
    _check_silhouette(got, ms.silhouette(D, labels), str(case))
    one = fc.pruner.silhouette_by_rmsd_sym(X, atoms, None, **kw)  # one group: a only
    _check_silhouette(one, ms.silhouette(D, None), "one group")
    assert np.all(np.isnan(one.values)) and np.all(one.nearest == -1) and np.isnan(one.score)
    if case == THE_CASE:  # the feature does something: a perfect clustering is no longer called bad
        plain = fc.pruner.silhouette_by_rmsd(X, atoms, labels)
        print(f"score under d_sym {got.score:.4f}, under d {plain.score:.4f}; nearest differs for "
              f"{int((plain.nearest != got.nearest).sum())} of {len(X)}")
        assert got.score > 0.9 and plain.score < 0.0 and (plain.nearest != got.nearest).sum() > 50


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kmedoids_sym_parity(fc, case):
    X, atoms, t, _, D, kw = _case(*case)
    N = len(X)
    n = min(5, N)
    ref = ms.kmedoids(D, n)
    got = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, n, **kw)
    _check_kmedoids(fc, X, atoms, kw, n, got, ref, str(case))
    # max_iter = 0 returns the start assigned: the picks of the symmetry-aware diverse selection
    start = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, n, max_iter=0, **kw)
    picks = fc.pruner.select_diverse(X, atoms, n=n, start=0, **kw).indices
    assert np.array_equal(start.medoids, picks) and start.n_iter == 1 and got.cost <= start.cost
    _check_kmedoids(fc, X, atoms, kw, n, start, ms.kmedoids(D, n, max_iter=0), "max_iter=0")
    if case == THE_CASE:
        plain = fc.pruner.kmedoids_by_rmsd(X, atoms, n)
        assert got.cost < plain.cost and not np.array_equal(plain.medoids, got.medoids)


@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
def test_kmedoids_sym_from_a_given_start(fc, case):
    X, atoms, t, _, D, kw = _case(*case)
    N, n = len(X), 5
    init = np.random.default_rng(N + n).permutation(N)[:n]
    given = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, n, init=init, max_iter=0, **kw)
    assert np.array_equal(given.medoids, init)
    _check_kmedoids(fc, X, atoms, kw, n, given, ms.kmedoids(D, n, init=init, max_iter=0), "init")
    moved = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, n, init=init, **kw)
    _check_kmedoids(fc, X, atoms, kw, n, moved, ms.kmedoids(D, n, init=init), "from init")
    assert moved.cost <= given.cost


def test_kmedoids_sym_one_and_all(fc):
    X, atoms, t, _, D, kw = _case(*CASES[2])
    one = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, 1, **kw)
    _check_kmedoids(fc, X, atoms, kw, 1, one, ms.kmedoids(D, 1))
    whole = fc.pruner.medoids_by_rmsd_sym(X, atoms, **kw)
    assert one.medoids.tolist() == [whole.medoids[0]] and np.all(one.labels == 0)
    assert abs(one.cost - whole.sums[whole.medoids[0]]) <= 64 * BAR
    every = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, 65, **kw)
    assert sorted(every.medoids.tolist()) == list(range(65)) and every.cost == 0.0 and every.n_iter == 1
    assert np.array_equal(every.medoids[every.labels], np.arange(65)) and np.all(every.distances == 0.0)


# ---- 2. exact, without the oracle: the same d_sym as the lists, bit for bit -------------------------------------------------
def _matrix_from_lists(ens, N, **kw):
    """D_gpu[i, j] = d_sym(row i, column j) as fc_ensemble_knn_perm lists it (k = N - 1: every pair)"""
    idx, dist = ens.knn(N - 1, **kw)
    D = np.zeros((N, N))
    D[np.arange(N)[:, None], idx] = dist
    return D


def _planar(N, A, seed):
    """planar conformers (z = 0 before a random rotation): a conformer and its mirror image coincide, so both
    handednesses tie for every pair"""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, A, 3))
    X[:, :, :2] = rng.normal(scale=1.5, size=(1, A, 2)) + rng.normal(scale=0.4, size=(N, A, 2))
    R = np.linalg.qr(rng.normal(size=(N, 3, 3)))[0]
    return np.ascontiguousarray(np.einsum("nac,ndc->nad", X, R))


@pytest.mark.parametrize("which", ["5-blocks-mirror", "40-path-mirror", "65-path", "40x80-swaps64", "planar-mirror", "mirror-only"])
def test_sums_are_those_of_the_lists_bit_for_bit(fc, which):
    if which == "planar-mirror":
        X, t, mirror = _planar(33, 9, 5), ds.table("path", 9), True
    elif which == "mirror-only":
        X, t, mirror = np.array(_case(*CASES[2])[0]), None, True
    else:
        case = {"5-blocks-mirror": CASES[0], "40-path-mirror": CASES[1], "65-path": CASES[2], "40x80-swaps64": CASES[6]}[which]
        X, _, t, _, _, _ = _case(*case)
        mirror = case[4]
    N = len(X)
    kw = dict(symmetry=t, prune_enantiomers=mirror)
    for labels in (None, np.arange(N) % 3, np.arange(N) % 7 if N > 7 else np.array([0, 0, 1, 1, 1])):
        with fc.DeviceEnsemble(X, center=True) as ens:
            D = _matrix_from_lists(ens, N, **kw)
            med = ens.medoids_sym(labels, **kw)
            got = ens.silhouette_sym(labels, **kw)
        ref = mr.medoids_from_rows(D, labels)
        assert np.array_equal(med[4], ref.sums_q32) and np.array_equal(med[5], ref.eccentricity)
        assert np.array_equal(med[0], ref.medoids)
        rs = sil.silhouette_from_rows(D, labels)
        assert np.array_equal(got[1], rs.intra, equal_nan=True) and np.array_equal(got[2], rs.nearest_mean, equal_nan=True)
        assert np.array_equal(got[3], rs.nearest) and np.array_equal(got[0], rs.values, equal_nan=True)
        assert got[6] == rs.score or (np.isnan(got[6]) and np.isnan(rs.score))
    if which == "planar-mirror":  # (both handednesses of every pair tie to rounding: the oracle could not carry this case)
        with fc.DeviceEnsemble(X, center=True) as ens:
            assert np.abs(_matrix_from_lists(ens, N, symmetry=t) - D).max() < 1e-7


# ---- 3. launch shapes ----------------------------------------------------------------------------------------------------
_SHAPES = (("1", None), ("3", None), ("7", None), (None, None), (None, "0"), ("3", "0"))


def _under(monkeypatch, strips, flt):
    for name, value in (("FC_MEDOID_STRIPS", strips), ("FC_SILHOUETTE_STRIPS", strips), ("FC_MEDOID_SYM_FILTER", flt)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def test_independent_of_the_launch_shape_and_the_filter(fc, monkeypatch):
    """one group of 400 of 600 conformers (10 chunks) plus small ones, K = 2 with the flag: the same bits under 1, 3, 7
    and the default strips, and with the explicit pass for every (p, h)"""
    X, atoms, t, _ = ds.ensemble("continuous", 600, 20, "path", True)
    sizes = [400, 1, 2, 63, 64, 70]
    labels = np.repeat(np.arange(len(sizes)), sizes)[np.random.default_rng(8).permutation(600)]
    kw = dict(symmetry=t, prune_enantiomers=True)
    runs, counts = [], []
    with fc.DeviceEnsemble(X, center=True) as ens:
        for strips, flt in _SHAPES:
            _under(monkeypatch, strips, flt)
            m = ens.medoids_sym(labels, want_ms=True, **kw)
            s = ens.silhouette_sym(labels, want_ms=True, **kw)
            k = ens.kmedoids_sym(4, max_iter=2, **kw)
            runs.append(m[:6] + s[:7] + k)
            counts.append((m[7], s[8]))
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a, b, equal_nan=True)
    assert runs[0][4].max() > 0 and runs[0][1].tolist() == sizes
    # the counters: all four (p, h) of every counting pair are formed; without the filter all of them go on
    pairs_tri = sum(s * (s - 1) // 2 for s in sizes)
    for (fm, fs), (strips, flt) in zip(counts, _SHAPES):
        assert fm[0] == 4 * pairs_tri and fs[0] == 4 * 600 * 599
        if flt == "0":
            assert fm[1] == fm[0] and fs[1] == fs[0]
        else:
            assert pairs_tri <= fm[1] <= fm[0] and 600 * 599 <= fs[1] <= fs[0]  # (a pair's first (p, h) is always explicit)
    print(f"explicit of formed: medoids {counts[3][0][1] / counts[3][0][0]:.3f}, silhouettes {counts[3][1][1] / counts[3][1][0]:.3f}")


# ---- 4. layout edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[10, 60, 125], [64, 64, 67]], ids=str)
def test_group_across_a_tile_and_a_chunk(fc, sizes):
    X, atoms, t, _, D, kw = _case(*CASES[7])
    labels = np.repeat(np.arange(3), sizes)
    _check_medoids(fc.pruner.medoids_by_rmsd_sym(X, atoms, labels, **kw), ms.medoids(D, labels), labels, str(sizes))
    _check_silhouette(fc.pruner.silhouette_by_rmsd_sym(X, atoms, labels, **kw), ms.silhouette(D, labels), str(sizes))


def test_unlabelled_conformers_and_empty_groups(fc):
    X, atoms, t, _, D, kw = _case(*CASES[8])
    labels = np.arange(257) % 6
    labels[labels == 2] = -1
    labels[labels == 4] = 7
    labels[5] = -9  # (any negative label)
    got = fc.pruner.medoids_by_rmsd_sym(X, atoms, labels, **kw)
    _check_medoids(got, ms.medoids(D, labels), labels)
    assert got.medoids[[2, 4, 6]].tolist() == [-1, -1, -1] and np.all(got.sums[labels < 0] == 0.0) and len(got.medoids) == 8
    s = fc.pruner.silhouette_by_rmsd_sym(X, atoms, labels, **kw)
    _check_silhouette(s, ms.silhouette(D, labels))
    assert np.all(np.isnan(s.values[labels < 0])) and np.all(s.nearest[labels < 0] == -1) and s.sizes[[2, 4, 6]].tolist() == [0, 0, 0]


@pytest.mark.parametrize("N", [1, 2, 3])
def test_tiny_ensembles(fc, N):
    X0, atoms, t, _ = ds.ensemble("continuous", 3, 7, "path", True)
    X = X0[:N]
    kw = dict(symmetry=t, prune_enantiomers=True)
    D = ms.rows(X, atoms, t, True)
    got = fc.pruner.medoids_by_rmsd_sym(X, atoms, **kw)
    _check_medoids(got, ms.medoids(D), None)
    assert got.sizes.tolist() == [N]
    if N == 1:
        assert got.sums.tolist() == [0.0] and got.mean_distance.tolist() == [0.0] and got.radius.tolist() == [0.0]
    if N == 2:
        assert got.sums[0] == got.sums[1] > 0.0 and got.medoids[0] == 0
    labels = np.arange(N) % 2
    _check_silhouette(fc.pruner.silhouette_by_rmsd_sym(X, atoms, labels, **kw), ms.silhouette(D, labels))
    km = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, 1, **kw)
    assert km.medoids.tolist() == [got.medoids[0]] and km.n_iter >= 1


def test_twins(fc):
    """a relabelled and reflected bitwise copy of one conformer: d_sym <= 1e-7, and as a group of two the pair ties
    exactly in S and goes to the lower index"""
    A = 13
    X, atoms, t = np.array(syn.continuous_ensemble(20, A, seed=21)), np.array(["C"] * A), ds.table("blocks", A)
    X[17] = er.reflect(X[4][t[3]][None], np.arange(1), axis=1)[0]
    kw = dict(symmetry=t, prune_enantiomers=True)
    labels = np.where(np.isin(np.arange(20), (4, 17)), 1, 0)
    with fc.DeviceEnsemble(X, center=True) as ens:
        med, sizes, mean, radius, sums, ecc = ens.medoids_sym(labels, **kw)
        s = ens.silhouette_sym(labels, **kw)
        plain = ens.medoids(labels)
    assert sizes.tolist() == [18, 2] and med[1] == 4 and sums[4] == sums[17] and ecc[4] == ecc[17] == radius[1] <= 1e-7
    assert sums[4] <= 1e-7 * Q and mean[1] <= 1e-7 and plain[4][4] > 1e-3 * Q
    assert s[1][4] <= 1e-7 and s[1][17] <= 1e-7 and s[0][4] > 0.99 and s[0][17] > 0.99  # a ~ 0: a perfect pair
    whole = fc.pruner.medoids_by_rmsd_sym(X, atoms, **kw)  # in one group the twins' sums agree within the bar
    assert abs(whole.sums[4] - whole.sums[17]) <= 19 * BAR + 2e-7


@pytest.mark.parametrize("mirror", [False, True])
def test_the_largest_admitted_shape(fc, mirror):
    """K = 64 at the most selected atoms the LDS admits (320: 160 KiB less 512 bytes), 20 conformers"""
    A = S.medoid_max_selected(64)
    assert A == 320 and S.medoid_lds_bytes(64, A) <= 160 * 1024 < S.medoid_lds_bytes(64, A + 1)
    rng = np.random.default_rng(11)
    X = rng.normal(scale=4.0, size=(1, A, 3)) + rng.normal(scale=0.3, size=(20, A, 3)) * rng.uniform(0.2, 1.0, size=(20, 1, 1))
    atoms, t = np.array(["C"] * A), sr.transposition_table(A, 6)
    assert len(t) == 64
    Y, _ = sr.relabel_half(X, t, 3)
    Y = np.ascontiguousarray(er.reflect(Y, np.arange(20) % 2 == 0) if mirror else Y)
    kw = dict(symmetry=t, prune_enantiomers=mirror)
    D = ms.rows(Y, atoms, t, mirror)
    labels = np.arange(20) % 2
    _check_medoids(fc.pruner.medoids_by_rmsd_sym(Y, atoms, labels, **kw), ms.medoids(D, labels), labels)
    _check_silhouette(fc.pruner.silhouette_by_rmsd_sym(Y, atoms, labels, **kw), ms.silhouette(D, labels))
    with pytest.raises(fc.FirecodeHipInputError, match="LDS"):
        fc.pruner.medoids_by_rmsd_sym(np.zeros((2, A + 1, 3)), np.array(["C"] * (A + 1)), symmetry=sr.transposition_table(A + 1, 6))


def test_identity_table_without_the_flag_is_the_default(fc):
    """K = 1, mirror = 0: the default's kernels, bit for bit; so is the call with neither keyword"""
    X, atoms, _, labels, _, _ = _case(*CASES[7])
    ident = np.arange(len(atoms))[None]
    for kw in (dict(symmetry=ident), dict()):
        for a, b in zip(fc.pruner.medoids_by_rmsd_sym(X, atoms, labels, **kw), fc.pruner.medoids_by_rmsd(X, atoms, labels)):
            assert np.array_equal(a, b, equal_nan=True)
        for a, b in zip(fc.pruner.silhouette_by_rmsd_sym(X, atoms, labels, **kw), fc.pruner.silhouette_by_rmsd(X, atoms, labels)):
            assert np.array_equal(a, b, equal_nan=True)
        for a, b in zip(fc.pruner.kmedoids_by_rmsd_sym(X, atoms, 5, **kw), fc.pruner.kmedoids_by_rmsd(X, atoms, 5)):
            assert np.array_equal(a, b)
    with fc.DeviceEnsemble(X, center=True) as ens:
        out = ens.medoids_sym(labels, symmetry=ident, want_ms=True)
        assert out[7] == (0, 0) and np.array_equal(out[4], ens.medoids(labels)[4])


def test_refusals_with_a_live_handle(fc):
    """behind the table's checks the plain twins' own, in their order; an A_sel that is not the ensemble's"""
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=1)
    lib = fc._lib.load()
    t32 = np.ascontiguousarray(sr.path_table(6), dtype=np.int32)
    tp = fc._lib.ptr(t32, C.c_int32)
    out = [np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(4), np.zeros(4)]
    ptrs = (fc._lib.pi(out[0]), fc._lib.pi(out[1]), fc._lib.pf(out[2]), fc._lib.pf(out[3]))
    lab = np.zeros(12, dtype=np.int32)
    lab[7] = 3
    lp = lab.ctypes.data_as(C.POINTER(C.c_int32))
    with fc.DeviceEnsemble(X, center=True) as ens:
        med = lambda *a: lib.fc_ensemble_medoids_perm(ens.handle, tp, 2, 6, 1, *a, None, None, None, None)  # noqa: E731
        assert med(lp, 3, *ptrs) == fc._lib.FC_E_INVALID and b"labels[7]" in lib.fc_last_error()
        assert med(lp, 0, *ptrs) == fc._lib.FC_E_INVALID and b"n_groups=0" in lib.fc_last_error()
        assert med(None, 2, ptrs[0], None, ptrs[2], ptrs[3]) == fc._lib.FC_E_INVALID and b"sizes_out" in lib.fc_last_error()
        t5 = np.ascontiguousarray(sr.path_table(5), dtype=np.int32)
        rc = lib.fc_ensemble_medoids_perm(ens.handle, fc._lib.ptr(t5, C.c_int32), 2, 5, 0, None, 1, *ptrs, None, None, None, None)
        assert rc == fc._lib.FC_E_INVALID and b"A_sel=5" in lib.fc_last_error()
        cost, n_iter, dist = C.c_uint64(0), C.c_int64(0), np.zeros(12)
        km = lambda init, n: lib.fc_ensemble_kmedoids_perm(ens.handle, tp, 2, 6, 0, init, n, 5, ptrs[0], lp, fc._lib.pf(dist),  # noqa: E731
                                                           C.byref(cost), C.byref(n_iter))
        assert km(None, 13) == fc._lib.FC_E_INVALID and b"n=13" in lib.fc_last_error()
        i64 = np.array([0, 12, 3], dtype=np.int64)
        assert km(fc._lib.pi(i64), 3) == fc._lib.FC_E_INVALID and b"init[1]" in lib.fc_last_error()
        score = C.c_double(0)
        f = [np.zeros(12) for _ in range(3)]
        rc = lib.fc_ensemble_silhouette_perm(ens.handle, tp, 2, 6, 1, lp, 3, *(fc._lib.pf(v) for v in f), lp, ptrs[2], ptrs[0],
                                             C.byref(score), None, None)
        assert rc == fc._lib.FC_E_INVALID and b"labels[7]" in lib.fc_last_error()
    assert not any(o.any() for o in out)
    with fc.DeviceEnsemble(X * 1e12, center=True) as far:  # a group too large for the 64-bit sum: FC_E_LIMIT, as the plain twin
        with pytest.raises(fc.FirecodeHipInputError) as err:
            far.medoids_sym(prune_enantiomers=True)
        assert err.value.code == fc._lib.FC_E_LIMIT


# ---- 5. the Python layers ------------------------------------------------------------------------------------------------
def test_scan_sym_against_separate_calls(fc):
    """the 100 x 13 ensemble over three thresholds with method="butina": the scan passes the keyword to the clusterer and
    to the silhouette of each step -- the scores of separate calls, bit for bit -- under the table and under the flag"""
    X, atoms, t, own, D, _ = _case(*THE_CASE)
    ts = [0.3, 0.6, 2.5]
    for kw in (dict(symmetry=t), dict(prune_enantiomers=True)):
        recs = fc.pruner.silhouette_scan_sym(X, atoms, ts, method="butina", **kw)
        scores = []
        for thr in ts:
            cl = fc.pruner.butina_by_rmsd(X, atoms, thr, **kw)
            scores.append(fc.pruner.silhouette_by_rmsd_sym(X, atoms, cl.labels, **kw).score)
        assert np.array_equal([r.score for r in recs], scores, equal_nan=True)
        assert [r.max_rmsd for r in recs] == ts and all(r.n_noise == 0 for r in recs)
    # neither keyword: silhouette_scan itself
    a, b = fc.pruner.silhouette_scan_sym(X, atoms, ts[:2]), fc.pruner.silhouette_scan(X, atoms, ts[:2])
    assert [tuple(r) for r in a] == [tuple(r) for r in b] or np.array_equal(np.array(a), np.array(b), equal_nan=True)
    # the other two clusterers, under the flag (min_samples = 2: the reflected halves alone leave no denser cores)
    kw = dict(prune_enantiomers=True)
    for method, cluster in (("components", lambda thr: fc.pruner.cluster_by_rmsd(X, atoms, thr, **kw)),
                            ("dbscan", lambda thr: fc.pruner.dbscan_by_rmsd(X, atoms, thr, min_samples=2, **kw))):
        recs = fc.pruner.silhouette_scan_sym(X, atoms, ts[:2], method=method, min_samples=2, **kw)
        for r, thr in zip(recs, ts):
            cl = cluster(thr)
            assert r.n_clusters == len(cl.sizes) >= 2 and r.n_noise == int((np.asarray(cl.labels) < 0).sum())
            assert r.score == fc.pruner.silhouette_by_rmsd_sym(X, atoms, cl.labels, **kw).score


def test_ensemble_and_most_diverse_layers(fc):
    X, atoms, t, own, D, kw = _case(*THE_CASE)
    ref = fc.pruner.kmedoids_by_rmsd_sym(X, atoms, 5, **kw)
    energies = np.arange(100, dtype=np.float64)
    log = []
    ens = fc.ensemble.Ensemble(atoms=atoms, coords=np.array(X), energies=energies, logfunction=log.append)
    assert np.array_equal(ens.medoids_sym(own, **kw).medoids, fc.pruner.medoids_by_rmsd_sym(X, atoms, own, **kw).medoids)
    assert ens.silhouette_sym(own, **kw).score == fc.pruner.silhouette_by_rmsd_sym(X, atoms, own, **kw).score
    assert len(ens.coords) == 100
    sel = ens.kmedoids_selection_sym(5, **kw)
    assert np.array_equal(sel.medoids, ref.medoids) and np.array_equal(ens.coords, X[ref.medoids])
    assert np.array_equal(ens.energies, energies[ref.medoids]) and "symmetry-aware RMSD medoids" in log[-1]
    md = fc.torsion_module.most_diverse_conformers(5, list(X), method="kmedoids_sym", atoms=atoms, **kw)
    assert np.array_equal(np.array(md), X[ref.medoids])
    plain = fc.torsion_module.most_diverse_conformers(5, list(X), method="kmedoids_sym", atoms=atoms)
    assert np.array_equal(np.array(plain), X[fc.pruner.kmedoids_by_rmsd(X, atoms, 5).medoids])
    assert len(fc.torsion_module.most_diverse_conformers(300, list(X[:30]), method="kmedoids_sym", **kw)) == 30
    with fc.DeviceEnsemble(X, center=True) as dev:
        med, lab, dist, cost_q32, n_iter = dev.kmedoids_sym(5, **kw)
    assert np.array_equal(med, ref.medoids) and isinstance(cost_q32, int) and cost_q32 / Q == ref.cost and n_iter == ref.n_iter
