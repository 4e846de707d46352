"""Cluster medoids and k-medoids under the RMSD on the GPU (fc_ensemble_medoids, fc_ensemble_kmedoids, fc_ensemble_subset
and the Python layers above them) against the NumPy restatement of their contract (tests/medoid_ref.py) on the oracle's
Kabsch RMSD.

Bars, where s is a group's size: |S - S_ref| <= (s - 1) * 2.5e-10 A (the project's 1e-10 per distance plus 2^-33 of
quantisation), |E - E_ref| < 1e-10, medoids, sizes and labels identical -- on ensembles whose every decision (the
second-smallest against the smallest sum of a group of three or more; the second-nearest against the nearest medoid of a
row; two costs of the alternation) the restatement recorded with a gap above 2 * s * 2.5e-10, so that rounding cannot
flip one.  Integer sums: every "same bits" below is an array_equal."""

import ctypes as C

import numpy as np
import pytest

import medoid_ref as mr
from firecode_amd import synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 2.5e-10
TOL = 1e-10
Q = 2.0 ** 32

_ROWS = {}  # the oracle's rows of an ensemble, computed once and shared by the cases that need them


def _ensemble(kind, N, A, seed):
    if kind == "clusters":
        return syn.synthetic_ensemble(N, A, seed=seed)
    return syn.continuous_ensemble(N, A, seed=seed), np.array(["C"] * A), None


def _rows(key, Xsel):
    if key not in _ROWS:
        D = mr.distance_rows(Xsel)
        D.setflags(write=False)
        _ROWS[key] = D
    return _ROWS[key]


def _case(kind, N, A):
    X, atoms, own = _ensemble(kind, N, A, seed=N + A)
    return X, atoms, own, _rows((kind, N, A), mr.prepared(X, atoms))


def _check(got, ref, labels, what=""):
    """got: RmsdMedoids (sums in A); ref: the restatement on the same labels"""
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
    # the per-group figures are those of the medoid
    live = np.flatnonzero(~empty)
    assert np.array_equal(got.radius[live], got.eccentricity[got.medoids[live]])
    assert np.array_equal(got.mean_distance[live],
                          np.where(ref.sizes[live] > 1, got.sums[got.medoids[live]] / np.maximum(ref.sizes[live] - 1, 1), 0.0))


# ---- the sums kernel
@pytest.mark.parametrize("grouping", ["own", "one", "mod7"])
@pytest.mark.parametrize("N,A", [(40, 5), (65, 7), (257, 50), (600, 80)])
def test_medoids_parity(fc, N, A, grouping):
    """the clustered ensemble under its own cluster labels, the continuous one as one group and with interleaved labels
    i % 7 (the sort); N that is no multiple of the wavefront or the row tile, 5, 7, 50 and 80 atoms"""
    X, atoms, own, D = _case("clusters" if grouping == "own" else "continuous", N, A)
    labels = own if grouping == "own" else None if grouping == "one" else np.arange(N) % 7
    got = fc.pruner.medoids_by_rmsd(X, atoms, labels)
    _check(got, mr.medoids_from_rows(D, labels), labels, grouping)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_medoids_of_tiny_ensembles(fc, N):
    X, atoms, _, D = _case("continuous", N, 5)
    got = fc.pruner.medoids_by_rmsd(X, atoms)
    _check(got, mr.medoids_from_rows(D), None)
    assert got.medoids.tolist() == [mr.medoids_from_rows(D).medoids[0]] and got.sizes.tolist() == [N]
    if N == 1:
        assert got.sums.tolist() == [0.0] and got.mean_distance.tolist() == [0.0] and got.radius.tolist() == [0.0]
    if N == 2:
        assert got.sums[0] == got.sums[1] > 0.0 and got.medoids[0] == 0


def test_medoids_group_sizes_around_the_wavefront(fc):
    """groups of 1, 2, 63, 64 and 65 members in one ensemble; the two-member group: equal integer sums, the lower index"""
    X, atoms, _, D = _case("continuous", 195, 20)
    labels = np.repeat(np.arange(5), [1, 2, 63, 64, 65])
    perm = np.random.default_rng(3).permutation(195)  # (scattered over the ensemble)
    labels = labels[perm]
    with fc.DeviceEnsemble(X, atom_mask=None, center=True) as ens:
        med, sizes, mean, radius, sums, ecc = ens.medoids(labels)
    got = fc.pruner.medoids_by_rmsd(X, atoms, labels)
    assert sums.dtype == np.uint64 and np.array_equal(sums.astype(np.float64) / Q, got.sums) and np.array_equal(med, got.medoids)
    _check(got, mr.medoids_from_rows(D, labels), labels)
    assert sizes.tolist() == [1, 2, 63, 64, 65]
    pair = np.flatnonzero(labels == 1)
    assert sums[pair[0]] == sums[pair[1]] > 0 and med[1] == pair[0] and ecc[pair[0]] == ecc[pair[1]] == radius[1]
    assert sums[np.flatnonzero(labels == 0)[0]] == 0 and mean[0] == 0.0


def test_medoids_group_across_a_tile_and_a_chunk(fc):
    """sorted positions 10 ... 69 are one group: it straddles the 16-row tiles and the 64-column chunk"""
    X, atoms, _, D = _case("continuous", 195, 20)
    labels = np.repeat(np.arange(3), [10, 60, 125])
    got = fc.pruner.medoids_by_rmsd(X, atoms, labels)
    _check(got, mr.medoids_from_rows(D, labels), labels)


def test_medoids_unlabelled_conformers_and_empty_groups(fc):
    X, atoms, _, D = _case("continuous", 257, 50)
    labels = np.arange(257) % 6
    labels[labels == 2] = -1
    labels[labels == 4] = 7
    labels[5] = -9  # (any negative label)
    got = fc.pruner.medoids_by_rmsd(X, atoms, labels)
    ref = mr.medoids_from_rows(D, labels)
    _check(got, ref, labels)
    assert got.medoids[[2, 4, 6]].tolist() == [-1, -1, -1] and got.sizes[[2, 4, 6]].tolist() == [0, 0, 0]
    assert np.all(got.sums[labels < 0] == 0.0) and len(got.medoids) == 8
    with fc.DeviceEnsemble(X, center=True) as ens:  # a given n_groups: trailing empty ids
        med = ens.medoids(labels, n_groups=11)[0]
    assert np.array_equal(med[:8], ref.medoids) and med[8:].tolist() == [-1, -1, -1]


def test_medoids_beyond_the_lds_stage(fc):
    """300 conformers of 300 selected atoms: the row conformers no longer fit the kernel's LDS stage"""
    rng = np.random.default_rng(7)
    X = rng.normal(scale=4.0, size=(1, 300, 3)) + rng.normal(scale=0.3, size=(300, 300, 3)) * rng.uniform(0.2, 1.0, size=(300, 1, 1))
    atoms = np.array(["C"] * 300)
    D = _rows("wide", X)
    for labels in (None, np.arange(300) % 3):
        _check(fc.pruner.medoids_by_rmsd(X, atoms, labels), mr.medoids_from_rows(D, labels), labels)


def test_medoids_of_twins(fc):
    """every conformer twice, bitwise: the medoid is one of the twin pair of the restatement's, and the twins' sums agree
    within the bar (their rows and columns change places, so not in the last bits)"""
    X0 = syn.continuous_ensemble(40, 20, seed=60)
    X = np.concatenate([X0, X0])
    atoms = np.array(["C"] * 20)
    ref = mr.medoids_from_rows(_rows("twins", X))
    srt = np.sort(ref.sums_q32)
    assert float(srt[2] - srt[0]) / Q > 2 * 80 * BAR  # the best pair of twins against the next one
    got = fc.pruner.medoids_by_rmsd(X, atoms)
    assert got.medoids[0] % 40 == ref.medoids[0] % 40 and got.sizes.tolist() == [80]
    assert np.all(np.abs(got.sums - ref.sums_q32 / Q) <= 79 * BAR)
    assert np.all(np.abs(got.sums[:40] - got.sums[40:]) <= 79 * BAR)
    assert np.all(np.abs(got.eccentricity - ref.eccentricity) < TOL)


def test_medoids_independent_of_the_launch_shape(fc, monkeypatch):
    X, atoms, _, D = _case("continuous", 600, 80)
    runs = []
    for labels in (None, np.arange(600) % 7):
        for strips in ("1", "3", "7", None):
            if strips is None:
                monkeypatch.delenv("FC_MEDOID_STRIPS", raising=False)
            else:
                monkeypatch.setenv("FC_MEDOID_STRIPS", strips)
            runs.append(fc.pruner.medoids_by_rmsd(X, atoms, labels))
        for m in runs[1:]:
            assert np.array_equal(m.sums, runs[0].sums) and np.array_equal(m.eccentricity, runs[0].eccentricity)
            assert np.array_equal(m.medoids, runs[0].medoids)
        assert runs[0].sums.max() > 0.0
        runs.clear()


def test_medoids_from_the_clusterers(fc):
    """the labels of the three clusterers as they come (DBSCAN's -1 is noise), and the Ensemble layer"""
    X, atoms, _, D = _case("clusters", 257, 50)
    for result in (fc.pruner.cluster_by_rmsd(X, atoms, 0.5), fc.pruner.dbscan_by_rmsd(X, atoms, 0.5, min_samples=5),
                   fc.pruner.butina_by_rmsd(X, atoms, 0.5)):
        got = fc.pruner.medoids_by_rmsd(X, atoms, result.labels)
        _check(got, mr.medoids_from_rows(D, result.labels), result.labels, type(result).__name__)
        assert np.array_equal(got.sizes, np.asarray(result.sizes)[:len(got.sizes)])
    ens = fc.ensemble.Ensemble(atoms=atoms, coords=X, logfunction=None)
    assert np.array_equal(ens.medoids(result.labels).medoids, got.medoids) and len(ens.coords) == 257


def test_medoids_refusals_with_a_live_handle(fc):
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=1)
    lib = fc._lib.load()
    out = [np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(4), np.zeros(4)]
    ptrs = (fc._lib.pi(out[0]), fc._lib.pi(out[1]), fc._lib.pf(out[2]), fc._lib.pf(out[3]))
    lab = np.zeros(12, dtype=np.int32)
    lab[7] = 3
    with fc.DeviceEnsemble(X, center=True) as ens:
        rc = lib.fc_ensemble_medoids(ens.handle, lab.ctypes.data_as(C.POINTER(C.c_int32)), 3, *ptrs, None, None, None)
        assert rc == fc._lib.FC_E_INVALID and b"labels[7]" in lib.fc_last_error()
        assert lib.fc_ensemble_medoids(ens.handle, None, 2, ptrs[0], None, ptrs[2], ptrs[3], None, None, None) == fc._lib.FC_E_INVALID
        assert b"sizes_out" in lib.fc_last_error()
        i64 = np.array([0, 12, 3], dtype=np.int64)
        cost, n_iter, sub = C.c_uint64(0), C.c_int64(0), C.c_void_p()
        dist = np.zeros(12)
        km = lambda init, n: lib.fc_ensemble_kmedoids(ens.handle, init, n, 5, ptrs[0], lab.ctypes.data_as(C.POINTER(C.c_int32)),  # noqa: E731
                                                      fc._lib.pf(dist), C.byref(cost), C.byref(n_iter))
        assert km(None, 13) == fc._lib.FC_E_INVALID and b"n=13" in lib.fc_last_error()
        assert km(fc._lib.pi(i64), 3) == fc._lib.FC_E_INVALID and b"init[1]" in lib.fc_last_error()
        i64[1] = 0
        assert km(fc._lib.pi(i64), 3) == fc._lib.FC_E_INVALID and b"repeated" in lib.fc_last_error()
        i64[1] = -1
        assert lib.fc_ensemble_subset(ens.handle, fc._lib.pi(i64), 3, C.byref(sub)) == fc._lib.FC_E_INVALID
        assert b"indices[1]" in lib.fc_last_error() and not sub.value
        for bad in (dict(labels=np.full(12, 4), n_groups=4), dict(labels=np.zeros(11, dtype=int)), dict(n_groups=0)):
            with pytest.raises(fc.FirecodeHipInputError):
                ens.medoids(**bad)
        for bad in (dict(n=0), dict(n=13), dict(n=2, max_iter=-1), dict(n=2, init=[0, 12]), dict(n=2, init=[4, 4])):
            with pytest.raises(fc.FirecodeHipInputError):
                ens.kmedoids(**bad)
        with pytest.raises(fc.FirecodeHipInputError):
            ens.subset([0, 12])
    assert not any(o.any() for o in out)
    # a group too large for the 64-bit sum, judged once the ensemble's largest G is known: FC_E_LIMIT
    with fc.DeviceEnsemble(X * 1e12, center=True) as far:
        with pytest.raises(fc.FirecodeHipInputError) as err:
            far.medoids()
        assert err.value.code == fc._lib.FC_E_LIMIT
        with pytest.raises(fc.FirecodeHipInputError) as err:
            far.kmedoids(2)
        assert err.value.code == fc._lib.FC_E_LIMIT
        assert far.medoids(np.arange(12))[0].tolist() == list(range(12))  # (singletons sum nothing)


# ---- the subset
def test_subset_keeps_the_bits(fc):
    X, atoms, _ = _ensemble("continuous", 257, 50, seed=307)
    idx = np.array([256, 0, 13, 13, 200, 64, 63, 65, 1], dtype=np.int64)
    pi_, pj_ = np.triu_indices(len(idx), 1)
    with fc.DeviceEnsemble(X, center=True) as ens:
        with ens.subset(idx) as sub:
            assert sub.N == len(idx) and sub.A_all == 50
            r, m = sub.rmsd_pairs(pi_, pj_)
            r0, m0 = ens.rmsd_pairs(idx[pi_], idx[pj_])
            assert np.array_equal(r, r0) and np.array_equal(m, m0)
            with sub.subset([4, 0]) as two:  # a subset of the subset
                assert np.array_equal(two.rmsd_pairs([0], [1])[0], ens.rmsd_pairs([200], [256])[0])
        with ens.subset(np.zeros(0, dtype=np.int64)) as none:
            assert none.N == 0 and none.knn(1)[0].shape == (0, 1)
        whole = ens.subset(np.arange(257))
        assert np.array_equal(whole.knn(3)[1], ens.knn(3)[1])
        assert np.array_equal(ens.knn_against(ens, 2)[1], whole.knn_against(whole, 2)[1])
        whole.close()


# ---- k-medoids
def _check_kmedoids(fc, X, atoms, D, n, got, ref, what=""):
    N = len(X)
    print(f"{what} N={N} n={n} gap={ref.min_gap:.3g} n_iter={ref.n_iter} cost {ref.cost0_q32 / Q:.6f} -> {ref.cost_q32 / Q:.6f}")
    assert ref.min_gap > 2 * N * BAR, f"the trajectory has a near-tie ({ref.min_gap:.3g}): choose another"
    assert np.array_equal(got.medoids, ref.medoids) and np.array_equal(got.labels, ref.labels) and got.n_iter == ref.n_iter
    assert got.labels.dtype == np.int32 and got.medoids.dtype == np.int64
    assert np.abs(got.distances - ref.distances).max() < TOL
    # the distances: the k = 1 list against the medoids, bit for bit, except the medoids' own zeros
    nb = fc.pruner.knn_by_rmsd_against(X, X[got.medoids], atoms, 1)
    others = np.ones(N, dtype=bool)
    others[got.medoids] = False
    assert np.array_equal(got.distances[others], nb.distances[others, 0]) and np.array_equal(got.labels[others], nb.indices[others, 0])
    assert np.all(got.distances[got.medoids] == 0.0) and np.array_equal(got.labels[got.medoids], np.arange(n))
    cost = int(np.rint(got.distances * Q).astype(np.uint64).astype(object).sum())
    assert got.cost == cost / Q and abs(cost - ref.cost_q32) <= N * BAR * Q
    assert got.cost <= ref.cost0_q32 / Q + N * BAR


@pytest.mark.parametrize("kind,N,A,n", [("clusters", 257, 50, 51), ("clusters", 257, 50, 20), ("continuous", 600, 80, 10),
                                        ("continuous", 300, 20, 25), ("clusters", 65, 7, 4)])
def test_kmedoids_parity(fc, kind, N, A, n):
    X, atoms, _, D = _case(kind, N, A)
    ref = mr.kmedoids_from_rows(D, n)
    got = fc.pruner.kmedoids_by_rmsd(X, atoms, n)
    _check_kmedoids(fc, X, atoms, D, n, got, ref, kind)
    # the cost is no greater than that of the initial picks, which max_iter = 0 returns assigned
    start = fc.pruner.kmedoids_by_rmsd(X, atoms, n, max_iter=0)
    picks = fc.pruner.select_diverse(X, atoms, n=n, start=0).indices
    assert np.array_equal(start.medoids, picks) and start.n_iter == 1 and got.cost <= start.cost
    _check_kmedoids(fc, X, atoms, D, n, start, mr.kmedoids_from_rows(D, n, max_iter=0), "max_iter=0")
    # a given init is honoured
    init = np.random.default_rng(N + n).permutation(N)[:n]
    given = fc.pruner.kmedoids_by_rmsd(X, atoms, n, init=init, max_iter=0)
    assert np.array_equal(given.medoids, init)
    _check_kmedoids(fc, X, atoms, D, n, given, mr.kmedoids_from_rows(D, n, init=init, max_iter=0), "init")
    moved = fc.pruner.kmedoids_by_rmsd(X, atoms, n, init=init)
    _check_kmedoids(fc, X, atoms, D, n, moved, mr.kmedoids_from_rows(D, n, init=init), "from init")
    assert moved.cost <= given.cost


def test_kmedoids_one_and_all(fc):
    X, atoms, _, D = _case("clusters", 65, 7)
    one = fc.pruner.kmedoids_by_rmsd(X, atoms, 1)
    _check_kmedoids(fc, X, atoms, D, 1, one, mr.kmedoids_from_rows(D, 1))
    whole = fc.pruner.medoids_by_rmsd(X, atoms)
    assert one.medoids.tolist() == [whole.medoids[0]] and np.all(one.labels == 0)
    assert abs(one.cost - whole.sums[whole.medoids[0]]) <= 64 * BAR
    every = fc.pruner.kmedoids_by_rmsd(X, atoms, 65)
    assert sorted(every.medoids.tolist()) == list(range(65)) and every.cost == 0.0 and every.n_iter == 1
    assert np.array_equal(every.medoids[every.labels], np.arange(65)) and np.all(every.distances == 0.0)


def test_kmedoids_python_layers(fc):
    X, atoms, _, D = _case("clusters", 257, 50)
    ref = fc.pruner.kmedoids_by_rmsd(X, atoms, 20)
    energies = np.arange(257, dtype=np.float64)
    log = []
    ens = fc.ensemble.Ensemble(atoms=atoms, coords=X.copy(), energies=energies, logfunction=log.append)
    sel = ens.kmedoids_selection(20)
    assert np.array_equal(sel.medoids, ref.medoids) and np.array_equal(ens.coords, X[ref.medoids])
    assert np.array_equal(ens.energies, energies[ref.medoids]) and "RMSD medoids" in log[-1]
    md = fc.torsion_module.most_diverse_conformers(20, list(X), method="kmedoids", atoms=atoms)
    assert np.array_equal(np.array(md), X[ref.medoids])
    md_all = fc.torsion_module.most_diverse_conformers(20, list(X), method="kmedoids")  # all atoms: the same here (all "C")
    assert np.array_equal(np.array(md_all), X[ref.medoids])
    assert len(fc.torsion_module.most_diverse_conformers(300, list(X[:30]), method="kmedoids")) == 30
    with fc.DeviceEnsemble(X, center=True) as dev:
        med, lab, dist, cost_q32, n_iter = dev.kmedoids(20)
    assert np.array_equal(med, ref.medoids) and isinstance(cost_q32, int) and cost_q32 / Q == ref.cost and n_iter == ref.n_iter
