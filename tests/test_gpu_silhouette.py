"""Silhouettes under the RMSD on the GPU (fc_ensemble_silhouette and the Python layers above it) against the NumPy
restatement of their contract (tests/silhouette_ref.py) on the oracle's Kabsch RMSD.

Bars, derived, not measured.  BAR = 2.5e-10 A is the per-distance bar of the medoid sums: the
project's 1e-10 per distance plus 2^-33 of quantisation.  a and b are means of distances: |a - a_ref| <= BAR and
|b - b_ref| <= BAR.  s = (b - a) / max(a, b) moves by at most 2 BAR / max(a, b) to first order; with a factor 2 of room
|s - s_ref| <= 4 BAR / max(a_ref, b_ref).  nearest and sizes are identical; score and cluster_means, means of s, stay
within the largest per-conformer bar.  Every comparison comes behind ``assert ref.min_gap > 2 * BAR``: the smallest
difference between the two closest other groups of any row, the only decision rounding could flip.  The sums are
integers: every "same bits" below is an array_equal."""

import ctypes as C

import numpy as np
import pytest

import silhouette_ref as sr
from firecode_amd import synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 2.5e-10

_ROWS = {}  # the oracle's rows of an ensemble, computed once and shared by the cases that need them


def _ensemble(kind, N, A, seed):
    if kind == "clusters":
        return syn.synthetic_ensemble(N, A, seed=seed)
    return syn.continuous_ensemble(N, A, seed=seed), np.array(["C"] * A), None


def _rows(key, Xsel):
    if key not in _ROWS:
        D = sr.distance_rows(Xsel)
        D.setflags(write=False)
        _ROWS[key] = D
    return _ROWS[key]


def _case(kind, N, A):
    X, atoms, own = _ensemble(kind, N, A, seed=N + A)
    return X, atoms, own, _rows((kind, N, A), sr.prepared(X, atoms))


def _check(got, ref, what=""):
    """got: RmsdSilhouette; ref: the restatement on the same labels"""
    a0, b0, s0 = ref.intra, ref.nearest_mean, ref.values
    lab = ~np.isnan(a0)
    top = np.fmax(a0, b0)  # (b is NaN with fewer than two non-empty groups: then s is NaN on both sides)
    with np.errstate(divide="ignore", invalid="ignore"):
        s_bar = np.where(top > 0.0, 4 * BAR / top, 0.0)
    both = lab & ~np.isnan(b0)
    print(f"{what} N={len(a0)} groups={len(ref.sizes)} gap={ref.min_gap:.3g} score={ref.score:.6f} "
          f"max|a - ref|={np.abs(got.intra - a0)[lab].max(initial=0.0):.3g} "
          f"max|b - ref|={np.abs(got.nearest_mean - b0)[both].max(initial=0.0):.3g} "
          f"max|s - ref|={np.abs(got.values - s0)[both].max(initial=0.0):.3g} (bar up to {s_bar[both].max(initial=0.0):.3g})")
    assert ref.min_gap > 2 * BAR, f"the ensemble has a near-tie ({ref.min_gap:.3g}): choose another"
    assert got.values.dtype == got.intra.dtype == got.nearest_mean.dtype == np.float64
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


# ---- 1. parity
@pytest.mark.parametrize("grouping", ["own", "mod7", "mod2"])
@pytest.mark.parametrize("N,A", [(40, 5), (65, 7), (257, 50), (600, 80)])
def test_silhouette_parity(fc, N, A, grouping):
    """the clustered ensemble under its own cluster labels, the continuous one with interleaved labels i % 7 and i % 2
    (the sort); N that is no multiple of the wavefront or the row tile, 5, 7, 50 and 80 atoms"""
    X, atoms, own, D = _case("clusters" if grouping == "own" else "continuous", N, A)
    labels = own if grouping == "own" else np.arange(N) % (7 if grouping == "mod7" else 2)
    _check(fc.pruner.silhouette_by_rmsd(X, atoms, labels), sr.silhouette_from_rows(D, labels), grouping)


# ---- 2. the scan and the carry
def test_silhouette_group_sizes_around_the_wavefront(fc):
    """groups of 1, 2, 63, 64 and 65 members, scattered over the ensemble: in the sorted copy the group of 64 starts at
    column 66 and ends in the next chunk, and the group of 65 spans the whole third chunk"""
    X, atoms, _, D = _case("continuous", 195, 20)
    labels = np.repeat(np.arange(5), [1, 2, 63, 64, 65])[np.random.default_rng(3).permutation(195)]
    got = fc.pruner.silhouette_by_rmsd(X, atoms, labels)
    _check(got, sr.silhouette_from_rows(D, labels))
    assert got.sizes.tolist() == [1, 2, 63, 64, 65]
    single = np.flatnonzero(labels == 0)[0]
    assert got.values[single] == 0.0 and got.intra[single] == 0.0 and got.nearest_mean[single] > 0.0


def test_silhouette_group_across_a_tile_and_a_chunk(fc):
    """sorted positions 10 ... 69 are one group: it straddles the 16-row tiles and the 64-column chunk; positions
    0 ... 63 and 64 ... 127: two groups that each fill a chunk exactly"""
    X, atoms, _, D = _case("continuous", 195, 20)
    for sizes in ([10, 60, 125], [64, 64, 67]):
        labels = np.repeat(np.arange(3), sizes)
        _check(fc.pruner.silhouette_by_rmsd(X, atoms, labels), sr.silhouette_from_rows(D, labels), str(sizes))


# ---- 3. launch shapes
def test_silhouette_independent_of_the_launch_shape(fc, monkeypatch):
    """one group of 400 of 600 conformers (10 chunks) plus small ones: under 3, 7 and 10 strips it is cut by several strip
    boundaries and holds strips that lie wholly inside it"""
    X, atoms, _, D = _case("continuous", 600, 80)
    labels = np.repeat(np.arange(5), [400, 50, 30, 100, 20])[np.random.default_rng(5).permutation(600)]
    runs = []
    for strips in ("1", "3", "7", None):
        if strips is None:
            monkeypatch.delenv("FC_SILHOUETTE_STRIPS", raising=False)
        else:
            monkeypatch.setenv("FC_SILHOUETTE_STRIPS", strips)
        runs.append(fc.pruner.silhouette_by_rmsd(X, atoms, labels))
    for r in runs[1:]:
        assert np.array_equal(r.intra, runs[0].intra) and np.array_equal(r.nearest_mean, runs[0].nearest_mean)
        assert np.array_equal(r.nearest, runs[0].nearest) and np.array_equal(r.values, runs[0].values)
        assert r.score == runs[0].score
    _check(runs[0], sr.silhouette_from_rows(D, labels))


# ---- 4. all singletons: the cross-check against the k-NN kernel
def test_silhouette_of_singletons_is_the_nearest_neighbour(fc):
    X, atoms, _ = _ensemble("continuous", 130, 20, seed=150)
    got = fc.pruner.silhouette_by_rmsd(X, atoms, np.arange(130))
    nb = fc.pruner.knn_by_rmsd(X, atoms, 1)
    assert np.all(got.values == 0.0) and np.all(got.intra == 0.0) and got.score == 0.0
    assert np.array_equal(got.nearest, nb.indices[:, 0])
    assert np.all(np.abs(got.nearest_mean - nb.distances[:, 0]) <= 2.0 ** -33)
    assert got.sizes.tolist() == [1] * 130 and np.all(got.cluster_means == 0.0)


# ---- 5. two groups
def test_silhouette_of_two_groups(fc):
    X, atoms, _, D = _case("continuous", 195, 20)
    labels = (np.random.default_rng(8).random(195) < 0.3).astype(np.int64)
    got = fc.pruner.silhouette_by_rmsd(X, atoms, labels)
    ref = sr.silhouette_from_rows(D, labels)
    assert ref.min_gap == np.inf  # (no row has two other groups: nothing to decide)
    _check(got, ref)
    assert np.array_equal(got.nearest, 1 - labels)


# ---- 6. one non-empty group
def test_silhouette_of_one_group(fc):
    X, atoms, _, D = _case("continuous", 257, 50)
    sums = fc.pruner.medoids_by_rmsd(X, atoms).sums
    for labels, n_groups in ((None, None), (np.full(257, 2), 4)):
        with fc.DeviceEnsemble(X, center=True) as ens:
            got = fc.pruner.RmsdSilhouette(*ens.silhouette(labels, n_groups))
        _check(got, sr.silhouette_from_rows(D, labels, n_groups))
        assert np.isnan(got.nearest_mean).all() and np.isnan(got.values).all() and np.isnan(got.score)
        assert np.all(got.nearest == -1) and np.all(got.intra > 0.0)
        # the medoids' S: one evaluation per unordered pair there, the full square here
        assert np.all(np.abs(got.intra * 256 - sums) <= 256 * BAR)
    assert got.sizes.tolist() == [0, 0, 257, 0] and np.isnan(got.cluster_means).all()


# ---- 7. unlabelled conformers and empty group ids
def test_silhouette_unlabelled_conformers_and_empty_groups(fc):
    """-1 (a DBSCAN result's noise) and any other negative label; empty group ids in the middle and at the end"""
    X, atoms, _, D = _case("continuous", 257, 50)
    labels = np.arange(257) % 6
    labels[labels == 2] = -1
    labels[labels == 4] = 7
    labels[5] = -9
    got = fc.pruner.silhouette_by_rmsd(X, atoms, labels)
    _check(got, sr.silhouette_from_rows(D, labels))
    out = labels < 0
    assert np.isnan(got.values[out]).all() and np.isnan(got.intra[out]).all() and np.isnan(got.nearest_mean[out]).all()
    assert np.all(got.nearest[out] == -1) and not np.isin(got.nearest[~out], [-1, 2, 4, 6]).any()
    assert len(got.sizes) == 8 and got.sizes[[2, 4, 6]].tolist() == [0, 0, 0] and np.isnan(got.cluster_means[[2, 4, 6]]).all()
    with fc.DeviceEnsemble(X, center=True) as ens:  # a given n_groups: trailing empty ids
        wide = fc.pruner.RmsdSilhouette(*ens.silhouette(labels, n_groups=11))
    _check(wide, sr.silhouette_from_rows(D, labels, 11))
    assert np.array_equal(wide.values, got.values, equal_nan=True) and wide.score == got.score


# ---- 8. rows from global memory
def test_silhouette_beyond_the_lds_stage(fc):
    """40 conformers of 300 selected atoms: the row conformers no longer fit the kernel's LDS stage"""
    rng = np.random.default_rng(7)
    X = rng.normal(scale=4.0, size=(1, 300, 3)) + rng.normal(scale=0.3, size=(40, 300, 3)) * rng.uniform(0.2, 1.0, size=(40, 1, 1))
    atoms = np.array(["C"] * 300)
    labels = np.arange(40) % 3
    _check(fc.pruner.silhouette_by_rmsd(X, atoms, labels), sr.silhouette_from_rows(_rows("wide", X), labels))


# ---- 9. twins
def test_silhouette_of_twins(fc):
    """bitwise copies: two of them as a group of their own (a = 0, b > 0: s = 1); one inside a larger group beside its
    original (the same bits in a and b: their rows are the same instruction sequence on the same numbers, and the one
    distance that differs, to the twin, is below the unit of q); four copies of one far-off conformer as two groups of
    two, whose a and b are all 0: max(a, b) == 0 gives s = 0, and nearest is the other group of twins.  (Those two groups
    tie exactly for every other row, by construction; they are far off so that they are never a row's two nearest, the
    decision the gap condition is about.)"""
    X0 = syn.continuous_ensemble(40, 20, seed=60)
    far = X0[7] + np.random.default_rng(61).normal(scale=3.0, size=X0[7].shape)
    X = np.concatenate([X0, X0[[0, 0, 3]], np.stack([far] * 4)])  # 40, 41: copies of 0; 42: of 3; 43 ... 46: the far one
    atoms = np.array(["C"] * 20)
    labels = np.concatenate([np.repeat([1, 2], 20), [0, 0, 1, 3, 3, 4, 4]])
    got = fc.pruner.silhouette_by_rmsd(X, atoms, labels)
    ref = sr.silhouette_from_rows(_rows("twins", X), labels)
    assert np.all(ref.intra[[40, 41, 43, 44, 45, 46]] == 0.0) and np.all(ref.nearest_mean[43:] == 0.0)  # (the oracle's twins)
    _check(got, ref)
    assert np.all(got.intra[[40, 41]] == 0.0) and np.all(got.nearest_mean[[40, 41]] > 0.0) and np.all(got.values[[40, 41]] == 1.0)
    assert got.intra[42] == got.intra[3] and got.nearest_mean[42] == got.nearest_mean[3] and got.values[42] == got.values[3]
    assert np.all(got.intra[43:] == 0.0) and np.all(got.nearest_mean[43:] == 0.0) and np.all(got.values[43:] == 0.0)
    assert got.nearest[43:].tolist() == [4, 4, 3, 3]


# ---- 10. tiny ensembles
@pytest.mark.parametrize("N", [1, 2, 3])
def test_silhouette_of_tiny_ensembles(fc, N):
    X, atoms, _, D = _case("continuous", N, 5)
    for labels in (None, np.arange(N), np.arange(N) // 2):
        got = fc.pruner.silhouette_by_rmsd(X, atoms, labels)
        _check(got, sr.silhouette_from_rows(D, labels), str(labels))
    if N == 1:
        assert got.intra.tolist() == [0.0] and np.isnan(got.values[0]) and got.nearest.tolist() == [-1] and np.isnan(got.score)
    if N == 3:  # groups {0, 1} and {2}
        assert got.nearest.tolist() == [1, 1, 0] and got.values[2] == 0.0 and got.sizes.tolist() == [2, 1]


# ---- 11. the clusterers' labels, and the layers
def test_silhouette_from_the_clusterers(fc):
    """the labels of the four clusterers as they come (DBSCAN's -1 is noise); all layers agree"""
    X, atoms, _, D = _case("clusters", 257, 50)
    for result in (fc.pruner.cluster_by_rmsd(X, atoms, 0.5), fc.pruner.dbscan_by_rmsd(X, atoms, 0.5, min_samples=6),
                   fc.pruner.butina_by_rmsd(X, atoms, 0.5), fc.pruner.kmedoids_by_rmsd(X, atoms, 40)):
        got = fc.pruner.silhouette_by_rmsd(X, atoms, result.labels)
        _check(got, sr.silhouette_from_rows(D, result.labels), type(result).__name__)
        with fc.DeviceEnsemble(X, center=True) as dev:
            low = dev.silhouette(result.labels)
        high = fc.ensemble.Ensemble(atoms=atoms, coords=X, logfunction=None).silhouette(result.labels)
        for x, y, z in zip(got, low, high):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)
        if hasattr(result, "sizes"):
            assert np.array_equal(got.sizes, np.asarray(result.sizes)[:len(got.sizes)])


# ---- 12. what the number means
def test_silhouette_tells_a_good_labelling_from_a_bad_one(fc):
    """the restatement gives 0.943 under the generator's own clusters and -0.031 under i % 7"""
    X, atoms, own, D = _case("clusters", 257, 50)
    good = fc.pruner.silhouette_by_rmsd(X, atoms, own)
    bad = fc.pruner.silhouette_by_rmsd(X, atoms, np.arange(257) % 7)
    print(f"own clusters {good.score:.4f}, i % 7 {bad.score:.4f}")
    assert good.score > 0.9 and bad.score < 0.1
    assert abs(good.score - sr.silhouette_from_rows(D, own).score) < 1e-6


# ---- 13. the scan
def test_silhouette_scan(fc):
    X, atoms, own, _ = _case("clusters", 257, 50)
    thresholds = [0.04, 0.09, 0.5, 1.6]
    recs = fc.pruner.silhouette_scan(X, atoms, thresholds)
    assert [r.max_rmsd for r in recs] == thresholds
    for r in recs:
        bu = fc.pruner.butina_by_rmsd(X, atoms, r.max_rmsd)
        score = fc.pruner.silhouette_by_rmsd(X, atoms, bu.labels).score
        print(r, score)
        assert r.n_clusters == len(bu.sizes) and r.n_noise == 0 and np.array_equal(r.score, score, equal_nan=True)
    best = recs[int(np.nanargmax([r.score for r in recs]))]
    assert best.n_clusters in (51, 52) and best.score > 0.9
    for method, separate in (("components", lambda t: fc.pruner.cluster_by_rmsd(X, atoms, t)),
                             ("dbscan", lambda t: fc.pruner.dbscan_by_rmsd(X, atoms, t, min_samples=6))):
        (r,) = fc.pruner.silhouette_scan(X, atoms, [0.5], method=method, min_samples=6)
        res = separate(0.5)
        assert r.n_clusters == len(res.sizes) and r.n_noise == int((res.labels < 0).sum())
        assert np.array_equal(r.score, fc.pruner.silhouette_by_rmsd(X, atoms, res.labels).score, equal_nan=True)


# ---- 14. refusals
def test_silhouette_refusals_with_a_live_handle(fc):
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=1)
    lib = fc._lib.load()
    f64 = [np.zeros(12) for _ in range(3)] + [np.zeros(4)]
    near, sizes, score = np.zeros(12, dtype=np.int32), np.zeros(4, dtype=np.int64), C.c_double(0)
    p32 = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    outs = [fc._lib.pf(f64[0]), fc._lib.pf(f64[1]), fc._lib.pf(f64[2]), p32(near), fc._lib.pf(f64[3]), fc._lib.pi(sizes),
            C.byref(score)]
    lab = np.zeros(12, dtype=np.int32)
    lab[7] = 3
    with fc.DeviceEnsemble(X, center=True) as ens:
        assert lib.fc_ensemble_silhouette(ens.handle, p32(lab), 3, *outs, None) == fc._lib.FC_E_INVALID
        assert b"labels[7]" in lib.fc_last_error()
        assert lib.fc_ensemble_silhouette(ens.handle, p32(lab), 0, *outs, None) == fc._lib.FC_E_INVALID
        assert b"n_groups" in lib.fc_last_error()
        for k in range(7):
            holed = outs[:k] + [None] + outs[k + 1:]
            assert lib.fc_ensemble_silhouette(ens.handle, None, 2, *holed, None) == fc._lib.FC_E_INVALID
            assert b"s_out" in lib.fc_last_error()
        for bad in (dict(labels=np.full(12, 4), n_groups=4), dict(labels=np.zeros(11, dtype=int)), dict(n_groups=0)):
            with pytest.raises(fc.FirecodeHipInputError):
                ens.silhouette(**bad)
    assert not any(a.any() for a in f64) and not near.any() and not sizes.any() and score.value == 0.0
    # too many labelled conformers for the 64-bit prefix over a row, judged once the ensemble's largest G is known
    with fc.DeviceEnsemble(X * 1e12, center=True) as far:
        for labels in (None, np.arange(12) % 3, np.arange(12)):
            with pytest.raises(fc.FirecodeHipInputError) as err:
                far.silhouette(labels)
            assert err.value.code == fc._lib.FC_E_LIMIT
        one = np.full(12, -1)
        one[4] = 0
        assert far.silhouette(one)[1][4] == 0.0  # (a single labelled conformer: no pair, no device, nothing to overflow)


def test_silhouette_refuses_a_stale_handle(fc):
    X, atoms, own = syn.synthetic_ensemble(12, 6, seed=1)
    old = fc.DeviceEnsemble(X, center=True)
    before = old.silhouette(own)
    assert np.isfinite(before[6])
    fc._lib.shutdown()
    fc._lib.init(0)
    with pytest.raises(fc.FirecodeHipInputError) as err:
        old.silhouette(own)
    assert err.value.code == fc._lib.FC_E_INVALID and "fc_shutdown" in str(err.value)
    old.close()
    with fc.DeviceEnsemble(X, center=True) as ens:
        assert ens.silhouette(own)[6] == before[6]
