"""Silhouettes under the RMSD without a device: the NumPy restatement of the contract (tests/silhouette_ref.py) against a
brute-force triple loop on 12 conformers and against the textbook formula on a hand-made distance matrix, every refusal
that is made before any device use -- through the Python layers and through the raw C entry point with a NULL handle:
the code and the argument named -- the ``_lib`` signature and the refusal of the keywords this feature does not have."""

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import firecode_amd as fc
import silhouette_ref as sr
from firecode_amd import _lib as L
from firecode_amd import synthetic as syn
from firecode_amd.ensemble import Ensemble
from firecode_amd.pruner import RmsdSilhouette, SilhouetteScanRecord, silhouette_by_rmsd, silhouette_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 2.0 ** 32


# ---- the restatement
@pytest.fixture(scope="module")
def twelve():
    X, atoms, _ = syn.synthetic_ensemble(12, 6, seed=5)
    return sr.distance_rows(sr.prepared(X, atoms))


def _brute(D, labels, n_groups):
    """the contract by a triple loop: conformer, group, member"""
    N = len(D)
    live = [g for g in range(n_groups) if any(labels[j] == g for j in range(N))]
    a, b, s, nearest = [np.nan] * N, [np.nan] * N, [np.nan] * N, [-1] * N
    for i in range(N):
        if labels[i] < 0:
            continue
        best = None
        for g in live:
            T, size = 0, 0
            for j in range(N):
                if labels[j] == g:
                    size += 1
                    if j != i:
                        T += int(np.rint(D[i, j] * Q))
            if g == labels[i]:
                own_size = size
                a[i] = float(T) / Q / (size - 1) if size > 1 else 0.0
            elif best is None or float(T) / Q / size < best[0]:
                best = (float(T) / Q / size, g)
        if len(live) >= 2:
            b[i], nearest[i] = best
            top = max(a[i], b[i])
            s[i] = 0.0 if own_size == 1 or top == 0.0 else (b[i] - a[i]) / top
    return a, b, s, nearest


@pytest.mark.parametrize("labels,n_groups", [
    (None, None),                                       # one group: b, s, score NaN
    ([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], None),
    ([0, 0, 0, 0, 0, 3, 3, -1, 1, -1, 3, 0], 5),       # a singleton, unlabelled conformers, two empty ids
    ([1, 0] + [2] * 10, None),                          # singletons in front
    (list(range(12)), None),                            # all singletons
    ([-1] * 12, 2),                                     # nobody labelled
])
def test_restatement_against_brute_force(twelve, labels, n_groups):
    D = twelve
    assert not np.array_equal(D, D.T)  # (the rows are used as they are: row i, column j)
    ref = sr.silhouette_from_rows(D, labels, n_groups)
    lab = [0] * 12 if labels is None else labels
    G = len(ref.sizes)
    assert G == (n_groups or max(max(lab) + 1, 1))
    a, b, s, nearest = _brute(D, lab, G)
    assert np.array_equal(ref.intra, a, equal_nan=True) and np.array_equal(ref.nearest_mean, b, equal_nan=True)
    assert np.array_equal(ref.values, s, equal_nan=True) and ref.nearest.tolist() == nearest and ref.nearest.dtype == np.int32
    labelled = [i for i in range(12) if lab[i] >= 0]
    for c in range(G):
        mem = [i for i in range(12) if lab[i] == c]
        assert ref.sizes[c] == len(mem)
        if not mem:
            assert np.isnan(ref.cluster_means[c])
        else:
            assert np.array_equal(ref.cluster_means[c], sum([s[i] for i in mem], 0.0) / len(mem), equal_nan=True)
    if labelled:
        assert np.array_equal(ref.score, sum([s[i] for i in labelled], 0.0) / len(labelled), equal_nan=True)
    else:
        assert np.isnan(ref.score)
    if len({c for c in lab if c >= 0}) < 2:
        assert np.isnan(ref.values).all() and np.isnan(ref.score) and (ref.nearest == -1).all() and ref.min_gap == np.inf
    else:
        assert np.all(np.abs(ref.values[labelled]) <= 1.0) and ref.min_gap > 0.0


def test_restatement_against_the_textbook_formula():
    rng = np.random.default_rng(11)
    D = rng.uniform(0.5, 3.0, size=(11, 11))
    D = (D + D.T) / 2
    np.fill_diagonal(D, 0.0)
    D[8, 9] = D[9, 8] = 0.0                     # an all-zero twin pair in a group of its own
    D[8, :8] = D[9, :8] = D[:8, 8] = D[:8, 9] = 2.0
    D[8, 10] = D[9, 10] = D[10, 8] = D[10, 9] = 2.0
    dense = np.array([0, 0, 0, 1, 1, 1, 1, 2, 3, 3, 0])  # 2: a singleton
    s0, a0, b0 = sr.textbook_from_matrix(D, dense)
    ref = sr.silhouette_from_rows(D, dense)
    assert np.abs(ref.intra - a0).max() < 2.0 ** -32 and np.abs(ref.nearest_mean - b0).max() < 2.0 ** -32
    assert np.abs(ref.values - s0).max() < 1e-8
    assert ref.values[7] == 0.0 and ref.intra[7] == 0.0 and ref.nearest_mean[7] > 0.0  # the singleton
    assert ref.intra[8] == ref.intra[9] == 0.0 and ref.values[8] == ref.values[9] == 1.0
    assert ref.score == pytest.approx(s0.mean(), abs=1e-8) and ref.cluster_means[1] == pytest.approx(s0[3:7].mean(), abs=1e-8)
    # an empty group id in the middle and at the end, unlabelled conformers: the same figures for the rest
    spread = np.array([0, 0, 0, 2, 2, 2, 2, 3, 5, 5, 0, -1, -4])
    D2 = np.full((13, 13), 7.0)
    D2[:11, :11] = D
    got = sr.silhouette_from_rows(D2, spread, 8)
    assert np.array_equal(got.values[:11], ref.values) and np.array_equal(got.intra[:11], ref.intra)
    assert np.array_equal(got.nearest[:11], np.array([0, 2, 3, 5])[ref.nearest]) and got.sizes.tolist() == [4, 0, 4, 1, 0, 2, 0, 0]
    assert np.isnan(got.values[11:]).all() and np.isnan(got.intra[11:]).all() and got.nearest[11:].tolist() == [-1, -1]
    assert np.isnan(got.cluster_means[[1, 4, 6, 7]]).all() and got.score == ref.score
    # max(a, b) == 0: twins in two different groups and nothing else
    Z = np.zeros((2, 2))
    two = sr.silhouette_from_rows(Z, [0, 1])
    assert two.values.tolist() == [0.0, 0.0] and two.nearest.tolist() == [1, 0] and two.score == 0.0
    pair = sr.silhouette_from_rows(np.zeros((4, 4)), [0, 0, 1, 1])
    assert pair.values.tolist() == [0.0] * 4 and pair.nearest_mean.tolist() == [0.0] * 4
    # a single non-empty group: a is still given
    one = sr.silhouette_from_rows(D, np.full(11, 2), 4)
    assert np.isnan(one.values).all() and np.isnan(one.nearest_mean).all() and (one.nearest == -1).all() and np.isnan(one.score)
    assert np.abs(one.intra - D.sum(axis=1) / 10).max() < 2.0 ** -32 and one.sizes.tolist() == [0, 0, 11, 0]
    assert np.isnan(one.cluster_means).all()
    # ties go to the lowest label, and the recorded gap is that of the closest decision
    T = np.array([[0.0, 1.0, 1.0, 1.5], [1.0, 0.0, 9.0, 9.0], [1.0, 9.0, 0.0, 9.0], [1.5, 9.0, 9.0, 0.0]])
    tie = sr.silhouette_from_rows(T, [3, 2, 1, 0])
    assert tie.nearest[0] == 1 and tie.min_gap == 0.0
    assert sr.silhouette_from_rows(T, [3, 2, 2, 0]).min_gap == pytest.approx(0.5)


# ---- refusals before any device use: the Python layers
X5, AT = np.zeros((6, 5, 3)), ["C"] * 5


@pytest.mark.parametrize("kwargs,name", [
    (dict(labels=[0, 1, 2]), "labels"),                          # not one per conformer
    (dict(labels=np.zeros((6, 1), dtype=int)), "labels"),
    (dict(labels=[0.0] * 6), "labels"),                          # not integers
    (dict(labels=[True] * 6), "labels"),
    (dict(structures=np.zeros((6, 5, 2))), "structures"),
    (dict(atoms=["C"] * 4), "atoms"),
    (dict(atoms=["H"] * 5), "atom selection"),
])
def test_silhouette_refuses_before_device_use(kwargs, name):
    args = dict(structures=X5, atoms=AT, labels=[0, 0, 0, 1, 1, 1])
    args.update(kwargs)
    with pytest.raises(fc.FirecodeHipInputError) as err:
        silhouette_by_rmsd(**args)
    assert err.value.code == L.FC_E_INVALID and name in str(err.value)
    with pytest.raises(fc.FirecodeHipInputError) as err:
        Ensemble.silhouette(SimpleNamespace(coords=args["structures"], atoms=args["atoms"]), args["labels"])
    assert err.value.code == L.FC_E_INVALID and name in str(err.value)


@pytest.mark.parametrize("kwargs,name", [
    (dict(labels=[0, 3], n_groups=3), "n_groups"),               # a label that is not below n_groups
    (dict(labels=[0, 1], n_groups=0), "n_groups"),
    (dict(labels=None, n_groups=-2), "n_groups"),
    (dict(labels=[0, 1], n_groups=2.0), "n_groups"),
    (dict(labels=[0, 1, 1]), "labels"),
    (dict(labels=[0.5, 1.0]), "labels"),
])
def test_device_ensemble_silhouette_refuses_before_device_use(kwargs, name):
    with pytest.raises(fc.FirecodeHipInputError) as err:
        L.DeviceEnsemble.silhouette(SimpleNamespace(N=2), **kwargs)  # (refused before the handle is looked at)
    assert err.value.code == L.FC_E_INVALID and name in str(err.value)


@pytest.mark.parametrize("kwargs,name", [
    (dict(method="pam"), "method"),
    (dict(thresholds=[[0.3, 0.5]]), "thresholds"),
    (dict(thresholds=[0.3, -0.5]), "max_rmsd"),
    (dict(thresholds=[0.3, 0.0]), "max_rmsd"),
    (dict(method="dbscan", min_samples=0), "min_samples"),
    (dict(structures=np.zeros((6, 5))), "structures"),
    (dict(atoms=["H"] * 5), "atom selection"),
])
def test_silhouette_scan_refuses_before_device_use(kwargs, name):
    args = dict(structures=X5, atoms=AT, thresholds=[0.3, 0.5])
    args.update(kwargs)
    with pytest.raises(fc.FirecodeHipInputError) as err:
        silhouette_scan(**args)
    assert err.value.code == L.FC_E_INVALID and name in str(err.value)


def test_no_symmetry_or_mirror_form():
    for call in (lambda **kw: silhouette_by_rmsd(X5, AT, [0] * 6, **kw), lambda **kw: silhouette_scan(X5, AT, [0.5], **kw),
                 lambda **kw: L.DeviceEnsemble.silhouette(None, **kw), lambda **kw: Ensemble.silhouette(None, [0] * 6, **kw)):
        for kw in (dict(symmetry=np.arange(5)[None]), dict(prune_enantiomers=True)):
            with pytest.raises(TypeError):
                call(**kw)


def test_empty_ensembles_need_no_device():
    none = np.zeros((0, 5, 3))
    r = silhouette_by_rmsd(none, AT, None)
    assert isinstance(r, RmsdSilhouette) and r.values.shape == r.intra.shape == r.nearest_mean.shape == (0,)
    assert r.nearest.dtype == np.int32 and r.nearest.shape == (0,) and r.sizes.tolist() == [0] and r.sizes.dtype == np.int64
    assert np.isnan(r.cluster_means).all() and np.isnan(r.score)
    e = Ensemble(atoms=np.array(AT), coords=none, logfunction=None)
    assert np.isnan(e.silhouette(np.zeros(0, dtype=int)).score)
    recs = silhouette_scan(none, AT, [0.25, 0.5])
    assert [tuple(x)[:3] for x in recs] == [(0.25, 0, 0), (0.5, 0, 0)] and all(np.isnan(x.score) for x in recs)
    assert isinstance(recs[0], SilhouetteScanRecord)


# ---- the raw C entry point with a NULL handle
def test_c_entry_point_refuses_before_device_use():
    lib = L.load()
    f64 = [np.zeros(4) for _ in range(4)]
    near, lab = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
    sizes, score = np.zeros(4, dtype=np.int64), C.c_double(0)
    p32 = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731

    def refused(rc, name):
        assert rc == L.FC_E_INVALID and name.encode() in lib.fc_last_error(), (rc, lib.fc_last_error())

    outs = (L.pf(f64[0]), L.pf(f64[1]), L.pf(f64[2]), p32(near), L.pf(f64[3]), L.pi(sizes), C.byref(score))
    refused(lib.fc_ensemble_silhouette(None, p32(lab), 2, *outs, None), "ens")
    refused(lib.fc_ensemble_silhouette(None, p32(lab), 0, *outs, None), "n_groups")   # the scalar is judged first
    refused(lib.fc_ensemble_silhouette(None, None, -1, *outs, None), "n_groups")
    refused(lib.fc_ensemble_silhouette(None, None, 2 ** 31, *outs, None), "n_groups")
    refused(lib.fc_ensemble_silhouette(None, None, 2, None, None, None, None, None, None, None, None), "ens")
    refused(lib.fc_ensemble_silhouette(None, None, 0, None, None, None, None, None, None, None, None), "n_groups")
    assert not any(a.any() for a in f64) and not near.any() and not sizes.any() and score.value == 0.0


def test_no_cpu_fallback():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    X, atoms, own = syn.synthetic_ensemble(12, 6, seed=1)
    with pytest.raises(fc.FirecodeHipDeviceError):
        silhouette_by_rmsd(X, atoms, own)
    with pytest.raises(fc.FirecodeHipDeviceError):
        silhouette_scan(X, atoms, [0.5])


def test_symbol_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "fc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    p32, ens = C.POINTER(C.c_int32), C.c_void_p
    name = "fc_ensemble_silhouette"
    argtypes = [ens, p32, L._i64, L._p_f64, L._p_f64, L._p_f64, p32, L._p_f64, L._p_i64, L._p_f64, L._p_f64]
    assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/fc_hip.h"
    assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert L._SIGNATURES[name] == argtypes and getattr(lib, name).argtypes == argtypes
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert len(decl.split(",")) == len(argtypes)
    for layer, attr in ((fc.DeviceEnsemble, "silhouette"), (fc.pruner, "silhouette_by_rmsd"), (fc.pruner, "silhouette_scan"),
                        (Ensemble, "silhouette")):
        assert callable(getattr(layer, attr))
    assert RmsdSilhouette._fields == ("values", "intra", "nearest_mean", "nearest", "cluster_means", "sizes", "score")
    assert SilhouetteScanRecord._fields == ("max_rmsd", "n_clusters", "n_noise", "score")
