"""RMSD-diverse selection without a device: argument checks before any device use, no CPU fallback, the
reference's random draw unchanged, and the NumPy restatement of the contract (tests/diverse_ref.py) checked
against the properties of greedy max-min selection."""

import numpy as np
import pytest

import firecode_amd as fc
from diverse_ref import brute_force_k_center, prepared, rmsd_row, select_diverse
from firecode_amd import synthetic as syn
from firecode_amd.pruner import select_diverse as gpu_select
from firecode_amd.torsion_module import most_diverse_conformers
from oracle import cpu_ref as o


def _ens(n=12, A=6, seed=1):
    X, atoms, _ = syn.synthetic_ensemble(n, A, seed=seed)
    return X, atoms


@pytest.mark.parametrize("kwargs", [
    dict(structures=np.zeros((4, 5, 2)), atoms=["C"] * 5, n=2),      # not (N, A, 3)
    dict(structures=np.zeros((4, 5)), atoms=["C"] * 5, n=2),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 4, n=2),      # len(atoms)
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5),           # neither n nor stop_rmsd
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, n=0),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, n=-3),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, n=2.5),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, stop_rmsd=-0.1),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, stop_rmsd=float("nan")),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, n=2, start=4),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, n=2, start=-1),
    dict(structures=np.zeros((4, 5, 3)), atoms=["C"] * 5, n=2, energies=np.zeros(3)),
    dict(structures=np.zeros((4, 5, 3)), atoms=["H"] * 5, n=2),      # no heavy atom to align
])
def test_bad_arguments_raise_before_device_use(kwargs):
    with pytest.raises(fc.FirecodeHipInputError):
        gpu_select(**kwargs)


def test_bad_method_and_diversity_keywords():
    X, _ = _ens()
    with pytest.raises(fc.FirecodeHipInputError):
        most_diverse_conformers(3, list(X), method="tfd")
    with pytest.raises(fc.FirecodeHipInputError):
        fc.torsion_module.clustered_csearch_core(X[0], [(0, 1, 2, 3, 3)], np.zeros((1, 6), bool), diversity="kmeans")


def test_no_cpu_fallback():
    if fc._lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    X, atoms = _ens()
    with pytest.raises(fc.FirecodeHipDeviceError):
        gpu_select(X, atoms, n=3)
    with pytest.raises(fc.FirecodeHipDeviceError):
        most_diverse_conformers(3, list(X), method="rmsd")


def test_random_draw_unchanged():
    """the default stays the reference's seeded draw, bit for bit"""
    X, _ = _ens(20)
    got = np.array(most_diverse_conformers(5, list(X), seed=3))
    idx = np.sort(np.random.RandomState(3).choice(20, size=5))
    assert np.array_equal(got, X[idx])
    assert np.array_equal(np.array(most_diverse_conformers(5, list(X), seed=3, method="random")), got)
    assert len(most_diverse_conformers(30, list(X), seed=3)) == 20


@pytest.mark.parametrize("seed", range(4))
def test_restatement_properties(seed):
    X, atoms = _ens(15, 7, seed)
    Xsel = prepared(X, atoms)
    idx, lab, dist, rad, rec = select_diverse(Xsel, 6, start=seed % 15)
    assert idx[0] == seed % 15 and len(idx) == 6 and len(set(idx.tolist())) == 6
    assert np.isinf(rad[0]) and np.all(np.diff(rad) <= 0.0)  # radii nonincreasing
    # labels / distances against the recorded rows: each conformer's distance is the row of its label's pick,
    # and no other pick is strictly closer
    rows = np.array([rec.rows[k] for k in range(len(idx))])
    for j in range(len(X)):
        if j in set(idx.tolist()):
            assert dist[j] == 0.0 and idx[lab[j]] == j
            continue
        assert dist[j] == rows[lab[j], j]
        assert dist[j] == rows[:, j].min()
        assert np.all(rows[: lab[j], j] > dist[j])  # ties keep the earlier pick: every earlier one is farther
    # a radius is the covering radius just before the pick: the largest distance to the picks before it
    for k in range(1, len(idx)):
        assert rad[k] == rows[:k, idx[k]].min()
        live = np.setdiff1d(np.arange(len(X)), idx[:k])
        assert rad[k] == rows[:k][:, live].min(axis=0).max()


def test_restatement_stop_and_start():
    X, atoms = _ens(20, 6, 5)
    Xsel = prepared(X, atoms)
    full = select_diverse(Xsel, 20)
    r = full[3]
    stop = 0.5 * (r[4] + r[5])
    idx, _, dist, rad, rec = select_diverse(Xsel, 20, stop_rmsd=stop)
    assert np.array_equal(idx, full[0][:5]) and dist.max() <= stop and rad[-1] > stop
    assert rec.stop_gap > 0.0


@pytest.mark.parametrize("seed", range(6))
def test_restatement_within_twice_the_optimal_k_center_radius(seed):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(4, 10))
    X = syn.continuous_ensemble(N, 6, seed=seed)
    dist = np.array([rmsd_row(X, i) for i in range(N)])
    dist = np.maximum(dist, dist.T)
    np.fill_diagonal(dist, 0.0)
    for k in (1, 2, 3):
        _, _, d, _, _ = select_diverse(X, k, start=int(rng.integers(N)))
        assert d.max() <= 2.0 * brute_force_k_center(dist, k) + 1e-12


def test_restatement_row_is_the_oracle_pair_value():
    X, atoms = _ens(6, 8, 2)
    Xsel = prepared(X, atoms)
    row = rmsd_row(Xsel, 2)
    for j in range(6):
        assert abs(row[j] - o.rmsd_and_max(Xsel[2], Xsel[j], center=True)[0]) < 1e-12
