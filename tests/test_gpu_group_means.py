"""Group means on the device (fc_ensemble_group_means; the kernels of fc_group_mean.hip) against the NumPy restatement of
the contract (tests/group_mean_ref.py).

Bars: at a FIXED turn count (tol = 0, so that no knife-edge stop can change the count) ``means``, ``rmsf``, ``distances``
and ``aligned`` within TOL = 1e-10 of the restatement -- two independent solvers agree to about 1e-14 there
(tests/test_group_mean_cpu.py) -- and ``closest``, ``sizes`` and ``n_iter`` exact, on inputs for which the restatement
shows the two smallest d_n of every group more than GAP = 1e-8 apart (asserted on the restatement for every group of
every case).  Two kinds of group cannot show such a gap, whatever the input, and are named by ``_exact_tie``:
  * a group of TWO members after one turn or more: its mean is the midpoint of the two superposed members, the
    covariance of either member with the midpoint is then symmetric positive semidefinite (X0^T X0 + X0^T R X1 with R
    optimal), so the rotation of the final pass is the identity and d_0 = d_1 = |X0 - R X1| / (2 sqrt A) in exact
    arithmetic; the restatement's gap there is rounding (asserted below 1e-12), the contract's "lowest index on ties"
    cannot be decided to the bit by two float64 evaluations, and ``closest`` has to be a member at the smallest distance;
  * one selected atom: every prepared coordinate is 0, every d is exactly 0 on both sides, and the tie goes to the
    lowest index exactly.
The same two kinds reach their fixed point after one turn (the pair) or at once (one atom): from then on the change c of
a turn is rounding, 1e-16 or exactly 0, and "c <= tol" at tol = 0 is decided by the last bit.  Where the restatement shows
a change below ROUNDING = 1e-13, and only there, ``n_iter`` may be anything from that turn to ``max_iter``; every other
group of every case -- asserted: all groups of three or more members -- has its ``n_iter`` compared exactly.
Every case runs in well under a second on the device; the restatements are computed once per module."""

import functools

import numpy as np
import pytest

import degenerate_ref as dg
import group_mean_ref as gr
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10
GAP = 1e-8

# group sizes on either side of a wavefront and of a chunk of the reduction (64), a singleton, a pair; unsorted and
# interleaved; four conformers in no group; group id 3 empty
MIXED = dict(sizes=[1, 2, 3, 63, 64, 65, 102], a_sel=13, n_h=3, n_unlabelled=4, sigma=0.3, seed=41, empty_ids=(3,))
CASES = {
    "mixed": MIXED,
    "one_group": dict(sizes=[300], a_sel=13, n_h=2, sigma=0.3, seed=42),
    "pairs": dict(sizes=[2] * 128 + [1], a_sel=13, n_h=1, sigma=0.3, seed=43),   # N = 257
    "a1": dict(sizes=[5, 40], a_sel=1, sigma=0.3, seed=44),
    "a3": dict(sizes=[5, 40], a_sel=3, n_h=2, sigma=0.3, seed=45),
    "a4": dict(sizes=[5, 40], a_sel=4, n_h=2, sigma=0.3, seed=46),
    "a50": dict(sizes=[5, 70], a_sel=50, n_h=7, sigma=0.3, seed=47),
    "stage_2048": dict(sizes=[3, 40], a_sel=2048, n_h=1, sigma=0.3, seed=48),      # the last A_sel whose mean is staged
    "stage_2049": dict(sizes=[3, 40], a_sel=2049, n_h=1, sigma=0.3, seed=49),      # the first that is read from global memory
    "n1": dict(sizes=[1], a_sel=13, n_h=2, seed=50),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    X, atoms, lab = gr.build_case(**CASES[name])
    for a in (X, lab):
        a.setflags(write=False)
    return X, atoms, lab, gr.prepared(X, atoms)


@functools.lru_cache(maxsize=None)
def _reference(name, max_iter):
    X, atoms, lab, Xp = _case(name)
    return gr.group_means(Xp, lab, max_iter=max_iter, tol=0.0)


def _exact_tie(size, a_sel, n_iter):
    return size >= 2 and (a_sel == 1 or (size == 2 and n_iter >= 1))


ROUNDING = 1e-13


def _first_rounding_turn(ref, g):
    """the first turn (counted from 1) whose change is rounding, or None"""
    small = [t + 1 for t, c in enumerate(ref.changes[g]) if c < ROUNDING]
    return small[0] if small else None


def _assert_gaps(ref, a_sel):
    """on the restatement itself, for every group: the two smallest d_n more than GAP apart, or one of the two exact
    ties of the module docstring, shown as such"""
    for g, size in enumerate(ref.sizes):
        if size < 2:
            continue
        if _exact_tie(size, a_sel, ref.n_iter[g]):
            assert ref.closest_gap[g] < 1e-12, (g, ref.closest_gap[g])
        else:
            assert ref.closest_gap[g] > GAP, (g, size, ref.closest_gap[g])
        if not (a_sel == 1 or size == 2):
            assert _first_rounding_turn(ref, g) is None, (g, size, ref.changes[g])


def _check(got, ref, lab, a_sel, what):
    assert np.array_equal(got.sizes, ref.sizes), what
    for g in range(len(ref.sizes)):
        t = _first_rounding_turn(ref, g)
        if t is None:
            assert got.n_iter[g] == ref.n_iter[g], (what, g, got.n_iter[g], ref.n_iter[g])
        else:
            assert t <= got.n_iter[g] <= max(t, len(ref.changes[g])), (what, g, got.n_iter[g], ref.changes[g])
    full = ref.sizes > 0
    for name in ("means", "rmsf", "distances"):
        u, v = getattr(got, name), getattr(ref, name)
        assert np.array_equal(np.isnan(u), np.isnan(v)), (what, name)
        err = np.nanmax(np.abs(u - v), initial=0.0)
        print(f"{what}: {name} off by {err:.3g}")
        assert err <= TOL, (what, name, err)
    assert np.isnan(got.means[~full]).all() and np.isnan(got.rmsf[~full]).all() and np.all(got.closest[~full] == -1)
    for g in np.flatnonzero(full):
        if _exact_tie(ref.sizes[g], a_sel, ref.n_iter[g]) and a_sel > 1:
            mem = np.flatnonzero(lab == g)
            assert got.closest[g] in mem and ref.distances[got.closest[g]] <= ref.distances[mem].min() + TOL, (what, g)
        else:
            assert got.closest[g] == ref.closest[g], (what, g)
    out = np.flatnonzero(lab < 0)
    assert np.isnan(got.distances[out]).all() and np.all(got.rotations[out] == np.eye(3)), what
    det = np.linalg.det(got.rotations)
    assert np.abs(det - 1.0).max() < 1e-12 and np.abs(got.rotations @ got.rotations.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12


# ---- against the restatement at a fixed turn count
@pytest.mark.parametrize("max_iter", [0, 1, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(fc, name, max_iter):
    X, atoms, lab, Xp = _case(name)
    a_sel = Xp.shape[1]
    ref = _reference(name, max_iter)
    _assert_gaps(ref, a_sel)
    got = fc.pruner.group_means_by_rmsd(X, atoms, lab, max_iter=max_iter, tol=0.0, aligned=True)
    _check(got, ref, lab, a_sel, f"{name} max_iter={max_iter}")
    multi = np.flatnonzero(ref.sizes >= 2)
    assert np.all(got.n_iter[ref.sizes >= 3] == (max_iter if a_sel > 1 else min(max_iter, 1))) and np.all(got.n_iter[ref.sizes < 2] == 0)
    if a_sel > 1:  # (one atom: every rotation is optimal, the block of a lone selected atom has nothing else in it)
        want = gr.aligned_block(X, atoms, ref.rotations)
        err = np.abs(got.aligned - want).max()
        print(f"{name} max_iter={max_iter}: aligned off by {err:.3g}")
        assert err <= TOL
    else:
        assert np.abs(got.aligned).max() <= TOL
    # the selected atoms of the block are the rotated prepared members, and the members of a group lie on their mean
    sel = atoms != "H"
    for g in multi:
        mem = np.flatnonzero(lab == g)
        dev = got.aligned[mem][:, sel] - got.means[g]
        assert np.abs(np.sqrt((dev ** 2).sum(axis=(1, 2)) / a_sel) - got.distances[mem]).max() <= TOL
    out = lab < 0
    assert np.abs(got.aligned[out] - (X[out] - X[out][:, sel].mean(axis=1, keepdims=True))).max(initial=0.0) <= 1e-12


def test_one_group_without_labels(fc):
    X, atoms, lab, Xp = _case("one_group")
    ref = _reference("one_group", 4)
    got = fc.pruner.group_means_by_rmsd(X, atoms, None, max_iter=4, tol=0.0)
    _check(got, ref, lab, Xp.shape[1], "labels=None")
    assert got.aligned is None and got.means.shape == (1, 13, 3)


# ---- max_iter = 0: the plain RMSD to the reference member
def test_zero_turns_give_the_pair_rmsd(fc):
    X, atoms, lab, Xp = _case("mixed")
    rng = np.random.default_rng(5)
    n_groups = int(lab.max()) + 1
    refs = np.array([rng.choice(np.flatnonzero(lab == g)) if np.any(lab == g) else -7 for g in range(n_groups)])
    got = fc.pruner.group_means_by_rmsd(X, atoms, lab, refs=refs, max_iter=0)
    assert np.all(got.n_iter == 0)
    for g in range(n_groups):
        mem = np.flatnonzero(lab == g)
        if len(mem) == 0:
            continue
        P = np.broadcast_to(Xp[refs[g]], Xp[mem].shape)
        want = o.rmsd_and_max_batch(P, Xp[mem])[0]
        assert np.abs(got.distances[mem] - want).max() <= TOL
        assert np.abs(got.means[g] - Xp[refs[g]]).max() <= 1e-12  # (the device's own centring)
        moved = np.einsum("nij,naj->nai", got.rotations[mem], Xp[mem])
        again = np.sqrt(((moved - Xp[refs[g]]) ** 2).sum(axis=(1, 2)) / Xp.shape[1])
        assert np.abs(again - got.distances[mem]).max() <= TOL
        assert got.closest[g] == refs[g] or len(mem) == 1


# ---- tol mode
# tight clouds of several widths: their changes per turn step over tol = 1e-9 from 4e-8 or more to 2.3e-11 or less
TIGHT = dict(sizes=[5, 40, 70, 2, 1, 33], a_sel=13, sigma=[0.02, 0.02, 0.02, 0.05, 0.05, 0.15], seed=61)


@functools.lru_cache(maxsize=None)
def _tight():
    X, atoms, lab = gr.build_case(**TIGHT)
    Xp = gr.prepared(X, atoms)
    return X, atoms, lab, Xp, gr.group_means(Xp, lab, max_iter=50, tol=1e-9)


def test_tol_stops_every_group_where_the_restatement_stops(fc):
    X, atoms, lab, Xp, ref = _tight()
    # no per-turn change of the restatement within a factor of 10 of tol: the stop is no knife edge
    every = np.array([c for g in ref.changes for c in g])
    assert len(every) >= 10 and not np.any((every > 1e-10) & (every < 1e-8)), np.sort(every)
    assert ref.n_iter.max() <= 6 and len(set(ref.n_iter.tolist())) >= 3
    got = fc.pruner.group_means_by_rmsd(X, atoms, lab, max_iter=50, tol=1e-9)
    print("turns", got.n_iter.tolist())
    _assert_gaps(ref, 13)
    _check(got, ref, lab, 13, "tol=1e-9")


def test_a_frozen_group_does_not_see_the_others(fc, monkeypatch):
    """the tight groups next to a broad one (sigma 2 A: tens of turns) and without it: the same bits, whenever the
    host looks at the word"""
    X, atoms, lab, Xp, _ = _tight()
    Xb, _, _ = gr.build_case([90], 13, sigma=2.0, seed=62)
    both = np.concatenate([X, Xb])
    n_tight = int(lab.max()) + 1
    alone = np.concatenate([lab, np.full(90, -1)])
    beside = np.concatenate([lab, np.full(90, n_tight)])
    base = fc.pruner.group_means_by_rmsd(both, atoms, alone, max_iter=50, tol=1e-9)
    for batch in ("4", "1", "7"):
        monkeypatch.setenv("FC_GROUP_MEAN_BATCH", batch)
        got = fc.pruner.group_means_by_rmsd(both, atoms, beside, max_iter=50, tol=1e-9)
        assert got.n_iter[n_tight] > 3 * base.n_iter[:n_tight].max(), got.n_iter
        rows = np.arange(len(lab))
        assert np.array_equal(got.means[:n_tight], base.means[:n_tight]) and np.array_equal(got.rmsf[:n_tight], base.rmsf[:n_tight])
        assert np.array_equal(got.distances[rows], base.distances[rows]) and np.array_equal(got.rotations[rows], base.rotations[rows])
        assert np.array_equal(got.n_iter[:n_tight], base.n_iter[:n_tight]) and np.array_equal(got.closest[:n_tight], base.closest[:n_tight])


# ---- without a reference
def test_the_mean_beats_the_medoid_and_rmsf_matches_d(fc):
    for X, atoms, lab in (_tight()[:3], _case("mixed")[:3]):
        mean = fc.pruner.group_means_by_rmsd(X, atoms, lab, max_iter=50, tol=1e-9)
        med = fc.pruner.group_means_by_rmsd(X, atoms, lab, refs="medoids", max_iter=0)
        assert np.all(mean.n_iter < 50)
        for g in np.flatnonzero(mean.sizes):
            mem = np.flatnonzero(lab == g)
            cost, cost_med = (mean.distances[mem] ** 2).sum(), (med.distances[mem] ** 2).sum()
            assert cost <= cost_med * (1 + 1e-12), (g, cost, cost_med)
            assert (mean.rmsf[g] ** 2).sum() * len(mem) == pytest.approx(cost * 13, rel=1e-9, abs=1e-300)


# ---- the same bits
def _same(u, v):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(u[:7], v[:7]))


@pytest.mark.parametrize("name,max_iter,tol", [("mixed", 50, 1e-9), ("pairs", 3, 0.0), ("one_group", 4, 0.0), ("stage_2048", 2, 0.0)])
def test_the_same_bits_for_every_launch_shape(fc, monkeypatch, name, max_iter, tol):
    X, atoms, lab, Xp = _case(name)
    run = lambda: fc.pruner.group_means_by_rmsd(X, atoms, lab, max_iter=max_iter, tol=tol)  # noqa: E731
    base = run()
    assert _same(run(), base), "two runs"
    for knob, values in (("FC_GROUP_MEAN_STAGE", ("0", "1")), ("FC_GROUP_MEAN_GRID", ("1", "3", "1000")),
                         ("FC_GROUP_MEAN_BATCH", ("1", "7", "64"))):
        for v in values:
            monkeypatch.setenv(knob, v)
            assert _same(run(), base), (knob, v)
        monkeypatch.delenv(knob)
    monkeypatch.setenv("FC_GROUP_MEAN_STAGE", "0")
    monkeypatch.setenv("FC_GROUP_MEAN_GRID", "2")
    monkeypatch.setenv("FC_GROUP_MEAN_BATCH", "3")
    assert _same(run(), base), "all three"


def test_medoid_starts_are_the_medoids(fc):
    X, atoms, lab, Xp = _case("mixed")
    med = fc.pruner.medoids_by_rmsd(X, atoms, lab).medoids
    assert med[3] == -1  # (the empty group's entry is not read)
    by_name = fc.pruner.group_means_by_rmsd(X, atoms, lab, refs="medoids", max_iter=2, tol=0.0)
    by_hand = fc.pruner.group_means_by_rmsd(X, atoms, lab, refs=med, max_iter=2, tol=0.0)
    assert _same(by_name, by_hand)
    first = fc.pruner.group_means_by_rmsd(X, atoms, lab, max_iter=0)
    zero = fc.pruner.group_means_by_rmsd(X, atoms, lab, refs="medoids", max_iter=0)
    assert np.array_equal(zero.closest[zero.sizes > 0], med[zero.sizes > 0]) and not _same(first, zero)
    with fc.DeviceEnsemble(X, atom_mask=atoms != "H") as ens:  # the resident form: one upload for both
        out = ens.group_means(lab, refs="medoids", max_iter=2, tol=0.0, want_ms=True)
        assert _same(out, by_hand) and out[7] > 0.0
        assert ens.group_means(lab, refs="medoids", max_iter=2, tol=0.0, want_rotations=False)[6] is None


# ---- degenerate members
def test_degenerate_members_stay_finite(fc):
    rng = np.random.default_rng(9)
    Xl, t = dg.collinear(40, 5, {}, seed=3)                          # all atoms on a line
    r = dg.two_atoms_lengths(40, seed=2)
    X2 = dg.two_atoms(40, r, seed=2)                                 # two atoms
    one = rng.normal(scale=2.0, size=(6, 3))
    Xd = np.repeat(one[None], 40, axis=0)                            # exact duplicates of the mean
    for X, exact in ((Xl, dg.collinear_distances(t)), (X2, dg.two_atoms_distances(r)), (Xd, np.zeros((40, 40)))):
        atoms = np.array(["C"] * X.shape[1])
        lab = np.arange(40) % 3
        refs = np.array([3, 7, 11])
        zero = fc.pruner.group_means_by_rmsd(X, atoms, lab, refs=refs, max_iter=0, aligned=True)
        assert np.abs(zero.distances - exact[refs[lab], np.arange(40)]).max() <= TOL
        for got in (zero, fc.pruner.group_means_by_rmsd(X, atoms, lab, max_iter=5, tol=1e-9, aligned=True)):
            for a in (got.means, got.rmsf, got.distances, got.rotations, got.aligned):
                assert np.isfinite(a).all()
            assert np.abs(np.linalg.det(got.rotations) - 1.0).max() < 1e-9 and got.sizes.tolist() == [14, 13, 13]
    same = fc.pruner.group_means_by_rmsd(Xd, np.array(["C"] * 6), None, max_iter=5, tol=1e-9)
    assert same.n_iter.tolist() == [1] and same.distances.max() <= 1e-13 and same.rmsf.max() <= 1e-13


# ---- the Ensemble layer
def test_align_by_groups_round_trips_through_xyz(fc, tmp_path):
    from firecode_amd.ensemble import Ensemble

    X, atoms, lab, Xp = _case("a50")
    before = fc.utils.align_structures(X)  # every conformer on the first: its own kernel, as it was
    assert np.abs(before - o.align_structures(X)).max() <= TOL * max(1.0, float(np.abs(before).max()))
    e = Ensemble(atoms=atoms.copy(), coords=X.copy(), basename="groups", logfunction=None)
    res = e.mean_structures(lab, max_iter=4, tol=0.0)
    assert res.aligned is None and np.array_equal(e.coords, X)
    res = e.align_by_groups(lab, max_iter=4, tol=0.0)
    ref = _reference("a50", 4)
    assert np.abs(e.coords - gr.aligned_block(X, atoms, ref.rotations)).max() <= TOL and e.coords is res.aligned
    path = tmp_path / "groups.xyz"
    e.to_xyz(str(path))
    back = Ensemble.from_xyz(str(path))
    assert back.coords.shape == X.shape and list(back.atoms) == list(atoms)
    assert np.array_equal(back.coords, np.array([[[float(f"{v:15.8f}") for v in row] for row in c] for c in e.coords]))
    assert np.array_equal(fc.utils.align_structures(X), before)
