"""The walk of tests/test_gpu_handle_order.py, checked without a GPU: the sequence covers what it says it covers, and the
two thresholds are sparse and dense on the three ensembles by the oracle's own count."""

import collections

import numpy as np
import pytest

import handle_walk_ref as hw
from oracle import cpu_ref as o


def test_every_ordered_pair_of_families_is_adjacent():
    seq = hw.sequence()
    assert len(hw.FAMILIES) == 13 and len(seq) == 13 * 13 + 1
    assert set(zip(seq, seq[1:])) == {(f, g) for f in hw.FAMILIES for g in hw.FAMILIES}
    assert seq[0] == seq[-1]  # a circuit
    # ... and for any other set of families
    for fams in ("a", "ab", "xyz"):
        s = hw.sequence(tuple(fams))
        assert len(s) == len(fams) ** 2 + 1 and set(zip(s, s[1:])) == {(f, g) for f in fams for g in fams}


def test_the_committed_table_has_two_or_three_steps_per_family_and_unique_names():
    names = [s.name for s in hw.STEPS]
    assert len(set(names)) == len(names)
    per_family = collections.Counter(s.family for s in hw.STEPS)
    assert set(per_family) == set("abcdefghijklm")
    assert all(2 <= n <= 4 for n in per_family.values()), per_family


@pytest.mark.parametrize("twin_at,start", [(2, 0), (130, 0), (2, 1)])
def test_every_step_and_every_modifier_appears(twin_at, start):
    visits = hw.plan(twin_at=twin_at, start=start)
    assert len(visits) == 170 and [v.index for v in visits] == list(range(170))
    assert {v.step.name for v in visits} == {s.name for s in hw.STEPS}
    mods = collections.Counter(m for v in visits for m in v.modifier.split("+"))
    for m in set(hw.MODIFIERS) - {"none"}:
        assert mods[m] >= 3, (m, mods)
    assert mods[hw.TWIN] == 1 and hw.TWIN in visits[twin_at].modifier
    # within a family the steps rotate: a family that follows itself runs two different steps
    for v, w in zip(visits, visits[1:]):
        assert w.previous == v.step.name
        if v.step.family == w.step.family:
            assert v.step.name != w.step.name
    # the stream goes to the second one and comes back, in that order, again and again
    streams = [m for v in visits for m in v.modifier.split("+") if m.startswith("stream_")]
    assert streams[0] == "stream_second" and all(a != b for a, b in zip(streams, streams[1:]))


def test_three_rounds_meet_with_other_steps_each_time():
    one, three = hw.plan(), hw.plan(rounds=3)
    assert len(three) == 3 * 169 + 1 and [v.step.name for v in three[:170]] == [v.step.name for v in one]
    assert [v.index for v in three] == list(range(len(three)))
    fams = [v.step.family for v in three]
    for r in range(3):  # every round is the whole circuit
        part = fams[169 * r:169 * (r + 1) + 1]
        assert set(zip(part, part[1:])) == {(f, g) for f in hw.FAMILIES for g in hw.FAMILIES}
    pairs = lambda visits: {(v.previous, v.step.name) for v in visits[1:]}  # noqa: E731
    print(f"ordered pairs of steps met: {len(pairs(one))} in one round, {len(pairs(three))} in three")
    assert len(pairs(one)) == 169 and len(pairs(three)) > 400
    for v, w in zip(three, three[1:]):
        assert w.previous == v.step.name and (v.step.family != w.step.family or v.step.name != w.step.name)


def test_the_sequence_is_the_same_on_two_calls():
    assert hw.sequence() == hw.sequence()
    a, b = hw.plan(), hw.plan()
    flat = lambda visits: [(v.index, v.step.name, v.modifier, v.previous) for v in visits]  # noqa: E731
    assert flat(a) == flat(b) and flat(hw.plan(rounds=3)) == flat(hw.plan(rounds=3))
    assert [v.step.name for v in hw.plan(start=1)] != [v.step.name for v in a]


@pytest.mark.parametrize("shape", sorted(hw.SHAPES))
def test_thresholds_are_sparse_and_dense_by_the_oracle(shape):
    """similar pairs below 5 % at SPARSE and above 50 % at DENSE; the ensemble holds what the walk counts on: exact
    duplicates, and planar conformers whose pairs alone overflow a fix-up queue of 1 000"""
    case = hw.build(shape)
    n = case.N
    assert case.X.shape == (n, case.A, 3) and case.X is hw.build(shape).X
    _, R, D = o.rmsd_similarity_matrix(case.X, case.atoms, hw.SPARSE[0], hw.SPARSE[1])
    iu = np.triu_indices(n, 1)
    frac = {}
    for name, (thr, dev) in (("sparse", hw.SPARSE), ("dense", hw.DENSE)):
        frac[name] = float(((R < thr) & (D < dev))[iu].mean())
    print(f"{shape}: similar pairs {frac['sparse']:.4f} at {hw.SPARSE}, {frac['dense']:.4f} at {hw.DENSE}")
    assert frac["sparse"] < 0.05 and frac["dense"] > 0.50, frac
    for t in hw.dup_targets(n):
        assert np.array_equal(case.X[t], case.X[hw.DUP_SOURCE]) and R[t, hw.DUP_SOURCE] < 1e-6
    flat = hw.degenerate_indices(n)
    assert not set(flat) & ({hw.DUP_SOURCE} | set(hw.dup_targets(n))) and len(set(flat)) == len(flat) and max(flat) < n
    for q, p in enumerate(flat):  # one planar conformer, the others collinear
        c = case.X[p] - case.X[p].mean(axis=0)
        s = np.linalg.svd(c, compute_uv=False)
        assert s[2] < 1e-9 * s[0] and (s[1] > 0.1 * s[0] if q == 0 else s[1] < 1e-9 * s[0])
    # the pairs with a collinear partner have no unique rotation (the oracle's bound says so) and alone overflow a queue of 1 000
    Xc = case.X - case.X.mean(axis=1, keepdims=True)
    partner = np.array([i for i in range(n) if i != flat[1]])
    assert np.isinf(o.rotation_error_bound_batch(Xc[np.full(n - 1, flat[1])], Xc[partner])).all()
    assert np.isfinite(o.rotation_error_bound_batch(Xc[[flat[0]] * 3], Xc[[0, 1, 2]])).all()
    assert hw.fix_up_pairs(n) > 1000
    # the energy window of the steps with energies keeps a real share of the pairs, and cuts a real share
    for e in (case.energies, case.energies2):
        inside = (np.abs(e[:, None] - e[None, :]) < hw.MAX_DE)[iu].mean()
        assert 0.3 < inside < 0.7, inside
