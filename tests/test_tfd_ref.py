"""CPU checks of tests/tfd_ref.py, the reference and the case builders of tests/test_gpu_tfd_kernels.py: a reference
that is wrong, or a planted case that does not exercise what it names, would make the GPU tests pass for nothing."""

import numpy as np
import pytest

import tfd_ref as R
from oracle import cpu_ref as o


def test_first_match_and_simbits_agree_with_the_oracle_pair_by_pair():
    """2 000 random pairs (Q = 1 ... 128; a third across the +-180 wrap, a third planted at the threshold) decided by
    oracle.cpu_ref.tfd_similarity == the reference's matrix and its first match"""
    rng = np.random.default_rng(5)
    n_wrap = n_q8 = n_sim = 0
    for k in range(2000):
        Q = int(rng.choice([1, 2, 3, 5, 7, 8, 9, 16, 17, 40, 128]))
        a = rng.uniform(-180, 180, size=Q)
        kind = k % 3
        if kind == 0:
            b = rng.uniform(-180, 180, size=Q) if k % 2 else R.wrap(a + rng.normal(scale=12.0 / Q, size=Q))
        elif kind == 1:  # across the wrap
            a = rng.choice([-1.0, 1.0], size=Q) * (180.0 - rng.uniform(0, 1, size=Q) * 8.0 / Q)
            b = R.wrap(a + np.sign(a) * rng.uniform(0, 1, size=Q) * 16.0 / Q)
            n_wrap += int(np.any(np.abs(a - b) > 180))
        else:  # at the threshold: the sum of the deltas is 10 -+ a few ulp
            tf2 = np.stack([a, a])
            R.plant(tf2, 0, 1, 10.0, rng, across_wrap=bool(k % 2))
            a, b = tf2[0].copy(), tf2[1].copy()
        tf = np.stack([a, b])
        for thresh in (10.0, R.pair_sum(a, b), np.nextafter(R.pair_sum(a, b), np.inf)):
            want = o.tfd_similarity(a, b, thresh)
            assert want == o.tfd_similarity(b, a, thresh)
            S = R.simbits(tf, thresh)
            assert S[0, 1] == want and S[1, 0] == want and not S[0, 0] and not S[1, 1]
            fm = R.first_match(tf, thresh)
            assert fm.tolist() == [1 if want else -1, -1]
            assert R.first_match(tf, thresh, rows=[0]).tolist() == [1 if want else -1]
            n_sim += int(want)
        n_q8 += int(Q >= 8)
    assert n_wrap > 500 and n_q8 > 500 and 1500 < n_sim < 4500


def test_first_match_rows_is_the_full_reference_restricted_and_sums_row_by_row():
    rng = np.random.default_rng(6)
    for Q in (1, 7, 8, 9, 33, 128):
        c = rng.uniform(-180, 180, size=(12, Q))
        tf = R.wrap(c[rng.integers(0, 12, 300)] + rng.uniform(-1, 1, size=(300, Q)) * 15.0 / Q)
        full = R.first_match(tf, 10.0)
        assert (full >= 0).sum() > 100 and (full < 0).sum() > 5
        rows = rng.permutation(300)[:40]
        assert np.array_equal(R.first_match(tf, 10.0, rows=rows), full[rows])
        S = R.simbits(tf, 10.0)
        assert np.array_equal(S, S.T) and not S.diagonal().any()
        for i in rows:  # the batched sum over the last axis is np.sum of every row, to the bit
            later = np.flatnonzero(S[i, i + 1:])
            assert full[i] == (i + 1 + later[0] if len(later) else -1)
            d = R.deltas(tf, tf[i])
            assert np.array_equal(np.sum(d, axis=-1), np.array([np.sum(np.ascontiguousarray(r)) for r in d]))


def test_lattice_has_no_similar_pair():
    tf = R.lattice(41, 5, 1.4, 3)
    assert tf.shape == (41 * 41, 5) and R.seam_gap(41, 1.4) > 1.0
    assert not R.simbits(tf, 1.0).any() and not R.simbits(tf, 1.4).any()
    assert R.simbits(tf[:, :2].copy(), 1.4 + 1e-9).any()  # (the grid's step is what keeps them apart)
    # 257 x 257: by the argument -- distinct grid points, step above the threshold, seam gap above it too
    tf = R.lattice(257, 2, 1.4, 11)
    assert tf.shape == (66049, 2) and len(np.unique(tf, axis=0)) == 66049
    g = np.unique(tf)
    assert len(g) == 257 and np.diff(g).min() > 1.0 and np.isclose(R.seam_gap(257, 1.4), 1.6) and 360.0 - (g[-1] - g[0]) > 1.0
    rows = np.random.default_rng(0).permutation(66049)[:300]
    assert (R.first_match(tf, 1.0, rows=rows) == -1).all()
    for dims, side, Q in ((1, 25, 1), (3, 7, 3), (4, 5, 9)):
        tf = R.lattice(side, Q, 300.0 / side, 1, dims=dims)
        assert len(tf) == side ** dims and not R.simbits(tf, 10.0).any()


@pytest.mark.parametrize("Q", [1, 2, 5, 8, 9, 128])
def test_plant_lands_where_it_says(Q):
    rng = np.random.default_rng(40 + Q)
    tf = rng.uniform(-180, 180, size=(50, Q))
    for k in range(40):
        i, j = rng.permutation(50)[:2]
        total = float(rng.choice([0.2, 4.0, 10.0, 10.5]))
        angles = None if k % 3 == 0 else np.sort(rng.permutation(Q)[:1 + k % min(Q, 3)])
        across = k % 2 == 1
        s = R.plant(tf, i, j, total, rng, angles=angles, across_wrap=across)
        assert abs(s - total) < 1e-12 and s == float(np.sum(R.deltas(tf[i], tf[j]))) and s == R.eight_lane_sum(R.deltas(tf[i], tf[j]))
        assert np.all(np.abs(tf[j]) <= 180.0)
        sel = np.arange(Q) if angles is None else angles
        rest = np.setdiff1d(np.arange(Q), sel)
        assert np.array_equal(tf[i, rest], tf[j, rest])
        if across:
            assert R.opposite_sides(tf, i, j, sel) and np.all(np.abs(tf[i, sel]) > 180.0 - total)


def test_eight_lane_order_is_numpys_up_to_128_elements_and_not_beyond():
    """why Q_MAX is 128: the order tfd_sum adds in equals np.sum for every length 1 ... 128 and differs from it beyond"""
    rng = np.random.default_rng(8)
    assert R.Q_MAX == 128
    for n in range(1, 129):
        for _ in range(20):
            v = rng.uniform(0, 180, size=n) * rng.choice([1e-3, 1.0], size=n)
            assert R.eight_lane_sum(v) == float(np.sum(v)), n
    for n in (129, 200):
        assert any(R.eight_lane_sum(v) != float(np.sum(v)) for v in rng.uniform(0, 180, size=(200, n))), n


def test_the_planted_cases_exercise_what_they_name():
    """the builders of the GPU cases, judged by the reference alone"""
    for Q in (1, 2, 4, 5, 8, 9, 12):
        tf, pos, neg = R.wrap_case(Q)
        assert tf.shape == (6000, Q) and len(pos) == min(Q, 9) + (Q > 1) and len(neg) == min(Q, 9)
        for i, j, ang, s in pos + neg:
            assert 3000 <= j - i <= 5010 and R.opposite_sides(tf, i, j, ang)
        assert all(abs(p[3] - 4.0) < 1e-12 for p in pos) and all(abs(p[3] - 10.5) < 1e-12 for p in neg)
        if Q >= 9:  # an angle that is in no box and in no 16-bit sum
            assert [8] in [p[2] for p in pos] and [8] in [p[2] for p in neg]
    tf, plants, sweep = R.boundary_case()
    assert sorted({(k, d) for _, _, k, d in plants}) == sorted(
        [(k, d) for k in ("box0", "dense", "win0", "win1") for d in (-1, 0, 1)] + [("last", 0)])
    for kind in {k for _, _, k, _ in plants}:
        assert {p[0] % 64 for p in plants if p[2] == kind} == {0, 1, 62, 63}
    for i, j, kind, d in plants:
        i0 = i - i % 64
        if kind == "dense":
            assert j == i0 + 128 + d
        elif kind != "last":
            assert (j - d) % (1024 if kind == "box0" else 256) == 0 and j - d > i0 + 129
    assert [j - i for i, j in sweep] == list(range(1, 1301)) and sweep[-1][0] > 5000
    tf, planted, check = R.launcher_case()
    assert len(planted) == 7 * 13 + 26 and sum(i < R.CHUNK <= j for i, j in planted) == 13
    assert {j - i for i, j in planted} >= set(R.F_GAPS)
