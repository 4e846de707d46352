"""tests/prep_ref.py on the CPU: the restated LDS arithmetic against the figures worked out by hand, the atom
selections, the placements, the all-pairs reference against the oracle's own matrix form, the threshold choice -- and
the inputs of every case of tests/test_gpu_prep.py: a threshold clear of every pair, both verdicts, the conditioning
bounds where the module claims them.  What fails here is a fault of a test's input, found without a GPU."""

import numpy as np
import pytest

import prep_ref as P
from oracle import cpu_ref as o


def test_lds_arithmetic():
    # 32 conformers x (3 A_all + 1) doubles + A_all ints + 8 bytes
    assert P.prep_lds_bytes(1) == 32 * 4 * 8 + 4 + 8
    assert [P.prep_lds_bytes(a) for a in (84, 85, 209, 210)] == [65112, 65884, 161612, 162384]
    assert not P.prep_raises_lds_attribute(84) and P.prep_raises_lds_attribute(85)
    assert P.prep_by_tiles(209) and not P.prep_by_tiles(210)
    assert max(a for a in range(1, 600) if P.complete_is_tiled(a)) == P.TILED_MAX_ATOMS == 416
    # rmsd_values: (A4 * 192 + 192) * 8 + 488 bytes
    assert (104 * 192 + 192) * 8 + 488 <= P.LDS_LIMIT < (108 * 192 + 192) * 8 + 488 and P.VALUES_MAX_ATOMS == 104
    assert P.load_tail_is_odd(33, 5) and P.load_tail_is_odd(63, 33) and P.load_tail_is_odd(1, 1)
    assert not P.load_tail_is_odd(64, 33) and not P.load_tail_is_odd(33, 84) and not P.load_tail_is_odd(34, 5)


@pytest.mark.parametrize("a_all", [33, 85, 210])
def test_masks(a_all):
    assert P.atom_mask("none", a_all) is None and len(P.selection(None, a_all)) == a_all
    count = {k: int(P.atom_mask(k, a_all).sum()) for k in P.MASKS[1:]}
    assert count["drop_first"] == count["drop_last"] == a_all - 1 and count["every_other"] == (a_all + 1) // 2
    assert not P.atom_mask("drop_first", a_all)[0] and not P.atom_mask("drop_last", a_all)[-1]
    assert count["single"] == 1 and count["three"] == 3 and not P.atom_mask("single", a_all)[0]
    assert [count[f"mod{k}"] % 4 for k in (1, 2, 3)] == [1, 2, 3] and all(count[f"mod{k}"] > a_all // 2 - 1 for k in (1, 2, 3))
    if a_all == 210:
        assert P.atom_mask("n104", 210).sum() == 104 and P.atom_mask("n105", 210).sum() == 105
    sel = P.selection(P.atom_mask("mod2", a_all), a_all)
    assert np.all(np.diff(sel) > 0) and not np.array_equal(sel, np.arange(len(sel)))  # ascending, and no prefix


def test_placements():
    X, c = P.build(7, 9, placement="centred", seed=1)
    assert c and X.shape == (9, 7, 3) and X.flags.c_contiguous
    Xo, c = P.build(7, 9, placement="origin", seed=1)
    assert not c and not Xo[:, 0].any() and np.allclose(Xo, X - X[:, :1])
    Xr, c = P.build(7, 9, placement="raw", seed=1)
    assert not c and np.array_equal(Xr, X)
    Xf, c = P.build(7, 9, placement="far", seed=1)
    assert c and np.allclose(Xf - X, P.FAR_SHIFT)
    Xd, _ = P.build(7, 9, seed=1, duplicate=True)
    assert np.array_equal(Xd[-1], Xd[1]) and np.array_equal(Xd[:-1], X[:-1]) and P.duplicated(9) == 1
    assert P.duplicated(2) == 0 and np.array_equal(*P.build(3, 2, seed=1, duplicate=True)[0])
    # about the origin the members of a cluster stay close without centring, as generated they do not
    ro = P.PairRef(Xo, False).r
    rr = P.PairRef(Xr, False).r
    assert ro.min() < 0.2 and rr.min() > 1.0
    for kind in ("blob", "far250", "linear"):
        assert P.build(5, 4, kind=kind, seed=2)[0].shape == (4, 5, 3)


def test_pair_reference_is_the_oracles_matrix():
    X, _ = P.build(12, 40, seed=3)
    mask = P.atom_mask("every_other", 12)
    ref = P.PairRef(X[:, mask], True, block=100)
    S0, R0, D0 = o.rmsd_similarity_matrix(X[:, mask], np.array(["C"] * 6), 0.5)
    assert np.array_equal(ref.R, R0) and np.array_equal(ref.D, D0) and np.array_equal(ref.similar(0.5), S0)
    assert np.array_equal(ref.R[ref.iu, ref.ju], ref.r) and not np.diag(ref.B).any()
    one = o.rmsd_and_max(X[3][mask], X[17][mask], center=True)
    assert abs(ref.R[17, 3] - one[0]) < 1e-14 and abs(ref.D[3, 17] - one[1]) < 1e-13
    # without centring: the plain rotation about the origin
    ref = P.PairRef(X[:, mask], False)
    one = o.rmsd_and_max(X[3][mask], X[17][mask])
    assert abs(ref.R[3, 17] - one[0]) < 1e-14


def test_split_threshold_and_pair_list():
    r = np.array([0.07, 0.071, 0.08, 1.0, 1.1, 1.4, 1.45, 1.5, 1.52, 1.53, 3.0, 3.1])
    thr, half = P.split_threshold(r)
    assert thr == pytest.approx(1.25) and half == pytest.approx(0.15)
    assert P.split_threshold([]) == (0.5, np.inf)
    thr, half = P.split_threshold([0.3])
    assert thr > 0.3 and half == pytest.approx(thr - 0.3)
    thr, half = P.split_threshold([0.2, 0.9, 0.4])
    assert thr == pytest.approx(0.55) and half == pytest.approx(0.15)
    i, j = P.pair_list(40, np.random.default_rng(0))
    assert len(i) == len(j) == 257 and (i > j).any() and (i < j).any() and (i == j).sum() >= 2
    assert (i[2], j[2]) == (i[3], j[3]) == (39, 0) and (i[P.DUPLICATE_AT], j[P.DUPLICATE_AT]) == (39, 1)
    assert i.min() >= 0 and i.max() < 40 and j.min() >= 0 and j.max() < 40
    i, j = P.pair_list(1, np.random.default_rng(0))
    assert not i.any() and not j.any()


def _all_cases():
    return [c + ("none",) for c in P.BASE_CASES] + [(a, n, "clusters", p, False, m) for a, n, m, p in P.masked_cases()]


def test_every_case_is_listed_once():
    cases = _all_cases()
    assert len(set(cases)) == len(cases)
    for a_all, n in P.MASK_SHAPES:
        assert {m for a, _, m, _ in P.masked_cases() if a == a_all} >= set(P.MASKS[1:])
    assert {c[3] for c in cases} == set(P.PLACEMENTS)
    assert {c[2] for c in cases} == {"clusters", "blob", "far250", "linear"} and any(c[4] for c in cases)
    assert all(a <= 209 for a, _, _, _ in P.TWIN_CASES) and {p for _, _, _, p in P.TWIN_CASES} == {"centred", "origin", "far"}


@pytest.mark.parametrize("a_all,n,kind,placement,duplicate,mask_kind", [c for c in _all_cases() if c[0] <= 85])
def test_case_inputs(a_all, n, kind, placement, duplicate, mask_kind):
    """The inputs of the GPU cases up to 85 atoms (the larger ones take the same path through this module and are
    checked where they run): thresholds clear of every pair, both verdicts, bounds as claimed, the far cases' margin."""
    X, center, mask, sel, ref = P.case(a_all, n, kind, placement, duplicate, mask_kind)
    P.check_bounds(ref, kind, len(sel), center)
    thr = P.case_threshold(ref, len(sel) == 1 and center)
    assert thr > 0
    if placement == "far":
        dr, dd = P.far_self_agreement(X, sel, ref)
        assert dr < 1e-13 and dd < 1e-11
    if duplicate and n >= 2:
        assert ref.R[P.duplicated(n), n - 1] < 1e-13


@pytest.mark.parametrize("a_all,n", [(33, 150), (211, 100)])
def test_gather_ensemble(a_all, n):
    X, atoms = P.gather_ensemble(a_all, n)
    assert X.shape == (n, a_all, 3) and (atoms == "H").any() and (atoms != "H").sum() > 3
    m1, both = P.gather_reference(X, atoms, 0.5)
    assert 1 < both.sum() < m1.sum() < n and not (both & ~m1).any()
