"""The references of tests/embed_ref.py against the oracle's literal loops at tiny sizes, and the input conditions
the GPU tests of the embed kernels (tests/test_gpu_embed_kernels.py) rely on, for exactly their seeds and shapes:
zero undecidable de-duplication groups at the 1e-9 margin, zero invalid string-embed cases at the 1e-7 margin, and
the regimes each case is there for (more than 128 poses kept, a hit found only beyond kept index 64, more than 256
fingerprints kept before the last chunk, ...).  Everything here uses the oracle's transforms; the GPU tests assert
the same conditions again on the GPU's own transforms."""

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import embed_ref as E
from oracle import cpu_ref as o


def _tiny(seed=11, n1=2, n2=3, A1=5, A2=4, nr1=2, nr2=1):
    m1, r1, pv1, m2, r2, pv2 = E.bimol_case(seed, n1, n2, A1, A2, nr1=nr1, nr2=nr2)
    a1, a2 = np.array([-40.0, 0.0, 25.0]), np.array([-10.0, 35.0])
    R1, t1 = E.mol_transforms(m1, r1, pv1, 0, a1)
    R2, t2 = E.mol_transforms(m2, r2, pv2, 1, a2)
    return m1, r1, pv1, m2, r2, pv2, a1, a2, R1, t1, R2, t2


def _oracle_poses(case):
    """pose of every (c2, c1, o, a2, a1) by the oracle's two-molecule call and get_embed"""
    m1, r1, pv1, m2, r2, pv2, a1, a2 = case[:8]
    out = {}
    for c2 in range(len(m2)):
        for c1 in range(len(m1)):
            for ori in (0, 1):
                for i2, ang2 in enumerate(a2):
                    for i1, ang1 in enumerate(a1):
                        Ra, ta, Rb, tb = o.bimol_pose_transforms(m1[c1], m2[c2], r1, r2, pv1[c1], pv2[c2], (ang1, ang2), ori)
                        out[c2, c1, ori, i2, i1] = (Ra, ta, Rb, tb, o.get_embed([m1[c1], m2[c2]], [Ra, Rb], [ta, tb]))
    return out


@pytest.mark.parametrize("nr1,nr2", [(2, 1), (1, 2)])
def test_transforms_and_tables_equal_the_two_molecule_oracle(nr1, nr2):
    """the one-molecule restatement (a stand-in in the other slot) gives the transforms of the oracle's
    two-molecule call bit for bit, and the tables are the oracle's poses to rounding"""
    case = _tiny(nr1=nr1, nr2=nr2)
    m1, _, _, m2, _, _, _, _, R1, t1, R2, t2 = case
    X1, X2 = E.tables(m1, R1, t1), E.tables(m2, R2, t2)
    for (c2, c1, ori, i2, i1), (Ra, ta, Rb, tb, pose) in _oracle_poses(case).items():
        assert np.array_equal(Ra, R1[c1, ori, i1]) and np.array_equal(ta, t1[c1, ori, i1])
        assert np.array_equal(Rb, R2[c2, ori, i2]) and np.array_equal(tb, t2[c2, ori, i2])
        assert np.abs(np.concatenate([X1[c1, ori, i1], X2[c2, ori, i2]]) - pose).max() < 1e-13


@pytest.mark.parametrize("thresh,max_clashes", [(1.5, 0), (2.2, 1), (2.6, 5), (9.0, 100), (1e-3, 0)])
def test_grid_reference_equals_literal_loops_and_oracle(thresh, max_clashes):
    case = _tiny()
    m1, _, _, m2 = case[:4]
    X1, X2 = E.tables(m1, case[8], case[9]), E.tables(m2, case[10], case[11])
    ok, cnt = E.grid_reference(X1, X2, thresh, max_clashes)
    ok_l, cnt_l = E.grid_literal(X1, X2, thresh, max_clashes)
    assert np.array_equal(ok, ok_l) and np.array_equal(cnt, cnt_l)
    full = np.zeros(ok.shape, dtype=np.int64)
    for key, (_, _, _, _, pose) in _oracle_poses(case).items():
        assert ok[key] == o.compenetration_check(pose, ids=[m1.shape[1], m2.shape[1]], thresh=thresh, max_clashes=max_clashes)
        full[key] = np.count_nonzero(cdist(pose[m1.shape[1]:], pose[:m1.shape[1]]) < thresh)
    # counts: equal to the full count until the limit is passed, then just above the limit and never above the full count
    assert np.array_equal(cnt[ok], full[ok])
    assert (cnt[~ok] > max_clashes).all() and (cnt <= full).all()
    if max_clashes == 5:
        assert (cnt < full).any() and ok.any() and not ok.all()  # the cut-off is visible in this case


def test_counts_ignore_nan_and_inf():
    case = _tiny()
    m1, m2 = case[0].copy(), case[3].copy()
    m1[0, 2, 1], m1[1, 2, 0], m2[0, 1, 2], m2[1, 1, 0] = np.nan, np.inf, np.nan, np.inf
    X1, X2 = E.tables(m1, case[8], case[9]), E.tables(m2, case[10], case[11])
    C1, C2 = E.tables(case[0], case[8], case[9]), E.tables(case[3], case[10], case[11])
    ok, cnt = E.grid_reference(X1, X2, 2.2, 50)
    # the same count as with those two atoms taken out of each molecule
    ref = np.zeros_like(cnt)
    for c2 in range(3):
        for c1 in range(2):
            k1 = [a for a in range(5) if not (c1 in (0, 1) and a == 2)]
            k2 = [b for b in range(4) if not (c2 in (0, 1) and b == 1)]
            _, ref[c2:c2 + 1, c1:c1 + 1] = E.grid_reference(C1[c1:c1 + 1][:, :, :, k1], C2[c2:c2 + 1][:, :, :, k2], 2.2, 50)
    assert np.array_equal(cnt, ref) and cnt.max() > 0


def test_pose_index_is_the_oracle_loop_order():
    n1, n2, na1, na2 = 2, 3, 3, 4
    k = 0
    for c1, c2 in o.cartesian_product(range(n1), range(n2)):
        for ori in (0, 1):
            for i1, i2 in o.cartesian_product(range(na1), range(na2)):
                assert E.pose_index(n1, n2, na1, na2, c2, c1, ori, i2, i1) == k
                assert np.ravel_multi_index((c2, c1, ori, i2, i1), (n2, n1, 2, na2, na1)) == k
                k += 1


def test_kabsch_equals_oracle_rmsd_and_max():
    rng = np.random.default_rng(5)
    p, Q = rng.normal(size=(7, 3)) + 2.0, rng.normal(size=(9, 7, 3)) + 2.0
    Q[3] = p  # identical structures
    Q[4] = -p  # the inverted structure: the proper rotation is not the identity
    r, m = E.kabsch_rmsd_max(p, Q)
    for k in range(len(Q)):
        r0, m0 = o.rmsd_and_max(p, Q[k])
        assert abs(r[k] - r0) < 1e-12 and abs(m[k] - m0) < 1e-12
    assert r[3] < 1e-12 and r[4] > 0.5


@pytest.mark.parametrize("thr", [0.4, 1.0])
def test_dedupe_reference_equals_oracle_loop(thr):
    case = _tiny(seed=13)
    m1, _, _, m2, _, _, a1, a2 = case[:8]
    X1, X2 = E.tables(m1, case[8], case[9]), E.tables(m2, case[10], case[11])
    ok, _ = E.grid_reference(X1, X2, 0.8, 0)
    ref = E.dedupe_reference(X1, X2, ok, thr)
    poses = _oracle_poses(case)
    acc = np.zeros_like(ok)
    for c1, c2 in o.cartesian_product(range(len(m1)), range(len(m2))):
        for ori in (0, 1):
            angular = []
            for i1, i2 in o.cartesian_product(range(len(a1)), range(len(a2))):
                pose = poses[c2, c1, ori, i2, i1][4]
                if ok[c2, c1, ori, i2, i1] and not o.rmsd_similarity(pose, np.array(angular), rmsd_thr=thr):
                    angular.append(pose)
                    acc[c2, c1, ori, i2, i1] = True
    assert ref["margin"].min() > 1e-6
    assert np.array_equal(ref["acc"], acc)
    assert 0 < acc.sum() and (thr < 0.5 or acc.sum() < ok.sum())
    assert np.array_equal(ref["n_kept"], acc.sum(axis=(-1, -2)))
    assert ((ref["first_hit"] >= 0) == (ok & ~acc)).all()


def check_dedupe_conditions(name, case, ok, ref):
    """what each de-duplication case is there for; shared with the GPU tests"""
    assert (ref["margin"] < E.DEDUPE_MARGIN).sum() == 0, "undecidable groups"  # the cap is zero
    na1, na2 = len(case["angles1"]), len(case["angles2"])
    if name == "kept":
        assert ok.all() and ref["n_kept"].max() > 128  # three trips over the kept poses
    elif name == "late_hit":
        late = ref["first_hit"][..., 11, :]             # poses (a1, 11) repeat poses (a1, 6)
        assert ok.all() and not ref["acc"][..., 11, :].any() and (late >= 64).all()
        assert ref["acc"][..., :11, :].all()
    elif name == "most_rejected":
        assert 0 < ref["acc"].sum() < 0.1 * ok.sum() and not ok.all()
    elif name == "all_clash":
        assert not ok.any() and not ref["acc"].any()
    elif name == "lds_limit":
        assert na1 * na2 == 4096 and ok.sum() > 4000 and ref["n_kept"].max() <= 4
    elif name == "stride":
        assert 0 < ok.sum() < ok.size and 0 < ref["acc"].sum() < ok.sum()


@pytest.mark.parametrize("name", E.DEDUPE_CASES)
def test_dedupe_cases_are_decidable_and_reach_their_regime(name):
    case = E.dedupe_case(name)
    if name == "stride":
        assert 2 * len(case["m1"]) * len(case["m2"]) > 32 * E.MI355X_CUS >= 2 * (len(case["m1"]) - 1) ** 2
    X1, X2 = E.dedupe_tables(case)
    ok, _ = E.grid_reference(X1, X2, case["thresh"], 0)
    check_dedupe_conditions(name, case, ok, E.dedupe_reference(X1, X2, ok, case["rmsd_thr"]))


def _string_reference(name):
    c = E.string_case(name)
    R2, t2, i1, i2 = E.string_transforms(c["c1"], c["v1"], c["c2"], c["v2"], c["angles"])
    ok = E.string_clash_pass(c, R2, t2, i1, i2)
    tf = E.string_fingerprints(c["m1"], c["m2"], i1, i2, R2, t2, c["quads"])
    return c, ok, tf, E.string_filter(tf, ok, c["tfd_thresh"]), (i1, i2)


def check_string_conditions(name, case, ok, f):
    """what each string-embed case is there for; shared with the GPU tests"""
    assert f["margin"] >= E.TFD_MARGIN, "a comparison within the exclusion margin"  # cap: zero invalid cases
    P = len(ok)
    assert P == {"P255": 255, "P256": 256, "P257": 257, "P700": 700}.get(name, 300)
    if name == "P257":
        assert f["kept_before"] == [0, 256] and f["kept_in"] == [256, 1]  # a full chunk kept, n_acc carried into the second
    if name == "P700":
        assert len(f["kept_before"]) == 3 and f["kept_before"][-1] > 256   # second trip over the kept list
        assert min(f["kept_in"]) > 0 and max(f["kept_in"]) > 64            # kept in every chunk, dense in one
        stale = [p for p in range(256, P) if not ok[p] and f["early"][p - 256]]
        assert stale  # a clash-failing pose where the previous chunk left rejected[] set
        assert 0 < ok.sum() < P and f["acc"].sum() < ok.sum()
    if name.startswith("Q"):
        assert len(case["quads"]) == int(name[1:]) and f["kept_before"][1] > 64 and f["early"].any()
        q = case["quads"]
        if len(q) >= 4:
            assert (q[2] < E.STRING_A1).all() and (q[3] >= E.STRING_A1).all()
        assert q[0].min() < E.STRING_A1 <= q[0].max()


@pytest.mark.parametrize("name", E.STRING_CASES)
def test_string_cases_are_valid_and_reach_their_regime(name):
    c, ok, tf, f, _ = _string_reference(name)
    check_string_conditions(name, c, ok, f)


@pytest.mark.parametrize("name", ["P256", "Q1", "Q9"])
def test_string_reference_equals_oracle_loop(name):
    """fingerprints, clash verdicts, the filter and the pose order against oracle.cpu_ref.string_embed"""
    c, ok, tf, f, (i1, i2) = _string_reference(name)
    ok0, acc0, poses0 = o.string_embed(c["m1"], c["m2"], c["c1"], c["v1"], c["c2"], c["v2"], c["angles"], c["quads"],
                                       thresh=c["thresh"], tfd_thresh=c["tfd_thresh"])
    assert np.array_equal(ok, ok0) and np.array_equal(f["acc"], acc0)
    sel = np.flatnonzero(acc0)
    tf0 = np.array([o.get_torsion_fingerprint(p, c["quads"]) for p in poses0])
    d = np.abs(tf[sel] - tf0)
    assert np.minimum(d, 360 - d).max() < 1e-9
    assert np.array_equal(poses0[:, :E.STRING_A1], c["m1"][i1[sel]])
    n1, n2, K1, K2, nA = len(c["m1"]), len(c["m2"]), c["c1"].shape[1], c["c2"].shape[1], len(c["angles"])
    p = 0
    for c1, c2 in o.cartesian_product(range(n1), range(n2)):
        for k1, k2 in o.cartesian_product(range(K1), range(K2)):
            for ia in range(nA):
                assert E.string_pose_index(n1, n2, K1, K2, nA, c1, c2, k1, k2, ia) == p and (i1[p], i2[p]) == (c1, c2)
                p += 1


def test_special_molecules_hit_their_branches():
    sp = E.special_mols()
    for name in ("degenerate2", "degenerate1"):
        x, r, pv = sp[name]
        assert np.array_equal(x[1][r].mean(axis=0), pv[1].mean(axis=0))       # exactly: the substitution happens
        assert not np.array_equal(x[0][r].mean(axis=0), pv[0].mean(axis=0))
    x, r, pv = sp["parallel"]
    direction, pivot = pv[0].mean(axis=0) - x[0][r].mean(axis=0), pv[0, 0] - pv[0, 1]
    assert np.array_equal(np.cross(direction, pivot), np.zeros(3)) and direction @ pivot > 0
    x, r, pv = sp["antiparallel_x"]
    pivot = pv[0, 0] - pv[0, 1]
    assert pivot[0] < 0 and pivot[1] == 0 and pivot[2] == 0 and (pv[0].mean(axis=0) - x[0][r].mean(axis=0))[0] == 0
