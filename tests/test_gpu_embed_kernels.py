"""The embed kernels (fc_embed.hip, fc_embed3.hip and the string embed's novelty filter in fc_prune.hip) across
shapes, strips, ties and LDS limits, each against a plain reference of the same operation (tests/embed_ref.py,
oracle.cpu_ref, oracle.cyclical_ref).

* transforms: the oracle to TOL = 1e-10 (R) and TOL * max(1, largest |coordinate or pivot|) (t: the error of R
  times the lever arm).
* pose grid: pass flags AND counts equal to a reference that has no tolerance -- the GPU's own R, t (the same
  deterministic kernel), the tables rebuilt on the host with the kernel's literal expression, cdist, ``< thresh``
  -- for both kernels (FC_GRID_F64=0 and 1).
* de-duplication, string embed: sequential walks; the references record how close any comparison came to a
  threshold.  Exclusion margins 1e-9 A and 1e-7 degrees, cap ZERO excluded groups / cases in every test below
  (asserted; tests/test_embed_ref.py asserts the same on the oracle's transforms without a GPU).  The measured
  kernel-versus-reference differences these margins stand on are in DESIGN.md ("What the embed tests pin down").
* trimolecular: the oracle group by group, as tests/test_gpu_parity.py does."""

import numpy as np
import pytest

import embed_ref as E
from firecode_amd import _lib as L
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o
from test_embed_ref import check_dedupe_conditions, check_string_conditions

pytestmark = pytest.mark.gpu

TOL = E.TOL


# ---------------------------------------------------------------------------------------------------------
# 1. per-molecule transforms
# ---------------------------------------------------------------------------------------------------------
def _check_transforms(fc, coords, reactive, pivots, mol, angles):
    R, t = fc.embeds.embed_mol_transforms(coords, reactive, pivots, mol, angles)
    R0, t0 = E.mol_transforms(coords, reactive, pivots, mol, angles)
    lever = max(1.0, float(np.abs(coords).max()), float(np.abs(pivots).max()))
    err_R, err_t = np.abs(R - R0).max(), np.abs(t - t0).max()
    print(f"transforms {R.shape[:3]} mol {mol}: |dR| {err_R:.2e}  |dt| {err_t:.2e}  lever {lever:.1f}")
    assert err_R < TOL and err_t < TOL * lever
    return R, t


@pytest.mark.parametrize("n,na", [(1, 1), (2, 1), (1, 2), (63, 1), (7, 9), (64, 1), (8, 8), (5, 13), (65, 1), (10, 13)])
@pytest.mark.parametrize("nr", [1, 2])
def test_mol_transforms_vs_oracle(fc, n, na, nr):
    """n*na in {1, 2, 63, 64, 65, 130} structures, i.e. 2, 4, 126, 128, 130 and 260 transforms (one lane each,
    64-thread blocks; the orientation doubles every count, so the odd totals of the plan are taken per
    orientation), both molecules, 1 and 2 reactive atoms at indices 0 and A-1, A in {1, 2, 65}"""
    for A in (1, 2, 65):
        if nr > A:
            continue
        rng = np.random.default_rng(1000 * n + 10 * na + A)
        coords = rng.normal(scale=1.8, size=(n, A, 3))
        reactive = np.array([0, A - 1][:nr])
        pivots = np.stack([coords[:, reactive[0]] * 1.6 + rng.normal(scale=0.3, size=(n, 3)),
                           coords[:, reactive[-1]] * 1.6 + rng.normal(scale=0.3, size=(n, 3)) + (0 if nr == 2 else 1.2)], axis=1)
        angles = np.linspace(-170.0, 175.0, na) if na > 1 else np.array([30.0])
        for mol in (0, 1):
            _check_transforms(fc, coords, reactive, pivots, mol, angles)


@pytest.mark.parametrize("name", ["degenerate2", "degenerate1", "antiparallel_x"])
def test_mol_transforms_special_alignments(fc, name):
    """the reactive atoms' mean exactly on the pivot midpoint (the molecule direction is replaced by the midpoint;
    dyadic coordinates make the equality exact), and a pivot antiparallel to the x axis (a 180-degree alignment):
    the alignment is unique in both, so the oracle is the reference"""
    coords, reactive, pivots = E.special_mols()[name]
    for mol in (0, 1):
        _check_transforms(fc, coords, reactive, pivots, mol, np.array([-60.0, 0.0, 45.0, 180.0]))


def test_mol_transforms_rank_one_alignment(fc):
    """a pivot parallel to the molecule direction: the covariance of the alignment has rank one and the best
    rotation is not unique (any turn about the pivot is as good), so kernel and oracle need not agree and the test
    asserts what every correct answer shares instead.  With pivot p and direction d both along the unit vector e,
    the covariance is u1 e^T with u1 ~ (s |p|^2, +-|d|, 0) (s: the sign of the polygon side, +- : +y for molecule
    0, -y for molecule 1), so every optimal alignment maps e onto u1/|u1| and is free only in the turn about it;
    with one reactive atom the step rotation turns about that very axis.  Hence: R is a proper rotation, R e =
    u1/|u1|, and the pose puts the pivot midpoint on the origin (the step rotation's centre, the reactive atom,
    lies on the axis through the midpoint).  The oracle is held to the same assertions, which shows that they are
    the operation's and not the kernel's."""
    coords, reactive, pivots = E.special_mols()["parallel"]
    angles = np.array([-60.0, 0.0, 45.0, 180.0])
    pivot, mid = pivots[0, 0] - pivots[0, 1], pivots[0].mean(axis=0)
    for mol in (0, 1):
        gpu = fc.embeds.embed_mol_transforms(coords, reactive, pivots, mol, angles)
        for R, t in (gpu, E.mol_transforms(coords, reactive, pivots, mol, angles)):
            assert np.isfinite(R).all() and np.isfinite(t).all()
            for ori in (0, 1):
                sgn, diry = (-1.0 if (ori == 1 and mol == 1) else 1.0), (1.0 if mol == 0 else -1.0)
                side = np.array([sgn * (pivot @ pivot), diry * np.linalg.norm(mid - coords[0, 0]), 0.0])
                side /= np.linalg.norm(side)
                for k in range(len(angles)):
                    Rk, tk = R[0, ori, k], t[0, ori, k]
                    assert np.abs(Rk @ Rk.T - np.eye(3)).max() < TOL and abs(np.linalg.det(Rk) - 1.0) < TOL
                    assert np.abs(Rk @ (pivot / np.linalg.norm(pivot)) - side).max() < TOL
                    assert np.abs(Rk @ mid + tk).max() < TOL * max(1.0, np.abs(pivots).max())


# ---------------------------------------------------------------------------------------------------------
# 2. pose grid
# ---------------------------------------------------------------------------------------------------------
def _grid_tables(fc, m1, r1, pv1, m2, r2, pv2, a1, a2):
    R1, t1 = fc.embeds.embed_mol_transforms(m1, r1, pv1, 0, a1)
    R2, t2 = fc.embeds.embed_mol_transforms(m2, r2, pv2, 1, a2)
    return E.tables(m1, R1, t1), E.tables(m2, R2, t2)


def _check_grid(fc, monkeypatch, mols, a1, a2, settings, D=None):
    """both kernels against the reference for every (thresh, max_clashes) of ``settings``; -> D, [(ok, counts)]"""
    m1, r1, pv1, m2, r2, pv2 = mols
    if D is None:
        D = E.grid_distances(*_grid_tables(fc, m1, r1, pv1, m2, r2, pv2, a1, a2))
    out = []
    for thresh, mc in settings:
        ref_ok, ref_cnt = E.grid_from_distances(D, thresh, mc)
        for f64 in ("0", "1"):
            monkeypatch.setenv("FC_GRID_F64", f64)
            ok, cnt, _ = fc.embeds.embed_grid_clash(m1, r1, pv1, m2, r2, pv2, a1, a2, thresh=thresh, max_clashes=mc,
                                                    return_counts=True)
            assert np.array_equal(ok, ref_ok), (thresh, mc, f64)
            assert np.array_equal(cnt, ref_cnt), (thresh, mc, f64)
        out.append((ref_ok, ref_cnt))
    return D, out


def _angles(na, lo=-150.0, hi=160.0):
    return np.linspace(lo, hi, na) if na > 1 else np.array([20.0])


@pytest.mark.parametrize("n2,na2", [(1, 1), (63, 1), (7, 9), (64, 1), (8, 8), (1, 64), (65, 1), (5, 13), (255, 1), (15, 17),
                                    (16, 16), (1, 256), (257, 1), (1, 257), (513, 1), (19, 27)])
def test_grid_strip_and_padding_edges(fc, monkeypatch, n2, na2):
    """n2*na2 molecule-2 structures around the 64-structure padding of the table and the 256-lane strip, in both
    factorisations (the lane's s2 -> (c2, a2)); one workgroup row (n1 = na1 = 1), an odd A1 (the padding atom)"""
    mols = E.bimol_case(500 + n2 + na2, 1, n2, 5, 3, scale=1.2)
    _, out = _check_grid(fc, monkeypatch, mols, _angles(1), _angles(na2), [(1.5, 0), (1.5, 1)])
    if n2 > 60:
        assert 0 < out[0][0].sum() < out[0][0].size


def _factor(k):
    d = max(f for f in range(1, int(k ** 0.5) + 1) if k % f == 0)
    return k // d, d


def test_grid_capped_strips(fc, monkeypatch):
    """more workgroup rows than half of 16 per compute unit: the launcher's formula grants 2 strips where the 704
    padded molecule-2 structures ask for 3, so lanes take a second s2 (s2 += strips*256)"""
    n_cu = fc.device_info()["n_cu"]
    n1, na1 = _factor(4 * n_cu + 1)        # g1 = n1*2*na1 = 8 n_cu + 2: just above 16 n_cu / 2
    n2, na2 = 28, 25
    g1, S2 = n1 * 2 * na1, -(-(n2 * na2) // 64) * 64
    want = -(-(16 * n_cu) // g1)
    assert S2 == 704 and -(-S2 // 256) == 3 and want == 2   # the cap is reached on this device
    mols = E.bimol_case(520, n1, n2, 2, 3, scale=1.2)
    _, out = _check_grid(fc, monkeypatch, mols, _angles(na1), _angles(na2), [(1.5, 0)])
    ok = out[0][0]
    assert 0 < ok.sum() < ok.size
    second = ok.transpose(0, 3, 1, 2, 4).reshape(n2 * na2, -1)[512:]   # rows s2 = c2*na2 + a2 of a lane's second turn
    assert 0 < second.sum() < second.size


@pytest.mark.parametrize("A1,A2", [(1, 9), (2, 9), (3, 9), (127, 9), (128, 9), (129, 9), (1636, 17),
                                   (5, 1), (5, 7), (5, 8), (5, 16), (5, 17)])
def test_grid_atom_count_edges(fc, monkeypatch, A1, A2):
    """A1: the odd-pair padding atom, the 256-thread LDS fill loops, the largest A1 accepted; A2 around the groups
    of FC_GRID_NB = 8 molecule-2 atoms (the tail group is clamped to A2-1)"""
    mols = E.bimol_case(540 + A1 + A2, 2, 3, A1, A2, scale=(1.8 if A1 < 100 else 6.0))
    thresh = 1.5 if A1 < 100 else 0.9
    _check_grid(fc, monkeypatch, mols, _angles(3), _angles(2), [(thresh, 0), (thresh, 1), (thresh, 5), (thresh, A1 * A2)])


def test_grid_refuses_a1_beyond_the_lds_stage_and_goes_on(fc, monkeypatch):
    big = E.bimol_case(560, 1, 1, 1637, 2)
    with pytest.raises(fc.FirecodeHipInputError) as err:
        fc.embeds.embed_grid_clash(*big, _angles(2), thresh=1.5)
    assert err.value.code == L.FC_E_LIMIT
    with pytest.raises(fc.FirecodeHipInputError) as err:
        fc.embeds.embed_grid_poses(*big, _angles(2), thresh=1.5)
    assert err.value.code == L.FC_E_LIMIT
    mols = E.bimol_case(561, 2, 2, 4, 3)
    _, out = _check_grid(fc, monkeypatch, mols, _angles(3), _angles(3), [(1.5, 0)])
    assert 0 < out[0][0].sum() < out[0][0].size


def test_grid_thresholds_on_distances_and_clash_limits(fc, monkeypatch):
    """300 molecule-2 structures (a second strip); thresholds exactly on interatomic distances of the rebuilt
    tables, one ulp below and above, tiny and huge; max_clashes 0, 1, 5 and A1*A2 (nothing ever stops)"""
    A1, A2 = 7, 9
    mols = E.bimol_case(570, 2, 20, A1, A2, scale=1.5)
    a1, a2 = _angles(3), _angles(15)
    D = E.grid_distances(*_grid_tables(fc, *mols, a1, a2))
    d = np.sort(np.concatenate([D[0].reshape(-1), D[1].reshape(-1)]))
    picks = [float(d[0]), float(d[5]), float(d[len(d) // 50]), float(d[len(d) // 4])]
    thresholds = [1e-3, 1e3] + [t for x in picks for t in (x, float(np.nextafter(x, 0.0)), float(np.nextafter(x, np.inf)))]
    settings = [(t, mc) for t in thresholds for mc in (0, 1, 5, A1 * A2)]
    _, out = _check_grid(fc, monkeypatch, mols, a1, a2, settings, D=D)
    rates = {s: ok.mean() for s, (ok, _) in zip(settings, out)}
    assert rates[(1e-3, 0)] == 1.0 and rates[(1e3, 5)] == 0.0 and rates[(1e3, A1 * A2)] == 1.0
    assert sum(0.0 < r < 1.0 for r in rates.values()) >= 8          # mixed
    # a threshold exactly ON the smallest distance: that pair is suspicious to the fp32 screen, the exact recount
    # finds no clash (d < d is false) and the lane resumes behind that atom -- every pose passes with count 0,
    # one ulp above exactly the poses holding that pair fail
    ok_on, cnt_on = out[settings.index((picks[0], 0))]
    ok_up, cnt_up = out[settings.index((float(np.nextafter(picks[0], np.inf)), 0))]
    b_of_pair = np.argwhere(np.stack(D) == picks[0])[0][3]
    assert ok_on.all() and cnt_on.max() == 0 and b_of_pair < A2 - 1 and not ok_up.all() and cnt_up.max() >= 1
    # and on a larger distance with max_clashes = 5: lanes that went on counting after a recount without a clash
    ok5, cnt5 = out[settings.index((picks[2], 5))]
    ok5u, cnt5u = out[settings.index((float(np.nextafter(picks[2], np.inf)), 5))]
    assert (cnt5u - cnt5).max() >= 1 and (cnt5 > 0).any() and ok5.any()


def test_grid_pose_index(fc, monkeypatch):
    """p = ((c2*n1 + c1)*2 + o)*(na1*na2) + a2*na1 + a1 on the flat output, n1 != n2, na1 != na2, own angles2"""
    n1, n2, na1, na2, A1, A2 = 2, 3, 3, 4, 5, 6
    m1, r1, pv1, m2, r2, pv2 = E.bimol_case(580, n1, n2, A1, A2)
    a1, a2 = _angles(na1), _angles(na2, -100.0, 75.0)
    X1, X2 = _grid_tables(fc, m1, r1, pv1, m2, r2, pv2, a1, a2)
    from scipy.spatial.distance import cdist

    for f64 in ("0", "1"):
        monkeypatch.setenv("FC_GRID_F64", f64)
        ok, cnt, _ = fc.embeds.embed_grid_clash(m1, r1, pv1, m2, r2, pv2, a1, a2, thresh=3.5, max_clashes=A1 * A2,
                                                return_counts=True)
        flat = cnt.reshape(-1)
        seen = set()
        for c2 in range(n2):
            for c1 in range(n1):
                for ori in (0, 1):
                    for i2 in range(na2):
                        for i1 in range(na1):
                            full = np.count_nonzero(cdist(X2[c2, ori, i2], X1[c1, ori, i1]) < 3.5)
                            assert flat[E.pose_index(n1, n2, na1, na2, c2, c1, ori, i2, i1)] == full
                            seen.add(full)
        assert len(seen) > 5  # the counts tell the poses apart


@pytest.mark.parametrize("far", [1e3, 1e5, 1e7, 1e15, 1e16])
def test_grid_far_from_the_origin(fc, monkeypatch, far):
    """The kernel header's claim that results stay exact far from the origin.  A rigid translation of a molecule
    WITH its pivot cancels in the tables (the pose is built around the pivot), so besides translating both
    molecules and their pivots by ``far`` (1e3 .. 1e7: the tables then carry the rounding of that cancellation)
    a non-reactive atom of one conformer of each molecule is put ``far`` away from its pivot: the largest table
    coordinate M is ~far, the fp32 band (~M^2 2^-24) widens until nearly every atom is recounted, and from 1e15 on
    Tf = inf sends every atom down the exact path."""
    m1, r1, pv1, m2, r2, pv2 = E.bimol_case(590, 3, 4, 6, 7, scale=1.5)
    if far < 1e15:
        shift = far * np.array([1.0, -0.5, 0.25])
        m1, pv1, m2, pv2 = m1 + shift, pv1 + shift, m2 - shift, pv2 - shift
    m1[1, 2] += far * np.array([0.6, 0.8, 0.0])
    m2[2, 3] += far * np.array([0.0, -0.6, 0.8])
    a1, a2 = _angles(3), _angles(4)
    X1, X2 = _grid_tables(fc, m1, r1, pv1, m2, r2, pv2, a1, a2)
    assert 0.3 * far < max(np.abs(X1).max(), np.abs(X2).max()) < 3.0 * far
    D, out = _check_grid(fc, monkeypatch, (m1, r1, pv1, m2, r2, pv2), a1, a2, [(1.5, 0), (1.5, 2), (2.5, 5)],
                         D=E.grid_distances(X1, X2))
    assert 0 < out[0][0].sum() < out[0][0].size


@pytest.mark.parametrize("kind", ["nan", "inf", "both"])
def test_grid_nan_and_inf_coordinates(fc, monkeypatch, kind):
    """The kernel header's claim about NaN and +-inf: a non-reactive atom of one conformer of each molecule is NaN
    and / or +inf.  R and t depend on reactive atoms and pivots only, so only that atom's distances are affected,
    and the reference's ``<`` is false for NaN and inf: such pairs never count, everything else counts as before."""
    m1, r1, pv1, m2, r2, pv2 = E.bimol_case(600, 3, 4, 6, 7, scale=1.5)
    clean = (m1.copy(), r1, pv1, m2.copy(), r2, pv2)
    if kind in ("nan", "both"):
        m1[0, 2, 1], m2[1, 3, 0] = np.nan, np.nan
    if kind in ("inf", "both"):
        m1[2, 3, 0], m2[3, 2, 2] = np.inf, np.inf
    a1, a2 = _angles(3), _angles(4)
    D, out = _check_grid(fc, monkeypatch, (m1, r1, pv1, m2, r2, pv2), a1, a2, [(1.5, 0), (1.5, 2), (2.5, 40)])
    assert not np.isfinite(D[0]).all() and 0 < out[0][0].sum() < out[0][0].size
    # untouched conformer pairs are exactly what they are without the poisoned atoms
    Dc, outc = _check_grid(fc, monkeypatch, clean, a1, a2, [(2.5, 40)])
    assert np.array_equal(out[2][1][0, 1], outc[0][1][0, 1]) and (out[2][1] <= outc[0][1]).all()
    assert (out[2][1] < outc[0][1]).any()


# ---------------------------------------------------------------------------------------------------------
# 3. in-group de-duplication
# ---------------------------------------------------------------------------------------------------------
def _dedupe_raw(case, sentinel=7):
    """fc_embed_grid_dedupe with its output buffers pre-filled: every pose must be written"""
    X1, X2 = L.f64(case["m1"]), L.f64(case["m2"])
    r1, r2 = L.i64(case["r1"]), L.i64(case["r2"])
    ps1, pe1 = np.ascontiguousarray(case["pv1"][:, 0]), np.ascontiguousarray(case["pv1"][:, 1])
    ps2, pe2 = np.ascontiguousarray(case["pv2"][:, 0]), np.ascontiguousarray(case["pv2"][:, 1])
    a1, a2 = L.f64(case["angles1"]), L.f64(case["angles2"])
    shape = (len(X2), len(X1), 2, len(a2), len(a1))
    ok, acc = np.full(shape, sentinel, dtype=np.uint8), np.full(shape, sentinel, dtype=np.uint8)
    L.call("fc_embed_grid_dedupe", L.pf(X1), X1.shape[0], X1.shape[1], L.pi(r1), len(r1), L.pf(ps1), L.pf(pe1),
           L.pf(X2), X2.shape[0], X2.shape[1], L.pi(r2), len(r2), L.pf(ps2), L.pf(pe2), L.pf(a1), len(a1), L.pf(a2), len(a2),
           float(case["thresh"]), 0, float(case["rmsd_thr"]), L.pb(ok), L.pb(acc))
    return ok, acc


@pytest.mark.parametrize("name", E.DEDUPE_CASES)
def test_dedupe_vs_sequential_reference(fc, name):
    """kept: > 128 poses kept (three trips of k0 += 64) | late_hit: angles2[11] == angles2[6], the repeat of a pose
    whose kept index is >= 64 is found only by a later trip | most_rejected: a large rmsd_thr | all_clash |
    lds_limit: 64 x 64 angle pairs, the largest kept list accepted | stride: more groups than one launch covers
    (2 n^2 > 4 * 8 n_cu, from the device), every group written"""
    n_cu = fc.device_info()["n_cu"]
    case = E.dedupe_case(name, n_cu)
    if name == "stride":
        assert 2 * len(case["m1"]) * len(case["m2"]) > 32 * n_cu
    ok, acc = _dedupe_raw(case)
    assert set(np.unique(ok)) <= {0, 1} and set(np.unique(acc)) <= {0, 1}  # no sentinel left: every pose was written
    X1, X2 = E.dedupe_tables(case, fc.embeds.embed_mol_transforms)
    ref_ok, _ = E.grid_reference(X1, X2, case["thresh"], 0)
    assert np.array_equal(ok.astype(bool), ref_ok)
    ref = E.dedupe_reference(X1, X2, ref_ok, case["rmsd_thr"])
    check_dedupe_conditions(name, case, ref_ok, ref)   # zero undecidable groups, and the regime of the case
    assert np.array_equal(acc.astype(bool), ref["acc"])
    if name in ("kept", "late_hit", "most_rejected"):
        # the margin's footing: the same comparisons on the oracle's tables, and the GPU's own Kabsch on the poses
        cpu = E.dedupe_reference(*E.dedupe_tables(case), ref_ok, case["rmsd_thr"])
        assert np.array_equal(cpu["acc"], ref["acc"]) and cpu["values"].shape == ref["values"].shape
        print(f"dedupe {name}: {len(ref['values'])} comparisons, margin {ref['margin'].min():.3e}, "
              f"GPU-table vs oracle-table rmsd/maxdev {np.abs(cpu['values'] - ref['values']).max():.3e}")
        poses = np.array([np.concatenate([X1[0, 0, i % 12], X2[0, 0, i // 12]]) for i in range(144)])
        pi, pj = np.triu_indices(144, 1)
        r_gpu, m_gpu = fc.rmsd.rmsd_and_max_batch(poses, pi, pj, center=False)
        worst = 0.0
        for i in range(1, 144):
            r, m = E.kabsch_rmsd_max(poses[i], poses[:i])
            sel = pj == i
            worst = max(worst, np.abs(r_gpu[sel] - r).max(), np.abs(m_gpu[sel] - m).max())
        print(f"dedupe {name}: GPU Kabsch vs reference Kabsch over {len(pi)} pose pairs {worst:.3e}")
        assert worst * 100 < E.DEDUPE_MARGIN


def test_dedupe_refuses_too_many_angle_pairs_and_goes_on(fc):
    case = E.dedupe_case("lds_limit")
    case["angles1"] = np.linspace(-90.0, 90.0, 65)
    with pytest.raises(fc.FirecodeHipInputError) as err:
        _dedupe_raw(case)
    assert err.value.code == L.FC_E_LIMIT
    small = E.dedupe_case("most_rejected")
    ok, acc = _dedupe_raw(small)
    X1, X2 = E.dedupe_tables(small, fc.embeds.embed_mol_transforms)
    ref_ok, _ = E.grid_reference(X1, X2, small["thresh"], 0)
    assert np.array_equal(ok.astype(bool), ref_ok)
    assert np.array_equal(acc.astype(bool), E.dedupe_reference(X1, X2, ref_ok, small["rmsd_thr"])["acc"])


# ---------------------------------------------------------------------------------------------------------
# 4. string embed
# ---------------------------------------------------------------------------------------------------------
def _string_raw(c, quads=None):
    X1, X2 = L.f64(c["m1"]), L.f64(c["m2"])
    c1, v1, c2, v2 = (L.f64(c[k]) for k in ("c1", "v1", "c2", "v2"))
    ang, quads = L.f64(c["angles"]), L.i64(c["quads"] if quads is None else quads)
    n1, n2, K1, K2, nA = X1.shape[0], X2.shape[0], c1.shape[1], c2.shape[1], len(ang)
    P = n1 * n2 * K1 * K2 * nA
    ok, acc = np.full(P, 7, dtype=np.uint8), np.full(P, 7, dtype=np.uint8)
    R2, t2 = np.empty((P, 3, 3)), np.empty((P, 3))
    L.call("fc_string_embed", L.pf(X1), n1, X1.shape[1], L.pf(c1), L.pf(v1), K1, L.pf(X2), n2, X2.shape[1], L.pf(c2),
           L.pf(v2), K2, L.pf(ang), nA, L.pi(quads), quads.shape[0], float(c["thresh"]), 0, float(c["tfd_thresh"]),
           L.pb(ok), L.pb(acc), L.pf(R2), L.pf(t2))
    return ok, acc, R2, t2


@pytest.mark.parametrize("name", E.STRING_CASES)
def test_string_embed_chunks_and_fingerprint_counts(fc, name):
    """P255 / P256 / P257: around one chunk of 256 poses (P257: a full chunk kept, n_acc carried into a chunk of
    one; P256: K1 = K2 = 2 with n1 != n2, the pose index (c1, c2, k1, k2, ia)) | P700: three chunks, > 256
    fingerprints kept before the last (second trip of j0 in k_leader_vs_kept, whose trips now end on a second
    barrier), kept poses in every chunk and > 64 inside one, clash-failing poses where the previous chunk left
    rejected[] set | Q1 .. Q128: the unrolled sum of 8 and its tails, quadruplets that straddle A1-1 | A1 and
    lie entirely in either molecule"""
    c = E.string_case(name)
    ok, acc, R2, t2 = _string_raw(c)
    assert set(np.unique(ok)) <= {0, 1} and set(np.unique(acc)) <= {0, 1}
    ok, acc = ok.astype(bool), acc.astype(bool)
    ok0, acc0, poses0 = o.string_embed(c["m1"], c["m2"], c["c1"], c["v1"], c["c2"], c["v2"], c["angles"], c["quads"],
                                       thresh=c["thresh"], tfd_thresh=c["tfd_thresh"])
    R0, t0, i1, i2 = E.string_transforms(c["c1"], c["v1"], c["c2"], c["v2"], c["angles"])
    tf = E.string_fingerprints(c["m1"], c["m2"], i1, i2, R2, t2, c["quads"])   # from the GPU's own transforms
    f = E.string_filter(tf, ok0, c["tfd_thresh"])
    check_string_conditions(name, c, ok0, f)             # margin >= 1e-7 (zero invalid cases), regime of the case
    assert np.array_equal(ok, ok0)
    assert np.array_equal(acc, acc0) and np.array_equal(acc, f["acc"])
    sel = np.flatnonzero(acc)
    poses = np.concatenate([c["m1"][i1[sel]], np.einsum("pij,paj->pai", R2[sel], c["m2"][i2[sel]]) + t2[sel, None]], axis=1)
    assert poses.shape == poses0.shape and np.abs(poses - poses0).max() < TOL
    d = np.abs(tf - E.string_fingerprints(c["m1"], c["m2"], i1, i2, R0, t0, c["quads"]))
    print(f"string {name}: kept {f['kept_before']} + {f['kept_in']}, margin {f['margin']:.3e} deg, fingerprints from the "
          f"GPU's transforms vs the oracle's {np.minimum(d, 360 - d).max():.3e} deg, |dR| {np.abs(R2 - R0).max():.2e}")
    assert np.minimum(d, 360 - d).max() * 100 * len(c["quads"]) < E.TFD_MARGIN


def test_string_embed_refuses_129_fingerprints_and_goes_on(fc):
    c = E.string_case("Q128")
    with pytest.raises(fc.FirecodeHipInputError) as err:
        _string_raw(c, quads=np.concatenate([c["quads"], c["quads"][:1]]))
    assert err.value.code == L.FC_E_LIMIT
    c = E.string_case("Q1")
    ok, acc, _, _ = _string_raw(c)
    ok0, acc0, _ = o.string_embed(c["m1"], c["m2"], c["c1"], c["v1"], c["c2"], c["v2"], c["angles"], c["quads"],
                                  thresh=c["thresh"], tfd_thresh=c["tfd_thresh"])
    assert np.array_equal(ok.astype(bool), ok0) and np.array_equal(acc.astype(bool), acc0)


# ---------------------------------------------------------------------------------------------------------
# 5. trimolecular
# ---------------------------------------------------------------------------------------------------------
def _tri_lds_bytes(n_atoms, U, S):
    """LDS of one (job, orientation) group as include/fc_hip.h documents it"""
    return (U * sum(n_atoms) * 24 + 3 * U * 96 + 3 * U * U * 4 + S * 5 + 15) // 16 * 16


# name -> (atoms, distinct angles per molecule U, angle range, clash thresh, seed, pairing that only some orientations realise)
_TRI = {
    "s343": ((9, 12, 8), 7, 45.0, 1.2, 2, False),          # S = 343 > 256: every loop over S strides
    "s343_pair": ((9, 12, 8), 7, 45.0, 1.2, 2, True),      # ... also where an orientation does not run
    "rect63": ((9, 7, 13), 6, 45.0, 1.2, 3, False),        # pair rectangles A[mb]*A[mc] = 63, 91, 117
    "rect64": ((8, 8, 16), 6, 45.0, 1.2, 4, False),        # 64, 128, 128
    "rect65": ((13, 5, 11), 6, 45.0, 1.2, 5, False),       # 65, 55, 143
    "kept": ((60, 50, 55), 6, 90.0, 0.2, 6, True),         # > 64 poses of a group kept (the oracle's rmsd_thr is 1),
                                                           # and repeats of late poses: a hit beyond kept index 64
    "lds": ((200, 150, 120), 6, 45.0, 0.25, 7, True),      # > 64 KiB of LDS: the hipFuncSetAttribute branch
    "lds_max": ((400, 372, 343), 6, 45.0, 0.5, 8, True),   # 32 bytes below the 160 KiB limit
}


_TRI_REPEATS = [150, 180, 200, 215]   # poses appended once more at the end of the "kept" case


def _tri_case(name):
    atoms, U, rng_deg, thresh, seed, pairing = _TRI[name]
    mols = syn.synthetic_trimolecular(n_conf=(1, 1, 1), n_atoms=atoms, seed=seed, pivots_per_conf=(1, 1, 1))
    angles = o.cartesian_product(*[range(U)] * 3) * 2 * rng_deg / (U - 1) - rng_deg
    if name == "kept":
        angles = np.concatenate([angles, angles[_TRI_REPEATS]])
    table = None
    if pairing:
        cum = [list(m["reactive_cumnums"].values()) for m in mols]
        table = {"a": tuple(sorted((cum[0][1], cum[1][0])))}
    return mols, angles, table, thresh


@pytest.mark.parametrize("name", list(_TRI))
def test_trimolecular_shapes_and_lds(fc, name):
    """directions to TOL, passed and accepted equal, poses to TOL, group by group against the oracle"""
    from oracle import cyclical_ref as cy

    mols, angles, table, thresh = _tri_case(name)
    atoms, U = _TRI[name][0], _TRI[name][1]
    S, lds = len(angles), _tri_lds_bytes(atoms, U, len(angles))
    objects = [cy.Mol(m["coords"], m["reactive_indices"], [[cy.Pivot(*p) for p in pl] for pl in m["pivots"]],
                      m["reactive_cumnums"]) for m in mols]
    trace = []
    ref_poses, ref_ci = cy.cyclical_embed_trimolecular(objects, angles, pairings_table=table, clash_thresh=thresh, trace=trace)
    poses, ci, det = fc.embeds.cyclical_embed_trimolecular(mols, angles, pairings_table=table, clash_thresh=thresh,
                                                          return_details=True)
    groups = {(g[0], g[1], g[2]): g for g in trace}
    assert len(det["jobs"]) == 1 and len(trace) > 0
    for v in range(8):
        key = det["jobs"][0] + (v,)
        assert det["run"][0, v] == (key in groups)
        if key not in groups:
            assert not det["passed"][0, v].any() and not det["accepted"][0, v].any()
            continue
        _, _, _, d_ref, p_ref, a_ref = groups[key]
        assert np.abs(det["directions"][0, v] - d_ref).max() < TOL
        assert np.array_equal(det["passed"][0, v], p_ref)
        assert np.array_equal(det["accepted"][0, v], a_ref)
    assert poses.shape == ref_poses.shape and len(poses) > 0
    assert np.abs(poses - ref_poses).max() < TOL
    assert np.array_equal(ci, ref_ci)
    kept = det["accepted"].sum(axis=-1).max()
    print(f"tri {name}: S {S}, LDS {lds} bytes, passed {int(det['passed'].sum())}, most kept in a group {int(kept)}")
    if name == "s343_pair":
        assert S == 343 and det["passed"][0, :, 256:].any()
    if name == "s343":
        assert S == 343 and det["passed"][0, :, 256:].any() and det["accepted"][0, :, 256:].any()
        assert 0 < det["passed"].sum() < det["passed"].size
    if name.startswith("rect"):
        a = atoms
        assert {"rect63": 63, "rect64": 64, "rect65": 65}[name] in (a[1] * a[0], a[2] * a[1], a[0] * a[2])
        assert max(a[1] * a[0], a[2] * a[1], a[0] * a[2]) >= (128 if name != "rect63" else 117)
        assert 0 < det["passed"].sum() < det["passed"].size
    if name in ("kept", "lds"):
        assert kept > 64
    if name == "kept":
        # a repeated pose is rejected, and the only kept pose it is similar to has a kept index >= 64: the hit of a
        # later trip of the walk over the kept poses
        late = 0
        for v in np.flatnonzero(det["run"][0]):
            p, a = det["passed"][0, v], det["accepted"][0, v]
            for k, s0 in enumerate(_TRI_REPEATS):
                assert p[216 + k] == p[s0] and not a[216 + k]
                late += bool(a[s0] and a[:s0].sum() >= 64)
        assert S == 220 and late >= 2
    if name == "lds":
        assert 64 * 1024 < lds < 160 * 1024
    if name == "lds_max":
        assert 0 <= 160 * 1024 - lds < 300
    if table is not None:
        assert 0 < det["run"].sum() < 8


def test_trimolecular_refuses_more_lds_than_the_cu_has_and_goes_on(fc):
    atoms = (400, 372, 344)   # one atom more than lds_max
    assert _tri_lds_bytes(atoms, 6, 216) > 160 * 1024 >= _tri_lds_bytes(_TRI["lds_max"][0], 6, 216)
    mols = syn.synthetic_trimolecular(n_conf=(1, 1, 1), n_atoms=atoms, seed=8, pivots_per_conf=(1, 1, 1))
    angles = o.cartesian_product(*[range(6)] * 3) * 18.0 - 45
    with pytest.raises(fc.FirecodeHipInputError) as err:
        fc.embeds.cyclical_embed_trimolecular(mols, angles, clash_thresh=0.5)
    assert err.value.code == L.FC_E_LIMIT
    from oracle import cyclical_ref as cy

    mols, angles, table, thresh = _tri_case("rect63")
    objects = [cy.Mol(m["coords"], m["reactive_indices"], [[cy.Pivot(*p) for p in pl] for pl in m["pivots"]],
                      m["reactive_cumnums"]) for m in mols]
    ref_poses, ref_ci = cy.cyclical_embed_trimolecular(objects, angles, clash_thresh=thresh)
    poses, ci = fc.embeds.cyclical_embed_trimolecular(mols, angles, clash_thresh=thresh)
    assert poses.shape == ref_poses.shape and np.abs(poses - ref_poses).max() < TOL and np.array_equal(ci, ref_ci)
