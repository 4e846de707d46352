"""The ensemble preparation (fc_kabsch.hip: k_prep_tile<32>, its one-lane-per-conformer fallback k_prep) on its own:
atom selection, centring, the two layouts, the squared norms and the zero padding, each through the consumer that
isolates it, at the kernel's own branch points.

What the preparation leaves on the device and who reads it:
  Xa   conformer-major copy          ens.rmsd_pairs (k_pairs_exact), the refine of simbits / prune
  Xs   conformer-minor SoA, padded   ens.rmsd_matrix / ens.rmsd_and_max_all (the tiled kernel; k_matrix_exact from 417 atoms)
  G    squared norm per conformer    ens.rmsd_values, the screens of ens.simbits / ens.prune, the eigenvalue form
  max G                              which screen simbits / prune take

The reference is the oracle applied to ``X[:, sel]`` -- it never sees a mask, so it cannot share a selection bug.
Bars: RMSD within 1e-10; max deviation within 1e-10 + oracle.rotation_error_bound_batch, with at least 95 % of a case's
pairs below 1e-10 in that bound wherever the optimal rotation is unique (it is not for one selected atom, for two
selected atoms about their centroid and for atoms on a line: every bound is then infinite, which the test asserts,
and those pairs are compared on the RMSD alone); similarity bits and masks bit for bit.

Which case reaches which branch (tests/prep_ref.py lists them at BASE_CASES; test_branch_points_are_where_the_cases_claim
asserts the arithmetic):
  aligned-load tail     odd A_all with an odd conformer count in the last tile, e.g. (A_all, N) = (5, 33), (33, 63), (85, 97)
  partial tile          every N but 64             padding columns   every N but 64 (Npad > N)
  padding rows          every A % 4 != 0, under a mask "mod1" / "mod2" / "mod3"; test_stale_padding puts data there first
  > 64 KB of LDS        A_all = 85 and 209 (84 below)
  tile / lane switch    A_all = 209 tile kernel, 210 and 417 lane kernel; FC_PREP_LANES in test_both_kernels_give_the_same_bits
  k_matrix_exact        417 atoms unmasked, N = 97 (two column tiles) and 129 (three)
  gather                test_gather_through_each_kernel: 33 atoms through the tile kernel, 211 through the lane kernel"""

import numpy as np
import pytest

import prep_ref as P
from firecode_amd import synthetic as syn
from firecode_amd._lib import FC_E_LIMIT, FirecodeHipInputError, unpack_bits
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = P.TOL


def _observe(fc, X, mask, center, thr, pairs, a_sel):
    """Everything observable of one prepared ensemble."""
    n = len(X)
    out = {}
    with fc.DeviceEnsemble(X, atom_mask=mask, center=center) as ens:
        out["pairs"] = [ens.rmsd_pairs(pairs[0][:p], pairs[1][:p]) for p in (0, 255, 256, 257)]
        out["matrix"] = ens.rmsd_matrix()
        out["all"] = ens.rmsd_and_max_all()[:2]
        if a_sel <= P.VALUES_MAX_ATOMS:
            out["values"] = ens.rmsd_values()[0]
        else:  # (no kernel for this size: an error, never another path)
            with pytest.raises(FirecodeHipInputError) as err:
                ens.rmsd_values()
            assert err.value.code == FC_E_LIMIT
            out["values"] = None
        bits, grey = ens.simbits(thr, 2 * thr)
        out["bits"], out["grey"] = unpack_bits(bits, n), grey
        out["mask"], stats = ens.prune(thr, 2 * thr)
        out["similar"] = int(stats[2])
    return out


def _close(name, r, d, r0, d0, bound):
    """RMSD within 1e-10; max deviation within 1e-10 + the pair's bound where that is finite."""
    fin = np.isfinite(bound)
    dr = np.abs(r - r0).max(initial=0.0)
    if d is None:
        print(f"{name}: rmsd off by {dr:.2e}")
    else:
        over = (np.abs(d - d0)[fin] - bound[fin]).max(initial=0.0)
        print(f"{name}: rmsd off by {dr:.2e}, max deviation beyond its bound by {over:.2e} ({int(fin.sum())} of {fin.size} bounded)")
    assert dr < TOL, name
    if d is not None:
        assert np.all(np.abs(d - d0)[fin] <= TOL + bound[fin]), name


def _check(fc, a_all, n, kind, placement, duplicate, mask_kind):
    X, center, mask, sel, ref = P.case(a_all, n, kind, placement, duplicate, mask_kind)
    a_sel = len(sel)
    all_zero = a_sel == 1 and center
    P.check_bounds(ref, kind, a_sel, center)
    if placement == "far":
        # the oracle alone, evaluated with the atoms in reverse order, agrees with itself at this shift a decimal order
        # below the bars of the comparison (asserted inside)
        print("far: the oracle against itself, rmsd %.2e, max deviation %.2e" % P.far_self_agreement(X, sel, ref))
    thr = P.case_threshold(ref, all_zero)
    pi_, pj_ = P.pair_list(n, np.random.default_rng(a_all * 1000 + n))
    got = _observe(fc, X, mask, center, thr, (pi_, pj_), a_sel)

    # Xa: the pair list, in no order, with i > j, i == j and repeated pairs, P = 0, 255, 256, 257
    for (r, d), p in zip(got["pairs"], (0, 255, 256, 257)):
        assert r.shape == d.shape == (p,)
        i, j = pi_[:p], pj_[:p]
        _close(f"rmsd_pairs[{p}]", r, d, ref.R[i, j], ref.D[i, j], ref.B[i, j])
        assert not r[i == j].any() and not d[i == j].any()  # a conformer against itself: exactly 0
        assert np.array_equal(r, got["pairs"][-1][0][:p]) and np.array_equal(d, got["pairs"][-1][1][:p])
    # Xs: the complete alignments of all pairs, by both entry points
    Rm, Dm = got["matrix"]
    Ra, Da = got["all"]
    _close("rmsd_matrix", Rm, Dm, ref.R, ref.D, ref.B)
    assert np.array_equal(Rm, Ra) and np.array_equal(Dm, Da)
    assert np.array_equal(Rm, Rm.T) and np.array_equal(Dm, Dm.T) and not np.diag(Rm).any() and not np.diag(Dm).any()
    # G: the values from the eigenvalue, the screens
    if got["values"] is not None:
        _close("rmsd_values", got["values"], None, ref.R, None, ref.B)
        assert not np.diag(got["values"]).any()
    S0 = ref.similar(thr)
    assert np.array_equal(got["bits"], np.triu(S0, 1)) and got["grey"] == 0
    assert np.array_equal(got["mask"], o.greedy_prune_from_matrix(S0)) and got["similar"] == int(np.triu(S0, 1).sum())
    if all_zero:
        assert not Rm.any() and not Dm.any() and not got["values"].any()
        assert not any(r.any() or d.any() for r, d in got["pairs"])
    if duplicate and n >= 2:  # the copied conformer: a true RMSD of 0 through every path
        a, b = P.duplicated(n), n - 1
        assert Rm[a, b] < 1e-12 and Dm[a, b] < 1e-12 and (got["values"] is None or got["values"][a, b] < 1e-12)
        r, d = got["pairs"][-1]
        assert (pi_[P.DUPLICATE_AT], pj_[P.DUPLICATE_AT]) == (b, a) and r[P.DUPLICATE_AT] < 1e-12 and d[P.DUPLICATE_AT] < 1e-12


def test_branch_points_are_where_the_cases_claim():
    """The LDS arithmetic of prep_by_tiles / launch_prep_tiles from its constants: 84 | 85 straddle the 64 KB above
    which the dynamic-LDS attribute is raised, 209 | 210 the switch to the lane kernel, 416 | 417 the last size of the
    tiled complete alignments -- and the cases sit on the sides their names claim."""
    assert P.prep_lds_bytes(84) == 65112 <= 64 * 1024 < P.prep_lds_bytes(85) == 65884
    assert P.prep_lds_bytes(209) + 2048 == 163660 <= 160 * 1024 < P.prep_lds_bytes(210) + 2048 == 164432
    assert P.complete_is_tiled(416) and not P.complete_is_tiled(417)
    sizes = sorted({c[0] for c in P.BASE_CASES})
    assert sizes == [1, 2, 3, 5, 7, 33, 84, 85, 209, 210, 417]
    assert [a for a in sizes if P.prep_raises_lds_attribute(a) and P.prep_by_tiles(a)] == [85, 209]
    assert [a for a in sizes if not P.prep_by_tiles(a)] == [210, 417]
    assert all(P.prep_by_tiles(c[0]) for c in P.TWIN_CASES)
    tails = {(c[0], c[1]) for c in P.BASE_CASES if P.prep_by_tiles(c[0]) and P.load_tail_is_odd(c[1], c[0])}
    assert {(1, 33), (5, 33), (33, 63), (85, 97), (209, 129)} <= tails
    assert sorted({c[1] for c in P.BASE_CASES}) == [1, 2, 31, 33, 63, 64, 65, 97, 129]


@pytest.mark.parametrize("a_all,n,kind,placement,duplicate", P.BASE_CASES)
def test_outputs_at_the_branch_points(fc, a_all, n, kind, placement, duplicate):
    """No atom mask: every A_all of the kernel's branch points with two or three N (prep_ref.BASE_CASES says which case
    reaches which branch), clustered / unrelated / far / collinear structures, centred, about the origin, uncentred and
    1000 A away, with and without a duplicated conformer."""
    _check(fc, a_all, n, kind, placement, duplicate, "none")


@pytest.mark.parametrize("a_all,n,mask_kind,placement", P.masked_cases())
def test_outputs_under_an_atom_mask(fc, a_all, n, mask_kind, placement):
    """Each selection (first / last atom dropped, every other atom, one atom, three atoms, A % 4 = 1, 2, 3, and 104 | 105
    of 210 atoms: the consumer's tile switch inside one A_all) at 33, 85 and 210 atoms, centred on the SELECTION's centroid
    and uncentred; three of them 1000 A away."""
    _check(fc, a_all, n, "clusters", placement, False, mask_kind)


@pytest.mark.parametrize("a_all,n,mask_kind,placement", P.TWIN_CASES)
def test_both_kernels_give_the_same_bits(fc, monkeypatch, a_all, n, mask_kind, placement):
    """k_prep_tile and k_prep (FC_PREP_LANES, read on every call) promise the same arithmetic in the same order: the running
    sum over the selected atoms, the division, x*x + y*y + z*z with nothing fused.  Everything observable is equal bit
    for bit -- no tolerance."""
    X, center = P.build(a_all, n, "clusters", placement, seed=P.case_seed(a_all, n, mask_kind))
    mask = P.atom_mask(mask_kind, a_all)
    a_sel = len(P.selection(mask, a_all))
    pairs = P.pair_list(n, np.random.default_rng(n))
    monkeypatch.delenv("FC_PREP_LANES", raising=False)
    with fc.DeviceEnsemble(X, atom_mask=mask, center=center) as ens:
        R0 = ens.rmsd_matrix()[0]
    thr, half = P.split_threshold(R0[np.triu_indices(n, 1)])
    assert half > 1e-6
    tiles = _observe(fc, X, mask, center, thr, pairs, a_sel)
    monkeypatch.setenv("FC_PREP_LANES", "1")
    lanes = _observe(fc, X, mask, center, thr, pairs, a_sel)
    monkeypatch.delenv("FC_PREP_LANES")
    for (r0, d0), (r1, d1) in zip(tiles["pairs"], lanes["pairs"]):
        assert np.array_equal(r0, r1) and np.array_equal(d0, d1)
    for key in ("matrix", "all"):
        assert np.array_equal(tiles[key][0], lanes[key][0]) and np.array_equal(tiles[key][1], lanes[key][1])
    assert np.array_equal(tiles["values"], lanes["values"])
    assert np.array_equal(tiles["bits"], lanes["bits"]) and tiles["grey"] == lanes["grey"]
    assert np.array_equal(tiles["mask"], lanes["mask"]) and tiles["similar"] == lanes["similar"]
    assert 0 < tiles["bits"].sum() < n * (n - 1) // 2 and R0.any()


@pytest.mark.parametrize("n_first,n_second", [(200, 70), (70, 200)])
def test_stale_padding(fc, n_first, n_second):
    """The zero rows A .. A4-1 and the zero columns N .. Npad-1 of Xs live in pooled device blocks: an ensemble of 8 atoms
    with coordinates of size 1e3 is prepared, used and destroyed, then one with 5 of 8 atoms selected (A4 = 8; 70
    conformers: Npad = 128, 200: Npad = 256) is prepared -- wherever the pool puts it, what the consumers of Xs and G
    give is the oracle's.  (Passes whether or not the same block comes back; fails if padding is ever left unwritten
    over such data.)"""
    rng = np.random.default_rng(n_first)
    big = rng.normal(scale=1e3, size=(n_first, 8, 3))
    with fc.DeviceEnsemble(big, center=False) as ens:
        r, _ = ens.rmsd_pairs([0], [n_first - 1])
        assert r[0] > 100.0
    X = syn.synthetic_ensemble(n_second, 8, seed=n_second, cluster_size=3)[0]
    mask = np.array([1, 0, 1, 1, 0, 1, 0, 1], dtype=bool)
    ref = P.PairRef(X[:, mask], True)
    thr = P.case_threshold(ref)
    with fc.DeviceEnsemble(X, atom_mask=mask, center=True) as ens:
        Ra, Da, _ = ens.rmsd_and_max_all()
        Rv, _ = ens.rmsd_values()
        bits, grey = ens.simbits(thr, 2 * thr)
        keep, _ = ens.prune(thr, 2 * thr)
    _close("rmsd_and_max_all", Ra, Da, ref.R, ref.D, ref.B)
    _close("rmsd_values", Rv, None, ref.R, None, ref.B)
    S0 = ref.similar(thr)
    assert np.array_equal(unpack_bits(bits, n_second), np.triu(S0, 1)) and grey == 0
    assert np.array_equal(keep, o.greedy_prune_from_matrix(S0))
    assert (ref.bound < TOL).mean() >= 0.95


@pytest.mark.parametrize("a_all,n", [(33, 150), (211, 100)])
def test_gather_through_each_kernel(fc, a_all, n):
    """``prune_similarity``: the MOI stage, then the RMSD stage on its survivors, which the preparation GATHERS on the
    device through ``conf_idx`` -- by the tile kernel at 33 atoms (hydrogens in the list: gather and selection together),
    by the lane kernel at 211.  The MOI stage removes some conformers, not all, and the RMSD stage some of the rest; masks
    and counts are those of the two separate calls and of the oracle."""
    from firecode_amd import pruner

    assert P.prep_by_tiles(a_all) == (a_all == 33)
    X, atoms = P.gather_ensemble(a_all, n)
    m_moi, m_both, counts = pruner.prune_similarity(X, atoms, max_rmsd=0.5)
    s1, a = pruner.prune_by_moment_of_inertia(X, atoms)
    _, b = pruner.prune_by_rmsd(s1, atoms, 0.5)
    two = np.zeros(n, dtype=bool)
    two[np.flatnonzero(a)[b]] = True
    assert np.array_equal(m_moi, a) and np.array_equal(m_both, two)
    assert counts.tolist() == [n, int(a.sum()), int(two.sum())]
    oa, ob = P.gather_reference(X, atoms, 0.5)
    assert np.array_equal(m_moi, oa) and np.array_equal(m_both, ob)
    assert 1 < two.sum() < a.sum() < n  # a real gather, and work left for the stage behind it
