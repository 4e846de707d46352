"""Argument checks of the C ABI happen on the host BEFORE any device is touched, so they
are testable without a GPU: a bad shape / index / threshold must come back as FC_E_INVALID
(FirecodeHipInputError), never reach a kernel."""

import ctypes as C

import numpy as np
import pytest

import firecode_amd as fc
from firecode_amd import _lib as L


def _tri_args(J=1, U=2, S=3, A=(4, 5, 3)):
    coords = [np.zeros((2, a, 3)) for a in A]
    reactive = [np.array([0, 1], dtype=np.int64) for _ in A]
    cptr = (C.POINTER(C.c_double) * 3)(*[L.pf(c) for c in coords])
    rptr = (C.POINTER(C.c_int64) * 3)(*[L.pi(r) for r in reactive])
    keep = (coords, reactive)
    a = dict(
        cptr=cptr, nconf=L.i64([2, 2, 2]), natm=L.i64(list(A)), rptr=rptr, nreact=L.i64([2, 2, 2]), J=J,
        conf=np.zeros((J, 3), dtype=np.int64), ps=np.zeros((J, 3, 3)), pe=np.ones((J, 3, 3)),
        vecs=np.zeros((J, 8, 3, 2, 3)), d0=np.zeros((J, 3, 3)), run=np.ones((J, 8), dtype=np.uint8),
        rtab=np.zeros((J, 8, 3, 3), dtype=np.int64), norms=np.ones((J, 3)), ua=np.zeros((3, U)), U=U,
        aidx=np.zeros((S, 3), dtype=np.int32), S=S, thresh=1.5, mc=0, rthr=1.0, dirs=np.zeros((J, 8, 3, 3)),
        Rt=np.zeros((J, 8, 3, U, 12)), ok=np.zeros((J, 8, S), dtype=np.uint8), acc=np.zeros((J, 8, S), dtype=np.uint8))
    return a, keep


def _call_tri(a):
    L.call("fc_embed_trimolecular", a["cptr"], L.pi(a["nconf"]), L.pi(a["natm"]), a["rptr"], L.pi(a["nreact"]),
           a["J"], L.pi(a["conf"]), L.pf(a["ps"]), L.pf(a["pe"]), L.pf(a["vecs"]), L.pf(a["d0"]), L.pb(a["run"]),
           L.pi(a["rtab"]), L.pf(a["norms"]), L.pf(a["ua"]), a["U"], a["aidx"].ctypes.data_as(C.POINTER(C.c_int32)),
           a["S"], a["thresh"], a["mc"], a["rthr"], L.pf(a["dirs"]), L.pf(a["Rt"]), L.pb(a["ok"]), L.pb(a["acc"]))


@pytest.mark.parametrize("what", ["conf", "rtab", "aidx", "thresh", "reactive"])
def test_trimolecular_rejects_out_of_range_indices(what):
    a, keep = _tri_args()
    if what == "conf":
        a["conf"][0, 1] = 2  # only 2 conformers
    elif what == "rtab":
        a["rtab"][0, 5, 2, 0] = 3  # molecule 2 has 3 atoms
    elif what == "aidx":
        a["aidx"][1, 2] = 2  # U = 2
    elif what == "thresh":
        a["thresh"] = 0.0
    else:
        keep[1][0][1] = 9
    with pytest.raises(fc.FirecodeHipInputError):
        _call_tri(a)


def test_rot_corr_rejects_bad_torsions_and_masks():
    X = np.zeros((3, 5, 3))
    heavy = np.ones(5, dtype=np.uint8)
    mask = np.zeros(3, dtype=np.uint8)
    ang = np.zeros((1, 3))
    na = np.array([3], dtype=np.int32)
    rot = np.zeros((1, 5), dtype=np.uint8)

    def call(tors, heavy=heavy, na=na, max_rmsd=0.25):
        tors = np.array(tors, dtype=np.int64).reshape(-1, 4)
        L.call("fc_prune_rmsd_rot_corr", L.pf(X), 3, 5, L.pb(heavy), L.pi(tors), len(tors), L.pb(rot), L.pf(ang),
               na.ctypes.data_as(C.POINTER(C.c_int32)), 3, max_rmsd, 0.5, None, 0.0, 20, L.pb(mask), None)

    with pytest.raises(fc.FirecodeHipInputError):
        call([[0, 1, 2, 5]])  # atom index == A
    with pytest.raises(fc.FirecodeHipInputError):
        call([[0, 1, 2, 3]], heavy=np.zeros(5, dtype=np.uint8))  # no heavy atom selected
    with pytest.raises(fc.FirecodeHipInputError):
        call([[0, 1, 2, 3]], na=np.array([4], dtype=np.int32))  # more angles than max_angles
    with pytest.raises(fc.FirecodeHipInputError):
        call([[0, 1, 2, 3]], max_rmsd=-1.0)


def test_python_wrappers_reject_bad_shapes():
    with pytest.raises(fc.FirecodeHipInputError):
        fc.pruner.prune_by_rmsd(np.zeros((4, 5)), ["C"] * 5)
    with pytest.raises(fc.FirecodeHipInputError):
        fc.pruner.prune_by_rmsd(np.zeros((4, 5, 3)), ["C"] * 4)
    with pytest.raises(fc.FirecodeHipInputError):
        fc.pruner.prune_by_rmsd_rot_corr(np.zeros((4, 5, 3)), ["C"] * 5, None, torsions=[(0, 1, 2, 3, 3)])
    with pytest.raises(fc.FirecodeHipInputError):
        fc.hypermolecule_class.align_by_moi(["C"] * 4, np.zeros((2, 5, 3)))
    with pytest.raises(fc.FirecodeHipInputError):
        fc.embeds.rototranslate(np.zeros((2, 5, 3)), np.zeros((3, 3, 3)), np.zeros((2, 3)))
    with pytest.raises(fc.FirecodeHipInputError):
        fc.embeds.cyclical_embed_trimolecular([{}, {}], np.zeros((1, 3)))
    with pytest.raises(fc.FirecodeHipInputError):
        fc.torsion_module.torsion_scan(np.zeros((5, 3)), [[0, 1, 2, 3]], np.zeros((1, 4), dtype=bool), [[0]])


def test_c_entry_points_reject_null_and_bad_sizes():
    out = np.zeros((2, 5, 3))
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_align_by_moi", None, 2, 5, L.pf(np.ones(5)), L.pf(out))
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_align_by_moi", L.pf(out), 2, 0, L.pf(np.ones(5)), L.pf(out))
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_rototranslate", L.pf(out), 2, 5, None, None, L.pf(out))
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_prune_export_pairs_dev", None, None, 4)
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_debug_kabsch_math", 0, None, 1, L.pf(out))
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_debug_kabsch_math", 3, L.pf(out), 1, L.pf(out))
    with pytest.raises(fc.FirecodeHipInputError):
        L.call("fc_debug_kabsch_math", 2, L.pf(out), -1, L.pf(out))


def test_prune_many_rejects_bad_lists():
    one = (C.c_void_p * 1)(None)
    masks = (C.POINTER(C.c_uint8) * 1)()
    with pytest.raises(fc.FirecodeHipInputError):  # n out of range
        L.call("fc_prune_rmsd_many", one, 5000, 0.5, 1.0, 20, masks, None)
    with pytest.raises(fc.FirecodeHipInputError):  # NULL list
        L.call("fc_prune_rmsd_many", None, 1, 0.5, 1.0, 20, masks, None)
    with pytest.raises(fc.FirecodeHipInputError):  # threshold
        L.call("fc_prune_rmsd_many", one, 1, 0.0, 1.0, 20, masks, None)
    L.call("fc_prune_rmsd_many", None, 0, 0.5, 1.0, 20, None, None)  # empty queue: nothing to do


# ---- size limits: FC_E_LIMIT comes back from the host checks, before any device call ---------------------
def _limit(fn):
    with pytest.raises(fc.FirecodeHipInputError) as e:
        fn()
    assert e.value.code == L.FC_E_LIMIT, e.value
    return str(e.value)


def test_clash_entry_points_refuse_more_atoms_than_the_lds_holds():
    A = 160 * 1024 // 24 + 1  # 6827
    X = np.zeros((1, A, 3))
    n, ok = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8)
    assert "6826" in _limit(lambda: L.call("fc_clash_self", L.pf(X), 1, A, 0.0, 0.5, L.pi(n)))
    assert "6826" in _limit(lambda: L.call("fc_clash_fragments", L.pf(X), 1, A, L.pi(L.i64([3, 4])), 2, 1.0, 0, L.pi(n), L.pb(ok)))
    assert "6826" in _limit(lambda: L.call("fc_clash_graph", L.pf(X), 1, A, L.pb(np.zeros((A, A), dtype=np.uint8)), 1.0, L.pi(n)))
    assert "6826" in _limit(lambda: fc.algebra.count_clashes_batch(X))
    _limit(lambda: fc.utils.compenetration_check_batch(X, ids=[3, 4, 5]))


def _pose_args(A1=3, A2=2, P=2):
    return dict(m1=np.zeros((2, A1, 3)), m2=np.zeros((3, A2, 3)), c1=np.zeros(P, dtype=np.int64), c2=np.zeros(P, dtype=np.int64),
                R1=np.tile(np.eye(3), (P, 1, 1)), t1=np.zeros((P, 3)), R2=np.tile(np.eye(3), (P, 1, 1)), t2=np.zeros((P, 3)))


def test_pose_kernel_refuses_too_many_atoms_and_bad_conformer_ids():
    assert "1707" in _limit(lambda: fc.embeds.embed_poses_clash(**_pose_args(A1=1707)))
    for which, bad in (("c1", 2), ("c1", -1), ("c2", 3), ("c2", -1)):
        a = _pose_args()
        a[which][1] = bad  # m1 has 2 conformers, m2 has 3
        with pytest.raises(fc.FirecodeHipInputError) as e:
            fc.embeds.embed_poses_clash(**a)
        assert e.value.code == L.FC_E_INVALID and "pose 1" in str(e.value)


def test_rot_corr_refuses_sizes_its_launch_cannot_take():
    def call(N, A):
        X = np.zeros((N, A, 3))
        mask = np.zeros(N, dtype=np.uint8)
        L.call("fc_prune_rmsd_rot_corr", L.pf(X), N, A, L.pb(np.ones(A, dtype=np.uint8)), None, 0, None, None, None, 1,
               0.25, 0.5, None, 0.0, 20, L.pb(mask), None)

    assert "1707" in _limit(lambda: call(3, 1707))  # 4 structures of 1707 atoms do not fit the 160 KiB of LDS
    msg = _limit(lambda: call(65536, 3))  # one grid row per structure: 65 535 is what every device guarantees
    assert "65535" in msg and "FC_ROTCORR_MAX_ROWS" in msg


def test_tfd_entry_points_refuse_more_than_128_angles():
    """np.sum adds more than 128 elements pairwise and the kernels' order would no longer be NumPy's: every TFD entry
    point says so before it touches a device (fc_tfd_simbits, and through it tfd_similarity, included)"""
    tf = np.zeros((3, 129))
    fm, bits, mask = np.zeros(3, dtype=np.int64), np.zeros((3, 1), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
    msgs = [_limit(lambda: L.call("fc_tfd_first_match", L.pf(tf), 3, 129, 10.0, L.pi(fm))),
            _limit(lambda: L.call("fc_tfd_simbits", L.pf(tf), 3, 129, 10.0, 0, 3, L.pw(bits))),
            _limit(lambda: L.call("fc_tfd_simbits", L.pf(tf), 3, 129, 10.0, 1, 2, L.pw(bits))),
            _limit(lambda: L.call("fc_tfd_prune", L.pf(tf), 3, 129, 10.0, L.pb(mask))),
            _limit(lambda: fc.torsion_module.tfd_simbits(tf, 10.0)),
            _limit(lambda: fc.torsion_module.tfd_similarity(tf[0], tf[1])),
            _limit(lambda: fc.torsion_module.prune_tfd_from_tf_mat(tf))]
    assert all("Q=129" in m and "128" in m for m in msgs) and len(set(msgs)) == 1  # (the same wording everywhere)


def test_tfd_first_match_without_angles_needs_no_device():
    """Q = 0: NumPy's empty sum is 0, below every positive threshold -- answered on the host, tf may be NULL"""
    fm = np.full(4, -7, dtype=np.int64)
    L.call("fc_tfd_first_match", None, 4, 0, 10.0, L.pi(fm))
    assert fm.tolist() == [1, 2, 3, -1]
    for thresh in (0.0, -1.0, float("nan")):
        L.call("fc_tfd_first_match", None, 4, 0, thresh, L.pi(fm))
        assert fm.tolist() == [-1] * 4
    form = L.tfd_last_form()
    assert isinstance(form[0], int) and form[1] >= 0
