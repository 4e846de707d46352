"""The complete all-pairs alignments in the shared frame: on its first complete-alignment call an
ensemble rotates every conformer once onto conformer 0 (k_frame: Xf, Gf, Xtf), the tiled kernel takes all its operands from
that copy, and where ONE ballot says that all 64 lanes' pairs certify it (a00^2 >= 0.6 nq, converged, simple) the wave
takes the rotation from column 0 of the adjugate alone (qcp_lean_quaternion_col0) instead of the general form's ten
cofactors and pick.  rmsd and maximum deviation do not depend on either conformer's frame, and a certified pair has the same
Q, nq and flag in both forms, so:

  1. the outputs equal the oracle's (rmsd within 1e-10, max deviation within 1e-10 + the pair's conditioning bound) for
     randomly oriented inputs, every instantiation of the kernel and both rmsd forms, and on a conformer family every
     sub-tile certifies (the general-form counter, stats[3] of the bench hooks, is 0);
  2. FC_COMPLETE_COL0=0 (the general form everywhere, same frame) gives the same BYTES, also where both forms run in one
     launch (a family followed by unrelated Gaussian clouds: the counter then lies between the block counts NumPy gives
     for thresholds 0.65 and 0.55 of q0^2, the certificate's "simple" test bracketed alike);
  3. FC_COMPLETE_FRAME=0 (the operands as given) agrees within 1e-11, the figure section 5.1 uses between the two rmsd
     forms; logical ranks and single-row-block items are bit-equal to the default pass;
  4. degenerate reference conformers (collinear, planar, one point), duplicates, mirror images, 3 and 4 atoms, coordinates
     250 A from the origin only decide how many sub-tiles certify, never a value;
  5. the frame follows the handle: another selection with centring, an ensemble made behind a destroyed one."""
import numpy as np
import pytest

from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10        # against the oracle (the project's figure for the complete alignments)
TOL_FRAMES = 1e-11  # two frames against each other (the figure between the two rmsd forms)
SWITCHES = ("FC_COMPLETE_FRAME", "FC_COMPLETE_COL0", "FC_COMPLETE_EIG", "FC_COMPLETE_ROW_CHUNK", "FC_COMPLETE_ROW_TILES",
            "FC_SCREEN_TAIL_SLOTS")
# (N, A): partial row tiles and row blocks, several row blocks; <4, 2, 64> up to 52 atoms, <8, 2, 64> at 53, the 32-column
# tile at 105, the 16-column tile at 209
SHAPES = [(17, 3), (65, 5), (130, 50), (513, 50), (130, 53), (65, 105), (33, 209)]


def _setenv(monkeypatch, **env):
    for name in SWITCHES:
        if env.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, env[name])


_CACHE = {}


def _family(n, a, seed=None):
    """synthetic_ensemble: a conformer family, every member in a random orientation (computed once per shape)"""
    key = (n, a, seed)
    if key not in _CACHE:
        X, _, _ = syn.synthetic_ensemble(n, a, seed=900 + n + a if seed is None else seed, cluster_size=5 if a <= 100 else 50)
        X.setflags(write=False)
        _CACHE[key] = X
    return _CACHE[key]


def _mixed(a):
    """64 family members followed by 66 unrelated Gaussian clouds (scale 3 A)"""
    key = ("mixed", a)
    if key not in _CACHE:
        rng = np.random.default_rng(4100 + a)
        X = np.concatenate([_family(64, a, seed=4000 + a), rng.normal(scale=3.0, size=(66, a, 3))])
        X.setflags(write=False)
        _CACHE[key] = X
    return _CACHE[key]


def _bits(M):
    return np.ascontiguousarray(M).view(np.uint64)


def _pass(ens):
    """both matrices of one pass and the general-form counter of one more"""
    R, D, _ = ens.rmsd_and_max_all()
    _, _, st = ens.bench_rmsd_and_max_all(1)
    assert int(st[2]) == 1
    return R, D, int(st[3])


def _check_oracle(X, R, D, what, count=384):
    """all pairs of a small ensemble, a seeded sample (a quarter of it in the last, partial row tile) of a larger one"""
    n = len(X)
    assert not np.isnan(R).any() and not np.isnan(D).any() and np.all(np.diag(R) == 0) and np.all(np.diag(D) == 0)
    assert np.array_equal(R, R.T) and np.array_equal(D, D.T)
    i, j = np.triu_indices(n, 1)
    if len(i) > count:
        rng = np.random.default_rng(n)
        pick = rng.choice(len(i), size=count, replace=False)
        last = np.flatnonzero(j >= (n - 1) // 16 * 16)
        pick[:count // 4] = rng.choice(last, size=count // 4)
        i, j = i[pick], j[pick]
    r0, d0 = o.rmsd_and_max_batch(X[i], X[j], center=True)
    bound = o.rotation_error_bound_batch(X[i], X[j], center=True)
    er, ed = np.abs(R[i, j] - r0), np.abs(D[i, j] - d0)
    print(f"{what}: n={n} a={X.shape[1]} pairs={len(i)}: max |rmsd - oracle| {er.max():.3e}, max |maxdev - oracle| {ed.max():.3e}, "
          f"largest finite conditioning allowance {np.max(bound[np.isfinite(bound)], initial=0.0):.3e}")
    assert er.max() < TOL and np.all(ed <= TOL + bound), what


# ---- 1. oracle parity with the frame on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("eig", [None, "0"])
@pytest.mark.parametrize("n,a", SHAPES)
def test_oracle_parity_in_the_frame(fc, monkeypatch, n, a, eig):
    X = _family(n, a)
    try:
        _setenv(monkeypatch, FC_COMPLETE_EIG=eig)
        with fc.DeviceEnsemble(X, center=True) as ens:
            R, D, general = _pass(ens)
        _check_oracle(X, R, D, f"frame, EIG={eig}")
        print(f"general-form sub-tiles: {general}")
        if a == 50:
            assert general == 0
    finally:
        _setenv(monkeypatch)


# ---- 2. column 0 against the general form, bit for bit --------------------------------------------------------------------
def _col0_against_general(fc, monkeypatch, X, eig=None):
    try:
        with fc.DeviceEnsemble(X, center=True) as ens:
            _setenv(monkeypatch, FC_COMPLETE_COL0="0", FC_COMPLETE_EIG=eig)
            R0, D0, general0 = _pass(ens)
            _setenv(monkeypatch, FC_COMPLETE_EIG=eig)
            R, D, general = _pass(ens)
        assert R.tobytes() == R0.tobytes() and D.tobytes() == D0.tobytes()
        assert general <= general0
        return R, D, general, general0
    finally:
        _setenv(monkeypatch)


@pytest.mark.parametrize("n,a", SHAPES)
def test_col0_equals_the_general_form_on_families(fc, monkeypatch, n, a):
    _, _, general, general0 = _col0_against_general(fc, monkeypatch, _family(n, a))
    blocks = (n + 15) // 16
    assert general0 == blocks * (blocks + 1) // 2  # every upper-triangle sub-tile, the diagonal ones included
    print(f"n={n} a={a}: general form in {general} of {general0} sub-tiles")


def _uncertified_blocks(X, thresholds):
    """NumPy: every conformer (centred) rotated onto conformer 0, then Horn's 4 x 4 matrix K of every pair in that frame:
    q0^2 of its leading eigenvector and |a00| / (3 |B|_F)^3 = q0^2 (l1 - l2)(l1 - l3)(l1 - l4) / (3 |B|_F)^3, the quantity
    the certificate's "simple" test holds above 2e-3 (unrelated clouds miss it now and then at any angle: with q0^2 alone
    the model called a block certified that held a pair at 1.07e-3).  -> for each (q0^2 threshold, simple threshold) the
    number of upper-triangle 16 x 16 blocks (diagonal ones included, as the kernel walks them) that hold a pair inside the
    matrix below either"""
    def rotations(P, Q):  # R q ~ p, as the oracle forms it
        B = np.einsum("kai,kaj->kij", P, Q)
        u, _, vh = np.linalg.svd(B)
        flip = np.linalg.det(u @ vh) < 0
        u[flip, :, -1] *= -1.0
        return u @ vh

    n = len(X)
    Xc = X - X.mean(axis=1, keepdims=True)
    R0 = rotations(np.broadcast_to(Xc[0], Xc.shape), Xc)
    Xf = np.einsum("kij,kaj->kai", R0, Xc)
    i, j = (m.ravel() for m in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    B = np.einsum("kai,kaj->kij", Xf[i], Xf[j])  # B[x][y] = sum p_x q_y; Horn's S_xy = B[y][x] (csrc/fc_kabsch_math.h)
    Sxx, Sxy, Sxz = B[:, 0, 0], B[:, 1, 0], B[:, 2, 0]
    Syx, Syy, Syz = B[:, 0, 1], B[:, 1, 1], B[:, 2, 1]
    Szx, Szy, Szz = B[:, 0, 2], B[:, 1, 2], B[:, 2, 2]
    K = np.zeros((len(i), 4, 4))
    K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 0, 3] = Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx
    K[:, 1, 1], K[:, 1, 2], K[:, 1, 3] = Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz
    K[:, 2, 2], K[:, 2, 3], K[:, 3, 3] = -Sxx + Syy - Szz, Syz + Szy, -Sxx - Syy + Szz
    K = K + np.triu(K, 1).transpose(0, 2, 1)
    w, v = np.linalg.eigh(K)
    q0sq = v[:, 0, 3] ** 2
    simple = q0sq * np.prod(w[:, 3:4] - w[:, :3], axis=1) / (27.0 * (B ** 2).sum(axis=(1, 2)) ** 1.5)
    q0sq, simple = q0sq.reshape(n, n), simple.reshape(n, n)
    nb = (n + 15) // 16
    counts = []
    for thr_q, thr_s in thresholds:
        c = 0
        for bi in range(nb):
            for bj in range(bi, nb):
                blk = (slice(bi * 16, (bi + 1) * 16), slice(bj * 16, (bj + 1) * 16))
                c += bool((q0sq[blk] < thr_q).any() or (simple[blk] < thr_s).any())
        counts.append(c)
    return counts


@pytest.mark.parametrize("eig", [None, "0"])
@pytest.mark.parametrize("a", [20, 50])
def test_both_forms_in_one_launch(fc, monkeypatch, a, eig):
    """N = 130: a family of 64, then 66 unrelated clouds -- some sub-tiles certify, most do not"""
    X = _mixed(a)
    R, D, general, general0 = _col0_against_general(fc, monkeypatch, X, eig=eig)
    _check_oracle(X, R, D, f"mixed, EIG={eig}")
    # the certificate's own figures are q0^2 >= 0.6 and simple > 2e-3: bracketed by (0.55, half) and (0.65, twice)
    lo, hi = _uncertified_blocks(X, ((0.55, 1e-3), (0.65, 4e-3)))
    print(f"a={a}: general form in {general} of {general0} sub-tiles; NumPy: {lo} blocks below (0.55, 1e-3), {hi} below (0.65, 4e-3)")
    assert general0 == 45 and 0 < lo <= hi < 45
    assert lo <= general <= hi


# ---- 3. frame against no frame --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,a", [(130, 50), (513, 50), (130, 53), (65, 105), (33, 209)])
def test_frame_against_no_frame(fc, monkeypatch, n, a):
    X = _family(n, a)
    try:
        with fc.DeviceEnsemble(X, center=True) as ens:
            _setenv(monkeypatch, FC_COMPLETE_FRAME="0")
            R0, D0, general0 = _pass(ens)
            _setenv(monkeypatch)
            R, D, _ = _pass(ens)
            _setenv(monkeypatch, FC_COMPLETE_ROW_CHUNK="1")
            R1, D1, _ = _pass(ens)
        er, ed = np.abs(R - R0).max(), np.abs(D - D0).max()
        print(f"n={n} a={a}: frame against no frame: rmsd {er:.3e}, maxdev {ed:.3e}")
        assert er <= TOL_FRAMES and ed <= TOL_FRAMES
        blocks = (n + 15) // 16
        assert general0 == blocks * (blocks + 1) // 2  # no frame: the general form everywhere
        assert R1.tobytes() == R.tobytes() and D1.tobytes() == D.tobytes()  # single row blocks against chunked items
    finally:
        _setenv(monkeypatch)


@pytest.mark.parametrize("world", [2, 3])
def test_logical_ranks_in_the_frame(fc, monkeypatch, world):
    from firecode_amd import _lib
    from firecode_amd import dist as fdist

    n, a = 513, 50
    X = _family(n, a)
    iu, ju = np.triu_indices(n, 0)
    owner = fdist.owner_of_rows(n, world, 128)
    try:
        _setenv(monkeypatch)
        with fc.DeviceEnsemble(X, center=True) as ens:
            R0, D0, _ = ens.rmsd_and_max_all()
            for rk in range(world):
                _lib.call("fc_debug_comm_loopback", rk, world)
                mine = owner[iu] == rk
                _, _, st, r, d = ens.bench_rmsd_and_max_all_sampled(iu[mine], ju[mine], reps=1)
                assert int(st[2]) == 1 and int(st[3]) == 0
                assert np.array_equal(_bits(r), _bits(R0[iu[mine], ju[mine]])), rk
                assert np.array_equal(_bits(d), _bits(D0[iu[mine], ju[mine]])), rk
    finally:
        _lib.call("fc_debug_comm_loopback", -1, 0)
        _setenv(monkeypatch)


# ---- 4. edge geometry -----------------------------------------------------------------------------------------------------
def _edge_case(name):
    n, a = 40, 20
    rng = np.random.default_rng(77)
    X = np.array(_family(n, a, seed=5000))
    if name == "collinear":
        X[0] = np.outer(np.linspace(-6.0, 6.0, a), [0.3, -0.5, 0.8])
    elif name == "planar":
        X[0] = X[0] * [1.0, 1.0, 0.0]
    elif name == "point":
        X[0] = np.tile([1.5, -2.0, 0.25], (a, 1))
    elif name == "duplicates":
        X[5], X[21] = X[3], X[3]
        X[7] = X[3] + 1e-5 * rng.normal(size=(a, 3))
        X[30] = X[17] + 1e-5 * rng.normal(size=(a, 3))
    elif name == "mirror":
        X[1::2] = X[1::2] * [-1.0, 1.0, 1.0]
    elif name == "far":
        shift = rng.normal(size=(n, 1, 3))
        X = X + 250.0 * shift / np.linalg.norm(shift, axis=2, keepdims=True)
    elif name in ("A3", "A4"):
        X = np.array(_family(n, int(name[1]), seed=5001))
    return X


@pytest.mark.parametrize("name", ["collinear", "planar", "point", "duplicates", "mirror", "A3", "A4", "far"])
def test_edge_geometry(fc, monkeypatch, name):
    X = _edge_case(name)
    try:
        _setenv(monkeypatch)
        with fc.DeviceEnsemble(X, center=True) as ens:
            R, D, general = _pass(ens)
        print(f"{name}: general-form sub-tiles {general} of 6")
        _check_oracle(X, R, D, name, count=10**6)
    finally:
        _setenv(monkeypatch)


# ---- 5. handle state ------------------------------------------------------------------------------------------------------
def test_the_frame_follows_the_handle(fc, monkeypatch):
    """a pass; the same conformers under another atom selection with centring (every conformer shifted by its own vector); a
    pass on an ensemble of the same shape created behind a destroyed one: none sees a frame that is not its own"""
    n, a_all = 130, 60
    rng = np.random.default_rng(93)
    X = np.array(_family(n, a_all, seed=5100)) + rng.normal(scale=25.0, size=(n, 1, 3))
    mask = np.zeros(a_all, dtype=bool)
    mask[rng.permutation(a_all)[:37]] = True
    try:
        _setenv(monkeypatch)
        first = fc.DeviceEnsemble(X, center=True)
        R, D, _ = _pass(first)
        _check_oracle(X, R, D, "all atoms")
        with fc.DeviceEnsemble(X, mask, center=True) as sel:
            R, D, _ = _pass(sel)
            _check_oracle(X[:, mask], R, D, "37 of 60 atoms")
            R, D, _ = _pass(first)  # the first handle's frame is still its own
            _check_oracle(X, R, D, "all atoms again")
        first.close()
        Y = np.array(_family(n, a_all, seed=5101))
        with fc.DeviceEnsemble(Y, center=True) as second:
            R, D, general = _pass(second)
            _check_oracle(Y, R, D, "behind a destroyed ensemble")
            R2, D2, _ = _pass(second)  # the second pass finds the frame made by the first
            assert R2.tobytes() == R.tobytes() and D2.tobytes() == D.tobytes()
    finally:
        _setenv(monkeypatch)
