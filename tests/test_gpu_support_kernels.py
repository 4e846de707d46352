"""The clash, pose, fitness, moment-of-inertia, rot-corr and alignment kernels across shapes and limits.

Every kernel here is compared with a plain reference of the same operation (tests/support_ref.py: cdist for the
counts, np.longdouble for the real-valued results; oracle.cpu_ref for the masks) at the shapes where such
kernels go wrong: atom counts around the 64-lane wavefront, the first and last workgroup of a launch, the
grid-stride loop of the pose kernel, the dynamic-LDS limit the entry points advertise, distances exactly on a
threshold, zero moments.  Counts and verdicts of the clash family and of the pose kernel are compared for
equality: no tolerance appears in those tests.

Tests that may leave cases out assert their cap.  What the references alone leave out (CPU, seeds as below):
  * MOI similarity bits: pairs whose longdouble relative deviation lies within 1e-10 of the tolerance, cap
    1e-5 of the pairs of a case -- 0 pairs at either tolerance for each of the six ensembles of
    test_moi_bits_and_mask and test_moi_bits_tell_the_divisor_apart (so every mask there is compared exactly), and
    0 of the 1.97e8 pairs of the sampled rows of test_moi_prune_100k_rows.
  * fitness verdicts: none (the thresholds are put into the widest gaps of the reference errors)."""

import ctypes as C

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import support_ref as R
from firecode_amd import _lib as L
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

pytestmark = pytest.mark.gpu

TOL = 1e-10  # coordinates, as in tests/test_gpu_parity.py
LDS_ATOMS = 160 * 1024 // 24  # 6826: one structure of a wavefront in the 160 KiB of LDS
POSE_ATOMS = 160 * 1024 // (4 * 24)  # 1706: four structures per workgroup


# ---------------------------------------------------------------------------------------------------------
# raw entry points (the Python wrappers return verdicts only)
# ---------------------------------------------------------------------------------------------------------
def _fragments_raw(X, ids, thresh, max_clashes):
    X, ids = L.f64(X), L.i64(ids)
    counts, ok = np.full(len(X), -1, dtype=np.int64), np.full(len(X), 7, dtype=np.uint8)
    L.call("fc_clash_fragments", L.pf(X), X.shape[0], X.shape[1], L.pi(ids), len(ids), float(thresh), int(max_clashes),
           L.pi(counts), L.pb(ok))
    return counts, ok.astype(bool)


def _graph_raw(X, adj, thresh):
    X, adj = L.f64(X), L.u8(adj)
    counts = np.full(len(X), -1, dtype=np.int64)
    L.call("fc_clash_graph", L.pf(X), X.shape[0], X.shape[1], L.pb(adj), float(thresh), L.pi(counts))
    return counts


def _chain(n):
    return [(k, k + 1) for k in range(n - 1)]


def _complete(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def _splits(A):
    """fragment lengths that put a boundary at 0, 1, 63, 64, 65, A-1, A (where A has room), the last fragment
    listed shorter than, equal to and longer than "the rest", which is what it takes"""
    cuts = sorted({c for c in (0, 1, 63, 64, 65, A - 1, A) if 0 <= c <= A})
    two = [[c, A - c] for c in cuts] + [[cuts[len(cuts) // 2], 0], [cuts[len(cuts) // 2], A + 5]]
    three = [[a, b - a, A - b] for a in cuts for b in cuts if a <= b]
    three += [[a, b - a, 0] for a, b in ((0, A), (1, A), (A // 2, A))]  # sum(ids[:-1]) == A: an empty last fragment
    three += [[A // 3, A // 3, 1]] if A >= 3 else []                   # sum(ids) < A: the last takes the rest
    return two, three


def _check_clash_family(fc, X, thresh, hi=0.5):
    """every kernel of the family on one block of structures; one cdist per structure feeds all references"""
    N, A = X.shape[:2]
    two, three = _splits(A)
    graphs = [[], _chain(A)] + ([_complete(A)] if A <= 200 else [])
    adjs = [R.adjacency(e, A) for e in graphs]
    ref_self, ref_lo, plain = (np.zeros(N, dtype=np.int64) for _ in range(3))
    ref_ids = np.zeros((len(two + three), N), dtype=np.int64)
    ref_graph = np.zeros((len(graphs), N), dtype=np.int64)
    for n, x in enumerate(X):
        d = cdist(x, x)
        ref_self[n], ref_lo[n], plain[n] = R.self_count(x, 0.0, hi, d=d), R.self_count(x, hi / 2, thresh, d=d), R.self_count(x, d=d)
        ref_ids[:, n] = [R.fragment_count(x, ids, thresh, d=d) for ids in two + three]
        ref_graph[:, n] = [R.graph_count(x, adj, thresh, d=d) for adj in adjs]
    assert np.array_equal(fc.algebra.count_clashes_batch(X, 0.0, hi), ref_self)
    assert np.array_equal(fc.algebra.count_clashes_batch(X, hi / 2, thresh), ref_lo)
    seen = set()
    for ids, ref in zip(two + three, ref_ids):
        exact = int(ref[N // 2])
        for mc in sorted({0, 1, max(exact - 1, 0), exact, exact + 1}):
            counts, ok = _fragments_raw(X, ids, thresh, mc)
            assert np.array_equal(counts, ref), (A, ids)
            assert np.array_equal(ok, ref <= mc), (A, ids, mc)
            assert np.array_equal(fc.utils.compenetration_check_batch(X, ids=ids, thresh=thresh, max_clashes=mc), ref <= mc)
            seen.update((ref <= mc).tolist())
    # graph mode first asks count_clashes (0 < d < 0.5), then counts the non-bonded pairs below thresh
    for edges, adj, ref in zip(graphs, adjs, ref_graph):
        assert np.array_equal(_graph_raw(X, adj, thresh), ref), (A, len(edges))
        if A > 1 and len(edges) == A * (A - 1) // 2:
            assert not ref.any()
        exact = int(ref[N // 2])
        for mc in sorted({0, 1, max(exact - 1, 0), exact, exact + 1}):
            got = fc.utils.compenetration_check_batch(X, graph=edges, thresh=thresh, max_clashes=mc)
            assert np.array_equal(got, (plain <= mc) & (ref <= mc))
            assert np.array_equal(fc.utils.compenetration_check_batch(X, max_clashes=mc), plain <= mc)
    return ref_self, seen


# ---------------------------------------------------------------------------------------------------------
# clash family
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1000])
def test_clash_family_shapes(fc, A):
    verdicts = set()
    for N, kind, seed in ((1, "blob", 1), (2, "far", 2), (257, "blob", 3)):
        scale = 0.7 * max(A, 2) ** (1.0 / 3.0)  # a few clashes per structure at every size
        X = R.ensemble(kind, N, A, seed=seed + A, scale=scale)
        ref_self, seen = _check_clash_family(fc, X, thresh=1.2)
        verdicts |= seen
        if N == 257 and A >= 63:
            assert ref_self.max() > 0  # the case set counts something
    if A >= 2:
        assert verdicts == {True, False}
    if 12 <= A <= 200:  # a real molecule's conformers: no clash but along the bonds
        from molecule_gen import random_branched_molecule

        graph = random_branched_molecule(A, seed=A)[2]
        X = R.ensemble("molecule", 5, A, seed=A)  # (the same seed: conformers of that molecule)
        adj, none = R.adjacency(graph.edges, A), R.adjacency([], A)
        ref = np.array([R.graph_count(x, adj, 1.6) for x in X])
        unbonded = np.array([R.graph_count(x, none, 1.6) for x in X])
        assert np.array_equal(_graph_raw(X, adj, 1.6), ref) and np.array_equal(_graph_raw(X, none, 1.6), unbonded)
        assert (unbonded > ref + A).all()  # most bonds are hits (1.5 A +- noise), and the graph takes them out


@pytest.mark.parametrize("A", [2730, 2731, 4096, LDS_ATOMS])
def test_clash_family_at_the_lds_limit(fc, A):
    """64 KiB of LDS hold 2730 atoms: above that the launch needs the dynamic-LDS attribute, up to the 6826
    atoms the entry points accept"""
    X = R.ensemble("blob", 3, A, seed=A, scale=12.0)
    D = [cdist(x, x) for x in X]
    ref = np.array([R.self_count(x, 0.0, 1.5, d=d) for x, d in zip(X, D)])
    assert ref.min() > 100  # (about 8 500 ordered pairs below 1.5 A at 6826 atoms)
    assert np.array_equal(fc.algebra.count_clashes_batch(X, 0.0, 1.5), ref)
    for ids in ([A // 2, A - A // 2], [64, 1], [A // 3, A // 3, A - 2 * (A // 3)], [1, A - 2, 1]):
        want = np.array([R.fragment_count(x, ids, 1.5, d=d) for x, d in zip(X, D)])
        counts, ok = _fragments_raw(X, ids, 1.5, int(want[1]))
        assert np.array_equal(counts, want) and np.array_equal(ok, want <= want[1])
        assert want.max() > 0 or ids[0] == 1
    adj = R.adjacency(_chain(A), A)
    adj[:64, A - 64:] = adj[A - 64:, :64] = True  # "bonds" across the whole index range
    want = np.array([R.graph_count(x, adj, 1.5, d=d) for x, d in zip(X, D)])
    assert np.array_equal(_graph_raw(X, adj, 1.5), want) and want.max() > 0


def test_clash_family_refuses_one_atom_too_many_and_goes_on(fc):
    X = np.zeros((1, LDS_ATOMS + 1, 3))
    for call in (lambda: fc.algebra.count_clashes_batch(X), lambda: _fragments_raw(X, [5, 5], 1.0, 0),
                 lambda: _graph_raw(X, np.zeros((LDS_ATOMS + 1,) * 2, dtype=np.uint8), 1.0)):
        with pytest.raises(fc.FirecodeHipInputError) as e:
            call()
        assert e.value.code == L.FC_E_LIMIT
        Y = R.ensemble("blob", 4, 30, seed=4, scale=1.0)  # the next ordinary call works
        assert np.array_equal(fc.algebra.count_clashes_batch(Y), [R.self_count(y) for y in Y])


@pytest.mark.parametrize("t", [0.5, 1.0, 1.2, 1.5, 1.7320508075688772, 2.5])
def test_clash_threshold_ties_in_bulk(fc, t):
    """distances on, just below and just above the threshold decide as cdist's rounded distance does: strict <
    for two fragments, the self count and graph mode, <= for three fragments, lo < d for the self count"""
    X2 = R.tie_structures(t, 4000, seed=1)
    X3 = R.tie_structures(t, 3000, seed=2, n_frag=3)
    d2 = np.array([cdist(x[:1], x[1:])[0, 0] for x in X2])
    D3 = np.array([cdist(x, x) for x in X3])
    # not vacuous (from the reference alone): exact ties exist, near and far from the origin, and < and <= part on them
    tie = d2 == t
    assert tie.sum() >= 20 and (tie & (np.abs(X2[:, 0]).max(axis=1) > 1.0)).sum() >= 5
    assert (d2 < t).sum() > 1000 and (d2 > t).sum() > 1000
    lt3 = np.array([np.count_nonzero(np.array([d[1, 0], d[2, 1], d[0, 2]]) < t) for d in D3])
    le3 = np.array([R.fragment_count(x, [1, 1, 1], t, d=d) for x, d in zip(X3, D3)])
    assert (lt3 != le3).sum() >= 20
    empty = np.zeros((2, 2), dtype=np.uint8)
    for thr in (t, np.nextafter(t, 0.0), np.nextafter(t, np.inf)):
        want2 = (d2 < thr).astype(np.int64)
        counts, ok = _fragments_raw(X2, [1, 1], thr, 0)
        assert np.array_equal(counts, want2) and np.array_equal(ok, want2 == 0)
        assert np.array_equal(_graph_raw(X2, empty, thr), 2 * want2)
        assert np.array_equal(fc.algebra.count_clashes_batch(X2, 0.0, thr), 2 * want2)
        assert np.array_equal(fc.algebra.count_clashes_batch(X2, thr, 1e9), 2 * (d2 > thr).astype(np.int64))  # lo < d
        want3 = np.array([R.fragment_count(x, [1, 1, 1], thr, d=d) for x, d in zip(X3, D3)])
        for mc in (0, 1, 2):
            counts, ok = _fragments_raw(X3, [1, 1, 1], thr, mc)
            assert np.array_equal(counts, want3) and np.array_equal(ok, want3 <= mc)
        if thr == t:
            assert set(want2[tie].tolist()) == {0} and set(want3.tolist()) >= {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------------------------------------
def _pose_case(A1, A2, P, seed, n1=3, n2=2, far=False, scale=None):
    rng = np.random.default_rng(seed)
    s1 = scale or 0.8 * max(A1, 2) ** (1.0 / 3.0)
    s2 = scale or 0.8 * max(A2, 2) ** (1.0 / 3.0)
    m1, m2 = rng.normal(scale=s1, size=(n1, A1, 3)), rng.normal(scale=s2, size=(n2, A2, 3))
    c1, c2 = rng.integers(0, n1, P), rng.integers(0, n2, P)
    R1, R2 = R.random_rotations(rng, P), R.random_rotations(rng, P)
    t1 = rng.normal(scale=1.0, size=(P, 3)) + (250.0 if far else 0.0)
    t2 = t1 + R.random_rotations(rng, P)[:, 0] * rng.uniform(0.0, 2.5 * (s1 + s2), size=(P, 1))  # from overlap to apart
    return m1, m2, c1, c2, R1, t1, R2, t2


def _check_poses(fc, case, rows, thresh=1.5):
    m1, m2, c1, c2, R1, t1, R2, t2 = case
    A1 = m1.shape[1]
    ok0, counts, poses = fc.embeds.embed_poses_clash(*case, thresh=thresh, max_clashes=0, return_poses=True)
    ok4, counts4 = fc.embeds.embed_poses_clash(*case, thresh=thresh, max_clashes=4)
    assert np.array_equal(counts, counts4)  # with and without the poses written
    assert np.array_equal(ok0, counts <= 0) and np.array_equal(ok4, counts <= 4)
    sub = tuple(a[rows] for a in (c1, c2, R1, t1, R2, t2))
    ref = R.pose_ld(m1, m2, *sub)
    bound = TOL * max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(poses[rows] - ref).max()) < bound
    # the count is cdist's on the float64 pose the kernel wrote (checked above): a reference pose rounded from
    # extended precision may differ from it in the last bit, and a count on that would not be a contract
    want = np.array([R.pose_count(p[:A1], p[A1:], thresh) for p in poses[rows]])
    assert np.array_equal(counts[rows], want)
    return counts, want


@pytest.mark.parametrize("A1,A2", [(1, 1), (1, 65), (63, 64), (64, 63), (65, 129), (200, 130), (682, 40), (683, 40), (POSE_ATOMS, 3)])
@pytest.mark.parametrize("P", [1, 3, 4, 5])
def test_pose_kernel_shapes(fc, A1, A2, P):
    for far in (False, True):
        case = _pose_case(A1, A2, P, seed=A1 * 7 + A2 + P, far=far)
        _check_poses(fc, case, np.arange(P))
    # rototranslate is the same expression without the count
    m1, m2, c1, c2, R1, t1, R2, t2 = case
    out = fc.embeds.rototranslate(m1[c1], R1, t1)
    ref = R.rototranslate_ld(m1[c1], R1, t1)
    assert float(np.abs(out - ref).max()) < TOL * max(1.0, float(np.abs(ref).max()))


def test_pose_kernel_counts_something_and_get_embed(fc):
    case = _pose_case(65, 129, 300, seed=5)
    counts, want = _check_poses(fc, case, np.arange(300))
    assert (want == 0).sum() > 10 and (want > 4).sum() > 10 and ((want > 0) & (want <= 4)).sum() > 3

    class Mol:
        pass

    m1, m2, c1, c2, R1, t1, R2, t2 = _pose_case(64, 65, 6, seed=6, far=True)
    a, b = Mol(), Mol()
    a.coords, b.coords = m1, m2
    for k in range(6):
        a.rotation, a.position, b.rotation, b.position = R1[k], t1[k], R2[k], t2[k]
        out = fc.embeds.get_embed([a, b], [c1[k], c2[k]])
        ref = R.pose_ld(m1, m2, c1[k:k + 1], c2[k:k + 1], R1[k:k + 1], t1[k:k + 1], R2[k:k + 1], t2[k:k + 1])[0]
        assert out.shape == (129, 3) and float(np.abs(out - ref).max()) < TOL * float(np.abs(ref).max())


def test_pose_kernel_grid_stride_loop(fc):
    """more poses than the launch has wavefronts (n_cu * 128): every wavefront walks its stride loop at least
    twice, the last pass is ragged"""
    n_cu = L.device_info()["n_cu"]
    assert n_cu > 0
    P = n_cu * 128 * 2 + 3
    case = _pose_case(9, 70, P, seed=11, n1=5, n2=4, scale=1.6)
    rng = np.random.default_rng(12)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(P - 8, P), rng.choice(P, 4096, replace=False)]))
    counts, want = _check_poses(fc, case, rows)
    assert (want == 0).sum() > 100 and (want > 4).sum() > 100
    assert counts.min() >= 0 and counts.max() <= 9 * 70


def test_pose_kernel_refuses_bad_sizes_and_ids_and_goes_on(fc):
    with pytest.raises(fc.FirecodeHipInputError) as e:
        fc.embeds.embed_poses_clash(*_pose_case(POSE_ATOMS + 1, 3, 2, seed=1))
    assert e.value.code == L.FC_E_LIMIT
    case = list(_pose_case(5, 6, 9, seed=2))
    case[3] = case[3].copy()
    case[3][8] = 2  # molecule 2 has conformers 0 and 1
    with pytest.raises(fc.FirecodeHipInputError) as e:
        fc.embeds.embed_poses_clash(*case)
    assert e.value.code == L.FC_E_INVALID
    _check_poses(fc, _pose_case(5, 6, 9, seed=2), np.arange(9))


# ---------------------------------------------------------------------------------------------------------
# fitness
# ---------------------------------------------------------------------------------------------------------
def _gap_thresholds(err):
    """midpoints of the widest gaps between neighbouring reference errors near the 30th and the 70th percentile,
    with the half-width of each gap"""
    e = np.sort(np.asarray(err, dtype=np.float64))
    n = len(e)
    if n == 1:
        return [(float(e[0]) - 1.0, 1.0), (float(e[0]) + 1.0, 1.0)]
    out = []
    for q in (0.3, 0.7):
        c, w = int(q * (n - 1)), max(2, n // 20)
        lo, hi = max(0, c - w), min(n - 1, c + w)
        k = lo + int(np.argmax(np.diff(e[lo:hi + 1])))
        out.append((0.5 * (e[k] + e[k + 1]), 0.5 * (e[k + 1] - e[k])))
    return out


@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("C_", [0, 1, 7])
def test_fitness_check_shapes(fc, N, C_):
    rng = np.random.default_rng(100 * C_ + N)
    A = 14
    seen = set()
    for kind, per_structure in (("blob", False), ("far", True)):
        X = R.ensemble(kind, N, A, seed=N + C_, scale=2.0)
        if per_structure:
            cons = rng.integers(0, A, size=(N, C_, 2))
            targets = rng.uniform(0.5, 4.0, size=(N, C_))
            if C_ == 7:
                targets[rng.random((N, C_)) < 0.2] = np.nan
        else:
            cons = rng.integers(0, A, size=(C_, 2))
            targets = rng.uniform(0.5, 4.0, size=(1, C_))
            if C_ == 7:
                targets[0, 3] = np.nan
        if C_ == 7:
            cons[..., 6, 1] = cons[..., 6, 0]  # a == b: distance exactly 0
        ref, scale = R.fitness_error_ld(X, cons, targets)
        bound = 8 * C_ * R.EPS * scale  # one root of a 3-term sum and one subtraction per term, C terms
        thresholds = _gap_thresholds(ref) if C_ else [(1.0, 1.0), (0.0, 0.0), (-1.0, 1.0)]
        for thr, half in thresholds:
            ok, err = fc.utils.fitness_check_batch(X, cons, targets, threshold=thr)
            dev = np.abs(err.astype(R.LD) - ref).astype(np.float64)
            print(f"fitness N={N} C={C_} {kind}: max deviation {dev.max():.3e}, bound {bound.max():.3e}")
            assert np.all(dev <= bound)
            if C_:
                assert half > bound.max()  # no structure is nearer to the threshold than the bound: none left out
            assert np.array_equal(ok, np.asarray(ref < thr))
            seen.update(ok.tolist())
        if C_ == 0:
            assert not err.any()  # no constraint: 0.0, and the verdict is 0.0 < threshold
        # every target None
        ok, err = fc.utils.fitness_check_batch(X, cons, [[None] * C_] if not per_structure else np.full((N, C_), np.nan), threshold=0.5)
        assert not err.any() and ok.all()
    assert seen == {True, False}


# ---------------------------------------------------------------------------------------------------------
# moments of inertia and the MOI prune
# ---------------------------------------------------------------------------------------------------------
def _atoms(A):
    return np.array((["C", "H", "N", "O", "H"] * (A // 5 + 1))[:A])


def _masses(atoms):
    return np.array([o.MASSES_TABLE[a] for a in atoms])


def _moi_bits(X, masses, tol, energies=None, max_dE=0.0):
    X = L.f64(X)
    N = len(X)
    bits = np.full((N, (N + 63) // 64), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    L.call("fc_moi_simbits", L.pf(X), N, X.shape[1], L.pf(L.f64(masses)), float(tol),
           None if energies is None else L.pf(L.f64(energies)), float(max_dE), L.pw(bits))
    return L.unpack_bits(bits, N)


@pytest.mark.parametrize("N,A", [(1, 5), (64, 3), (65, 65), (1000, 3), (2000, 65), (500, 200), (100000, 8)])
def test_inertia_moments_shapes(fc, N, A):
    masses = _masses(_atoms(A))
    for kind in ("blob", "far") + (("molecule",) if A >= 12 and N <= 2000 else ()):
        X = R.ensemble(kind, N, A, seed=N + A, scale=0.9 * A ** (1.0 / 3.0))
        ref = R.inertia_moments_ld(X, masses)
        mom = fc.algebra.get_inertia_moments_batch(X, masses)
        # symmetric eigenvalues are perfectly conditioned: relative to the largest moment (about the centre of
        # mass, wherever the structure lies: the 'far' kind is 433 A from the origin)
        dev = float(np.abs(mom - ref).max())
        print(f"moments {N}x{A} {kind}: max deviation {dev:.3e}, bound {1e-13 * ref.max():.3e}")
        assert dev < 1e-13 * ref.max()
        assert np.all(np.diff(mom, axis=1) >= 0)
    if N <= 65:
        one = fc.algebra.get_inertia_moments(X[0], masses)
        assert np.array_equal(one, mom[0])


def _scaled_copies(N, A, seed, spread=0.3):
    """one structure breathing: scale factors drawn so that the squared ratio of a pair (the ratio of its moments)
    is spread evenly over [1, 1 + spread] -- relative deviations on both sides of a 1 % or 5 % tolerance, and many
    in the band where dividing by the first or the second structure of the pair decides differently"""
    rng = np.random.default_rng(seed)
    base = rng.normal(scale=0.9 * A ** (1.0 / 3.0), size=(A, 3))
    s = np.sqrt(1.0 + spread * rng.random(N))
    X = np.einsum("nij,aj->nai", R.random_rotations(rng, N), base) * s[:, None, None] + rng.normal(scale=3.0, size=(N, 1, 3))
    return np.ascontiguousarray(X)


def _check_moi_case(fc, X, atoms, asymmetric=False):
    """bits (fc_moi_simbits) and mask (fc_prune_moi) of one ensemble, both tolerances, with and without energies.
    Returns (pairs left out of the bit comparison, masks compared) per tolerance."""
    N = len(X)
    masses = _masses(atoms)
    ref_mom = R.inertia_moments_ld(X, masses)
    en = np.round(np.random.default_rng(16).uniform(0, 2, N), 2)
    iu = np.triu_indices(N, 1)
    out = []
    for tol in (0.01, 0.05):
        band = R.moi_band(ref_mom, tol)[iu]
        left_out = int(band.sum())
        print(f"moi {X.shape} tol={tol}: {left_out} of {len(band)} pairs within 1e-10 of the tolerance")
        assert left_out <= 1e-5 * len(band)
        want = R.moi_similar(ref_mom, tol)
        if asymmetric:  # the case set tells the divisor apart: pairs similar one way round only
            assert (want != want.T).sum() >= 10
        compared = 0
        for energies, dE in ((None, 0.0), (en, 0.5), (en, 0.0)):
            got = _moi_bits(X, masses, tol, energies, dE)
            assert not np.tril(got).any()  # bits of j > i only
            w = want if energies is None else want & (np.abs(en[:, None] - en[None, :]) < dE)
            assert np.array_equal(got[iu][~band], w[iu][~band])
            kw = {} if energies is None else dict(energies=energies, max_dE=dE)
            _, ref_mask = o.prune_by_moment_of_inertia(X, atoms, max_deviation=tol, **kw)
            _, mask = fc.pruner.prune_by_moment_of_inertia(X, atoms, max_deviation=tol, **kw)
            if left_out == 0:
                assert np.array_equal(mask, ref_mask)
                compared += 1
            if energies is not None and dE == 0.0:
                assert mask.all()  # |dE| < 0 never holds
            elif energies is None:
                assert 0 < mask.sum() < N
        out.append((left_out, compared))
    return out


def test_moi_bits_and_mask(fc):
    exact_shapes = 0
    for N, A in ((260, 22), (1000, 3), (2000, 65), (500, 200)):
        res = _check_moi_case(fc, syn.synthetic_ensemble(N, A, seed=15)[0], _atoms(A))
        exact_shapes += all(left_out == 0 and compared == 3 for left_out, compared in res)
    assert exact_shapes >= 3  # the mask was compared exactly, at both tolerances, for at least three of the four shapes


@pytest.mark.parametrize("N,A", [(300, 65), (257, 5)])
def test_moi_bits_tell_the_divisor_apart(fc, N, A):
    res = _check_moi_case(fc, _scaled_copies(N, A, seed=15), _atoms(A), asymmetric=True)
    assert all(compared == 3 for _, compared in res)


def test_moi_prune_100k_rows(fc):
    """1.6e8 (row, word) wavefronts of the bit kernel.  The mask is judged on a seeded sample of rows by what the
    last ladder level (one chunk: the whole ensemble) guarantees under the "earlier falls" rule: no survivor has
    a later survivor similar to it, and every structure that fell has a later structure similar to it"""
    N, A, tol = 100000, 8, 0.01
    X = syn.synthetic_ensemble(N, A, seed=15)[0]
    atoms = _atoms(A)
    mom = R.inertia_moments_ld(X, _masses(atoms))
    _, mask = fc.pruner.prune_by_moment_of_inertia(X, atoms, max_deviation=tol)
    _, again = fc.pruner.prune_by_moment_of_inertia(X, atoms, max_deviation=tol)
    assert np.array_equal(mask, again) and 0 < mask.sum() < N
    rng = np.random.default_rng(17)
    order = np.argsort(mom[:, 2])
    big = mom[order, 2]
    skipped = pairs = 0
    for rows, is_kept in ((rng.choice(np.flatnonzero(mask), 2000, replace=False), True),
                          (rng.choice(np.flatnonzero(~mask), 2000, replace=False), False)):
        for i in rows:
            # only structures whose largest moment lies within 2 tol of row i's can be similar to it
            cand = order[np.searchsorted(big, mom[i, 2] * (1 - 2 * tol)):np.searchsorted(big, mom[i, 2] * (1 + 2 * tol))]
            cand = cand[cand > i]
            both = np.concatenate([[i], cand])
            S = R.moi_similar(mom[both], tol, rows=[0])[0, 1:]
            band = R.moi_band(mom[both], tol, rows=[0])[0, 1:]
            skipped += int(band.sum())
            pairs += N - 1 - i
            if is_kept:
                assert not (S & ~band & mask[cand]).any()
            else:
                assert (S | band).any()
    print(f"moi 100k: {skipped} of {pairs} sampled pairs within 1e-10 of the tolerance")
    assert skipped <= 1e-5 * pairs


def test_moi_zero_moments(fc):
    """0/0 does not tell two structures apart (the oracle's early exit, DESIGN.md "MOI prune: zero moments")"""
    # diatomics on the x axis: the smallest moment is an exact zero
    X = np.zeros((40, 2, 3))
    X[:, 1, 0] = np.repeat([1.0, 1.2, 1.5, 1.5000001], 10)
    atoms = np.array(["C", "O"])
    mom = fc.algebra.get_inertia_moments_batch(X, _masses(atoms))
    assert not mom[:, 0].any() and (mom[:, 1:] > 1.0).all()
    _, ref = o.prune_by_moment_of_inertia(X, atoms)
    _, mask = fc.pruner.prune_by_moment_of_inertia(X, atoms)
    assert np.array_equal(mask, ref) and mask.sum() == 3 and mask[[9, 19, 39]].all()
    bits = _moi_bits(X, _masses(atoms), 0.01)
    assert np.array_equal(bits, np.triu(R.moi_similar(R.inertia_moments_ld(X, _masses(atoms)), 0.01), 1))
    Xa = R.ensemble("axis", 64, 4, seed=3)  # four atoms on the axis, all different: nothing collapses
    _, ref = o.prune_by_moment_of_inertia(Xa, _atoms(4))
    _, mask = fc.pruner.prune_by_moment_of_inertia(Xa, _atoms(4))
    assert np.array_equal(mask, ref)
    # one atom, centred exactly ((x m) / m == x in float64: the others carry rounding noise as moments)
    P = R.ensemble("one", 400, 1, seed=4)
    m = o.MASSES_TABLE["C"]
    P = P[np.all((P * m) / m == P, axis=(1, 2))]
    assert len(P) >= 100
    ref_mom = np.array([o.get_inertia_moments(p, np.array([m])) for p in P])
    assert not ref_mom.any() and not fc.algebra.get_inertia_moments_batch(P, np.array([m])).any()
    _, ref = o.prune_by_moment_of_inertia(P, np.array(["C"]))
    _, mask = fc.pruner.prune_by_moment_of_inertia(P, np.array(["C"]))
    assert np.array_equal(mask, ref) and mask.sum() == 1 and mask[-1]
    # a line along (1, 1, 1): the smallest moment is rounding noise of either sign, not zero -- the rule is then
    # decided by noise; only "runs, and the same twice" is asked
    Xl = R.ensemble("linear", 200, 3, seed=5)
    _, m1 = fc.pruner.prune_by_moment_of_inertia(Xl, _atoms(3))
    _, m2 = fc.pruner.prune_by_moment_of_inertia(Xl, _atoms(3))
    assert np.array_equal(m1, m2) and m1.sum() >= 1


@pytest.mark.parametrize("case", ["A65", "moi_removes_nothing", "moi_leaves_one"])
def test_fused_similarity_stages_equal_the_two_calls(fc, case):
    from firecode_amd import pruner

    rng = np.random.default_rng(21)
    if case == "A65":
        X, atoms = syn.synthetic_ensemble(400, 65, seed=22)[0], _atoms(65)
        X[50:90] *= 1.04
    elif case == "moi_removes_nothing":  # one structure, each copy 3 % larger than the one before: moments 6 % apart
        base = rng.normal(scale=2.0, size=(20, 3))
        X = np.einsum("nij,aj->nai", R.random_rotations(rng, 40), base) * (1.03 ** rng.permutation(40))[:, None, None]
        X = np.ascontiguousarray(X + rng.normal(scale=3.0, size=(40, 1, 3)))
        atoms = _atoms(20)
    else:  # rigid copies of one structure with noise far below either tolerance
        base = rng.normal(scale=2.0, size=(30, 3))
        X = np.einsum("nij,aj->nai", R.random_rotations(rng, 150), base) + rng.normal(scale=1e-7, size=(150, 30, 3))
        atoms = _atoms(30)
    m_moi, m_both, counts = pruner.prune_similarity(X, atoms, max_rmsd=0.5)
    s1, a = pruner.prune_by_moment_of_inertia(X, atoms)
    _, b = pruner.prune_by_rmsd(s1, atoms, 0.5)
    ref = np.zeros(len(X), dtype=bool)
    ref[np.flatnonzero(a)[b]] = True
    assert np.array_equal(m_moi, a) and np.array_equal(m_both, ref)
    assert counts.tolist() == [len(X), int(a.sum()), int(ref.sum())]
    _, oa = o.prune_by_moment_of_inertia(X, atoms)
    assert np.array_equal(a, oa)
    if case == "moi_removes_nothing":
        assert a.all() and ref.sum() < len(X)
    if case == "moi_leaves_one":
        assert a.sum() == 1 and ref.sum() == 1
    if case == "A65":
        assert 1 < ref.sum() < a.sum() < len(X)


# ---------------------------------------------------------------------------------------------------------
# prune_by_rmsd_rot_corr
# ---------------------------------------------------------------------------------------------------------
def _rotcorr(X, atoms, quads, masks, angle_sets, max_angles, max_rmsd=0.25, max_dev=None):
    X = L.f64(X)
    N, A = X.shape[:2]
    T = len(quads)
    angles = np.zeros((T, max_angles))
    n_angles = np.zeros(T, dtype=np.int32)
    for k, a in enumerate(angle_sets):
        angles[k, :len(a)] = a
        n_angles[k] = len(a)
    mask = np.zeros(N, dtype=np.uint8)
    bits = np.zeros((N, (N + 63) // 64), dtype=np.uint64)
    L.call("fc_prune_rmsd_rot_corr", L.pf(X), N, A, L.pb(L.u8(atoms != "H")), L.pi(L.i64(quads)), T, L.pb(L.u8(masks)),
           L.pf(angles), n_angles.ctypes.data_as(C.POINTER(C.c_int32)), max_angles, max_rmsd, 2 * max_rmsd if max_dev is None else max_dev, None, 0.0, 20,
           L.pb(mask), L.pw(bits))
    return L.unpack_bits(bits, N), mask.astype(bool)


def _angle_sets(max_angles):
    if max_angles == 1:
        return [(0.0,), (0.0,)]  # no trial but "leave it": the plain heavy-atom RMSD of the centred structures
    step = 360.0 / 64  # 64 trials; 0, 120 +- 0, 240 and 180 are not all on the grid: the nearest ones win
    return [tuple(step * k for k in range(64)), tuple(step * k for k in range(0, 64, 2))]


@pytest.mark.parametrize("A,N", [(12, 2), (12, 3), (12, 4), (12, 5), (12, 9), (63, 9), (64, 9), (65, 9), (130, 9), (682, 6), (683, 6)])
@pytest.mark.parametrize("max_angles", [1, 64])
def test_rot_corr_bits_shapes(fc, A, N, max_angles):
    from test_gpu_parity import _tbu_ensemble

    X, atoms, graph, torsions, masks = _tbu_ensemble(seed=A + N, n_backbone=2, n_spectators=A - 12)
    assert X.shape == (12, A, 3)
    X = X[:N]
    quads = [t[:4] for t in torsions]
    sets = _angle_sets(max_angles)
    # the default thresholds, and an RMSD threshold in the widest gap of the middle half of the pairs' corrected
    # RMSDs with the max deviation out of play: both verdicts occur whatever the angle set
    hv = o.heavy_mask(atoms)
    Xc = X - X.mean(axis=1, keepdims=True)
    r = np.sort([o.rot_corr_rmsd_and_max(Xc[a], Xc[b], hv, quads, masks, sets)[0] for a in range(N) for b in range(a + 1, N)])
    mid = r[len(r) // 4: len(r) - len(r) // 4] if len(r) >= 4 else np.array([r[0], 2 * r[-1]])
    k = int(np.argmax(np.diff(mid)))
    split = 0.5 * (mid[k] + mid[k + 1])
    assert 0.5 * (mid[k + 1] - mid[k]) > 1e-6  # far from any pair's value
    for max_rmsd, max_dev in ((0.25, 0.5), (split, 100.0)):
        S0 = o.prune_by_rmsd_rot_corr(X, atoms, quads, masks, sets, max_rmsd=max_rmsd, max_dev=max_dev, return_matrix=True)
        ref_mask = o.greedy_prune_from_matrix(S0 | S0.T)  # (the ladder over the same matrix: N <= 9 is one level)
        bits, mask = _rotcorr(X, atoms, quads, masks, sets, max_angles, max_rmsd, max_dev)
        assert np.array_equal(bits, S0) and np.array_equal(mask, ref_mask)
        if max_dev == 100.0 and N >= 4:
            assert 0 < S0.sum() < N * (N - 1) // 2
    if N == 9:
        plain = o.prune_by_rmsd_rot_corr(X, atoms, [], [], [], max_rmsd=0.25, return_matrix=True)
        S0 = o.prune_by_rmsd_rot_corr(X, atoms, quads, masks, sets, max_rmsd=0.25, return_matrix=True)
        if max_angles == 1:
            assert np.array_equal(S0, plain)
        else:
            assert S0.sum() > plain.sum()  # the correction is what makes rotamers alike


# ---------------------------------------------------------------------------------------------------------
# align_structures / align_by_moi
# ---------------------------------------------------------------------------------------------------------
def _rmsd(a, b):
    return float(np.sqrt(((a - b) ** 2).sum() / len(a)))


@pytest.mark.parametrize("A", [3, 64, 65, 200])
@pytest.mark.parametrize("N", [1, 70])
def test_align_structures_shapes(fc, A, N):
    rng = np.random.default_rng(A + N)
    for kind in ("blob", "far", "linear"):
        X = R.ensemble(kind, N, A, seed=A + N, scale=2.0)
        for idx in (None, rng.choice(A, 3, replace=False), np.arange(A), rng.integers(0, A, size=A + 5)):
            out = fc.utils.align_structures(X, idx)
            ref = o.align_structures(X, idx)
            sel = np.arange(A) if idx is None else np.asarray(idx)
            bound = o.rotation_error_bound_batch(np.broadcast_to(X[0][sel], (N, len(sel), 3)), X[:, sel], center=True)
            unique = np.isfinite(bound)
            if kind == "linear":
                assert not unique[1:].any()
            elif A > 3:
                assert unique[1:].all()
            scale = max(1.0, float(np.abs(ref).max()))
            if unique.any():
                assert float(np.abs(out - ref)[unique].max()) < TOL * scale
            for k in np.flatnonzero(~unique):  # no unique rotation: as good a fit as the oracle's, atom for atom on the line
                assert abs(_rmsd(out[k][sel], out[0][sel]) - _rmsd(ref[k][sel], ref[0][sel])) < TOL * scale
                assert np.abs(cdist(out[k], out[k]) - cdist(X[k], X[k])).max() < TOL * scale  # still rigid


@pytest.mark.parametrize("A", [3, 64, 65, 200])
@pytest.mark.parametrize("N", [1, 70])
def test_align_by_moi_shapes(fc, A, N):
    atoms = _atoms(A)
    masses = np.array([fc.pt.pt.mass(a) for a in atoms])
    for kind in ("blob", "far"):
        X = R.ensemble(kind, N, A, seed=2 * A + N, scale=2.0)
        ref = o.align_by_moi(masses, X.copy())
        mine = X.copy()
        out = fc.hypermolecule_class.align_by_moi(atoms, mine)
        scale = max(1.0, float(np.abs(X - X.mean(axis=1, keepdims=True)).max()))
        assert float(np.abs(out - ref).max()) < TOL * scale
        assert float(np.abs(mine.mean(axis=1)).max()) < 1e-12 * max(1.0, float(np.abs(X).max()))
