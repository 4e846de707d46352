"""The bond-topology check on the GPU (fc_bond_changes / fc_bond_changes_list; molecule_check, scramble_check,
scramble_refining) against the NumPy restatement of its contract (tests/topology_ref.py).  Counts, verdicts and bond
lists are compared for equality: no tolerance appears here.

Shapes are where such kernels go wrong: atom counts around the 64-lane step, one structure of 6 900 atoms split in
many row tiles (changes planted at its first pair (0, 1) and its last pair (A-2, A-1)), 100 000 structures (more than
a y or z grid dimension holds), distances exactly on a bond threshold."""

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import support_ref as R
import topology_ref as ref
from firecode_amd import _lib as L
from firecode_amd import refining, utils
from firecode_amd.torsion_perception import RADII_TABLE, graphize

pytestmark = pytest.mark.gpu

ELEMENTS = np.array(["C", "H", "N", "O", "S", "Pd", "Xx"])  # Xx: not in the table, radius 1.5


def cloud(rng, A, density=0.08):
    """A atoms uniform in a cube at about molecular density: every atom has neighbours near a bond threshold."""
    side = max(2.0, (A / density) ** (1 / 3))
    return rng.uniform(0, side, size=(A, 3))


def plant_ends(X, ref_X):
    """A change at the first pair (0, 1) and at the last pair (A-2, A-1) of every structure: bonded (0.6 A apart,
    below the smallest threshold, H-H's 0.744) in X, far apart in the reference."""
    A = X.shape[1]
    for P, d in ((X, 0.6), (ref_X, 25.0)):
        P[..., 1, :] = P[..., 0, :] + [d, 0, 0]
        P[..., A - 1, :] = P[..., A - 2, :] + [0, d, 0]


def assert_equal(got, want):
    ok, cnt = got[:2]
    assert np.array_equal(cnt, want[1]), np.flatnonzero(cnt != want[1])[:10]
    assert np.array_equal(ok, want[0])
    assert ok.dtype == bool and cnt.dtype == np.int64
    if len(want) > 2:
        assert np.array_equal(got[2][0], want[2][0])
        assert np.array_equal(got[2][1], want[2][1])


@pytest.mark.parametrize("A", [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 6900])
def test_shapes_molecule_and_scramble(fc, A):
    rng = np.random.default_rng(A)
    N = 2 if A > 1000 else 6
    atoms = rng.choice(ELEMENTS, size=A)
    X0 = cloud(rng, A)
    X = X0[None] + rng.normal(scale=0.15, size=(N, A, 3))
    Xr = np.repeat(X0[None], N, axis=0).copy()
    if A >= 3:
        plant_ends(X, Xr)
        X0 = Xr[0]
    for m in (-1, 0, 3):
        want = ref.bond_changes(atoms, X, ref_X=X0, max_newbonds=m, return_bonds=True)
        assert_equal(utils.molecule_check_batch(atoms, X0, X, max_newbonds=m, return_bonds=True), want)
    if A >= 3:  # the first and the last pair of a structure are among the changes
        bonds = want[2][1]
        for n in range(N):
            b = bonds[want[2][0][n]:want[2][0][n + 1]]
            assert tuple(b[0]) == (0, 1, 1) and tuple(b[-1]) == (A - 2, A - 1, 1)
    # per-structure reference
    Xr += rng.normal(scale=0.05, size=Xr.shape)
    want = ref.bond_changes(atoms, X, ref_X=Xr, return_bonds=True)
    assert_equal(utils.molecule_check_batch(atoms, Xr, X, return_bonds=True), want)
    # scramble mode: the reference's bonds as one graph, ragged per-structure exclusions
    g = graphize(atoms, X0)
    excl = [rng.integers(-3, A + 3, size=int(rng.integers(0, 6))) for _ in range(N)]
    excl[0] = np.array([0, 0, A + 7, -1])
    want = ref.bond_changes(atoms, X, ref_bonds=ref.ref_bits_from_edges(g.edges, A), excluded=excl, max_newbonds=1,
                            return_bonds=True)
    assert_equal(utils.scramble_check_batch(atoms, X, excl, [g], max_newbonds=1, return_bonds=True), want)


def test_100k_structures(fc):
    """N = 100 000 > 65 535: a launcher that put the structure index on a y or z grid dimension fails here."""
    rng = np.random.default_rng(5)
    A, N = 50, 100_000
    atoms = rng.choice(ELEMENTS[:5], size=A)
    X0 = cloud(rng, A)
    X = X0[None] + rng.normal(scale=0.05, size=(N, A, 3))
    want = ref.bond_changes(atoms, X, ref_X=X0, return_bonds=True)
    assert want[0].any() and not want[0].all() and want[1][-1000:].any()
    assert_equal(utils.molecule_check_batch(atoms, X0, X, return_bonds=True), want)


@pytest.mark.parametrize("pair", [("H", "H"), ("C", "H"), ("C", "C"), ("C", "S"), ("Xx", "Xx"), ("Pd", "Pd")])
def test_exact_ties(fc, pair):
    """Two-atom structures at thr, one ulp below and above (support_ref.tie_structures), thr in graphize's rounding
    order: fl(1.2 * fl(r_i + r_j)).  Bonded means strictly closer than thr."""
    r = [RADII_TABLE.get(a, 1.5) for a in pair]
    thr = 1.2 * (r[0] + r[1])
    atoms = np.array(pair)
    X = R.tie_structures(thr, 4000, seed=3)
    d = np.array([cdist(x[:1], x[1:])[0, 0] for x in X])
    assert (d == thr).sum() > 0 and (d < thr).any() and (d > thr).any()
    far = np.array([[0.0, 0, 0], [50.0, 0, 0]])
    want = ref.bond_changes(atoms, X, ref_X=far)
    assert np.array_equal(want[1], (d < thr).astype(np.int64))
    assert_equal(utils.molecule_check_batch(atoms, far, X), want)
    edgeless = graphize(atoms, far)
    assert_equal(utils.scramble_check_batch(atoms, X, [], [edgeless]), want)


def test_scramble_fragments_and_exclusions(fc):
    rng = np.random.default_rng(11)
    for n_frag in (1, 2, 3):
        sizes = [int(s) for s in rng.integers(20, 70, size=n_frag)]
        A, N = sum(sizes), 300
        atoms = rng.choice(ELEMENTS, size=A)
        X0 = cloud(rng, A)
        X = X0[None] + rng.normal(scale=0.12, size=(N, A, 3))
        starts = np.concatenate([[0], np.cumsum(sizes)])
        graphs = [graphize(atoms[a:b], X0[a:b]) for a, b in zip(starts[:-1], starts[1:])]
        ref_edges, _ = ref.graphs_reference(graphs)
        B = ref.ref_bits_from_edges(ref_edges, A)
        shared = [0, 3, 3, -2, A, A + 5]
        ragged = [rng.integers(-2, A + 2, size=int(rng.integers(0, 8))) for _ in range(N)]
        ragged[1] = np.zeros(0, dtype=np.int64)
        for excl in (shared, ragged, []):
            for m in (-1, 0, 2):
                want = ref.bond_changes(atoms, X, ref_bonds=B, excluded=excl, max_newbonds=m, return_bonds=True)
                assert_equal(utils.scramble_check_batch(atoms, X, excl, graphs, max_newbonds=m, return_bonds=True),
                             want)
        # the exclusions matter in this set
        none = ref.bond_changes(atoms, X, ref_bonds=B)[1]
        assert (ref.bond_changes(atoms, X, ref_bonds=B, excluded=ragged)[1] < none).any()


def test_bond_list_equals_graphize(fc):
    """Scramble mode against an edgeless graph lists every bond of each structure as formed: graphize's edges."""
    rng = np.random.default_rng(2)
    A, N = 90, 40
    atoms = rng.choice(ELEMENTS, size=A)
    X = cloud(rng, A)[None] + rng.normal(scale=0.1, size=(N, A, 3))
    edgeless = graphize(atoms, np.full((A, 3), 1e3) * np.arange(A)[:, None])
    assert edgeless.number_of_edges() == 0
    _, cnt, (off, bonds) = utils.scramble_check_batch(atoms, X, [], [edgeless], return_bonds=True)
    assert (bonds[:, 2] == 1).all()
    for n in range(N):
        want = sorted((int(i), int(j)) for i, j in graphize(atoms, X[n]).edges)
        got = [(int(i), int(j)) for i, j, _ in bonds[off[n]:off[n + 1]]]
        assert got == want and cnt[n] == len(want)


@pytest.fixture(scope="module")
def catalyst(golden):
    return golden["fx_catalyst_atoms"], golden["fx_catalyst_coords"][0]


def test_perturbed_catalyst(fc, catalyst):
    """fx_catalyst with seeded Gaussian noise at 0.03, 0.05 and 0.1 A, 2 000 structures each.  Not vacuous, from the
    restatement alone: both verdicts occur, and every changed-bond count from 0 to 5."""
    atoms, X0 = catalyst
    seen, verdicts = set(), set()
    for sigma in (0.03, 0.05, 0.1):
        X = X0[None] + np.random.default_rng(7).normal(scale=sigma, size=(2000,) + X0.shape)
        want = ref.bond_changes(atoms, X, ref_X=X0, return_bonds=True)
        seen |= set(want[1].tolist())
        verdicts |= set(want[0].tolist())
        assert_equal(utils.molecule_check_batch(atoms, X0, X, return_bonds=True), want)
    assert verdicts == {True, False}
    assert set(range(6)) <= seen


def test_drop_ins_and_refining(fc, catalyst):
    """The drop-ins one structure at a time and scramble_refining, against the restatement.  The catalyst is cut into
    two fragment graphs; the bonds across the cut are what the constrained (excluded) atoms of an embed look like."""
    atoms, X0 = catalyst
    rng = np.random.default_rng(13)
    X = X0[None] + rng.normal(scale=0.06, size=(64,) + X0.shape)
    A, cut = len(atoms), 40
    graphs = [graphize(atoms[:cut], X0[:cut]), graphize(atoms[cut:], X0[cut:])]
    ref_edges, _ = ref.graphs_reference(graphs)
    B = ref.ref_bits_from_edges(ref_edges, A)
    crossing = sorted({int(v) for a, b in graphize(atoms, X0).edges if a < cut <= b for v in (a, b)})
    inputs = (X.copy(), X0.copy())
    # molecule_check
    for m in (0, 2):
        want = ref.bond_changes(atoms, X, ref_X=X0, max_newbonds=m)[0]
        assert [utils.molecule_check(atoms, X0, x, max_newbonds=m) for x in X] == want.tolist()
    # scramble_check with the reference's log line
    excl = crossing + [crossing[0], -4, A + 1]
    ok, cnt, (off, bonds) = ref.bond_changes(atoms, X, ref_bonds=B, excluded=excl, return_bonds=True)
    assert ok.any() and not ok.all()
    for n in range(len(X)):
        lines = []
        got = utils.scramble_check(atoms, X[n], excl, graphs, logfunction=lines.append, title=f"Candidate_{n + 1}")
        assert got == ok[n]
        if ok[n]:
            assert lines == []
        else:
            delta = {(int(i), int(j)) for i, j, _ in bonds[off[n]:off[n + 1]]}
            assert lines == [f"Candidate_{n + 1}, scramble_check - found {cnt[n]} extra bonds: {delta}"]
        assert utils.scramble_check(atoms, X[n], excl, graphs) == ok[n]
    # scramble_refining: excluded(i) = concat(constrained_indices[i], internal_constraints).ravel(), exit_status kept
    cons = [rng.integers(0, A, size=(int(rng.integers(1, 3)), 2)) for _ in range(len(X))]
    internal = np.array(crossing + crossing[-1:] * (len(crossing) % 2)).reshape(-1, 2)
    status = rng.random(len(X)) < 0.7
    for inter in (internal, ()):
        excl_i = [np.concatenate([c, internal]).ravel() if len(inter) else c.ravel() for c in cons]
        want = ref.bond_changes(atoms, X, ref_bonds=B, excluded=excl_i)[0]
        if len(inter):
            assert (status & want).any() and (status & ~want).any()
        got = refining.scramble_refining(X, atoms, graphs, cons, internal_constraints=inter, exit_status=status)
        assert got.dtype == bool and np.array_equal(got, status & want)
        assert np.array_equal(refining.scramble_refining(X, atoms, graphs, cons, inter), want)
    assert np.array_equal(inputs[0], X) and np.array_equal(inputs[1], X0)


def test_empty_batch(fc):
    atoms = np.array(["C", "H"])
    ok, cnt, (off, bonds) = utils.molecule_check_batch(atoms, np.zeros((2, 3)), np.zeros((0, 2, 3)), return_bonds=True)
    assert ok.shape == (0,) and cnt.shape == (0,) and off.tolist() == [0] and bonds.shape == (0, 3)


def test_list_refuses_offsets_that_disagree_with_the_counts(fc):
    rng = np.random.default_rng(4)
    atoms = np.array(["C"] * 10)
    X = cloud(rng, 10)[None] + rng.normal(scale=0.2, size=(8, 10, 3))
    _, cnt, (off, _) = utils.molecule_check_batch(atoms, X[0], X, return_bonds=True)
    cls, thr = np.zeros(10, dtype=np.int32), np.array([[1.2 * (0.76 + 0.76)]])
    bad = off.copy()
    bad[1:] += 1  # one bond too many in structure 0
    bonds = np.full((int(bad[-1]), 3), -7, dtype=np.int64)
    X0 = np.ascontiguousarray(X[0])
    rc = L.load().fc_bond_changes_list(L.pf(X), 8, 10, cls.ctypes.data_as(L.C.POINTER(L.C.c_int32)), 1, L.pf(thr),
                                       L.pf(X0), 0, None, None, None, 0, L.pi(bad), L.pi(bonds))
    assert rc == L.FC_E_INVALID and (bonds == -7).all()
