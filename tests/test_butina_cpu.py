"""Sphere-exclusion (Butina) RMSD clusters, the part that needs no GPU: the restatement's walk against its independent
checker (tests/butina_ref.py) and the input errors of the Python layer and of the C entry points, all raised before any
device use."""

import ctypes as C

import numpy as np
import pytest

import butina_ref as br
import cluster_ref as cr

ATOMS = np.array(["C"] * 4)


def _random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    ei, ej = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keep = ei != ej
    return ei[keep], ej[keep]


def _checked(n, ei, ej):
    ref = br.walk(n, ei, ej)
    br.check(n, ei, ej, ref.labels, ref.centroids, ref.sizes, ref.degrees)
    assert ref.labels.dtype == np.int32 and ref.centroids.dtype == np.int64 and ref.sizes.dtype == np.int64
    assert ref.degrees.dtype == np.int32
    return ref


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.SMALL_GRAPHS + ["path_3000", "thick_3000", "gnp_300_0.3"])
def test_walk_satisfies_the_checker(name):
    n, ei, ej = br.graph(name)
    ref = _checked(n, ei, ej)
    if name.startswith("complete"):
        assert ref.centroids.tolist() == [0] and ref.sizes.tolist() == [n] and ref.depth == 2
    if name.startswith("ring"):  # all degrees tie: the index decides, every second vertex
        assert ref.centroids.tolist() == list(range(0, n - 1, 2)) and (ref.degrees == 2).all()
    if name == "star":
        assert ref.centroids.tolist() == [33] and ref.sizes.tolist() == [70]
    if name == "bridge":  # the two bridge ends have the largest degrees; the smaller index wins, the other joins it
        assert ref.centroids.tolist() == [5, 7] and ref.labels[6] == 0 and ref.sizes.tolist() == [7, 4]
    if name == "two_apart":
        assert ref.labels.tolist() == [0, 1] and ref.depth == 1
    if name == "two_joined":
        assert ref.labels.tolist() == [0, 0] and ref.centroids.tolist() == [0] and ref.depth == 2
    if name == "path_3000":  # a path in index order decides one vertex per round: the depth worst case
        assert ref.depth >= 1500
    if name == "thick_3000":
        assert 100 < ref.depth < 3000


def test_disjoint_cliques_are_the_components():
    n, ei, ej = br.graph("cliques")
    ref = _checked(n, ei, ej)
    comp = cr.components(n, ei, ej)
    for a, b in zip(ref[:3], comp):
        assert np.array_equal(a, b)


def test_late_claim_goes_to_the_earlier_centroid():
    n, ei, ej = br.late_claim()
    ref = _checked(n, ei, ej)
    assert ref.degrees[:5].tolist() == [10, 9, 8, 5, 2] and ref.depth == 4
    assert ref.centroids[:3].tolist() == [0, 2, 3] and ref.labels[1] == 0
    assert ref.labels[4] == ref.labels[2] != ref.labels[3]      # u is c2's, although c1 was a centroid two rounds earlier


@pytest.mark.parametrize("n,m,seed", [(1, 0, 0), (5, 0, 1), (64, 40, 2), (65, 90, 3), (500, 300, 4), (500, 2000, 5),
                                      (500, 20000, 6)])
def test_random_graphs(n, m, seed):
    ei, ej = _random_graph(n, m, seed)
    ref = _checked(n, ei, ej)
    rng = np.random.default_rng(seed)
    perm, swap = rng.permutation(len(ei)), rng.random(len(ei)) < 0.5   # order, direction and duplicates do not show
    a, b = np.where(swap, ej, ei)[perm], np.where(swap, ei, ej)[perm]
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    for got in (br.walk(n, a, b), br.walk_from_pairs(cr.pack_pairs(a, b), n), br.walk_from_bits(cr.pack_bits(n, lo, hi), n)):
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))


def test_checker_rejects_wrong_answers():
    n, ei, ej = br.late_claim()
    ref = br.walk(n, ei, ej)
    wrong = ref.labels.copy()
    wrong[4] = ref.labels[3]                                      # u given to c1, the centroid that claimed it first
    sizes = np.bincount(wrong, minlength=len(ref.centroids))
    with pytest.raises(AssertionError):
        br.check(n, ei, ej, wrong, ref.centroids, sizes, ref.degrees)
    n, ei, ej = br.graph("ring_6")                                 # RDKit's tie rule (highest index first) is another answer
    with pytest.raises(AssertionError):
        br.check(n, ei, ej, np.array([0, 0, 1, 1, 2, 2], np.int32)[::-1].copy(), np.array([1, 3, 5]), np.array([2, 2, 2]),
                 np.full(6, 2))
    with pytest.raises(AssertionError):                            # a maximal independent set, but not the first one
        br.check(3, [0, 1], [1, 2], np.array([0, 0, 1], np.int32), np.array([0, 2]), np.array([2, 1]), np.array([1, 2, 1]))


def test_matrix_form_energy_order_and_window():
    S = np.zeros((5, 5), dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 4)):
        S[i, j] = S[j, i] = True
    ref = br.walk_from_matrix(S)                                   # the path: 1 (degree 2, smallest index), then 3
    assert ref.centroids.tolist() == [1, 3] and ref.labels.tolist() == [0, 0, 0, 1, 1] and ref.sizes.tolist() == [3, 2]
    energies = np.array([4.0, 3.0, 2.0, 0.5, 0.0])
    ref = br.walk_from_matrix(S, energies, max_dE=10.0)            # processed from the other end: 3, then 1
    assert ref.centroids.tolist() == [3, 1] and ref.labels.tolist() == [1, 1, 0, 0, 0]
    ref = br.walk_from_matrix(S, energies, max_dE=1.2)             # |E2 - E3| = 1.5 cuts it into 0-1-2 and 3-4
    assert ref.degrees.tolist() == [1, 2, 1, 1, 1] and ref.centroids.tolist() == [4, 1] and ref.labels.tolist() == [1, 1, 1, 0, 0]


# ---- input errors, before any device use ---------------------------------------------------------------------------------
def test_new_names_exist():
    import firecode_amd as fc
    from firecode_amd import _lib

    assert fc.pruner.RmsdButina._fields == ("labels", "centroids", "sizes", "degrees")
    for name in ("fc_rmsd_butina", "fc_rmsd_butina_enant", "fc_rmsd_butina_perm", "fc_butina_from_pairs", "fc_butina_from_bits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert hasattr(_lib.DeviceEnsemble, "butina") and hasattr(fc.ensemble.Ensemble, "butina_by_rmsd")
    assert _lib.load().fc_abi_version() == 1
    got = fc.pruner.RmsdButina(np.array([0, 1, 0], np.int32), np.array([0, 1]), np.array([2, 1]), np.array([1, 0, 1], np.int32))
    assert got.members(0).tolist() == [0, 2] and got.members(1).tolist() == [1]
    for bad in (2, -1, True, 0.5):
        with pytest.raises(IndexError):
            got.members(bad)


def test_butina_by_rmsd_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    X = np.zeros((3, 4, 3))
    with pytest.raises(E):
        fc.pruner.butina_by_rmsd(np.zeros((3, 4, 2)), ATOMS, 0.5)
    with pytest.raises(E):
        fc.pruner.butina_by_rmsd(np.zeros((3, 4)), ATOMS, 0.5)
    with pytest.raises(E):
        fc.pruner.butina_by_rmsd(X, ATOMS[:3], 0.5)
    for flag in (1, "yes", None, np.array([True])):
        with pytest.raises(E):
            fc.pruner.butina_by_rmsd(X, ATOMS, 0.5, prune_enantiomers=flag)
    table = np.array([[0, 1, 2, 3], [1, 0, 2, 3]])
    with pytest.raises(E):  # refused together, as in prune_by_rmsd and cluster_by_rmsd
        fc.pruner.butina_by_rmsd(X, ATOMS, 0.5, symmetry=table, prune_enantiomers=True)
    with pytest.raises(E):  # not closed under inverse: the table's own checks come first
        fc.pruner.butina_by_rmsd(X, ATOMS, 0.5, symmetry=np.array([[0, 1, 2, 3], [1, 2, 0, 3]]))
    out = fc.pruner.butina_by_rmsd(np.zeros((0, 4, 3)), ATOMS, 0.5)  # the empty ensemble needs no device
    assert isinstance(out, fc.pruner.RmsdButina)
    for arr, dt in zip(out, (np.int32, np.int64, np.int64, np.int32)):
        assert arr.shape == (0,) and arr.dtype == dt


def test_butina_from_graph_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    ok = cr.pack_pairs([0, 1], [1, 2])
    for pairs, n in ((ok, -1), (ok, 2), (cr.pack_pairs([0, 2], [1, 2]), 3), (np.array([[0, 1], [1, 3]]), 3),
                     (np.array([[0, 1], [-1, 2]]), 3), (np.zeros((2, 3), dtype=np.uint64), 3), (np.array([0.5, 1.5]), 3),
                     (ok, 2 ** 31), (ok, True), (ok, 2.5)):
        with pytest.raises(E):
            fc.pruner.butina_from_pairs(pairs, n)
    for flag in (1, None, "no"):
        with pytest.raises(E):
            fc.pruner.butina_from_pairs(ok, 3, assume_unique=flag)
    for bits, n in ((np.zeros((3, 1), dtype=np.uint64), -3), (np.zeros((3, 2), dtype=np.uint64), 3),
                    (np.zeros((4, 1), dtype=np.uint64), 3), (np.zeros(3, dtype=np.uint64), 3),
                    (np.zeros((3, 1), dtype=np.int64), 3), (np.zeros((3, 1), dtype=np.uint64), True)):
        with pytest.raises(E):
            fc.pruner.butina_from_bits(bits, n)


def test_c_checks_precede_the_device():
    """the C entry points' own checks (a caller of the library without the Python layer): FC_E_INVALID, not the no-device
    error, whether or not a device is present"""
    from firecode_amd import _lib

    lib = _lib.load()
    lab, deg = np.zeros(3, np.int32), np.zeros(3, np.int32)
    reps, sizes, k = np.zeros(3, np.int64), np.zeros(3, np.int64), C.c_int64(7)
    outs = (_lib.ptr(lab, C.c_int32), _lib.pi(reps), _lib.pi(sizes), _lib.ptr(deg, C.c_int32), C.byref(k))
    INV = _lib.FC_E_INVALID
    one = cr.pack_pairs([0], [1])
    for pairs, n in ((cr.pack_pairs([0], [3]), 3), (cr.pack_pairs([1], [1]), 3), (one, -1), (one, 0)):
        assert lib.fc_butina_from_pairs(_lib.pw(pairs), len(pairs), n, *outs) == INV
    assert lib.fc_butina_from_pairs(None, 1, 3, *outs) == INV
    assert lib.fc_butina_from_pairs(None, 0, 0, *outs) == _lib.FC_OK and k.value == 0
    assert lib.fc_butina_from_pairs(_lib.pw(one), 1, 3, *outs[:-1], None) == INV
    for missing in range(4):  # a NULL output with N > 0
        args = list(outs)
        args[missing] = None
        assert lib.fc_butina_from_pairs(_lib.pw(one), 1, 3, *args) == INV
        assert lib.fc_butina_from_bits(_lib.pw(np.zeros((3, 1), np.uint64)), 3, *args) == INV
    assert lib.fc_butina_from_bits(None, -1, *outs) == INV
    assert lib.fc_butina_from_bits(None, 0, *outs) == _lib.FC_OK and k.value == 0
    assert lib.fc_butina_from_bits(None, 3, *outs) == INV
    assert lib.fc_rmsd_butina(None, 0.5, 1.0, None, 0.0, *outs, None) == INV
    assert lib.fc_rmsd_butina_enant(None, 0.5, 1.0, None, 0.0, *outs, None) == INV
    assert lib.fc_rmsd_butina_perm(None, None, 1, 4, 0.5, 1.0, None, 0.0, *outs, None) == INV
    ident = np.arange(4, dtype=np.int32)
    assert lib.fc_rmsd_butina_perm(None, _lib.ptr(ident, C.c_int32), 1, 4, 0.5, 1.0, None, 0.0, *outs, None) == INV
