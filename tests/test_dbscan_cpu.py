"""Density-based RMSD clusters, the part that needs no GPU: the restatement's own properties (tests/dbscan_ref.py) and
the input errors of the Python layer and of the C entry points, all raised before any device use."""

import ctypes as C

import numpy as np
import pytest

import cluster_ref as cr
import dbscan_ref as dr

ATOMS = np.array(["C"] * 4)


def _random_graph(n, m, seed):
    """distinct unordered pairs"""
    rng = np.random.default_rng(seed)
    ei, ej = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keep = ei != ej
    lo, hi = np.unique(np.stack([np.minimum(ei, ej)[keep], np.maximum(ei, ej)[keep]]), axis=1)
    return lo, hi


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


CASES = [(1, 0, 0), (5, 0, 1), (64, 40, 2), (65, 90, 3), (500, 300, 4), (500, 2000, 5)]


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m_edges,seed", CASES)
def test_m1_is_the_components_and_m2_turns_singletons_into_noise(n, m_edges, seed):
    ei, ej = _random_graph(n, m_edges, seed)
    comp = cr.components(n, ei, ej)
    one = dr.dbscan(n, ei, ej, 1)
    assert _same(one[:3], comp) and one.core.all() and (one.labels >= 0).all()
    two = dr.dbscan(n, ei, ej, 2)
    single = comp.sizes[comp.labels] == 1
    assert np.array_equal(two.labels < 0, single) and np.array_equal(two.core, ~single)
    assert np.array_equal(two.representatives, comp.representatives[comp.sizes > 1])
    assert np.array_equal(two.sizes, comp.sizes[comp.sizes > 1])
    assert cr.same_partition(two.labels[~single], comp.labels[~single])


@pytest.mark.parametrize("n,m_edges,seed", CASES)
def test_restatement_properties(n, m_edges, seed):
    ei, ej = _random_graph(n, m_edges, seed)
    A = np.zeros((n, n), dtype=bool)
    A[ei, ej] = A[ej, ei] = True
    previous_core = np.ones(n, dtype=bool)
    for m in (1, 2, 3, 4, 6, 9, n + 1):
        ref = dr.dbscan(n, ei, ej, m)
        K = len(ref.sizes)
        assert ref.labels.dtype == np.int32 and ref.degrees.dtype == np.int32 and ref.core.dtype == bool
        assert np.array_equal(ref.degrees, A.sum(axis=1))
        assert np.array_equal(ref.core, ref.degrees + 1 >= m)
        assert not (ref.core & ~previous_core).any()                           # the core set shrinks as m grows
        previous_core = ref.core
        assert np.array_equal(ref.sizes, np.bincount(ref.labels[ref.labels >= 0], minlength=K))
        assert np.all(np.diff(ref.representatives) > 0) and ref.core[ref.representatives].all()
        for c in range(K):                                                      # the representative: smallest CORE member
            assert ref.representatives[c] == np.flatnonzero((ref.labels == c) & ref.core).min()
        cc = ref.core[ei] & ref.core[ej]
        assert np.array_equal(ref.labels[ei[cc]], ref.labels[ej[cc]])          # a core-core edge never crosses clusters
        for i in np.flatnonzero(~ref.core):                                     # borders are never core; the border rule
            nb = np.flatnonzero(A[i] & ref.core)
            assert ref.labels[i] == (ref.labels[nb.min()] if len(nb) else -1)
        if m == n + 1:
            assert K == 0 and (ref.labels == -1).all() and not ref.core.any()


def test_restatement_invariant_under_pair_order_and_form():
    n = 300
    ei, ej = _random_graph(n, 700, 7)
    rng = np.random.default_rng(8)
    for m in (1, 3, 5):
        ref = dr.dbscan(n, ei, ej, m)
        perm = rng.permutation(len(ei))
        swap = rng.random(len(ei)) < 0.5
        a, b = np.where(swap, ej, ei)[perm], np.where(swap, ei, ej)[perm]
        for got in (dr.dbscan(n, a, b, m), dr.dbscan_from_pairs(cr.pack_pairs(a, b), n, m),
                    dr.dbscan_from_bits(cr.pack_bits(n, ei, ej), n, m)):
            assert _same(got, ref)


def test_restatement_bits_below_the_diagonal_are_ignored():
    n = 70
    bits = cr.pack_bits(n, np.array([3, 10, 3]), np.array([68, 11, 10]))
    noisy = bits.copy()
    noisy[40, 0] |= np.uint64(1) << np.uint64(5)   # (40, 5): j < i
    noisy[69, 1] |= np.uint64(1) << np.uint64(5)   # (69, 69): the diagonal
    for m in (1, 2, 3):
        assert _same(dr.dbscan_from_bits(noisy, n, m), dr.dbscan_from_bits(bits, n, m))
    ref = dr.dbscan_from_bits(bits, n, 3)
    assert ref.degrees[[3, 10, 11, 68]].tolist() == [2, 2, 1, 1] and ref.core.sum() == 2
    assert ref.labels[[3, 10, 11, 68]].tolist() == [0, 0, 0, 0] and (ref.labels < 0).sum() == n - 4


def test_restatement_duplicated_pair():
    """a pair listed twice: removed under unique=True (what the Python wrapper does), counted twice otherwise (what the C
    entry point does, and the wrapper with assume_unique=True)"""
    ei, ej = np.array([0, 1, 1]), np.array([1, 2, 0])   # the path 0 - 1 - 2 with (0, 1) twice
    clean = dr.dbscan(3, ei, ej, 3)
    assert clean.degrees.tolist() == [1, 2, 1] and clean.core.tolist() == [False, True, False]
    assert clean.labels.tolist() == [0, 0, 0] and clean.representatives.tolist() == [1]
    raw = dr.dbscan(3, ei, ej, 3, unique=False)
    assert raw.degrees.tolist() == [2, 3, 1] and raw.core.tolist() == [True, True, False]
    assert raw.labels.tolist() == [0, 0, 0] and raw.representatives.tolist() == [0]


def test_restatement_energy_order_and_window():
    S = np.zeros((5, 5), dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 4)):
        S[i, j] = S[j, i] = True
    ref = dr.dbscan_from_matrix(S, 3)                         # the path: interior core, the ends border
    assert ref.core.tolist() == [False, True, True, True, False] and ref.labels.tolist() == [0] * 5
    assert ref.representatives.tolist() == [1] and ref.sizes.tolist() == [5]
    energies = np.array([4.0, 3.0, 2.0, 0.5, 0.0])
    ref = dr.dbscan_from_matrix(S, 3, energies, max_dE=10.0)  # processed from the other end
    assert ref.representatives.tolist() == [3] and ref.labels.tolist() == [0] * 5
    ref = dr.dbscan_from_matrix(S, 3, energies, max_dE=1.2)  # |E2 - E3| = 1.5 cuts the path into 0-1-2 and 3-4
    assert ref.degrees.tolist() == [1, 2, 1, 1, 1] and ref.core.tolist() == [False, True, False, False, False]
    assert ref.labels.tolist() == [0, 0, 0, -1, -1] and ref.representatives.tolist() == [1] and ref.sizes.tolist() == [3]


def test_the_issue_ensembles():
    """the 1-D ensembles of the GPU tests, on the restatement alone"""
    X, atoms = dr.line_ensemble(dr.DUMBBELL_T)
    S, gap = cr.default_similarity(X, atoms, 0.5)
    assert gap > 0.04 and int(np.triu(S, 1).sum()) == 934 and cr.clusters_from_matrix(S).sizes.tolist() == [65]
    for m in range(4, 33):
        ref = dr.dbscan_from_matrix(S, m)
        assert ref.sizes.tolist() == [32, 32] and ref.labels[30:35].tolist() == [0, 0, -1, 1, 1], m
    assert dr.dbscan_from_matrix(S, 32).core.sum() == 2 and dr.dbscan_from_matrix(S, 32).core[[30, 34]].all()
    assert (dr.dbscan_from_matrix(S, 33).labels == -1).all()
    X, atoms = dr.line_ensemble(dr.TIE_T)
    S, gap = cr.default_similarity(X, atoms, 0.5)
    ref = dr.dbscan_from_matrix(S, 5)
    assert gap > 0.03 and ref.degrees.tolist() == [4, 4, 4, 4, 5, 2, 5, 4, 4, 4, 4]
    assert not ref.core[5] and S[5, 4] and S[5, 6] and ref.labels[4] != ref.labels[6] and ref.labels[5] == ref.labels[4]


# ---- input errors, before any device use ---------------------------------------------------------------------------------
def test_new_names_exist():
    import firecode_amd as fc
    from firecode_amd import _lib

    assert fc.pruner.RmsdDbscan._fields == ("labels", "representatives", "sizes", "core", "degrees")
    for name in ("fc_rmsd_dbscan", "fc_rmsd_dbscan_enant", "fc_rmsd_dbscan_perm", "fc_dbscan_from_pairs", "fc_dbscan_from_bits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert hasattr(_lib.DeviceEnsemble, "dbscan") and hasattr(fc.ensemble.Ensemble, "dbscan_by_rmsd")
    assert _lib.load().fc_abi_version() == 1


BAD_MIN_SAMPLES = (0, -1, True, False, 2.0, 2.5, None, "3", np.float64(3.0), np.bool_(True))


def test_dbscan_by_rmsd_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    X = np.zeros((3, 4, 3))
    for bad in BAD_MIN_SAMPLES:
        with pytest.raises(E):
            fc.pruner.dbscan_by_rmsd(X, ATOMS, 0.5, min_samples=bad)
    with pytest.raises(E):
        fc.pruner.dbscan_by_rmsd(np.zeros((3, 4, 2)), ATOMS, 0.5)
    with pytest.raises(E):
        fc.pruner.dbscan_by_rmsd(np.zeros((3, 4)), ATOMS, 0.5)
    with pytest.raises(E):
        fc.pruner.dbscan_by_rmsd(X, ATOMS[:3], 0.5)
    for flag in (1, "yes", None, np.array([True])):
        with pytest.raises(E):
            fc.pruner.dbscan_by_rmsd(X, ATOMS, 0.5, prune_enantiomers=flag)
    table = np.array([[0, 1, 2, 3], [1, 0, 2, 3]])
    with pytest.raises(E):  # refused together, as in prune_by_rmsd and cluster_by_rmsd
        fc.pruner.dbscan_by_rmsd(X, ATOMS, 0.5, symmetry=table, prune_enantiomers=True)
    with pytest.raises(E):  # not closed under inverse: the table's own checks come first
        fc.pruner.dbscan_by_rmsd(X, ATOMS, 0.5, symmetry=np.array([[0, 1, 2, 3], [1, 2, 0, 3]]))
    out = fc.pruner.dbscan_by_rmsd(np.zeros((0, 4, 3)), ATOMS, 0.5, min_samples=np.int64(3))
    assert isinstance(out, fc.pruner.RmsdDbscan)
    for arr, dt in zip(out, (np.int32, np.int64, np.int64, bool, np.int32)):
        assert arr.shape == (0,) and arr.dtype == dt


def test_dbscan_from_pairs_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    ok = cr.pack_pairs([0, 1], [1, 2])
    for bad in BAD_MIN_SAMPLES:
        with pytest.raises(E):
            fc.pruner.dbscan_from_pairs(ok, 3, bad)
        with pytest.raises(E):
            fc.pruner.dbscan_from_bits(np.zeros((3, 1), dtype=np.uint64), 3, bad)
    for pairs, n in ((ok, -1), (ok, 2), (cr.pack_pairs([0, 2], [1, 2]), 3), (np.array([[0, 1], [1, 3]]), 3),
                     (np.array([[0, 1], [-1, 2]]), 3), (np.zeros((2, 3), dtype=np.uint64), 3), (np.array([0.5, 1.5]), 3),
                     (ok, 2 ** 31), (ok, True)):
        with pytest.raises(E):
            fc.pruner.dbscan_from_pairs(pairs, n, 2)
    for flag in (1, None, "no"):
        with pytest.raises(E):
            fc.pruner.dbscan_from_pairs(ok, 3, 2, assume_unique=flag)


def test_dbscan_from_bits_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    for bits, n in ((np.zeros((3, 1), dtype=np.uint64), -3), (np.zeros((3, 2), dtype=np.uint64), 3),
                    (np.zeros((4, 1), dtype=np.uint64), 3), (np.zeros(3, dtype=np.uint64), 3),
                    (np.zeros((3, 1), dtype=np.int64), 3)):
        with pytest.raises(E):
            fc.pruner.dbscan_from_bits(bits, n, 2)


def test_c_checks_precede_the_device():
    """the C entry points' own checks (a caller of the library without the Python layer): FC_E_INVALID, not the no-device
    error, whether or not a device is present"""
    from firecode_amd import _lib

    lib = _lib.load()
    lab, deg = np.zeros(3, np.int32), np.zeros(3, np.int32)
    reps, sizes, core, k = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(3, np.uint8), C.c_int64(7)
    outs = (_lib.ptr(lab, C.c_int32), _lib.pi(reps), _lib.pi(sizes), _lib.pb(core), _lib.ptr(deg, C.c_int32), C.byref(k))
    INV = _lib.FC_E_INVALID
    one = cr.pack_pairs([0], [1])
    for pairs, n, m in ((cr.pack_pairs([0], [3]), 3, 2), (cr.pack_pairs([1], [1]), 3, 2), (one, -1, 2), (one, 0, 2),
                        (one, 3, 0), (one, 3, -4)):
        assert lib.fc_dbscan_from_pairs(_lib.pw(pairs), len(pairs), n, m, *outs) == INV
    assert lib.fc_dbscan_from_pairs(None, 1, 3, 2, *outs) == INV
    assert lib.fc_dbscan_from_pairs(None, 0, 0, 2, *outs) == _lib.FC_OK and k.value == 0
    assert lib.fc_dbscan_from_pairs(None, 0, 0, 0, *outs) == INV
    assert lib.fc_dbscan_from_pairs(_lib.pw(one), 1, 3, 2, *outs[:-1], None) == INV
    for missing in range(5):  # a NULL output with N > 0
        args = list(outs)
        args[missing] = None
        assert lib.fc_dbscan_from_pairs(_lib.pw(one), 1, 3, 2, *args) == INV
        assert lib.fc_dbscan_from_bits(_lib.pw(np.zeros((3, 1), np.uint64)), 3, 2, *args) == INV
    assert lib.fc_dbscan_from_bits(None, -1, 2, *outs) == INV
    assert lib.fc_dbscan_from_bits(None, 0, 2, *outs) == _lib.FC_OK and k.value == 0
    assert lib.fc_dbscan_from_bits(None, 0, 0, *outs) == INV
    assert lib.fc_dbscan_from_bits(None, 3, 2, *outs) == INV
    assert lib.fc_rmsd_dbscan(None, 0.5, 1.0, 2, None, 0.0, *outs, None) == INV
    assert lib.fc_rmsd_dbscan_enant(None, 0.5, 1.0, 2, None, 0.0, *outs, None) == INV
    assert lib.fc_rmsd_dbscan_perm(None, None, 1, 4, 0.5, 1.0, 2, None, 0.0, *outs, None) == INV
    ident = np.arange(4, dtype=np.int32)
    assert lib.fc_rmsd_dbscan_perm(None, _lib.ptr(ident, C.c_int32), 1, 4, 0.5, 1.0, 2, None, 0.0, *outs, None) == INV
