"""RMSD similarity clusters, the part that needs no GPU: the restatement's own properties (tests/cluster_ref.py) and the
input errors of the Python layer, which are raised before any device use."""

import numpy as np
import pytest

import cluster_ref as cr

ATOMS = np.array(["C"] * 4)


def _random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    ei, ej = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keep = ei != ej
    return ei[keep], ej[keep]


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,seed", [(1, 0, 0), (5, 0, 1), (64, 40, 2), (65, 30, 3), (500, 300, 4), (500, 2000, 5)])
def test_restatement_properties(n, m, seed):
    ei, ej = _random_graph(n, m, seed)
    ref = cr.components(n, ei, ej)
    K = len(ref.sizes)
    assert ref.labels.shape == (n,) and ref.labels.dtype == np.int32
    assert np.array_equal(np.unique(ref.labels), np.arange(K))              # a partition into K non-empty clusters
    assert int(ref.sizes.sum()) == n and np.array_equal(ref.sizes, np.bincount(ref.labels, minlength=K))
    for c in range(K):                                                        # the representative is the minimum
        assert ref.representatives[c] == np.flatnonzero(ref.labels == c).min()
    assert np.all(np.diff(ref.representatives) > 0)                          # numbered by ascending smallest member
    assert np.array_equal(ref.labels[ei], ref.labels[ej])                    # an edge never crosses clusters
    # brute force: labels equal <=> connected (closure of the adjacency matrix)
    if n <= 100:
        reach = np.eye(n, dtype=bool)
        reach[ei, ej] = reach[ej, ei] = True
        for _ in range(8):
            reach = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        assert np.array_equal(reach, ref.labels[:, None] == ref.labels[None, :])


def test_restatement_invariant_under_pair_order_and_form():
    n = 300
    ei, ej = _random_graph(n, 260, 7)
    ref = cr.components(n, ei, ej)
    rng = np.random.default_rng(8)
    perm = rng.permutation(len(ei))
    swap = rng.random(len(ei)) < 0.5
    a, b = np.where(swap, ej, ei)[perm], np.where(swap, ei, ej)[perm]
    for got in (cr.components(n, a, b), cr.components(n, np.r_[a, a[:50]], np.r_[b, b[:50]]),
                cr.components_from_pairs(cr.pack_pairs(a, b), n), cr.components_from_bits(cr.pack_bits(n, ei, ej), n)):
        for x, y in zip(got, ref):
            assert np.array_equal(x, y)


def test_restatement_bits_below_the_diagonal_are_ignored():
    n = 70
    bits = cr.pack_bits(n, np.array([3, 10]), np.array([68, 11]))
    noisy = bits.copy()
    noisy[40, 0] |= np.uint64(1) << np.uint64(5)   # (40, 5): j < i
    noisy[69, 1] |= np.uint64(1) << np.uint64(5)   # (69, 69): the diagonal
    for x, y in zip(cr.components_from_bits(noisy, n), cr.components_from_bits(bits, n)):
        assert np.array_equal(x, y)
    assert len(cr.components_from_bits(bits, n).sizes) == n - 2


def test_restatement_energy_order_and_window():
    S = np.zeros((4, 4), dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 3)):
        S[i, j] = S[j, i] = True
    ref = cr.clusters_from_matrix(S)
    assert ref.labels.tolist() == [0, 0, 0, 0] and ref.representatives.tolist() == [0] and ref.sizes.tolist() == [4]
    energies = np.array([3.0, 2.0, 0.5, 0.0])
    ref = cr.clusters_from_matrix(S, energies, max_dE=10.0)
    assert ref.representatives.tolist() == [3] and ref.labels.tolist() == [0, 0, 0, 0]
    ref = cr.clusters_from_matrix(S, energies, max_dE=1.2)       # |E1 - E2| = 1.5 cuts the path
    assert ref.representatives.tolist() == [3, 1] and ref.labels.tolist() == [1, 1, 0, 0] and ref.sizes.tolist() == [2, 2]
    assert cr.same_partition([0, 0, 1], [5, 5, 2]) and not cr.same_partition([0, 0, 1], [0, 1, 1])


def test_path_ensemble_is_a_path():
    X, atoms, k = cr.path_ensemble(200, 20)
    S, gap = cr.default_similarity(X, atoms, 0.5)
    assert np.array_equal(S, np.abs(k[:, None] - k[None, :]) == 1) and gap > 0.05
    ref = cr.clusters_from_matrix(S)
    assert ref.sizes.tolist() == [200]
    Xc, atoms, kc = cr.path_ensemble(60, 20, cuts=(10, 11, 40))
    ref, gap = cr.cluster_by_rmsd(Xc, atoms, 0.5)
    assert sorted(ref.sizes.tolist()) == [10, 19, 28] and gap > 0.05
    assert cr.same_partition(ref.labels, np.digitize(kc, [10, 40]))


# ---- input errors, before any device use ---------------------------------------------------------------------------------
def test_new_names_exist():
    import firecode_amd as fc
    from firecode_amd import _lib

    assert fc.pruner.RmsdClusters._fields == ("labels", "representatives", "sizes")
    for name in ("fc_rmsd_clusters", "fc_rmsd_clusters_enant", "fc_clusters_from_pairs", "fc_clusters_from_bits"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.DeviceEnsemble, "clusters") and hasattr(fc.ensemble.Ensemble, "cluster_by_rmsd")


def test_cluster_by_rmsd_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    with pytest.raises(E):
        fc.pruner.cluster_by_rmsd(np.zeros((3, 4, 2)), ATOMS, 0.5)
    with pytest.raises(E):
        fc.pruner.cluster_by_rmsd(np.zeros((3, 4)), ATOMS, 0.5)
    with pytest.raises(E):
        fc.pruner.cluster_by_rmsd(np.zeros((3, 4, 3)), ATOMS[:3], 0.5)
    for flag in (1, "yes", None, np.array([True])):
        with pytest.raises(E):
            fc.pruner.cluster_by_rmsd(np.zeros((3, 4, 3)), ATOMS, 0.5, prune_enantiomers=flag)
    out = fc.pruner.cluster_by_rmsd(np.zeros((0, 4, 3)), ATOMS, 0.5)
    assert isinstance(out, fc.pruner.RmsdClusters)
    assert out.labels.shape == (0,) and out.labels.dtype == np.int32
    assert out.representatives.shape == (0,) and out.representatives.dtype == np.int64
    assert out.sizes.shape == (0,) and out.sizes.dtype == np.int64


def test_clusters_from_pairs_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    ok = cr.pack_pairs([0, 1], [1, 2])
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(ok, -1)
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(ok, 2)                                   # index >= n
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(cr.pack_pairs([0, 2], [1, 2]), 3)       # i == j
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(np.array([[0, 1], [1, 3]]), 3)          # (P, 2) form, index >= n
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(np.array([[0, 1], [-1, 2]]), 3)
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(np.zeros((2, 3), dtype=np.uint64), 3)   # wrong shape
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(np.array([0.5, 1.5]), 3)                # not integers
    with pytest.raises(E):
        fc.pruner.clusters_from_pairs(ok, 2 ** 31)


def test_clusters_from_pairs_c_checks_precede_the_device():
    """the C entry point's own checks (a caller of the library without the Python layer): FC_E_INVALID, not the no-device
    error, whether or not a device is present"""
    import ctypes as C

    from firecode_amd import _lib

    lib = _lib.load()
    lab, reps, sizes, k = np.zeros(3, np.int32), np.zeros(3, np.int64), np.zeros(3, np.int64), C.c_int64(7)
    args = (_lib.ptr(lab, C.c_int32), _lib.pi(reps), _lib.pi(sizes), C.byref(k))
    for pairs, n in ((cr.pack_pairs([0], [3]), 3), (cr.pack_pairs([1], [1]), 3), (cr.pack_pairs([0], [1]), -1),
                     (cr.pack_pairs([0], [1]), 0)):
        assert lib.fc_clusters_from_pairs(_lib.pw(pairs), len(pairs), n, *args) == _lib.FC_E_INVALID
    assert lib.fc_clusters_from_pairs(None, 0, 0, *args) == _lib.FC_OK and k.value == 0
    assert lib.fc_clusters_from_bits(None, -1, *args) == _lib.FC_E_INVALID
    assert lib.fc_clusters_from_bits(None, 0, *args) == _lib.FC_OK and k.value == 0
    assert lib.fc_clusters_from_bits(None, 3, *args) == _lib.FC_E_INVALID
    assert lib.fc_rmsd_clusters(None, 0.5, 1.0, None, 0.0, *args, None) == _lib.FC_E_INVALID
    assert lib.fc_rmsd_clusters_enant(None, 0.5, 1.0, None, 0.0, *args, None) == _lib.FC_E_INVALID


def test_clusters_from_bits_input_errors():
    import firecode_amd as fc

    E = fc.FirecodeHipInputError
    with pytest.raises(E):
        fc.pruner.clusters_from_bits(np.zeros((3, 1), dtype=np.uint64), -3)
    with pytest.raises(E):
        fc.pruner.clusters_from_bits(np.zeros((3, 2), dtype=np.uint64), 3)    # wrong number of words
    with pytest.raises(E):
        fc.pruner.clusters_from_bits(np.zeros((4, 1), dtype=np.uint64), 3)    # wrong number of rows
    with pytest.raises(E):
        fc.pruner.clusters_from_bits(np.zeros(3, dtype=np.uint64), 3)         # not a matrix
    with pytest.raises(E):
        fc.pruner.clusters_from_bits(np.zeros((3, 1), dtype=np.int64), 3)     # wrong dtype
