"""NumPy / SciPy restatement of the RMSD similarity clusters (include/fc_hip.h, "similarity clusters"; DESIGN.md section
13), built from ``oracle.cpu_ref`` and ``enant_ref`` without touching them.

G has an edge (i, j) exactly where the similarity bit of the pair is set: ``S_default`` / ``S`` of
``enant_ref.similarity`` (or ``o.rmsd_similarity_matrix``'s S), with the energy window applied as ``enant_ref.pack_bits``
applies it.  The clusters are G's connected components (``scipy.sparse.csgraph.connected_components``), numbered by
ascending smallest member; that member is the representative."""

from collections import namedtuple

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import enant_ref as er
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

RefClusters = namedtuple("RefClusters", ["labels", "representatives", "sizes"])


def components(n, ei, ej):
    """components of the undirected graph on n vertices with edges (ei[k], ej[k]) -> RefClusters"""
    n = int(n)
    ei, ej = np.asarray(ei, dtype=np.int64).reshape(-1), np.asarray(ej, dtype=np.int64).reshape(-1)
    if n == 0:
        return RefClusters(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    graph = coo_matrix((np.ones(len(ei), dtype=np.int8), (ei, ej)), shape=(n, n))
    _, raw = connected_components(graph, directed=False)
    _, first = np.unique(raw, return_index=True)      # smallest member of each raw label
    renumber = np.empty(len(first), dtype=np.int64)
    renumber[np.argsort(first, kind="stable")] = np.arange(len(first))
    labels = renumber[raw]
    return RefClusters(labels.astype(np.int32), np.sort(first).astype(np.int64),
                       np.bincount(labels, minlength=len(first)).astype(np.int64))


def components_from_pairs(pairs, n):
    """the same from the device's pair words (i << 32) | j"""
    pairs = np.asarray(pairs, dtype=np.uint64)
    return components(n, (pairs >> np.uint64(32)).astype(np.int64), (pairs & np.uint64(0xFFFFFFFF)).astype(np.int64))


def components_from_bits(bits, n):
    """the same from an (n, ceil(n / 64)) uint64 bit matrix; only bits j > i count"""
    if n == 0:
        return components(0, [], [])
    dense = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    ei, ej = np.nonzero(np.triu(dense, 1))
    return components(n, ei, ej)


def pack_pairs(ei, ej):
    return (np.asarray(ei, dtype=np.uint64) << np.uint64(32)) | np.asarray(ej, dtype=np.uint64)


def pack_bits(n, ei, ej):
    """edges -> the bit matrix, upper triangle only"""
    S = np.zeros((n, n), dtype=bool)
    S[np.minimum(ei, ej), np.maximum(ei, ej)] = True
    return er.pack_bits(S | S.T)


def edges(S, energies=None, max_dE=0.0):
    """(i, j), i < j, of a symmetric similarity matrix, the window applied as ``enant_ref.pack_bits`` does"""
    U = np.triu(np.asarray(S, dtype=bool), 1)
    if energies is not None:
        e = np.asarray(energies, dtype=np.float64)
        U = U & (np.abs(e[:, None] - e[None, :]) < max_dE)
    return np.nonzero(U)


def default_similarity(structures, atoms, max_rmsd, max_dev=None):
    """(S_default, min_gap) through ``o.rmsd_similarity_matrix``: half the work of ``enant_ref.similarity`` where the
    mirror-image values are not needed; ``min_gap`` by the same rule (r always, m where r passes)"""
    max_dev = o.CONVENTIONS["maxdev_factor"] * max_rmsd if max_dev is None else max_dev
    S, R, D = o.rmsd_similarity_matrix(structures, atoms, max_rmsd, max_dev)
    iu = np.triu_indices(len(S), 1)
    r, m = R[iu], D[iu]
    gap = np.abs(r - max_rmsd)
    gap = np.where(r < max_rmsd, np.minimum(gap, np.abs(m - max_dev)), gap)
    return S, (float(gap.min()) if len(gap) else float("inf"))


def processing_order(n, energies):
    """the order the pruner processes conformers in: the stable argsort of usable energies, else as given"""
    if energies is None or len(energies) != n or n == 0:
        return np.arange(n)
    return np.argsort(np.asarray(energies, dtype=np.float64), kind="stable")


def clusters_from_matrix(S, energies=None, max_dE=0.0):
    """RefClusters in the CALLER's order from a similarity matrix in the caller's order: components of the windowed graph
    in processing order, labels scattered back, representatives as indices into the caller's arrays"""
    n = len(S)
    order = processing_order(n, energies)
    Ss = np.asarray(S)[np.ix_(order, order)]
    en = None if energies is None or len(energies) != n else np.asarray(energies, dtype=np.float64)[order]
    ref = components(n, *edges(Ss, en, max_dE))
    labels = np.empty(n, dtype=np.int32)
    labels[order] = ref.labels
    return RefClusters(labels, order[ref.representatives].astype(np.int64), ref.sizes)


def cluster_by_rmsd(structures, atoms, max_rmsd, max_dev=None, energies=None, max_dE=0.0, prune_enantiomers=False):
    """the restatement of ``firecode_amd.pruner.cluster_by_rmsd`` -> (RefClusters, min_gap)"""
    if prune_enantiomers:
        mats = er.similarity(structures, atoms, max_rmsd, max_dev)
        S, gap = mats.S, mats.min_gap
    else:
        S, gap = default_similarity(structures, atoms, max_rmsd, max_dev)
    return clusters_from_matrix(S, energies, max_dE), gap


def same_partition(labels_a, labels_b):
    """two labellings describe the same partition"""
    a, b = np.asarray(labels_a), np.asarray(labels_b)
    if a.shape != b.shape:
        return False
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def path_ensemble(n, A, step=0.3, seed=5, cuts=()):
    """Conformers on a line in conformation space: the skeleton of ``synthetic_ensemble(1, A, seed=2)`` displaced by
    ``k * step * sqrt(A)`` along one centred unit mode, k a random permutation of 0 .. n-1 with the values in ``cuts``
    left out.  Unaligned, neighbours (|dk| = 1) are exactly ``step`` apart in RMSD and second neighbours ``2 step``; the
    best rotation takes off a little.  With ``max_rmsd`` between the two the similarity graph is the path, broken at
    the cuts.  Returns (coords (n - len(cuts), A, 3), atoms, k)."""
    rng = np.random.default_rng(seed)
    base = syn.synthetic_ensemble(1, A, seed=2)[0][0]
    mode = rng.normal(size=(A, 3))
    mode -= mode.mean(axis=0, keepdims=True)
    mode /= np.linalg.norm(mode)
    k = rng.permutation(n)
    k = k[~np.isin(k, np.asarray(cuts, dtype=np.int64))]
    X = base[None] + (k * step * np.sqrt(A))[:, None, None] * mode[None]
    return np.ascontiguousarray(X), np.array(["C"] * A), k
