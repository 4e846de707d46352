"""NumPy / SciPy restatement of the density-based RMSD clusters (include/fc_hip.h, "density-based clusters"; DESIGN.md
section 16), on top of ``cluster_ref``: the same similarity matrix, window, processing order and ``min_gap``.

From the edges of G: degrees (each unordered pair once, the vertex itself excluded); core where ``degree + 1 >= m``;
clusters = SciPy's components of the subgraph induced on the core vertices, numbered by ascending smallest core member,
which is the representative; a vertex that is not core takes the label of its smallest-index core neighbour (border)
or -1 (noise)."""

from collections import namedtuple

import numpy as np

import cluster_ref as cr

RefDbscan = namedtuple("RefDbscan", ["labels", "representatives", "sizes", "core", "degrees"])


def dbscan(n, ei, ej, m, unique=True):
    """RefDbscan of the undirected graph on n vertices; ``unique=True``: the edge list is a set of unordered pairs
    (brought to (min, max) and deduplicated first); ``unique=False``: every list entry counts, as the C entry point does"""
    n = int(n)
    ei, ej = np.asarray(ei, dtype=np.int64).reshape(-1), np.asarray(ej, dtype=np.int64).reshape(-1)
    if unique and len(ei):
        lo, hi = np.unique(np.stack([np.minimum(ei, ej), np.maximum(ei, ej)]), axis=1)
        ei, ej = lo, hi
    deg = (np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)).astype(np.int32)
    core = deg.astype(np.int64) + 1 >= m
    cc = core[ei] & core[ej]
    comp = cr.components(n, ei[cc], ej[cc])                  # non-core vertices: components of one, dropped below
    is_cluster = core[comp.representatives]
    renumber = np.cumsum(is_cluster) - 1
    labels = np.where(core, renumber[comp.labels], -1).astype(np.int64)
    attach = np.full(n, n, dtype=np.int64)                    # smallest core neighbour of each vertex
    for a, b in ((ei, ej), (ej, ei)):
        sel = core[b]
        np.minimum.at(attach, a[sel], b[sel])
    border = ~core & (attach < n)
    labels[border] = labels[attach[border]]
    K = int(is_cluster.sum())
    return RefDbscan(labels.astype(np.int32), comp.representatives[is_cluster].astype(np.int64),
                     np.bincount(labels[labels >= 0], minlength=K).astype(np.int64), core, deg)


def dbscan_from_pairs(pairs, n, m, unique=True):
    pairs = np.asarray(pairs, dtype=np.uint64)
    return dbscan(n, (pairs >> np.uint64(32)).astype(np.int64), (pairs & np.uint64(0xFFFFFFFF)).astype(np.int64), m, unique)


def dbscan_from_bits(bits, n, m):
    if n == 0:
        return dbscan(0, [], [], m)
    dense = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    return dbscan(n, *np.nonzero(np.triu(dense, 1)), m)


def dbscan_from_matrix(S, m, energies=None, max_dE=0.0):
    """RefDbscan in the CALLER's order from a similarity matrix in the caller's order (as ``cr.clusters_from_matrix``)"""
    n = len(S)
    order = cr.processing_order(n, energies)
    Ss = np.asarray(S)[np.ix_(order, order)]
    en = None if energies is None or len(energies) != n else np.asarray(energies, dtype=np.float64)[order]
    ref = dbscan(n, *cr.edges(Ss, en, max_dE), m)
    labels, core, deg = np.empty(n, np.int32), np.empty(n, bool), np.empty(n, np.int32)
    labels[order], core[order], deg[order] = ref.labels, ref.core, ref.degrees
    return RefDbscan(labels, order[ref.representatives].astype(np.int64), ref.sizes, core, deg)


def line_ensemble(t, A=20, seed=5):
    """conformers on a line, as ``cr.path_ensemble``: the skeleton of ``synthetic_ensemble(1, A, seed=2)`` displaced by
    ``t[k] * sqrt(A)`` along one centred unit mode (unaligned RMSD between two of them: ``|t_a - t_b|``)"""
    from firecode_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    base = syn.synthetic_ensemble(1, A, seed=2)[0][0]
    mode = rng.normal(size=(A, 3))
    mode -= mode.mean(axis=0, keepdims=True)
    mode /= np.linalg.norm(mode)
    X = base[None] + (np.asarray(t, dtype=np.float64) * np.sqrt(A))[:, None, None] * mode[None]
    return np.ascontiguousarray(X), np.array(["C"] * A)


DUMBBELL_T = np.r_[0.002 * np.arange(30), 0.458 + 0.4 * np.arange(5), 2.458 + 0.002 * np.arange(30)]
TIE_T = np.array([0, .1, .2, .3, .4, .85, 1.3, 1.4, 1.5, 1.6, 1.7])
