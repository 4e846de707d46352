"""NumPy restatement of the sphere-exclusion (Butina) RMSD clusters (include/fc_hip.h, "sphere-exclusion clusters";
DESIGN.md section 23), on top of ``cluster_ref``: the same similarity matrix, window and processing order.

``walk``: the literal sequential algorithm -- rank the vertices by (degree descending, index ascending), visit them in
that order, an unassigned vertex becomes a centroid and takes its unassigned neighbours -- plus the depth of the
synchronous rounds the device runs.  ``check``: an independent checker that uses no walk, only the two statements the
contract gives as equivalent to it, and the invariants that follow.  Both take an edge list with every unordered pair
once."""

from collections import namedtuple

import numpy as np

import cluster_ref as cr

RefButina = namedtuple("RefButina", ["labels", "centroids", "sizes", "degrees", "depth"])


def _edges(n, ei, ej):
    ei, ej = np.asarray(ei, dtype=np.int64).reshape(-1), np.asarray(ej, dtype=np.int64).reshape(-1)
    if len(ei):
        ei, ej = np.unique(np.stack([np.minimum(ei, ej), np.maximum(ei, ej)]), axis=1)
    return ei, ej


def _rank(deg):
    """position of every vertex in the priority order: more neighbours first, the smaller index on ties"""
    n = len(deg)
    order = np.lexsort((np.arange(n), -deg.astype(np.int64)))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return order, rank


def depth(n, ei, ej, rank):
    """rounds of the synchronous rule until nothing is undecided: per round, over the edges (a before b), a centroid
    claims an undecided b and an undecided a blocks an undecided b; then claimed -> member, not blocked -> centroid"""
    first = rank[ei] < rank[ej]
    a, b = np.where(first, ei, ej), np.where(first, ej, ei)
    state = np.zeros(n, dtype=np.int8)  # 0 undecided, 1 centroid, 2 member
    rounds = 0
    while (state == 0).any():
        rounds += 1
        und_b = state[b] == 0
        claimed, blocked = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        claimed[b[und_b & (state[a] == 1)]] = True
        blocked[b[und_b & (state[a] == 0)]] = True
        und = state == 0
        state[und & claimed] = 2
        state[und & ~claimed & ~blocked] = 1
        assert rounds <= n
    return rounds


def walk(n, ei, ej):
    """RefButina of the undirected graph on n vertices"""
    n = int(n)
    ei, ej = _edges(n, ei, ej)
    deg = (np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)).astype(np.int32)
    order, rank = _rank(deg)
    src, dst = np.r_[ei, ej], np.r_[ej, ei]
    by_src = np.argsort(src, kind="stable")
    dst = dst[by_src]
    start = np.r_[0, np.cumsum(np.bincount(src, minlength=n))]
    centroid_of = np.full(n, -1, dtype=np.int64)
    for v in order:
        if centroid_of[v] >= 0:
            continue
        centroid_of[v] = v
        nb = dst[start[v]:start[v + 1]]
        centroid_of[nb[centroid_of[nb] < 0]] = v
    centroids = np.flatnonzero(centroid_of == np.arange(n)).astype(np.int64)  # ascending
    labels = np.searchsorted(centroids, centroid_of).astype(np.int32)
    return RefButina(labels, centroids, np.bincount(labels, minlength=len(centroids)).astype(np.int64), deg,
                     depth(n, ei, ej, rank) if n else 0)


def check(n, ei, ej, labels, centroids, sizes, degrees):
    """asserts that (labels, centroids, sizes, degrees) is THE sphere-exclusion result of the graph, without walking it"""
    n = int(n)
    ei, ej = _edges(n, ei, ej)
    labels, centroids, sizes = np.asarray(labels), np.asarray(centroids), np.asarray(sizes)
    K = len(centroids)
    assert labels.shape == (n,) and sizes.shape == (K,) and np.asarray(degrees).shape == (n,)
    deg = np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)
    assert np.array_equal(degrees, deg)
    assert int(sizes.sum()) == n and np.array_equal(sizes, np.bincount(labels, minlength=K))
    if n == 0:
        assert K == 0
        return
    assert labels.min() >= 0 and labels.max() == K - 1
    assert np.all(np.diff(centroids) > 0)                                    # numbered by ascending centroid index
    assert np.array_equal(labels[centroids], np.arange(K))
    is_cen = np.zeros(n, dtype=bool)
    is_cen[centroids] = True
    assert not (is_cen[ei] & is_cen[ej]).any()                               # centroids pairwise non-adjacent
    _, rank = _rank(deg)
    first = rank[ei] < rank[ej]
    a, b = np.where(first, ei, ej), np.where(first, ej, ei)
    earlier_centroid = np.zeros(n, dtype=bool)
    earlier_centroid[b[is_cen[a]]] = True
    assert np.array_equal(is_cen, ~earlier_centroid)                         # statement 1
    best = np.full(n, n, dtype=np.int64)                                     # rank of the first centroid neighbour
    for x, y in ((ei, ej), (ej, ei)):
        np.minimum.at(best, x[is_cen[y]], rank[y[is_cen[y]]])
    members = np.flatnonzero(~is_cen)
    assert (best[members] < n).all()                                         # every member adjacent to a centroid ...
    assert np.array_equal(rank[centroids[labels[members]]], best[members])   # ... and owned by the first one: statement 2


def walk_from_pairs(pairs, n):
    pairs = np.asarray(pairs, dtype=np.uint64)
    return walk(n, (pairs >> np.uint64(32)).astype(np.int64), (pairs & np.uint64(0xFFFFFFFF)).astype(np.int64))


def walk_from_bits(bits, n):
    if n == 0:
        return walk(0, [], [])
    dense = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    return walk(n, *np.nonzero(np.triu(dense, 1)))


def sorted_edges(S, energies=None, max_dE=0.0):
    """-> (order, ei, ej): the processing order and the windowed graph of a similarity matrix in that order"""
    n = len(S)
    order = cr.processing_order(n, energies)
    Ss = np.asarray(S)[np.ix_(order, order)]
    en = None if energies is None or len(energies) != n else np.asarray(energies, dtype=np.float64)[order]
    return (order,) + tuple(cr.edges(Ss, en, max_dE))


def walk_from_matrix(S, energies=None, max_dE=0.0):
    """RefButina in the CALLER's order from a similarity matrix in the caller's order (as ``cr.clusters_from_matrix``)"""
    n = len(S)
    order, ei, ej = sorted_edges(S, energies, max_dE)
    ref = walk(n, ei, ej)
    labels, deg = np.empty(n, np.int32), np.empty(n, np.int32)
    labels[order], deg[order] = ref.labels, ref.degrees
    return RefButina(labels, order[ref.centroids].astype(np.int64), ref.sizes, deg, ref.depth)


# ---- the graphs of the tests, by name: -> (n, ei, ej), every unordered pair once ------------------------------------------
def _clique(lo, hi):
    iu, ju = np.triu_indices(hi - lo, 1)
    return iu + lo, ju + lo


def late_claim():
    """h0 (9 leaves + m), m (7 leaves + h0, c2), c2 (6 leaves + m, u), c1 (4 leaves + u), u (c1, c2): c1 is a centroid in
    round 1 and claims u in round 2, c2 -- before c1 in priority -- becomes one only in round 3, and u is c2's"""
    h0, m, c2, c1, u = 0, 1, 2, 3, 4
    e = [(h0, m), (m, c2), (c2, u), (c1, u)]
    nxt = 5
    for hub, leaves in ((h0, 9), (m, 7), (c2, 6), (c1, 4)):
        e += [(hub, nxt + k) for k in range(leaves)]
        nxt += leaves
    e = np.array(e)
    return nxt, e[:, 0], e[:, 1]


def graph(name):
    none = np.zeros(0, np.int64)
    kind, *args = name.split("_")
    if name == "single":
        return 1, none, none
    if name == "two_apart":
        return 2, none, none
    if name == "two_joined":
        return 2, np.array([1]), np.array([0])
    if name == "star":  # the hub in the middle of the indices
        n = 70
        leaves = np.r_[0:33, 34:n]
        return n, np.full(n - 1, 33), leaves
    if name == "bridge":  # two cliques of 6 and 5 joined by one edge
        a, b = _clique(0, 6), _clique(6, 11)
        return 11, np.r_[a[0], b[0], 5], np.r_[a[1], b[1], 6]
    if kind == "complete":
        n = int(args[0])
        return (n,) + _clique(0, n)
    if kind == "ring":
        n = int(args[0])
        return n, np.arange(n), (np.arange(n) + 1) % n
    if name == "cliques":  # disjoint cliques of several sizes under a random relabelling
        rng = np.random.default_rng(7)
        sizes = [1, 2, 3, 7, 64, 65, 30, 1, 12]
        relabel = rng.permutation(sum(sizes))
        ei, ej, lo = [], [], 0
        for s in sizes:
            a, b = _clique(lo, lo + s)
            ei.append(a), ej.append(b)
            lo += s
        return lo, relabel[np.concatenate(ei)], relabel[np.concatenate(ej)]
    if name == "late_claim":
        return late_claim()
    if kind == "path":
        n = int(args[0])
        return n, np.arange(n - 1), np.arange(1, n)
    if kind == "thick":  # i ~ j when |i - j| <= 10
        n = int(args[0])
        ei = np.concatenate([np.arange(n - d) for d in range(1, 11)])
        ej = np.concatenate([np.arange(d, n) for d in range(1, 11)])
        return n, ei, ej
    if kind == "gnp":  # G(n, p)
        n, p = int(args[0]), float(args[1])
        rng = np.random.default_rng(n)
        iu, ju = np.triu_indices(n, 1)
        keep = rng.random(len(iu)) < p
        return n, iu[keep], ju[keep]
    raise KeyError(name)


SMALL_GRAPHS = ["single", "two_apart", "two_joined", "star", "bridge", "complete_63", "complete_64", "complete_65",
                "complete_130", "ring_6", "ring_129", "cliques", "late_claim", "path_2", "path_3", "path_65"]
