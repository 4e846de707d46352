"""NumPy restatement of the k nearest neighbours under the RMSD -- the contract of fc_ensemble_knn (include/fc_hip.h;
DESIGN.md section 18) line by line, on the oracle's Kabsch RMSD over the selected, centred atoms.  Test
infrastructure: the product never imports it.

Like ``diverse_ref`` it records where rounding could change a correct device result: the smallest gap between
consecutive sorted distances of a row among positions 1 ... k + 1 -- the ordering inside the list and the cut at its
end."""

from collections import namedtuple

import numpy as np

from diverse_ref import prepared, rmsd_row  # noqa: F401  (prepared: re-exported for the tests)

RefNeighbours = namedtuple("RefNeighbours", ["indices", "distances", "min_gap"])


def distance_rows(Xsel):
    """(N, N): row i = d(i, .) = ``rmsd_row(Xsel, i)``; the diagonal is whatever the oracle gives, it is never read"""
    N = Xsel.shape[0]
    D = np.empty((N, N))
    for i in range(N):
        D[i] = rmsd_row(Xsel, i)
    return D


def knn_from_rows(D, k):
    """The contract on given rows ``D[i] = d(i, .)``: per row the diagonal left out BY INDEX, a stable sort on
    (d, j), the first k kept, -1 / +inf where the row has fewer than k other conformers."""
    D = np.asarray(D, dtype=np.float64)
    N, k = D.shape[0], int(k)
    idx = np.full((N, k), -1, dtype=np.int32)
    dist = np.full((N, k), np.inf)
    gap = np.inf
    for i in range(N):
        others = np.concatenate([np.arange(i), np.arange(i + 1, N)])  # ascending j: a stable sort keeps it on ties
        d = D[i, others]
        order = np.argsort(d, kind="stable")
        m = min(k, N - 1)
        idx[i, :m] = others[order[:m]]
        dist[i, :m] = d[order[:m]]
        head = d[order[:k + 1]]  # positions 1 ... k + 1
        if len(head) > 1:
            gap = min(gap, float(np.diff(head).min()))
    return RefNeighbours(idx, dist, gap)


def knn(Xsel, k):
    """The contract on prepared coordinates (``prepared``)."""
    return knn_from_rows(distance_rows(np.asarray(Xsel, dtype=np.float64)), k)


def pairs(indices, mutual=False):
    """The undirected edge list of the lists, by sets: (M, 2) int64, i < j, sorted"""
    indices = np.asarray(indices)
    directed = {(i, int(j)) for i in range(indices.shape[0]) for j in indices[i] if j >= 0}
    if mutual:
        und = {(min(i, j), max(i, j)) for i, j in directed if (j, i) in directed}
    else:
        und = {(min(i, j), max(i, j)) for i, j in directed}
    return np.array(sorted(und), dtype=np.int64).reshape(-1, 2)
