"""NumPy restatement of the nearest neighbours ACROSS two ensembles under the RMSD -- the contract of
fc_ensemble_knn_cross (include/fc_hip.h) line by line, on the oracle's Kabsch RMSD over the
selected, centred atoms.  Test infrastructure: the product never imports it.

Like ``knn_ref`` it records where rounding could change a correct device result: the smallest gap between consecutive
sorted distances of a row among positions 1 ... k + 1 (the ordering inside the list and the cut at its end) and, with a
cap, the smallest ``|d - max_rmsd|`` over ALL pairs (every ``d < max_rmsd`` decision)."""

from collections import namedtuple

import numpy as np

from diverse_ref import prepared  # noqa: F401  (re-exported for the tests)
from oracle import cpu_ref as o

RefCrossNeighbours = namedtuple("RefCrossNeighbours", ["indices", "distances", "min_gap"])


def distance_rows(Qsel, Rsel):
    """(Nq, Nr): row i = d(i, .) = rmsd_and_max(Q[i], R[j], center=True)[0] for every j, the oracle's stacked form"""
    Qsel, Rsel = np.asarray(Qsel, dtype=np.float64), np.asarray(Rsel, dtype=np.float64)
    D = np.empty((Qsel.shape[0], Rsel.shape[0]))
    for i in range(Qsel.shape[0]):
        if Rsel.shape[0]:
            D[i] = o.rmsd_and_max_batch(np.broadcast_to(Qsel[i], Rsel.shape), Rsel, center=True)[0]
    return D


def knn_from_rows(D, k, max_rmsd=None):
    """The contract on given rows ``D[i] = d(i, .)`` (Nq, Nr): per row a stable sort on (d, j) -- nothing left out --
    then the cap (only ``d < max_rmsd`` stays), then -1 / +inf in the slots that are left."""
    D = np.asarray(D, dtype=np.float64)
    Nq, Nr, k = D.shape[0], D.shape[1], int(k)
    idx = np.full((Nq, k), -1, dtype=np.int32)
    dist = np.full((Nq, k), np.inf)
    gap = np.inf
    for i in range(Nq):
        order = np.argsort(D[i], kind="stable")  # ascending j on ties
        head = D[i, order[:k + 1]]  # positions 1 ... k + 1
        if len(head) > 1:
            gap = min(gap, float(np.diff(head).min()))
        keep = order[:k]
        if max_rmsd is not None:
            keep = keep[D[i, keep] < max_rmsd]
        idx[i, :len(keep)] = keep
        dist[i, :len(keep)] = D[i, keep]
    if max_rmsd is not None and D.size:
        gap = min(gap, float(np.abs(D - max_rmsd).min()))
    return RefCrossNeighbours(idx, dist, gap)


def knn(Qsel, Rsel, k, max_rmsd=None):
    """The contract on prepared coordinates (``prepared``)."""
    return knn_from_rows(distance_rows(Qsel, Rsel), k, max_rmsd)


def novel(D, max_rmsd):
    """(Nq,) bool: no reference with ``d < max_rmsd``"""
    D = np.asarray(D, dtype=np.float64)
    return ~(D < max_rmsd).any(axis=1)


def coverage(D_refs_against_structures, max_rmsd):
    """On the rows of the REFERENCES against the structures (Nr, Nq): (covered (Nr,), fraction, nearest (Nr,) int32,
    distances (Nr,)) -- the nearest structure of every reference (lowest index on ties), -1 / +inf when there is none"""
    D = np.asarray(D_refs_against_structures, dtype=np.float64)
    if D.shape[1] == 0:
        nearest, dist = np.full(D.shape[0], -1, dtype=np.int32), np.full(D.shape[0], np.inf)
    else:
        nearest = np.argmin(D, axis=1).astype(np.int32)  # (the first of equal minima)
        dist = D[np.arange(D.shape[0]), nearest]
    covered = dist < max_rmsd
    return covered, (float(covered.mean()) if len(covered) else float("nan")), nearest, dist
