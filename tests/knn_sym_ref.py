"""NumPy restatement of the symmetry- and mirror-aware distance of the nearest-neighbour lists (fc_ensemble_knn_perm,
fc_ensemble_knn_cross_perm, include/fc_hip.h), built from ``oracle.cpu_ref`` without touching it.
Test infrastructure: the product never imports it.

For the prepared ensembles Q and R (atom selection applied, every conformer centred on the centroid of its selected
atoms) and a (K, A_sel) table ``perms`` (identity first, closed under inverse):

    d_sym(i, j) = min over p < K, h in H of rmsd_and_max(Q[i], h * R[j][perms[p]])[0]
    H = {+1}, or {+1, -1} with ``mirror`` (-1: the partner inverted through the origin)

The lists are then those of ``knn_ref.knn_from_rows`` (one ensemble: the diagonal left out by index) and
``knn_cross_ref.knn_from_rows`` (two: nothing left out, the cap) on these rows, with their ``min_gap``."""

import numpy as np

import knn_cross_ref as xr
import knn_ref
from diverse_ref import prepared  # noqa: F401  (re-exported for the tests)
from diverse_sym_ref import centred
from oracle import cpu_ref as o


def distance_rows(Qsel, Rsel, perms, mirror=False):
    """(Nq, Nr): row i = d_sym(i, .), as ``diverse_sym_ref.sym_row`` forms its rows, but Q against R"""
    Q, R = centred(Qsel), centred(Rsel)
    perms = np.asarray(perms)
    D = np.full((Q.shape[0], R.shape[0]), np.inf)
    if not R.shape[0]:
        return D
    for i in range(Q.shape[0]):
        P = np.broadcast_to(Q[i], R.shape)
        for perm in perms:
            for h in ((1.0, -1.0) if mirror else (1.0,)):
                D[i] = np.minimum(D[i], o.rmsd_and_max_batch(P, h * R[:, perm])[0])
    return D


def self_rows(Xsel, perms, mirror=False):
    """(N, N): d_sym of every ordered pair of one ensemble; the diagonal is never read"""
    return distance_rows(Xsel, Xsel, perms, mirror)


def knn_from_rows(D, k):
    """the self form on given rows -> ``knn_ref.RefNeighbours``"""
    return knn_ref.knn_from_rows(D, k)


def knn_cross_from_rows(D, k, max_rmsd=None):
    """the cross form on given rows -> ``knn_cross_ref.RefCrossNeighbours``"""
    return xr.knn_from_rows(D, k, max_rmsd)


novel = xr.novel
coverage = xr.coverage


def mean_distance(dist):
    """the mean of the finite entries, nan when there is none"""
    dist = np.asarray(dist, dtype=np.float64)
    finite = dist[np.isfinite(dist)]
    return float(finite.mean()) if finite.size else float("nan")
