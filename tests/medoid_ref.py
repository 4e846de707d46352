"""NumPy restatement of the medoids and of k-medoids under the RMSD -- the contract of fc_ensemble_medoids and
fc_ensemble_kmedoids (include/fc_hip.h) line by line, on the oracle's Kabsch RMSD over the
selected, centred atoms (``knn_ref.prepared`` / ``knn_ref.distance_rows``).  Test infrastructure: the product never
imports it.

Like ``knn_ref`` it records the smallest gap at every decision it makes, so that a test can show that rounding cannot
flip one: the second-smallest minus the smallest sum of a group of three or more (a two-member group is an exact tie by
contract and goes to the lower index), and the second-nearest minus the nearest medoid of a row."""

from collections import namedtuple

import numpy as np

from diverse_ref import select_diverse
from knn_ref import distance_rows, prepared  # noqa: F401  (re-exported for the tests)

Q = 2.0 ** 32

RefMedoids = namedtuple("RefMedoids", ["medoids", "sizes", "mean_distance", "radius", "sums_q32", "eccentricity", "min_gap"])
RefKMedoids = namedtuple("RefKMedoids", ["medoids", "labels", "distances", "cost_q32", "n_iter", "min_gap", "cost0_q32"])


def q32(d):
    """q(d) = (uint64) rint(d * 2^32)"""
    return np.rint(np.asarray(d, dtype=np.float64) * Q).astype(np.uint64)


def symmetrised(D):
    """d is evaluated once per unordered pair, as (row i, column j) with i < j, and serves both partners"""
    U = np.triu(np.asarray(D, dtype=np.float64), 1)
    return U + U.T


def medoids_from_rows(D, labels=None, n_groups=None):
    """The contract of fc_ensemble_medoids on given rows ``D[i] = d(i, .)`` (only i < j is read)."""
    D = symmetrised(D)
    N = D.shape[0]
    labels = np.zeros(N, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if n_groups is None:
        n_groups = max(int(labels.max(initial=-1)) + 1, 1)
    S, E = np.zeros(N, dtype=np.uint64), np.zeros(N)
    med, sizes = np.full(n_groups, -1, dtype=np.int64), np.zeros(n_groups, dtype=np.int64)
    mean, radius = np.full(n_groups, np.nan), np.full(n_groups, np.nan)
    gap = np.inf
    for c in range(n_groups):
        mem = np.flatnonzero(labels == c)  # ascending index
        sizes[c] = len(mem)
        if len(mem) == 0:
            continue
        sub = D[np.ix_(mem, mem)]  # (zero diagonal)
        S[mem] = q32(sub).sum(axis=1, dtype=np.uint64)
        E[mem] = sub.max(axis=1)
        s = S[mem]
        m = int(np.argmin(s))  # the first of equal minima: the lowest index
        med[c] = mem[m]
        if len(mem) >= 3:
            srt = np.sort(s)
            gap = min(gap, float(srt[1] - srt[0]) / Q)
        mean[c] = float(s[m]) / Q / (len(mem) - 1) if len(mem) > 1 else 0.0
        radius[c] = E[mem[m]]
    return RefMedoids(med, sizes, mean, radius, S, E, gap)


def assign(D, M):
    """every conformer to the nearest member of M (row j of D: j is the row conformer of the pair), ties to the earlier
    position; a medoid gets its own position and distance 0 by index -> (labels, distances, cost, gap)"""
    M = np.asarray(M, dtype=np.int64)
    cols = D[:, M]
    lab = np.argmin(cols, axis=1).astype(np.int32)
    dist = cols[np.arange(D.shape[0]), lab].copy()
    gap = np.inf
    if len(M) > 1:
        two = np.sort(cols, axis=1)[:, :2]
        others = np.ones(D.shape[0], dtype=bool)
        others[M] = False
        if others.any():
            gap = float((two[others, 1] - two[others, 0]).min())
    lab[M] = np.arange(len(M), dtype=np.int32)
    dist[M] = 0.0
    return lab, dist, int(q32(dist).astype(object).sum()), gap


def kmedoids_from_rows(D, n, init=None, max_iter=50):
    """The contract of fc_ensemble_kmedoids on given rows; ``init=None``: the picks of the diverse selection from 0, taken
    on the same rows."""
    D = np.asarray(D, dtype=np.float64)
    N = D.shape[0]
    gap = np.inf
    if init is None:
        picks, _, _, _, rec = select_diverse(np.zeros((N, 1, 3)), n, start=0, row=lambda _x, s: D[s])
        init, gap = picks, min(gap, rec.min_gap)
    M = np.asarray(init, dtype=np.int64).copy()
    prev, cost0, n_iter, t = None, None, 0, 0
    while True:
        lab, dist, cost, g = assign(D, M)
        n_iter += 1
        cur = (M, lab, dist, cost)
        if t == 0:
            cost0 = cost
        if t > 0:
            gap = min(gap, abs(cost - prev[3]) / Q)  # the comparison of two costs, each a sum of N distances
        if t > 0 and cost >= prev[3]:
            cur = prev
            break
        gap = min(gap, g)  # (only the assignments that are kept or continued from decide anything)
        if t == max_iter:
            break
        ref = medoids_from_rows(D, lab, n)
        gap = min(gap, ref.min_gap)
        if np.array_equal(ref.medoids, M):
            break
        prev, M, t = cur, ref.medoids.copy(), t + 1
    return RefKMedoids(cur[0], cur[1], cur[2], cur[3], n_iter, gap, cost0)
