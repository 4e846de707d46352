"""NumPy restatement of the silhouettes under the RMSD -- the contract of fc_ensemble_silhouette (include/fc_hip.h;
DESIGN.md section 26) line by line, on the oracle's Kabsch RMSD over the selected, centred atoms (``knn_ref.prepared`` /
``knn_ref.distance_rows``).  The FULL rows are used as they are: d(i, j) is row i, column j, never symmetrised.  Test
infrastructure: the product never imports it.

It records ``min_gap``, the smallest difference between the second-smallest and the smallest m[i, .] over all rows that
have at least two other non-empty groups -- the only decision rounding could flip (which group is ``nearest``)."""

from collections import namedtuple

import numpy as np

from knn_ref import distance_rows, prepared  # noqa: F401  (re-exported for the tests)

Q = 2.0 ** 32

RefSilhouette = namedtuple("RefSilhouette", ["values", "intra", "nearest_mean", "nearest", "cluster_means", "sizes", "score",
                                             "min_gap"])


def q32(d):
    """q(d) = (uint64) rint(d * 2^32)"""
    return np.rint(np.asarray(d, dtype=np.float64) * Q).astype(np.uint64)


def silhouette_from_rows(D, labels=None, n_groups=None):
    """The contract of fc_ensemble_silhouette on given rows ``D[i] = d(i, .)`` (the diagonal is never read)."""
    D = np.asarray(D, dtype=np.float64)
    N = D.shape[0]
    labels = np.zeros(N, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if n_groups is None:
        n_groups = max(int(labels.max(initial=-1)) + 1, 1)
    members = [np.flatnonzero(labels == c) for c in range(n_groups)]  # ascending index
    sizes = np.array([len(m) for m in members], dtype=np.int64)
    live = [c for c in range(n_groups) if sizes[c] > 0]
    s, a, b = np.full(N, np.nan), np.full(N, np.nan), np.full(N, np.nan)
    nearest = np.full(N, -1, dtype=np.int32)
    gap = np.inf
    qD = q32(D)
    for i in range(N):
        own = labels[i]
        if own < 0:
            continue
        mem = members[own]
        T_own = qD[i, mem[mem != i]].sum(dtype=np.uint64)
        a[i] = float(T_own) / Q / (sizes[own] - 1) if sizes[own] > 1 else 0.0
        if len(live) < 2:
            continue  # b = s = NaN, nearest = -1
        others = [g for g in live if g != own]
        m = np.array([float(qD[i, members[g]].sum(dtype=np.uint64)) / Q / sizes[g] for g in others])
        k = int(np.argmin(m))  # the first of equal minima: the lowest label
        b[i], nearest[i] = m[k], others[k]
        if len(m) >= 2:
            srt = np.sort(m)
            gap = min(gap, float(srt[1] - srt[0]))
        top = max(a[i], b[i])
        s[i] = 0.0 if sizes[own] == 1 or top == 0.0 else (b[i] - a[i]) / top
    means = np.full(n_groups, np.nan)
    for c in live:
        total = 0.0
        for i in members[c]:
            total += s[i]
        means[c] = total / sizes[c]
    total, count = 0.0, 0
    for i in range(N):
        if labels[i] >= 0:
            total, count = total + s[i], count + 1
    return RefSilhouette(s, a, b, nearest, means, sizes, total / count if count else float("nan"), gap)


def textbook_from_matrix(D, labels):
    """Rousseeuw's formula in floating point on a full matrix, for labels 0 ... K - 1 with at least two non-empty groups
    and no negative label: a = the mean distance to the other members of the own group, b = the smallest mean distance
    to the members of another group, s = (b - a) / max(a, b), 0 for a singleton -> (s, a, b)"""
    D, labels = np.asarray(D, dtype=np.float64), np.asarray(labels)
    N = len(labels)
    s, a, b = np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        same = labels == labels[i]
        same[i] = False
        a[i] = D[i, same].mean() if same.any() else 0.0
        b[i] = min(D[i, labels == g].mean() for g in np.unique(labels) if g != labels[i])
        s[i] = 0.0 if not same.any() or max(a[i], b[i]) == 0.0 else (b[i] - a[i]) / max(a[i], b[i])
    return s, a, b
