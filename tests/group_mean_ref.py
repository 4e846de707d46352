"""NumPy restatement of the group means -- the contract of fc_ensemble_group_means (include/fc_hip.h; DESIGN.md section
30) turn for turn, on the oracle's rotation (``oracle.cpu_ref.get_alignment_matrix``) over the selected, centred atoms.
Plain ``np.sum`` stands for the contract's summation order: the comparison tolerance covers the difference.  Test
infrastructure: the product never imports it.

It records what a test needs to show that rounding cannot flip a decision: per group the per-turn changes ``c`` of the
mean (the stop ``c <= tol``) and the gap between the two smallest ``d_n`` (the choice of ``closest``).  It also holds the
case builder of the tests."""

from collections import namedtuple

import numpy as np

from oracle import cpu_ref as o

RefGroupMeans = namedtuple("RefGroupMeans", ["means", "rmsf", "distances", "closest", "sizes", "n_iter", "rotations",
                                             "changes", "closest_gap"])


def prepared(X, atoms=None, heavy_atoms_only=True):
    """(N, A_sel, 3): the atom selection applied, every conformer centred on its selected atoms"""
    X = np.asarray(X, dtype=np.float64)
    if atoms is not None and heavy_atoms_only:
        X = X[:, np.asarray(atoms) != "H"]
    return X - X.mean(axis=1, keepdims=True)


def svd_rotation(p, q):
    """A second solver: the rotation that takes q onto p from the SVD of q^T p with the determinant fix on the smallest
    singular direction (Kabsch 1978 as it is usually written, the transpose of the oracle's arrangement)"""
    H = np.asarray(q).T @ np.asarray(p)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    return Vt.T @ D @ U.T


def _rotated(M, members, rotation):
    R = np.stack([rotation(M, x) for x in members])
    return R, np.einsum("nij,naj->nai", R, members)


def group_means(Xp, labels=None, n_groups=None, refs=None, max_iter=50, tol=1e-9, rotation=o.get_alignment_matrix):
    """The contract on prepared coordinates (``prepared``)."""
    Xp = np.asarray(Xp, dtype=np.float64)
    N, A = Xp.shape[0], Xp.shape[1]
    labels = np.zeros(N, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if n_groups is None:
        n_groups = max(int(labels.max(initial=-1)) + 1, 1)
    means, rmsf = np.full((n_groups, A, 3), np.nan), np.full((n_groups, A), np.nan)
    dist, rot = np.full(N, np.nan), np.tile(np.eye(3), (N, 1, 1))
    closest, sizes = np.full(n_groups, -1, dtype=np.int64), np.zeros(n_groups, dtype=np.int64)
    n_iter = np.zeros(n_groups, dtype=np.int64)
    changes, gaps = [[] for _ in range(n_groups)], np.full(n_groups, np.inf)
    for g in range(n_groups):
        mem = np.flatnonzero(labels == g)  # ascending index
        sizes[g] = len(mem)
        if len(mem) == 0:
            continue
        ref = int(mem[0]) if refs is None else int(refs[g])
        assert labels[ref] == g
        M = Xp[ref].copy()
        if len(mem) == 1:  # mean = itself, rmsf = 0, d = 0, n_iter = 0
            means[g], rmsf[g], dist[mem[0]], closest[g] = M, 0.0, 0.0, mem[0]
            continue
        for t in range(max_iter):
            _, Y = _rotated(M, Xp[mem], rotation)
            M_new = Y.sum(axis=0) / len(mem)
            c = float(np.sqrt(((M_new - M) ** 2).sum() / A))
            changes[g].append(c)
            M, n_iter[g] = M_new, t + 1
            if c <= tol:
                break
        R, Y = _rotated(M, Xp[mem], rotation)
        sq = ((Y - M) ** 2).sum(axis=2)  # (members, A)
        d = np.sqrt(sq.sum(axis=1) / A)
        means[g], rmsf[g] = M, np.sqrt(sq.sum(axis=0) / len(mem))
        dist[mem], rot[mem] = d, R
        closest[g] = mem[int(np.argmin(d))]  # the first of equal minima: the lowest index
        srt = np.sort(d)
        gaps[g] = srt[1] - srt[0]
    return RefGroupMeans(means, rmsf, dist, closest, sizes, n_iter, rot, changes, gaps)


def aligned_block(X, atoms, rotations, heavy_atoms_only=True):
    """every conformer of the whole block moved rigidly by its rotation about the centroid of its selected atoms"""
    X = np.asarray(X, dtype=np.float64)
    sel = (np.asarray(atoms) != "H") if heavy_atoms_only else np.ones(X.shape[1], dtype=bool)
    c = X[:, sel].mean(axis=1, keepdims=True)
    return np.einsum("nij,naj->nai", rotations, X - c)


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def build_case(sizes, a_sel, n_h=0, n_unlabelled=0, sigma=0.3, seed=0, spread=2.0, empty_ids=()):
    """Clouds: group k has ``sizes[k]`` members = one random structure (atoms N(0, spread^2)) + N(0, sigma^2) per atom,
    every member under a random proper rotation and a translation N(0, 5^2); ``n_h`` hydrogens behind the ``a_sel``
    selected atoms; ``n_unlabelled`` more conformers labelled -1; the conformers shuffled, so that the labels come
    unsorted and interleaved; ``empty_ids``: group ids left without members (the other groups keep their order).
    ``sigma`` may be one value or one per group.  Returns (X (N, a_sel + n_h, 3), atoms, labels int64)."""
    rng = np.random.default_rng(seed)
    A = a_sel + n_h
    ids = [g for g in range(len(sizes) + len(empty_ids)) if g not in set(empty_ids)]
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(sizes),))
    X, lab = [], []
    for k, size in enumerate(sizes):
        centre = rng.normal(scale=spread, size=(A, 3))
        for _ in range(size):
            x = centre + rng.normal(scale=sig[k], size=(A, 3))
            X.append(x @ _random_rotation(rng).T + rng.normal(scale=5.0, size=3))
            lab.append(ids[k])
    for _ in range(n_unlabelled):
        X.append(rng.normal(scale=spread, size=(A, 3)) + rng.normal(scale=5.0, size=3))
        lab.append(-1)
    order = rng.permutation(len(X))
    atoms = np.array(["C"] * a_sel + ["H"] * n_h)
    return np.asarray(X)[order], atoms, np.asarray(lab, dtype=np.int64)[order]
