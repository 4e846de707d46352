"""NumPy restatement of the symmetry-aware RMSD prune (include/fc_hip.h, "symmetry-aware forms"),
built from ``oracle.cpu_ref`` without touching it.

For the prepared ensemble X (atom selection applied, every conformer centred on the centroid of its selected atoms) and a
(K, A_sel) table ``perms`` of permutations of the selected atoms (identity first, closed under inverse), for i < j:

    (r_k, m_k) = rmsd_and_max(X[i], X[j][perms[k]])            k = 0 .. K-1
    similar_sym(i, j) = any_k (r_k < max_rmsd and m_k < max_dev)

and the prune is the oracle's greedy k-ladder with that predicate; the clusters are the components of that graph."""

import itertools
from collections import namedtuple

import numpy as np

from enant_ref import pack_bits, prepared  # noqa: F401  (the same prepared ensemble, the same bit layout)
from oracle import cpu_ref as o

SymmMatrices = namedtuple("SymmMatrices", ["S", "S_default", "R", "M", "min_gap"])


def selected(table, atom_mask):
    """a table over all atoms -> selected-atom indices (the selection must be mapped onto itself)"""
    table = np.asarray(table, dtype=np.int64)
    mask = np.asarray(atom_mask, dtype=bool)
    sel = np.flatnonzero(mask)
    assert mask[table[:, sel]].all()
    pos = np.full(table.shape[1], -1)
    pos[sel] = np.arange(len(sel))
    return pos[table[:, sel]]


def similar_sym(p, q, perms, max_rmsd, max_dev):
    """the predicate on one ordered pair of prepared structures: the OR of K complete tests"""
    q = np.asarray(q)
    for perm in perms:
        r, m = o.rmsd_and_max(p, q[perm])
        if r < max_rmsd and m < max_dev:
            return True
    return False


def pair_values(X, perms, block=200000):
    """(r, m), each (K, P): the values of all pairs i < j, flat, in ``np.triu_indices(n, 1)`` order, for every k"""
    n = len(X)
    iu, ju = np.triu_indices(n, 1)
    perms = np.asarray(perms)
    r, m = np.zeros((len(perms), len(iu))), np.zeros((len(perms), len(iu)))
    for k, perm in enumerate(perms):
        for s in range(0, len(iu), block):
            sl = slice(s, s + block)
            r[k, sl], m[k, sl] = o.rmsd_and_max_batch(X[iu[sl]], X[ju[sl]][:, perm])
    return iu, ju, r, m


def _gap(r, m, max_rmsd, max_dev):
    """distance of the decisive values from their thresholds: r always, m where r passes"""
    g = np.abs(r - max_rmsd)
    return np.where(r < max_rmsd, np.minimum(g, np.abs(m - max_dev)), g)


def similarity(structures, atoms, perms, max_rmsd, max_dev=None, heavy_atoms_only=True):
    """All-pairs matrices of the predicate.  ``perms``: (K, A_sel) in selected-atom indices.  S (symmetric, False
    diagonal), S_default (k = 0 alone), R and M (K, n, n) with the values of (i, j), i < j, in the upper triangle, and
    ``min_gap`` = the smallest distance of any decisive value (every r_k, and m_k where its r_k passes) from its
    threshold, over all pairs and all k (inf without pairs)."""
    if max_dev is None:
        max_dev = o.CONVENTIONS["maxdev_factor"] * max_rmsd
    X = prepared(structures, atoms, heavy_atoms_only)
    n = len(X)
    perms = np.asarray(perms)
    assert perms.ndim == 2 and perms.shape[1] == X.shape[1] and np.array_equal(perms[0], np.arange(X.shape[1]))
    iu, ju, r, m = pair_values(X, perms)
    R, M = np.zeros((len(perms), n, n)), np.zeros((len(perms), n, n))
    R[:, iu, ju], M[:, iu, ju] = r, m
    passes = (r < max_rmsd) & (m < max_dev)
    S, S0 = np.zeros((n, n), dtype=bool), np.zeros((n, n), dtype=bool)
    S[iu, ju] = passes.any(axis=0)
    S0[iu, ju] = passes[0]
    gaps = _gap(r, m, max_rmsd, max_dev)
    return SymmMatrices(S | S.T, S0 | S0.T, R, M, float(gaps.min()) if gaps.size else float("inf"))


def prune_by_rmsd_sym(structures, atoms, perms, max_rmsd=None, max_dev=None, energies=None, max_dE=0.0, min_per_group=20,
                      drop=None, heavy_atoms_only=True, from_matrix=True):
    """``o.prune_by_rmsd`` with ``similar_sym`` as the predicate -> (structures[mask], mask, SymmMatrices or None).
    ``from_matrix``: all pairs up front and ``o.greedy_prune_from_matrix``; otherwise ``o.greedy_prune`` pair by pair."""
    cv = o.CONVENTIONS
    max_rmsd = cv["default_max_rmsd"] if max_rmsd is None else max_rmsd
    max_dev = cv["maxdev_factor"] * max_rmsd if max_dev is None else max_dev
    drop = cv["drop"] if drop is None else drop
    structures = np.asarray(structures, dtype=np.float64)
    if from_matrix:
        mats = similarity(structures, atoms, perms, max_rmsd, max_dev, heavy_atoms_only)
        mask = o.greedy_prune_from_matrix(mats.S, energies=energies, max_dE=max_dE, min_per_group=min_per_group, drop=drop)
        return structures[mask], mask, mats
    X = prepared(structures, atoms, heavy_atoms_only)
    mask = o.greedy_prune(len(X), lambda a, b: similar_sym(X[a], X[b], perms, max_rmsd, max_dev),
                          energies=energies, max_dE=max_dE, min_per_group=min_per_group, drop=drop)
    return structures[mask], mask, None


def components(S):
    """labels of the connected components of S, numbered by ascending smallest member -> (labels, reps, sizes)"""
    n = S.shape[0]
    labels = np.full(n, -1, dtype=np.int32)
    reps = []
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = len(reps)
        stack = [s]
        while stack:
            v = stack.pop()
            for w in np.flatnonzero(S[v] & (labels < 0)):
                labels[w] = len(reps)
                stack.append(int(w))
        reps.append(s)
    return labels, np.array(reps, dtype=np.int64), np.bincount(labels, minlength=len(reps)).astype(np.int64)


def brute_force_automorphisms(n, edges, colours):
    """every colour-preserving permutation of 0..n-1 that maps the edge set onto itself, sorted, identity first"""
    es = {frozenset(e) for e in edges}
    out = []
    for perm in itertools.permutations(range(n)):
        if all(colours[a] == colours[perm[a]] for a in range(n)) and \
                {frozenset((perm[a], perm[b])) for a, b in es} == es:
            out.append(perm)
    out.sort(key=lambda p: (p != tuple(range(n)), p))
    return np.array(out, dtype=np.int64)


# ---- tables and ensembles of the tests -----------------------------------------------------------------------------------
def path_table(A):
    """a path of A atoms: the identity and the reversal"""
    return np.stack([np.arange(A), np.arange(A)[::-1]])


def block_table(A, size, first=0, blocks=3):
    """``blocks`` runs of ``size`` atoms from atom ``first`` on, permuted as wholes (blocks! rows); every other atom fixed"""
    rows = []
    for order in itertools.permutations(range(blocks)):
        row = np.arange(A)
        for m, src in enumerate(order):
            row[first + m * size:first + (m + 1) * size] = np.arange(first + src * size, first + (src + 1) * size)
        rows.append(row)
    return np.array(rows)


def star_table(arms=3, length=4):
    """``arms`` chains of ``length`` atoms on a centre (atom 0; arm m holds atoms 1 + m length ...): arms! permutations"""
    return block_table(1 + arms * length, length, first=1, blocks=arms)


def transposition_table(A, n_swaps):
    """the group generated by ``n_swaps`` disjoint transpositions (a, a + 1): 2^n_swaps involutions that commute"""
    rows = []
    for bits in itertools.product((0, 1), repeat=n_swaps):
        row = np.arange(A)
        for s, on in enumerate(bits):
            if on:
                row[2 * s], row[2 * s + 1] = 2 * s + 1, 2 * s
        rows.append(row)
    return np.array(rows)


def relabel_half(X, table, seed):
    """a copy of X with a random half of the conformers relabelled by a random non-identity row of ``table`` -> (Y, which)"""
    rng = np.random.default_rng(seed)
    Y = np.array(X, dtype=np.float64)
    which = rng.random(len(X)) < 0.5
    if len(table) > 1:
        for n in np.flatnonzero(which):
            Y[n] = Y[n][table[rng.integers(1, len(table))]]
    return Y, which


def two_arm_families(n_each, L, delta, seed, noise=0.01, outlier=1.2):
    """Two families of conformers of a molecule of 2 L + 1 atoms whose arms (atoms 1..L and L+1..2L) are related by a
    twofold axis up to a displacement of ``delta`` per atom of the second arm -- ``outlier`` for its first atom.  Family
    U is that structure; family V is U with atoms 1 and L + 1 moved so that V, relabelled by the swap of the arms and
    turned about the axis, meets U there: under the identity U - V differ by ``outlier`` at two atoms and nowhere else,
    under the swap by ``delta`` everywhere else.  -> (X (2 n_each, A, 3), atoms, table (2, A), family (2 n_each,))"""
    rng = np.random.default_rng(seed)
    A = 2 * L + 1
    Rz = np.diag([-1.0, -1.0, 1.0])
    arm = rng.normal(scale=2.0, size=(L, 3))
    d = rng.normal(size=(L, 3))
    d *= delta / np.linalg.norm(d, axis=1, keepdims=True)
    d[0] *= outlier / delta
    U = np.concatenate([np.zeros((1, 3)), arm, arm @ Rz.T + d])
    V = U.copy()
    V[L + 1] = U[L + 1] - d[0]
    V[1] = U[1] + Rz @ d[0]
    family = np.arange(2 * n_each) % 2
    rng.shuffle(family)
    X = np.where(family[:, None, None] == 0, U[None], V[None]) + rng.normal(scale=noise, size=(2 * n_each, A, 3))
    X = np.stack([x @ _rotation(rng).T for x in X]) + rng.normal(scale=3.0, size=(2 * n_each, 1, 3))
    table = np.stack([np.arange(A), np.concatenate([[0], np.arange(L + 1, 2 * L + 1), np.arange(1, L + 1)])])
    return np.ascontiguousarray(X), np.array(["C"] * A), table, family


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q
