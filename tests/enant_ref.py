"""NumPy restatement of the enantiomer-aware RMSD prune (include/fc_hip.h, "enantiomer-aware forms"; DESIGN.md section
12), built from ``oracle.cpu_ref`` without touching it.

For the prepared ensemble X (atom selection applied, every conformer centred on the centroid of its selected atoms):

    (r+, m+) = rmsd_and_max(X[i],  X[j])        best proper rotation
    (r-, m-) = rmsd_and_max(X[i], -X[j])        partner inverted through the origin: its mirror image
    similar_enant(i, j) = (r+ < max_rmsd and m+ < max_dev) or (r- < max_rmsd and m- < max_dev)

and the prune is the oracle's greedy k-ladder with that predicate."""

from collections import namedtuple

import numpy as np

from oracle import cpu_ref as o

EnantMatrices = namedtuple("EnantMatrices", ["S", "S_default", "Rp", "Mp", "Rm", "Mm", "min_gap"])


def prepared(structures, atoms, heavy_atoms_only=True):
    """the ensemble as the RMSD stage sees it: selected atoms, centred on their centroid"""
    X = np.asarray(structures, dtype=np.float64)
    hv = o.heavy_mask(atoms) if heavy_atoms_only else np.ones(X.shape[1], dtype=bool)
    X = X[:, hv, :]
    return X - X.mean(axis=1, keepdims=True)


def similar_enant(p, q, max_rmsd, max_dev):
    """the predicate on one pair of prepared structures"""
    rp, mp = o.rmsd_and_max(p, q)
    rm, mm = o.rmsd_and_max(p, -np.asarray(q))
    return bool((rp < max_rmsd and mp < max_dev) or (rm < max_rmsd and mm < max_dev))


def pair_values(X, block=200000):
    """(r+, m+, r-, m-) of all pairs i < j of the prepared ensemble, flat, in ``np.triu_indices(n, 1)`` order (in
    blocks, as ``o.rmsd_similarity_matrix`` does it)"""
    n = len(X)
    iu, ju = np.triu_indices(n, 1)
    out = [np.zeros(len(iu)) for _ in range(4)]
    for s in range(0, len(iu), block):
        sl = slice(s, s + block)
        out[0][sl], out[1][sl] = o.rmsd_and_max_batch(X[iu[sl]], X[ju[sl]])
        out[2][sl], out[3][sl] = o.rmsd_and_max_batch(X[iu[sl]], -X[ju[sl]])
    return iu, ju, out


def _gap(r, m, max_rmsd, max_dev):
    """distance of the decisive values from their thresholds: r always, m where r passes"""
    g = np.abs(r - max_rmsd)
    return np.where(r < max_rmsd, np.minimum(g, np.abs(m - max_dev)), g)


def similarity(structures, atoms, max_rmsd, max_dev=None, heavy_atoms_only=True):
    """All-pairs matrices of the predicate: S (enantiomer-aware, symmetric, False diagonal), S_default (the proper
    handedness alone), the four value matrices, and ``min_gap`` = the smallest distance of any decisive value (r+, r-,
    and m+/- where its r+/- passes) from its threshold, over all pairs (inf without pairs)."""
    if max_dev is None:
        max_dev = o.CONVENTIONS["maxdev_factor"] * max_rmsd
    X = prepared(structures, atoms, heavy_atoms_only)
    n = len(X)
    iu, ju, (rp, mp, rm, mm) = pair_values(X)
    mats = []
    for v in (rp, mp, rm, mm):
        M = np.zeros((n, n))
        M[iu, ju] = v
        mats.append(M + M.T)
    sp = (rp < max_rmsd) & (mp < max_dev)
    sm = (rm < max_rmsd) & (mm < max_dev)
    S, S0 = np.zeros((n, n), dtype=bool), np.zeros((n, n), dtype=bool)
    S[iu, ju] = sp | sm
    S0[iu, ju] = sp
    gaps = np.minimum(_gap(rp, mp, max_rmsd, max_dev), _gap(rm, mm, max_rmsd, max_dev))
    return EnantMatrices(S | S.T, S0 | S0.T, *mats, float(gaps.min()) if len(gaps) else float("inf"))


def prune_by_rmsd_enant(structures, atoms, max_rmsd=None, max_dev=None, energies=None, max_dE=0.0, min_per_group=20,
                        drop=None, heavy_atoms_only=True, from_matrix=True):
    """``o.prune_by_rmsd`` with ``similar_enant`` as the predicate -> (structures[mask], mask, EnantMatrices or None).
    ``from_matrix``: all pairs up front and ``o.greedy_prune_from_matrix``; otherwise ``o.greedy_prune`` pair by pair."""
    cv = o.CONVENTIONS
    max_rmsd = cv["default_max_rmsd"] if max_rmsd is None else max_rmsd
    max_dev = cv["maxdev_factor"] * max_rmsd if max_dev is None else max_dev
    drop = cv["drop"] if drop is None else drop
    structures = np.asarray(structures, dtype=np.float64)
    if from_matrix:
        mats = similarity(structures, atoms, max_rmsd, max_dev, heavy_atoms_only)
        mask = o.greedy_prune_from_matrix(mats.S, energies=energies, max_dE=max_dE, min_per_group=min_per_group, drop=drop)
        return structures[mask], mask, mats
    X = prepared(structures, atoms, heavy_atoms_only)
    mask = o.greedy_prune(len(X), lambda a, b: similar_enant(X[a], X[b], max_rmsd, max_dev), energies=energies,
                          max_dE=max_dE, min_per_group=min_per_group, drop=drop)
    return structures[mask], mask, None


def pack_bits(S, energies=None, max_dE=0.0):
    """the upper triangle of a similarity matrix as the device's bit matrix: (n, ceil(n / 64)) uint64, bit j of row i
    set iff j > i and S[i, j] [and |E_i - E_j| < max_dE]"""
    n = S.shape[0]
    U = np.triu(S, 1)
    if energies is not None:
        e = np.asarray(energies, dtype=np.float64)
        U = U & (np.abs(e[:, None] - e[None, :]) < max_dE)
    W = (max(n, 1) + 63) // 64
    padded = np.zeros((n, W * 64), dtype=bool)
    padded[:, :n] = U
    return np.packbits(padded.reshape(n, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, W)


def reflect(X, flip, axis=0):
    """a copy of X with the conformers ``flip`` mirrored in the plane perpendicular to ``axis``"""
    Y = np.array(X, dtype=np.float64)
    Y[np.asarray(flip), :, axis] *= -1.0
    return Y
