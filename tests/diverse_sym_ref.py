"""NumPy restatement of the symmetry- and mirror-aware distance of the RMSD-diverse selection
(fc_ensemble_select_diverse_perm, include/fc_hip.h) as a ``row=`` function for
``diverse_ref.select_diverse``, built from ``oracle.cpu_ref`` without touching it.  Test infrastructure: the product never
imports it.

For the prepared ensemble X (atom selection applied, every conformer centred on the centroid of its selected atoms) and a
(K, A_sel) table ``perms`` (identity first, closed under inverse):

    d_sym(i, j) = min over k < K, h in H of rmsd_and_max(X[i], h * X[j][perms[k]])[0]
    H = {+1}, or {+1, -1} with ``mirror`` (-1: the partner inverted through the origin)"""

import numpy as np

import enant_ref as er
import symm_ref as sr
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o


def centred(Xsel):
    X = np.asarray(Xsel, dtype=np.float64)
    return X - X.mean(axis=1, keepdims=True)


def sym_row(perms, mirror=False):
    """-> row(Xsel, s) = d_sym(s, j) for every j"""
    perms = np.asarray(perms)

    def row(Xsel, s):
        X = centred(Xsel)
        P = np.broadcast_to(X[s], X.shape)
        best = np.full(len(X), np.inf)
        for perm in perms:
            for h in ((1.0, -1.0) if mirror else (1.0,)):
                best = np.minimum(best, o.rmsd_and_max_batch(P, h * X[:, perm])[0])
        return best

    return row


def matrix(Xsel, perms, mirror=False):
    """d_sym of every ordered pair, (N, N)"""
    row = sym_row(perms, mirror)
    return np.stack([row(Xsel, s) for s in range(len(Xsel))])


# ---- tables and ensembles of the tests -----------------------------------------------------------------------------------
def table(kind, A):
    if kind == "identity":
        return np.arange(A)[None]
    if kind == "path":
        return sr.path_table(A)
    if kind == "blocks":  # three runs of (A - 1) // 3 atoms behind atom 0 (A = 3: the three atoms themselves), K = 6
        return sr.block_table(A, 1, first=0) if A == 3 else sr.block_table(A, (A - 1) // 3, first=1)
    if kind == "swaps64":
        return sr.transposition_table(A, 6)
    raise ValueError(kind)


def ensemble(kind, N, A, table_kind, mirror, seed=3):
    """``synthetic_ensemble`` (clusters of 5) or ``continuous_ensemble``, a random half relabelled by a random non-identity
    row of the table, and -- ``mirror`` -- a random half reflected -> (X, atoms, table, cluster ids or None)"""
    if kind == "clusters":
        X, atoms, cid = syn.synthetic_ensemble(N, A, seed=seed)
    else:
        X, atoms, cid = syn.continuous_ensemble(N, A, seed=seed), np.array(["C"] * A), None
    t = table(table_kind, A)
    Y, _ = sr.relabel_half(X, t, seed)
    if mirror:
        Y = er.reflect(Y, np.random.default_rng(seed + 100).random(len(Y)) < 0.5)
    return np.ascontiguousarray(Y), atoms, t, cid
