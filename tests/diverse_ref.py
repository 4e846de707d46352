"""NumPy restatement of the RMSD-diverse selection (greedy max-min, Gonzalez k-center) -- the contract of
fc_ensemble_select_diverse (include/fc_hip.h) line by line, on the oracle's Kabsch RMSD over the selected, centred
atoms.  Test infrastructure: the product never imports it.

While it runs it records the smallest gap of every decision the contract makes -- each argmax (the chosen value
against the next one), each ``t < D[j]`` comparison and each radius-stop comparison -- so that a test can show that
its ensemble has no near-tie where a correct device result may differ from this one by rounding."""

from dataclasses import dataclass, field

import numpy as np

from oracle import cpu_ref as o


def prepared(X, atoms=None, heavy_atoms_only=True):
    """(N, A_sel, 3) coordinates of the atom selection prune_by_rmsd uses: heavy atoms (or all)."""
    X = np.asarray(X, dtype=np.float64)
    if atoms is None or not heavy_atoms_only:
        return X
    return X[:, np.asarray(atoms) != "H"]


def rmsd_row(Xsel, s):
    """d(s, j) for every j: rmsd_and_max(X[s], X[j], center=True)[0], through the oracle's stacked form."""
    P = np.broadcast_to(Xsel[s], Xsel.shape)
    return o.rmsd_and_max_batch(P, Xsel, center=True)[0]


@dataclass
class Record:
    rows: dict = field(default_factory=dict)  # k -> d(s_k, .) (N,)
    argmax_gap: float = np.inf                # smallest (chosen max - next value) over every argmax
    update_gap: float = np.inf                # smallest |t - D[j]| over every t < D[j] decision
    stop_gap: float = np.inf                  # smallest |m - stop_rmsd| over every radius-stop decision

    @property
    def min_gap(self):
        return min(self.argmax_gap, self.update_gap, self.stop_gap)


def select_diverse(Xsel, n_max, start=0, stop_rmsd=None, row=rmsd_row):
    """The contract on prepared coordinates (``prepared``).  Returns (indices, labels, distances, radii, Record)."""
    N = Xsel.shape[0]
    rec = Record()
    if N == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0), rec
    selected = np.zeros(N, dtype=bool)
    r = row(Xsel, start)
    rec.rows[0] = r
    D = r.copy()
    D[start] = 0.0
    L = np.zeros(N, dtype=np.int32)
    selected[start] = True
    indices, radii = [start], [np.inf]
    for k in range(1, min(int(n_max), N)):
        cand = np.flatnonzero(~selected)
        vals = D[cand]
        m = vals.max()
        s = int(cand[np.flatnonzero(vals == m)[0]])  # ties -> lowest index
        others = vals[cand != s]
        if others.size:
            rec.argmax_gap = min(rec.argmax_gap, float(m - others.max()) if others.max() < m else 0.0)
        if stop_rmsd is not None:
            rec.stop_gap = min(rec.stop_gap, abs(float(m) - float(stop_rmsd)))
            if m <= stop_rmsd:
                break
        radii.append(float(m))
        indices.append(s)
        selected[s] = True
        D[s] = 0.0
        L[s] = k
        t = row(Xsel, s)
        rec.rows[k] = t
        live = ~selected
        if live.any():
            rec.update_gap = min(rec.update_gap, float(np.abs(t[live] - D[live]).min()))
        upd = live & (t < D)
        D[upd] = t[upd]
        L[upd] = k
    return np.array(indices, dtype=np.int64), L, D, np.array(radii), rec


def replay(rows_by_pick, start_row_index, N, K, stop_rmsd=None):
    """The greedy loop again on given rows: ``rows_by_pick[k]`` = d(s_k, .) for the k-th pick of a selection
    (``start_row_index`` = s_0).  The picks must come out as the rows were given; returns (indices, labels, D)."""
    selected = np.zeros(N, dtype=bool)
    D = np.array(rows_by_pick[0], dtype=np.float64).copy()
    D[start_row_index] = 0.0
    selected[start_row_index] = True
    L = np.zeros(N, dtype=np.int32)
    indices = [start_row_index]
    for k in range(1, K):
        cand = np.flatnonzero(~selected)
        vals = D[cand]
        m = vals.max()
        s = int(cand[np.flatnonzero(vals == m)[0]])
        if stop_rmsd is not None and m <= stop_rmsd:
            break
        indices.append(s)
        selected[s] = True
        D[s] = 0.0
        L[s] = k
        t = rows_by_pick[k]
        upd = ~selected & (t < D)
        D[upd] = t[upd]
        L[upd] = k
    return np.array(indices, dtype=np.int64), L, D


def brute_force_k_center(dist, k):
    """Optimal k-center radius of a small symmetric distance matrix (every subset of size k)."""
    from itertools import combinations

    N = dist.shape[0]
    best = np.inf
    for S in combinations(range(N), min(k, N)):
        best = min(best, float(dist[list(S)].min(axis=0).max()))
    return best
