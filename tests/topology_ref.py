"""NumPy restatement of the bond-topology contract (include/fc_hip.h, fc_bond_changes) -- test
infrastructure, never imported by the product.

    bonded(X, i, j)  = fl(sqrt(((dx*dx) + dy*dy) + dz*dz)) < fl(1.2 * fl(r_i + r_j))      i < j, graphize's rule
    delta(n)         = { i < j : bonded(X[n], i, j) != (i, j) in B_ref(n) }  minus pairs touching excluded(n)
    count(n)         = |delta(n)|,  ok(n) = count(n) <= max_newbonds

Distances are taken with the square root and compared with the distance threshold itself, literally as cdist and
graphize do -- not with the squared thresholds of the kernel.  Work is chunked (structures x rows) so that 10^5
structures or 8 192 atoms fit in memory.
"""

import numpy as np

from firecode_amd.torsion_perception import RADII_TABLE

_CHUNK = 1 << 21  # distances per block


def thresholds(atoms):
    radii = np.array([RADII_TABLE.get(str(a), 1.5) for a in np.asarray(atoms).reshape(-1)], dtype=np.float64)
    return 1.2 * (radii[:, None] + radii[None, :])


def _blocks(N, A):
    """(structure slice, row slice) blocks of at most ~_CHUNK distances, structure-major then row-major."""
    rows = max(1, min(A, _CHUNK // max(A, 1)))
    per = max(1, _CHUNK // max(A * A, 1)) if rows == A else 1
    for n0 in range(0, N, per):
        for r0 in range(0, A, rows):
            yield slice(n0, min(N, n0 + per)), slice(r0, min(A, r0 + rows))


def _dist(X, rs):
    """cdist(X[n][rs], X[n]) for a block of structures, in cdist's order of operations."""
    d = X[:, rs, None, :] - X[:, None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def ref_bits_from_edges(edges, A):
    """(A, A) bool, symmetric, from (i, j) pairs (self-loops dropped)."""
    B = np.zeros((A, A), dtype=bool)
    for i, j in edges:
        if i != j:
            B[i, j] = B[j, i] = True
    return B


def graphs_reference(graphs):
    """scramble_check's reference bond set: edges of each graph shifted by the node count of the graphs before it."""
    edges, pos = [], 0
    for g in graphs:
        edges += [(a + pos, b + pos) for a, b in g.edges if a != b]
        pos += len(g.nodes)
    return edges, pos


def exclusion_mask(excluded, A):
    m = np.zeros(A, dtype=bool)
    for a in np.asarray(list(excluded), dtype=np.int64).reshape(-1):
        if 0 <= a < A:
            m[a] = True
    return m


def _changed(now, was, ex, rs, upper):
    """the contract's delta on a block: bonded now != bonded in the reference, i < j, neither atom excluded"""
    return (now != was) & ~(ex[:, rs, None] | ex[:, None, :]) & upper[rs]


def delta_from_edges(now_edges, ref_edges, A, excluded=None):
    """The same delta on given bond sets (the golden cases hold graphs, not coordinates) -> set of (i, j)."""
    now = ref_bits_from_edges(now_edges, A)[None]
    was = ref_bits_from_edges(ref_edges, A)[None]
    ex = (np.zeros(A, dtype=bool) if excluded is None else exclusion_mask(excluded, A))[None]
    upper = np.triu(np.ones((A, A), dtype=bool), 1)
    ii, jj = np.nonzero(_changed(now, was, ex, slice(0, A), upper)[0])
    return {(int(i), int(j)) for i, j in zip(ii, jj)}


def bond_changes(atoms, X, ref_X=None, ref_bonds=None, excluded=None, max_newbonds=0, return_bonds=False):
    """X (N, A, 3).  Reference: ref_X ((A, 3) shared or (N, A, 3)) or ref_bonds ((A, A) bool).  excluded: None,
    one collection, or a list of N collections.  -> (ok (N,), count (N,)[, (offsets (N+1,), bonds (E, 3))])."""
    X = np.asarray(X, dtype=np.float64)
    N, A = X.shape[0], X.shape[1]
    thr = thresholds(atoms)
    if ref_X is not None:
        ref_X = np.asarray(ref_X, dtype=np.float64)
        ref_X = ref_X[None] if ref_X.ndim == 2 else ref_X
    if excluded is None:
        ex = np.zeros((1, A), dtype=bool)
    elif len(excluded) == N and N > 0 and all(np.ndim(e) > 0 or isinstance(e, (set, frozenset)) for e in excluded):
        ex = np.array([exclusion_mask(e, A) for e in excluded]).reshape(N, A)
    else:
        ex = exclusion_mask(excluded, A)[None]
    upper = np.triu(np.ones((A, A), dtype=bool), 1)
    counts = np.zeros(N, dtype=np.int64)
    parts = [[] for _ in range(N)] if return_bonds else None
    for ns, rs in _blocks(N, A):
        now = _dist(X[ns], rs) < thr[rs]
        if ref_X is not None:
            R = ref_X if ref_X.shape[0] == 1 else ref_X[ns]
            was = _dist(R, rs) < thr[rs]
        else:
            was = np.broadcast_to(ref_bonds[rs], now.shape)
        changed = _changed(now, was, ex if ex.shape[0] == 1 else ex[ns], rs, upper)
        counts[ns] += changed.reshape(changed.shape[0], -1).sum(axis=1)
        if return_bonds:
            for k, n in enumerate(range(*ns.indices(N))):
                ii, jj = np.nonzero(changed[k])
                if ii.size:
                    parts[n].append(np.stack([ii + rs.start, jj, np.where(now[k][ii, jj], 1, -1)], axis=1))
    ok = counts <= max_newbonds
    if not return_bonds:
        return ok, counts
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    bonds = np.concatenate([b for p in parts for b in p]) if offsets[-1] else np.zeros((0, 3))
    return ok, counts, (offsets, bonds.astype(np.int64).reshape(-1, 3))
