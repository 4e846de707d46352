"""Drop-in for the geometry half of ``firecode.utils`` and for
``prism_pruner.utils.{align_structures, rotate_dihedral}``."""

import numpy as np

from firecode_amd import _lib as L
from firecode_amd.algebra import count_clashes_batch
from firecode_amd.rmsd import rmsd_and_max_batch


def cartesian_rows_at(arrays, rows):
    """Rows ``rows`` of ``cartesian_product(*arrays)`` without building the product: the mixed-radix digits of a row
    number in the reference's order (firecode/utils.py:219-221: array #2 slowest, then #1, then #3 ... #n)."""
    flat = [np.asarray(a).reshape(-1) for a in arrays]
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    T = len(flat)
    out = np.empty((len(rows), T), dtype=np.result_type(*flat) if flat else np.float64)
    order = ([1, 0] + list(range(2, T))) if T >= 2 else list(range(T))  # slowest first
    rem = rows.copy()
    for t in reversed(order):
        out[:, t] = flat[t][rem % len(flat[t])]
        rem //= len(flat[t])
    return out


def cartesian_product(*arrays):
    """firecode/utils.py:219-221: ``np.stack(np.meshgrid(*arrays), -1).reshape(-1, len(arrays))`` -- array #2
    varies slowest, then #1, then #3..#n.  Integer and floating inputs are written row by row by the library
    (fc_cartesian_product_*, host threads: the NumPy expression takes ~1 s for the 1 679 616 x 8 angle grid of a
    conformational search); anything else (no arrays, strings, objects, complex) takes the reference's expression."""
    arrays_converted = [np.asarray(arr) for arr in arrays]
    if arrays_converted:
        try:
            common = np.result_type(*arrays_converted)
        except TypeError:
            common = None
        if common is not None and (common.kind in "iub" or common.kind == "f") and common.itemsize <= 8 and common != np.uint64:
            flat = [a.reshape(-1) for a in arrays_converted]
            counts = np.array([len(a) for a in flat], dtype=np.int64)
            rows = int(np.prod(counts, dtype=object))
            if rows < 4096:  # small grids: NumPy is as fast and the result identical
                return np.stack(np.meshgrid(*arrays_converted), -1).reshape(-1, len(arrays))
            work = np.int64 if common.kind in "iub" else np.float64
            values = np.ascontiguousarray(np.concatenate([a.astype(work) for a in flat]))
            out = np.empty((rows, len(flat)), dtype=work)
            if work is np.int64:
                L.call("fc_cartesian_product_i64", L.pi(values), L.pi(counts), len(flat), L.pi(out))
            else:
                L.call("fc_cartesian_product_f64", L.pf(values), L.pi(counts), len(flat), L.pf(out))
            return out if out.dtype == common else out.astype(common)
    return np.stack(np.meshgrid(*arrays_converted), -1).reshape(-1, len(arrays))


def align_structures(structures, indices=None):
    """prism_pruner.utils.align_structures (call sites embedder.py:1704,1910,
    2218,2300): every conformer superposed on the first."""
    X = L.f64(structures)
    if X.ndim != 3 or X.shape[2] != 3:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {X.shape}")
    out = np.empty_like(X)
    idx = None if indices is None else L.i64(indices)
    L.call("fc_align_to_first", L.pf(X), X.shape[0], X.shape[1], L.pi(idx),
           0 if idx is None else idx.shape[0], L.pf(out))
    return out


def rmsd_similarity(ref, structures, rmsd_thr=0.5):
    """firecode/utils.py:494-504: True when any structure has
    ``rmsd < rmsd_thr and maxdev < 2*rmsd_thr`` to ref (no centring)."""
    structures = L.f64(structures)
    if structures.size == 0:
        return False
    X = np.concatenate([L.f64(ref)[None], structures.reshape(-1, *np.shape(ref))])
    K = X.shape[0] - 1
    r, m = rmsd_and_max_batch(X, np.zeros(K, dtype=np.int64), np.arange(1, K + 1), center=False)
    return bool(np.any((r < rmsd_thr) & (m < 2 * rmsd_thr)))


def _adjacency(graph, n_atoms):
    """(A, A) byte adjacency from a networkx graph or an iterable of (i, j) bonds."""
    adj = np.zeros((n_atoms, n_atoms), dtype=np.uint8)
    edges = graph.edges if hasattr(graph, "edges") else graph
    for i, j in edges:
        adj[int(i), int(j)] = 1
        adj[int(j), int(i)] = 1
    return adj


def compenetration_check_batch(structures, graph=None, ids=None, thresh=1.0, max_clashes=0):
    """Per-structure ``compenetration_check`` -> bool (N,).  ``graph``: networkx
    graph or iterable of bonds, used only when ``ids`` is None (utils.py:522-542)."""
    X = L.f64(structures)
    if X.ndim != 3 or X.shape[2] != 3:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"structures must be (N, A, 3), got {X.shape}")
    if ids is None:
        ok = count_clashes_batch(X) <= max_clashes
        if graph is None:
            return ok
        counts = np.zeros(X.shape[0], dtype=np.int64)
        adj = _adjacency(graph, X.shape[1])
        L.call("fc_clash_graph", L.pf(X), X.shape[0], X.shape[1], L.pb(adj), float(thresh), L.pi(counts))
        return ok & (counts <= max_clashes)
    ids = L.i64(ids)
    if ids.shape[0] not in (2, 3):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "ids must list 2 or 3 fragment lengths")
    ok = np.zeros(X.shape[0], dtype=np.uint8)
    L.call("fc_clash_fragments", L.pf(X), X.shape[0], X.shape[1], L.pi(ids), ids.shape[0], float(thresh),
           int(max_clashes), None, L.pb(ok))
    return ok.astype(bool)


def compenetration_check(coords, graph=None, ids=None, thresh=1.0, max_clashes=0):
    """firecode/utils.py:507-575 -- all three modes on the GPU."""
    return bool(compenetration_check_batch(L.f64(coords)[None], graph=graph, ids=ids, thresh=thresh,
                                           max_clashes=max_clashes)[0])


# ---- bond-topology check: molecule_check / scramble_check (firecode/utils.py:341-400) ------------------------------
# The bond rule is graphize's (firecode_amd.torsion_perception): i < j bonded iff cdist < 1.2 * (r_i + r_j), the radii
# from its RADII_TABLE (1.5 for anything else).  Contract: include/fc_hip.h (fc_bond_changes), DESIGN.md section 11.
def _bad(msg):
    return L.FirecodeHipInputError(L.FC_E_INVALID, msg)


def _structures(X, what):
    X = L.f64(X)
    if X.ndim != 3 or X.shape[2] != 3:
        raise _bad(f"{what} must be (N, A, 3), got {X.shape}")
    return X


def _bond_classes(atoms, A):
    """atoms -> (class per atom (A,) int32, (C, C) thresholds fl(1.2 * fl(r_p + r_q)) over the distinct radii)."""
    from firecode_amd.torsion_perception import RADII_TABLE

    atoms = np.asarray(atoms).reshape(-1)
    if atoms.shape[0] != A:
        raise _bad(f"{atoms.shape[0]} atom symbols for structures of {A} atoms")
    radii = np.array([RADII_TABLE.get(str(a), 1.5) for a in atoms], dtype=np.float64)
    uniq, cls = np.unique(radii, return_inverse=True)
    return np.ascontiguousarray(cls.reshape(-1), dtype=np.int32), np.ascontiguousarray(1.2 * (uniq[:, None] + uniq[None, :]))


def _exclusions(excluded_atoms, N):
    """One integer collection, or a sequence of N of them -> (offsets (S + 1,), atoms, S) with S = 1 or N."""
    def collection(e):
        return isinstance(e, (set, frozenset, list, tuple, range)) or (isinstance(e, np.ndarray) and e.ndim > 0)

    if excluded_atoms is None:
        return None, None, 0
    items = list(excluded_atoms) if collection(excluded_atoms) else [excluded_atoms]
    nested = [collection(e) for e in items]
    if any(nested) and not all(nested):
        raise _bad("excluded_atoms mixes atom indices and per-structure collections")
    if items and all(nested):
        if len(items) != N:
            raise _bad(f"excluded_atoms holds {len(items)} collections for {N} structures")
        sets = [np.asarray(list(e)).reshape(-1) for e in items]
    else:
        sets = [np.asarray(items).reshape(-1)]
    for s in sets:
        if s.size and s.dtype.kind not in "iub":
            raise _bad(f"excluded atoms must be integers, got dtype {s.dtype}")
    lens = np.array([s.size for s in sets], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    atoms = np.ascontiguousarray(np.concatenate([s.astype(np.int64) for s in sets]) if lens.sum() else np.zeros(0, np.int64))
    return offsets, atoms, len(sets)


def _graph_bits(mols_graphs, A):
    """scramble_check's reference bond set (utils.py:371-376) as (A, ceil(A/64)) uint64 words: molecule m's edges
    (a, b), a != b, shifted by the node count of the graphs before it."""
    graphs = list(mols_graphs)
    sizes = [len(g.nodes) for g in graphs]
    if sum(sizes) != A:
        raise _bad(f"the graphs hold {sum(sizes)} nodes for structures of {A} atoms")
    edges, pos = [], 0
    for g, n in zip(graphs, sizes):
        for a, b in g.edges:
            if a != b:
                a, b = int(a) + pos, int(b) + pos
                if not (0 <= a < A and 0 <= b < A):
                    raise _bad(f"bond ({a}, {b}) of the graphs is outside the {A} atoms")
                edges.append((a, b))
        pos += n
    adj = _adjacency(edges, A)
    W = (A + 63) // 64
    packed = np.zeros((A, W * 8), dtype=np.uint8)
    packed[:, : (A + 7) // 8] = np.packbits(adj, axis=1, bitorder="little")
    return np.ascontiguousarray(packed.view("<u8"))


def _bond_changes(atoms, X, ref=None, ref_bits=None, excl=(None, None, 0), max_newbonds=0, return_bonds=False):
    N, A = X.shape[0], X.shape[1]
    if A < 1:
        raise _bad("structures need at least one atom")
    cls, thr = _bond_classes(atoms, A)
    stride = 0 if ref is None or ref.ndim == 2 else 3 * A
    eo, ea, es = excl
    args = (L.pf(X), N, A, L.ptr(cls, L.C.c_int32), thr.shape[0], L.pf(thr), L.pf(ref), stride, L.pw(ref_bits),
            L.pi(eo), L.pi(ea), es)
    counts = np.zeros(N, dtype=np.int64)
    ok = np.zeros(N, dtype=np.uint8)
    L.call("fc_bond_changes", *args, int(max_newbonds), L.pi(counts), L.pb(ok))
    if not return_bonds:
        return ok.astype(bool), counts
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    bonds = np.zeros((int(offsets[-1]), 3), dtype=np.int64)
    L.call("fc_bond_changes_list", *args, L.pi(offsets), L.pi(bonds))
    return ok.astype(bool), counts, (offsets, bonds)


def molecule_check_batch(atoms, old_structures, new_structures, max_newbonds=0, return_bonds=False):
    """``molecule_check`` (firecode/utils.py:341-353) for N structures at once: the bonds of ``new_structures[n]``
    against those of ``old_structures`` -- one (A, 3) reference for all, or (N, A, 3), one per structure.
    -> (ok (N,) bool, count (N,) int64 changed bonds[, (offsets (N+1,), bonds (E, 3) int64: i, j, +1 formed /
    -1 broken, per structure in row-major order)])."""
    X = _structures(new_structures, "new_structures")
    old = L.f64(old_structures)
    if not (old.ndim == 2 and old.shape == X.shape[1:]) and not (old.ndim == 3 and old.shape == X.shape):
        raise _bad(f"old_structures must be (A, 3) or (N, A, 3) like new_structures {X.shape}, got {old.shape}")
    return _bond_changes(atoms, X, ref=old, max_newbonds=max_newbonds, return_bonds=return_bonds)


def scramble_check_batch(atoms, structures, excluded_atoms, mols_graphs, max_newbonds=0, return_bonds=False):
    """``scramble_check`` (firecode/utils.py:356-400) for N structures at once: the bonds of each structure against
    the union of the fragment graphs (node offsets as the reference's), changed bonds touching an excluded atom not
    counted.  ``excluded_atoms``: one integer collection for all structures, or a sequence of N of them.  Returns as
    ``molecule_check_batch``."""
    X = _structures(structures, "structures")
    bits = _graph_bits(mols_graphs, X.shape[1])
    excl = _exclusions(excluded_atoms, X.shape[0])
    return _bond_changes(atoms, X, ref_bits=bits, excl=excl, max_newbonds=max_newbonds, return_bonds=return_bonds)


def molecule_check(atoms, old_coords, new_coords, max_newbonds=0):
    """firecode/utils.py:341-353 on the GPU."""
    old, new = L.f64(old_coords), L.f64(new_coords)
    if new.ndim != 2 or old.ndim != 2:
        raise _bad(f"old_coords and new_coords must be (A, 3), got {old.shape} and {new.shape}")
    ok, _ = molecule_check_batch(atoms, old, new[None], max_newbonds=max_newbonds)
    return bool(ok[0])


def scramble_check(embedded_atoms, embedded_structure, excluded_atoms, mols_graphs, max_newbonds=0,
                   logfunction=None, title=None):
    """firecode/utils.py:356-400 on the GPU, with the reference's log line on failure."""
    X = L.f64(embedded_structure)
    if X.ndim != 2:
        raise _bad(f"embedded_structure must be (A, 3), got {X.shape}")
    res = scramble_check_batch(embedded_atoms, X[None], [np.asarray(list(excluded_atoms)).reshape(-1)], mols_graphs,
                               max_newbonds=max_newbonds, return_bonds=logfunction is not None)
    if res[0][0]:
        return True
    if logfunction is not None:
        delta_bonds = {(int(i), int(j)) for i, j, _ in res[2][1]}
        logfunction(f"{title}, scramble_check - found {len(delta_bonds)} extra bonds: {delta_bonds}")
    return False


def fitness_check_batch(structures, constraints, targets, threshold):
    """``fitness_check`` (optimization_methods.py:163-180) for N structures:
    constraints (N, C, 2) or (C, 2); targets (N, C) or (C,), ``None``/NaN = no
    target.  Returns (pass (N,) bool, error (N,))."""
    X = L.f64(structures)
    N = X.shape[0]
    cons = L.i64(constraints)
    if cons.ndim == 2:
        cons = np.ascontiguousarray(np.broadcast_to(cons, (N,) + cons.shape))
    tg = np.array([[np.nan if t is None else t for t in row] for row in np.atleast_2d(np.asarray(targets, dtype=object))],
                  dtype=np.float64)
    if tg.shape[0] == 1 and N != 1:
        tg = np.broadcast_to(tg, (N, tg.shape[1]))
    tg = np.ascontiguousarray(tg)
    C = cons.shape[1]
    ok = np.zeros(N, dtype=np.uint8)
    err = np.zeros(N)
    L.call("fc_fitness_check", L.pf(X), N, X.shape[1], L.pi(cons), L.pf(tg), C, float(threshold), L.pf(err), L.pb(ok))
    return ok.astype(bool), err


def fitness_check(coords, constraints, targets, threshold):
    ok, _ = fitness_check_batch(L.f64(coords)[None], L.i64(constraints).reshape(-1, 2), [list(targets)], threshold)
    return bool(ok[0])


def rotate_dihedral(coords, dihedral, angle, mask=None, indices_to_be_moved=None):
    """prism_pruner.utils.rotate_dihedral (call sites torsion_module.py:529,537,
    825,834): rotate ``coords[mask]`` by ``angle`` degrees about the i2-i3 bond.
    Returns a new array."""
    from firecode_amd.torsion_module import torsion_scan

    X = L.f64(coords)
    if indices_to_be_moved is not None:
        mask = np.isin(np.arange(len(X)), np.asarray(indices_to_be_moved))
    if mask is None:
        mask = np.zeros(len(X), dtype=bool)
        mask[dihedral[0]] = True
    if float(angle) != int(angle):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "rotate_dihedral takes whole degrees on the GPU path")
    # thresh=0 -> the clash test can never fail, so exactly one rotation is applied
    out, _ = torsion_scan(X, [dihedral], [mask], [[int(angle)]], thresh=0.0)
    return out[0]


def write_xyz(atoms, coords, output, title="temp"):
    """firecode/utils.py:105-116 for one structure or a whole (N, A, 3) block:
    ``output`` is a path (the reference takes an open text file; a path lets the
    library stream millions of conformers without Python string work)."""
    from firecode_amd._lib import xyz_write

    xyz_write(output, atoms, coords, label=title, mode=1)
