"""Atom permutations of equivalent atoms for the symmetry-aware RMSD forms (include/fc_hip.h, "symmetry-aware forms";
DESIGN.md section 14): perception from the bond graph, the checks the contract lists, and the conversion of a table over
all atoms to the selected-atom indices the library takes.  Host glue only: every check here runs before any device use.

``symmetry=`` of the calls that take it is ``None`` (the path as it is), a networkx graph (the automorphisms are perceived
by ``graph_automorphisms``; needs the element symbols, so only the calls that know ``atoms``) or an explicit ``(K, A)``
table over all atoms, used as given."""

import numpy as np

from firecode_amd import _lib as L

PERM_MAX = 64  # FC_PERM_MAX


def graph_automorphisms(graph, atoms, heavy_atoms_only=True, max_perms=PERM_MAX):
    """The permutations of equivalent atoms of a molecule -> ``(K, A)`` int64 over ALL atoms, identity first, atoms
    outside the selection fixed; row k maps atom a to ``table[k, a]``.

    ``heavy_atoms_only=True``: the automorphisms of the heavy-atom subgraph, atoms coloured by element and by the number
    of attached hydrogens (a CH3 and a CH2 of equal heavy-atom environment are not exchanged).  ``False``: of the whole
    graph, coloured by element.  The enumeration stops at ``max_perms + 1`` matches and then raises an input error that
    names the count: a truncated set is not closed under inverse and is never returned."""
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher

    atoms = np.asarray(atoms)
    A = int(atoms.shape[0])
    if isinstance(max_perms, (bool, np.bool_)) or int(max_perms) != max_perms or not 1 <= int(max_perms) <= PERM_MAX:
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"max_perms={max_perms!r} outside [1, {PERM_MAX}]")
    if set(graph.nodes) - set(range(A)):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"the graph has nodes outside 0..{A - 1}, the indices of atoms")
    selected = [a for a in range(A) if not (heavy_atoms_only and atoms[a] == "H")]
    chosen = set(selected)
    coloured = nx.Graph()
    for a in selected:
        nbrs = list(graph.neighbors(a)) if a in graph else []
        n_h = sum(1 for b in nbrs if atoms[b] == "H") if heavy_atoms_only else 0
        coloured.add_node(a, colour=(str(atoms[a]), n_h))
    coloured.add_edges_from((a, b) for a, b in graph.edges if a in chosen and b in chosen and a != b)
    matcher = GraphMatcher(coloured, coloured, node_match=lambda x, y: x["colour"] == y["colour"])
    rows = []
    for mapping in matcher.isomorphisms_iter():
        if len(rows) == int(max_perms):
            raise L.FirecodeHipInputError(
                L.FC_E_LIMIT, f"the graph has at least {len(rows) + 1} automorphisms, more than max_perms={int(max_perms)}: "
                "pass a smaller, inverse-closed table explicitly")
        row = np.arange(A, dtype=np.int64)
        for a, b in mapping.items():
            row[a] = b
        rows.append(row)
    rows.sort(key=lambda r: (not np.array_equal(r, np.arange(A)), r.tolist()))  # the identity first, then a fixed order
    return np.stack(rows) if rows else np.arange(A, dtype=np.int64)[None]


def check_table(table, n_atoms):
    """The contract's checks on a table over ``n_atoms`` atoms -> (K, n_atoms) int64, C-contiguous.  FC_E_LIMIT: more
    than ``PERM_MAX`` rows.  FC_E_INVALID: not a 2-D integer array of that width, a row that is not a permutation, row 0
    not the identity, a row whose inverse is missing."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != n_atoms or t.shape[0] < 1 or t.dtype.kind not in "iu":
        raise L.FirecodeHipInputError(
            L.FC_E_INVALID, f"symmetry must be a (K, {n_atoms}) integer table of atom permutations, got "
            f"{t.shape} {t.dtype}")
    if t.shape[0] > PERM_MAX:
        raise L.FirecodeHipInputError(L.FC_E_LIMIT, f"K={t.shape[0]} permutations exceed FC_PERM_MAX={PERM_MAX}")
    t = np.ascontiguousarray(t, dtype=np.int64)
    ident = np.arange(n_atoms, dtype=np.int64)
    if not np.array_equal(np.sort(t, axis=1), np.broadcast_to(ident, t.shape)):
        bad = int(np.flatnonzero((np.sort(t, axis=1) != ident).any(axis=1))[0])
        raise L.FirecodeHipInputError(L.FC_E_INVALID, f"row {bad} of symmetry is not a permutation of 0..{n_atoms - 1}")
    if not np.array_equal(t[0], ident):
        raise L.FirecodeHipInputError(L.FC_E_INVALID, "row 0 of symmetry is not the identity")
    have = {row.tobytes() for row in t}
    for k, row in enumerate(t):
        if np.argsort(row).astype(np.int64).tobytes() not in have:
            raise L.FirecodeHipInputError(
                L.FC_E_INVALID, f"symmetry is not closed under inverse: the inverse of row {k} is not in the table")
    return t


def resolve(symmetry, atoms=None, heavy_atoms_only=True, n_atoms=None):
    """``symmetry=`` as a checked (K, A) int64 table over all atoms, or None."""
    if symmetry is None:
        return None
    if hasattr(symmetry, "nodes") and hasattr(symmetry, "edges"):
        if atoms is None:
            raise L.FirecodeHipInputError(
                L.FC_E_INVALID, "a graph as symmetry= needs the element symbols: pass "
                "firecode_amd.symmetry.graph_automorphisms(graph, atoms) instead")
        return check_table(graph_automorphisms(symmetry, atoms, heavy_atoms_only), len(atoms))
    return check_table(symmetry, len(atoms) if n_atoms is None else int(n_atoms))


def selected_table(table, atom_mask):
    """A checked table over all atoms -> (K, A_sel) int32 in selected-atom indices, the form the library takes.  A
    permutation that maps a selected atom onto an unselected one is an input error."""
    A = table.shape[1]
    mask = np.ones(A, dtype=bool) if atom_mask is None else np.asarray(atom_mask, dtype=bool)
    sel = np.flatnonzero(mask)
    images = table[:, sel]
    if not mask[images].all():
        k, a = (int(v[0]) for v in np.nonzero(~mask[images]))
        raise L.FirecodeHipInputError(
            L.FC_E_INVALID, f"row {k} of symmetry maps the selected atom {int(sel[a])} onto atom {int(images[k, a])}, "
            "which is outside the atom selection")
    position = np.full(A, -1, dtype=np.int64)
    position[sel] = np.arange(len(sel))
    return np.ascontiguousarray(position[images], dtype=np.int32)


LDS_LIMIT = 160 * 1024  # kLdsLimit
DIVERSE_STATIC_LDS = 64  # kDiverseSymStaticLds


def diverse_lds_bytes(n_perms, n_selected):
    """LDS of one workgroup of the symmetry-aware diverse selection (fc_ensemble_select_diverse_perm): the
    representative, the table as 16-bit indices rounded up to 8 bytes, the kernel's own 64."""
    return 24 * int(n_selected) + ((2 * int(n_perms) * int(n_selected) + 7) & ~7) + DIVERSE_STATIC_LDS


def diverse_max_selected(n_perms):
    """the largest number of selected atoms the symmetry-aware diverse selection takes with ``n_perms`` permutations"""
    a = (LDS_LIMIT - DIVERSE_STATIC_LDS) // (24 + 2 * int(n_perms))
    while diverse_lds_bytes(n_perms, a) > LDS_LIMIT:
        a -= 1
    return a


def diverse_lds_check(n_perms, n_selected):
    """FC_E_LIMIT, before any device use, where the library itself would refuse the selection for its LDS"""
    need = diverse_lds_bytes(n_perms, n_selected)
    if need > LDS_LIMIT:
        raise L.FirecodeHipInputError(
            L.FC_E_LIMIT, f"A_sel={int(n_selected)} selected atoms with K={int(n_perms)} permutations need {need} bytes of "
            f"LDS (limit {LDS_LIMIT}): at most {diverse_max_selected(n_perms)} selected atoms")


def diverse_table(symmetry, prune_enantiomers, atom_mask, n_atoms):
    """``symmetry=`` (a checked table over all atoms, or None) and the mirror flag of the diverse selection -> the
    (K, A_sel) int32 table the library takes, or None when neither is set; the LDS limit checked on the way"""
    if symmetry is None and not prune_enantiomers:
        return None
    table = np.arange(int(n_atoms), dtype=np.int64)[None] if symmetry is None else symmetry
    t = selected_table(table, atom_mask)
    diverse_lds_check(t.shape[0], t.shape[1])
    return t


KNN_TILE_ROWS = 16  # kKnnTileRows


def knn_lds_bytes(n_perms, n_selected):
    """LDS of one workgroup of the symmetry-aware nearest-neighbour lists (fc_ensemble_knn_perm, fc_ensemble_knn_cross_perm):
    its 16 row conformers and the table as 16-bit indices rounded up to 8 bytes."""
    return KNN_TILE_ROWS * 24 * int(n_selected) + ((2 * int(n_perms) * int(n_selected) + 7) & ~7)


def knn_max_selected(n_perms):
    """the largest number of selected atoms the symmetry-aware nearest-neighbour lists take with ``n_perms`` permutations"""
    a = LDS_LIMIT // (KNN_TILE_ROWS * 24 + 2 * int(n_perms)) + 1
    while knn_lds_bytes(n_perms, a) > LDS_LIMIT:
        a -= 1
    return a


def knn_lds_check(n_perms, n_selected):
    """FC_E_LIMIT, before any device use, where the library itself would refuse the lists for their LDS"""
    need = knn_lds_bytes(n_perms, n_selected)
    if need > LDS_LIMIT:
        raise L.FirecodeHipInputError(
            L.FC_E_LIMIT, f"A_sel={int(n_selected)} selected atoms with K={int(n_perms)} permutations need {need} bytes of "
            f"LDS (limit {LDS_LIMIT}): at most {knn_max_selected(n_perms)} selected atoms")


def medoid_lds_bytes(n_perms, n_selected):
    """LDS of one workgroup of the symmetry-aware medoid sums and silhouettes (fc_ensemble_medoids_perm,
    fc_ensemble_kmedoids_perm, fc_ensemble_silhouette_perm): the tile of the nearest-neighbour lists -- 16 row conformers
    and the table -- and no static LDS on top."""
    return knn_lds_bytes(n_perms, n_selected)


def medoid_max_selected(n_perms):
    """the largest number of selected atoms the symmetry-aware medoids and silhouettes take with ``n_perms`` permutations"""
    return knn_max_selected(n_perms)


def medoid_lds_check(n_perms, n_selected):
    """FC_E_LIMIT, before any device use, where the library itself would refuse the sums for their LDS"""
    knn_lds_check(n_perms, n_selected)


def knn_table(symmetry, prune_enantiomers, atom_mask, n_atoms):
    """``symmetry=`` (a checked table over all atoms, or None) and the mirror flag of the nearest-neighbour lists -> the
    (K, A_sel) int32 table the library takes, or None when neither is set; the LDS limit checked on the way"""
    if symmetry is None and not prune_enantiomers:
        return None
    table = np.arange(int(n_atoms), dtype=np.int64)[None] if symmetry is None else symmetry
    t = selected_table(table, atom_mask)
    knn_lds_check(t.shape[0], t.shape[1])
    return t


def refuse_with_enantiomers(table, prune_enantiomers):
    if table is not None and prune_enantiomers:
        raise L.FirecodeHipInputError(
            L.FC_E_INVALID, "prune_enantiomers=True cannot be combined with symmetry=: the symmetry-aware forms have no "
            "enantiomer-aware variant")
