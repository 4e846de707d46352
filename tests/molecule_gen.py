"""Seeded branched 3-D test molecules for the torsion scan (not a test module: imported by
test_molecule_gen.py and test_gpu_molecules.py).

A random tree of heavy atoms at 1.5 A, a few planar rings hung on it, hydrogens at 1.1 A, the atom order
shuffled so that hydrogens sit between heavy atoms.  Every pair of atoms that is not bonded is kept farther
apart than ``graphize``'s bond cut-off (1.2 x the sum of the covalent radii), so the bond graph the
coordinates imply is the one the generator built.  Torsions are taken about non-ring heavy-atom bonds with
n-folds from {2, 3, 4, 6}; their rotation masks are ``pruner.rotation_mask`` of the built graph, so
moving sets are interleaved, branched index sets rather than the suffixes of a chain."""

import networkx as nx
import numpy as np

BOND, BOND_H = 1.5, 1.1
MIN_HEAVY, MIN_HEAVY_H, MIN_HH = 2.3, 1.75, 1.5  # non-bonded distances kept (graphize bonds C-C < 1.82, C-H < 1.28)
VALENCE = {"C": 4, "N": 3, "O": 2}


def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def _far_enough(pts, syms, cand, cand_sym, bonded_to):
    """cand is no closer than the non-bonded limits to any atom but the ones listed in bonded_to"""
    if not pts:
        return True
    d = np.linalg.norm(np.asarray(pts) - cand, axis=1)
    for k, (dk, s) in enumerate(zip(d, syms)):
        if k in bonded_to:
            continue
        lim = MIN_HH if s == "H" and cand_sym == "H" else MIN_HEAVY_H if "H" in (s, cand_sym) else MIN_HEAVY
        if dk < lim:
            return False
    return True


def random_branched_molecule(n_atoms, seed, n_rings=2):
    """(atoms (A,), coords (A, 3), graph) with A == n_atoms (n_atoms >= 12), atom order shuffled; the graph's
    nodes are 0 .. A-1 with the element symbol under "atoms", as graphize leaves them."""
    rng = np.random.default_rng(seed)
    for _ in range(200):  # (a grown tree that cannot take its hydrogens: start over)
        out = _grow(n_atoms, rng, n_rings)
        if out is not None:
            return out
    raise RuntimeError(f"no {n_atoms}-atom molecule for seed {seed}")


def _grow(n_atoms, rng, n_rings):
    pts, syms, edges = [np.zeros(3)], ["C"], []
    n_heavy = max(6, int(round(n_atoms * 0.5)))
    deg = [0]

    def free(a):
        return VALENCE[syms[a]] - deg[a]

    def add(p, s, parent):
        pts.append(p)
        syms.append(s)
        deg.append(1)
        deg[parent] += 1
        edges.append((parent, len(pts) - 1))

    rings_left = n_rings
    tries = 0
    while len(pts) < n_heavy and tries < 20000:
        tries += 1
        open_ = [a for a in range(len(pts)) if free(a) >= 2]  # (room for this bond and a hydrogen or a branch)
        if not open_:
            return None
        p = int(rng.choice(open_))
        d = _unit(rng)
        if rings_left and len(pts) > 3 and len(pts) + 6 <= n_heavy and rng.random() < 0.25:
            # a planar six-ring (side 1.5 A) whose first atom bonds to p
            r0 = pts[p] + BOND * d
            e = np.cross(d, _unit(rng))
            e /= np.linalg.norm(e)
            centre = r0 + BOND * d
            ring = [centre + BOND * (np.cos(np.radians(60 * k)) * -d + np.sin(np.radians(60 * k)) * e) for k in range(6)]
            ok = all(_far_enough(pts, syms, c, "C", {p} if k == 0 else set()) for k, c in enumerate(ring))
            if ok:
                base = len(pts)
                add(ring[0], "C", p)
                for k in range(1, 6):
                    add(ring[k], "C", base + k - 1)
                edges.append((base + 5, base))
                deg[base] += 1
                deg[base + 5] += 1
                rings_left -= 1
            continue
        s = str(rng.choice(["C", "C", "C", "C", "N", "O"]))
        cand = pts[p] + BOND * d
        if _far_enough(pts, syms, cand, s, {p}):
            add(cand, s, p)
    if len(pts) < n_heavy:
        return None
    # hydrogens on the open valences, one at a time, until the molecule has n_atoms atoms
    heavy = len(pts)
    while len(pts) < n_atoms:
        open_ = [a for a in range(heavy) if free(a) > 0]
        if not open_:
            return None
        a = int(rng.choice(open_))
        for _ in range(200):
            cand = pts[a] + BOND_H * _unit(rng)
            if _far_enough(pts, syms, cand, "H", {a}):
                add(cand, "H", a)
                break
        else:
            deg[a] = VALENCE[syms[a]]  # (crowded: no hydrogen fits here)
    perm = rng.permutation(n_atoms)  # new index of old atom k: perm[k]
    coords = np.empty((n_atoms, 3))
    atoms = np.empty(n_atoms, dtype="<U1")
    coords[perm] = np.asarray(pts)
    atoms[perm] = syms
    g = nx.Graph()
    g.add_nodes_from((i, {"atoms": str(atoms[i])}) for i in range(n_atoms))
    g.add_edges_from((int(perm[u]), int(perm[v])) for u, v in edges)
    return atoms, coords, g


def random_torsions(atoms, graph, n_tors, seed, folds=(2, 3, 4, 6), max_sets=None):
    """n_tors torsions (i1, i2, i3, i4, n_fold) about distinct non-ring heavy-atom bonds whose two ends carry
    further neighbours, in a random order, with n-folds drawn from ``folds`` (the grid kept under ``max_sets``)."""
    rng = np.random.default_rng(seed)
    bridges = [tuple(b) for b in nx.bridges(graph)]
    cand = [(u, v) for u, v in bridges if atoms[u] != "H" and atoms[v] != "H" and graph.degree(u) > 1 and graph.degree(v) > 1]
    pick = rng.permutation(len(cand))[:n_tors]
    out, n_sets = [], 1
    for k in pick:
        u, v = cand[k]
        if rng.random() < 0.5:
            u, v = v, u
        i1 = int(rng.choice(sorted(n for n in graph.neighbors(u) if n != v)))
        i4 = int(rng.choice(sorted(n for n in graph.neighbors(v) if n != u)))
        f = int(rng.choice(folds))
        while max_sets is not None and f > 2 and n_sets * f > max_sets:
            f = {3: 2, 4: 3, 6: 4}[f]
        if max_sets is not None and n_sets * f > max_sets:
            break
        n_sets *= f
        out.append((i1, int(u), int(v), i4, f))
    return out
