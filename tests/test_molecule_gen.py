"""The generator of branched test molecules (tests/molecule_gen.py) builds what it claims: the bond graph
graphize perceives from its coordinates is the graph it built, with rings, shuffled hydrogens and
torsions whose rotation masks are not index ranges -- the inputs the GPU molecule tests rely on."""

import numpy as np
import pytest

nx = pytest.importorskip("networkx")

from firecode_amd import torsion_perception as tp  # noqa: E402
from firecode_amd.pruner import rotation_mask  # noqa: E402
from molecule_gen import random_branched_molecule, random_torsions  # noqa: E402


@pytest.mark.parametrize("n_atoms,seed", [(20, 1), (48, 2), (64, 3), (97, 4), (128, 5), (150, 6)])
def test_graphize_reproduces_the_generated_graph(n_atoms, seed):
    atoms, coords, graph = random_branched_molecule(n_atoms, seed)
    assert atoms.shape == (n_atoms,) and coords.shape == (n_atoms, 3)
    g = tp.graphize(atoms, coords)
    assert sorted(map(sorted, g.edges)) == sorted(map(sorted, graph.edges))
    assert all(g.nodes[i]["atoms"] == graph.nodes[i]["atoms"] == atoms[i] for i in range(n_atoms))
    assert nx.is_connected(g)
    # bonds where bonds belong: heavy - heavy 1.5 A, X - H 1.1 A
    d = np.array([np.linalg.norm(coords[u] - coords[v]) for u, v in graph.edges])
    hyd = np.array([atoms[u] == "H" or atoms[v] == "H" for u, v in graph.edges])
    assert np.allclose(d[hyd], 1.1) and np.allclose(d[~hyd], 1.5)
    # hydrogens interleaved with heavy atoms, rings present from a size on
    h = np.flatnonzero(atoms == "H")
    assert 0 < len(h) < n_atoms and h.min() < np.flatnonzero(atoms != "H").max()
    if n_atoms >= 48:
        assert len(nx.cycle_basis(g)) >= 1
    # the torsions: non-ring heavy-atom bonds, masks that are not contiguous index ranges (for most)
    tors = random_torsions(atoms, graph, 4, seed)
    assert len(tors) >= 3
    bridges = {frozenset(b) for b in nx.bridges(g)}
    scattered = 0
    for t in tors:
        assert frozenset(t[1:3]) in bridges and t[4] in (2, 3, 4, 6)
        assert graph.has_edge(t[0], t[1]) and graph.has_edge(t[2], t[3])
        mv = np.flatnonzero(rotation_mask(g, t[:4], n_atoms))
        assert t[3] in mv and t[1] not in mv and t[2] not in mv
        scattered += mv[-1] - mv[0] + 1 != len(mv)
    assert scattered >= len(tors) - 1
