"""Symmetry-aware RMSD prune without a device: the restatement (tests/symm_ref.py), the perception of atom permutations
(firecode_amd.symmetry.graph_automorphisms) against brute-force enumeration, and the refusals the contract lists
(include/fc_hip.h, "symmetry-aware forms"), each raised before any device use."""

import ctypes as C
import inspect
import os
import re

import networkx as nx
import numpy as np
import pytest

import molecule_gen as mg
import symm_ref as sr
from firecode_amd import _lib
from firecode_amd import symmetry as S
from firecode_amd import synthetic as syn
from oracle import cpu_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fc_prune_rmsd_perm", "fc_rmsd_simbits_perm", "fc_rmsd_clusters_perm", "fc_ensemble_rmsd_pairs_perm")


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [sr.path_table(9), sr.star_table(), sr.transposition_table(14, 3)], ids=["path", "star", "swaps"])
def test_predicate_is_symmetric_for_inverse_closed_tables(table):
    """similar_sym(p, q) == similar_sym(q, p): (q[perm], p) has the values of (q, p[inverse perm]), and the inverse is in
    the table.  Random pairs, thresholds in the middle of their value range so that both verdicts occur."""
    rng = np.random.default_rng(3)
    A = table.shape[1]
    verdicts = []
    for _ in range(60):
        p = rng.normal(size=(A, 3))
        p -= p.mean(axis=0)
        q = p[table[rng.integers(len(table))]] @ syn.random_rotation(rng).T + rng.normal(scale=rng.choice([0.05, 0.4]), size=(A, 3))
        q -= q.mean(axis=0)
        a, b = sr.similar_sym(p, q, table, 0.5, 1.0), sr.similar_sym(q, p, table, 0.5, 1.0)
        assert a == b
        verdicts.append(a)
        for k, perm in enumerate(table):  # value by value: (p, q[perm]) against (q, p[perm^-1])
            r1, m1 = o.rmsd_and_max(p, q[perm])
            r2, m2 = o.rmsd_and_max(q, p[np.argsort(perm)])
            assert abs(r1 - r2) < 1e-12 and abs(m1 - m2) < 1e-10
    assert 5 < sum(verdicts) < 55


def test_identity_table_reproduces_the_default_prune():
    X, atoms, _ = syn.synthetic_ensemble(120, 9, seed=4)
    ident = np.arange(9)[None]
    _, mask0 = o.prune_by_rmsd(X, atoms, 0.5)
    _, mask_m, mats = sr.prune_by_rmsd_sym(X, atoms, ident, 0.5)
    _, mask_p, _ = sr.prune_by_rmsd_sym(X, atoms, ident, 0.5, from_matrix=False)
    assert np.array_equal(mask_m, mask0) and np.array_equal(mask_p, mask0)
    assert np.array_equal(mats.S, mats.S_default) and mats.min_gap > 1e-9
    en = np.random.default_rng(0).normal(size=120)
    for drop in ("earlier", "later"):
        _, m0 = o.prune_by_rmsd(X, atoms, 0.5, energies=en, max_dE=0.8, drop=drop)
        _, m1, _ = sr.prune_by_rmsd_sym(X, atoms, ident, 0.5, energies=en, max_dE=0.8, drop=drop)
        assert np.array_equal(m0, m1)


@pytest.mark.parametrize("table,seed,kept", [(sr.path_table(9), 1, 30), (sr.star_table(), 2, 30)], ids=["path9", "star13"])
def test_relabelled_half_is_recognised(table, seed, kept):
    """150 clustered conformers, a random half relabelled by a random non-identity permutation: the symmetry-aware
    predicate keeps one per cluster, the default prune about twice as many; matrix and pair-by-pair forms agree"""
    A = table.shape[1]
    X, atoms, assign = syn.synthetic_ensemble(150, A, seed=seed)
    Y, _ = sr.relabel_half(X, table, seed)
    _, mask, mats = sr.prune_by_rmsd_sym(Y, atoms, table, 0.5)
    assert mats.min_gap > 0.05
    assert int(mask.sum()) == kept == len(np.unique(assign))
    _, mask0 = o.prune_by_rmsd(Y, atoms, 0.5)
    assert int(mask0.sum()) > 1.5 * kept
    _, mask_p, _ = sr.prune_by_rmsd_sym(Y, atoms, table, 0.5, from_matrix=False)
    assert np.array_equal(mask_p, mask)
    labels, reps, sizes = sr.components(mats.S)
    assert len(reps) == kept and sizes.sum() == 150
    for a in range(len(reps)):  # the components are the generator's clusters
        assert len(set(assign[labels == a])) == 1


def test_or_of_complete_tests_not_the_smallest_rmsd():
    """a pair whose permuted rmsd passes and whose permuted max deviation fails is dissimilar even when that rmsd is the
    smallest of all k"""
    rng = np.random.default_rng(0)
    table = sr.path_table(30)
    p = rng.normal(size=(30, 3))
    p -= p.mean(axis=0)
    q = p[::-1].copy()
    q[0] += (0.0, 0.0, 1.2)  # one atom far off: r_1 ~ 1.2 / sqrt(30) = 0.22 < 0.5, m_1 ~ 1.2 > 1.0
    q -= q.mean(axis=0)
    r1, m1 = o.rmsd_and_max(p, q[table[1]])
    r0, _ = o.rmsd_and_max(p, q)
    assert r1 < 0.5 < r0 and m1 > 1.0
    assert not sr.similar_sym(p, q, table, 0.5, 1.0)
    assert sr.similar_sym(p, q, table, 0.5, 1.5)


# ---- 2. perception -------------------------------------------------------------------------------------------------------
def _graph(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


def _biphenyl_like(ring=4):
    """two rings of ``ring`` atoms joined by one bond (ring = 4: 8 atoms, small enough for 8! brute force)"""
    e = [(a, (a + 1) % ring) for a in range(ring)] + [(ring + a, ring + (a + 1) % ring) for a in range(ring)] + [(0, ring)]
    return 2 * ring, e


CASES = {
    "path5": (5, [(a, a + 1) for a in range(4)], 2),
    "path8": (8, [(a, a + 1) for a in range(7)], 2),
    "ring5": (5, [(a, (a + 1) % 5) for a in range(5)], 10),
    "ring6": (6, [(a, (a + 1) % 6) for a in range(6)], 12),
    "star7": (7, [(0, 1), (1, 2), (0, 3), (3, 4), (0, 5), (5, 6)], 6),
    "biphenyl-like": _biphenyl_like() + (8,),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_graph_automorphisms_against_brute_force(name):
    n, edges, count = CASES[name]
    atoms = np.array(["C"] * n)
    table = S.graph_automorphisms(_graph(n, edges), atoms)
    brute = sr.brute_force_automorphisms(n, edges, ["C"] * n)
    assert len(brute) == count
    assert table.dtype == np.int64 and table.shape == (count, n)
    assert np.array_equal(table[0], np.arange(n))
    assert sorted(map(tuple, table)) == sorted(map(tuple, brute))
    assert S.check_table(table, n) is not None  # identity first, permutations, closed under inverse
    # colours by element: a hetero atom at one end of the path removes the reversal
    if name.startswith("path"):
        atoms2 = atoms.copy()
        atoms2[0] = "N"
        assert len(S.graph_automorphisms(_graph(n, edges), atoms2)) == 1


def _heavy_brute_force(graph, atoms):
    """brute force over the heavy atoms, coloured by element and hydrogen count, as a table over all atoms"""
    heavy = np.flatnonzero(atoms != "H")
    pos = {int(a): k for k, a in enumerate(heavy)}
    edges = [(pos[a], pos[b]) for a, b in graph.edges if a in pos and b in pos]
    colours = [(str(atoms[a]), sum(1 for b in graph.neighbors(a) if atoms[b] == "H")) for a in heavy]
    small = sr.brute_force_automorphisms(len(heavy), edges, colours)
    table = np.tile(np.arange(len(atoms)), (len(small), 1))
    table[:, heavy] = heavy[small]
    return table


@pytest.mark.parametrize("n_atoms,seed,count", [(14, 3, 1), (16, 15, 2)])
def test_graph_automorphisms_of_a_random_branched_molecule(n_atoms, seed, count):
    """shuffled atom order, hydrogens in between: the table is over all atoms and the hydrogens stay.  (14, 3) is
    asymmetric (K = 1), (16, 15) has one symmetry"""
    atoms, _, graph = mg.random_branched_molecule(n_atoms, seed=seed)
    table = S.graph_automorphisms(graph, atoms)
    brute = _heavy_brute_force(graph, atoms)
    assert len(table) == count and np.array_equal(table[0], np.arange(n_atoms))
    assert sorted(map(tuple, table)) == sorted(map(tuple, brute))
    hyd = atoms == "H"
    assert np.array_equal(table[:, hyd], np.broadcast_to(np.arange(n_atoms)[hyd], (len(table), int(hyd.sum()))))


def test_hydrogen_count_colours_the_heavy_atoms():
    """C1(-C0H3)(-C2H2-...): a CH3 arm and a CH2 arm of equal heavy-atom length are not exchanged; two CH3 arms are"""
    #  heavy skeleton: 1 is the centre with arms 0 and 2; atom 3 hangs on the centre to break nothing else
    atoms = np.array(["C", "C", "C", "N"] + ["H"] * 5)
    edges = [(0, 1), (1, 2), (1, 3), (0, 4), (0, 5), (0, 6), (2, 7), (2, 8)]  # C0 has 3 H, C2 has 2 H
    assert len(S.graph_automorphisms(_graph(9, edges), atoms)) == 1
    atoms3 = np.array(["C", "C", "C", "N"] + ["H"] * 6)
    edges3 = edges + [(2, 9)]  # now both arms are CH3
    table = S.graph_automorphisms(_graph(10, edges3), atoms3)
    assert len(table) == 2 and table[1, 0] == 2 and table[1, 2] == 0
    assert np.array_equal(table[1, 4:], np.arange(4, 10))  # unselected atoms stay where they are


def test_graph_automorphisms_respects_its_cap():
    n, edges, count = CASES["ring6"]
    atoms = np.array(["C"] * n)
    assert len(S.graph_automorphisms(_graph(n, edges), atoms, max_perms=12)) == 12
    with pytest.raises(_lib.FirecodeHipInputError, match="at least 12 automorphisms") as err:
        S.graph_automorphisms(_graph(n, edges), atoms, max_perms=11)
    assert err.value.code == _lib.FC_E_LIMIT
    star = _graph(8, [(0, a) for a in range(1, 8)])  # 7! = 5040 automorphisms: the enumeration stops at 65
    with pytest.raises(_lib.FirecodeHipInputError, match="at least 65 automorphisms"):
        S.graph_automorphisms(star, np.array(["C"] * 8))
    for bad in (0, 65, 2.5, True):
        with pytest.raises(_lib.FirecodeHipInputError):
            S.graph_automorphisms(_graph(n, edges), atoms, max_perms=bad)


# ---- 3. the boundary -------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fc_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/fc_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define\s+FC_PERM_MAX\s+64\b", text) and S.PERM_MAX == 64
    assert lib.fc_abi_version() == 1


def test_keyword_defaults():
    import firecode_amd as fc

    for fn in (fc.pruner.prune_by_rmsd, fc.pruner.cluster_by_rmsd, fc.ensemble.Ensemble.similarity_pruning,
               fc.ensemble.Ensemble.cluster_by_rmsd, _lib.DeviceEnsemble.simbits, _lib.DeviceEnsemble.prune,
               _lib.DeviceEnsemble.clusters, _lib.DeviceEnsemble.rmsd_pairs, fc.rmsd.rmsd_and_max_batch):
        assert inspect.signature(fn).parameters["symmetry"].default is None, fn
    assert list(inspect.signature(fc.pruner.prune_by_rmsd).parameters)[:4] == ["structures", "atoms", "max_rmsd", "max_dev"]


def _bad_tables(A):
    ident = np.arange(A)
    cyc = np.roll(ident, 1)  # a -> a - 1: its inverse is the other rotation
    not_perm = ident.copy()
    not_perm[1] = 0
    return {
        "too many": (np.stack([ident] * 65), _lib.FC_E_LIMIT, "FC_PERM_MAX"),
        "not a permutation": (np.stack([ident, not_perm]), _lib.FC_E_INVALID, "not a permutation"),
        "out of range": (np.stack([ident, ident + 1]), _lib.FC_E_INVALID, "not a permutation"),
        "no identity": (np.stack([ident[::-1], ident]), _lib.FC_E_INVALID, "identity"),
        "not closed": (np.stack([ident, cyc]), _lib.FC_E_INVALID, "closed under inverse"),
    }


@pytest.mark.parametrize("what", ["too many", "not a permutation", "out of range", "no identity", "not closed"])
def test_bad_tables_are_refused_before_any_device_use(what):
    """by every Python call that takes symmetry= (no device is needed to get the error) and by the C entry points
    themselves, which look at the table before they look at the handle"""
    import firecode_amd as fc

    A = 6
    table, code, text = _bad_tables(A)[what]
    X, atoms = np.zeros((3, A, 3)), np.array(["C"] * A)
    calls = [
        lambda: fc.pruner.prune_by_rmsd(X, atoms, 0.5, symmetry=table),
        lambda: fc.pruner.cluster_by_rmsd(X, atoms, 0.5, symmetry=table),
        lambda: fc.ensemble.Ensemble(atoms, X, logfunction=None).similarity_pruning(symmetry=table),
        lambda: fc.ensemble.Ensemble(atoms, X, logfunction=None).cluster_by_rmsd(0.5, symmetry=table),
        lambda: fc.rmsd.rmsd_and_max_batch(X, [0], [1], center=True, symmetry=table),
    ]
    for call in calls:
        with pytest.raises(fc.FirecodeHipInputError, match=text) as err:
            call()
        assert err.value.code == code
    lib = _lib.load()
    t32 = np.ascontiguousarray(table, dtype=np.int32)
    p32 = _lib.ptr(t32, C.c_int32)
    out = np.zeros(8)
    rcs = [
        lib.fc_prune_rmsd_perm(None, p32, len(t32), A, 0.5, 1.0, None, 0.0, 20, None, None),
        lib.fc_rmsd_simbits_perm(None, p32, len(t32), A, 0.5, 1.0, None, 0.0, 0, 0, None, None),
        lib.fc_rmsd_clusters_perm(None, p32, len(t32), A, 0.5, 1.0, None, 0.0, None, None, None, None, None),
        lib.fc_ensemble_rmsd_pairs_perm(None, p32, len(t32), A, None, None, 0, _lib.pf(out), _lib.pf(out)),
    ]
    assert rcs == [code] * 4
    assert text in lib.fc_last_error().decode()


def test_good_table_then_null_handle_is_an_input_error():
    lib = _lib.load()
    t32 = np.ascontiguousarray(sr.path_table(6), dtype=np.int32)
    rc = lib.fc_prune_rmsd_perm(None, _lib.ptr(t32, C.c_int32), 2, 6, 0.5, 1.0, None, 0.0, 20, None, None)
    assert rc == _lib.FC_E_INVALID and "ens is NULL" in lib.fc_last_error().decode()
    assert lib.fc_prune_rmsd_perm(None, None, 2, 6, 0.5, 1.0, None, 0.0, 20, None, None) == _lib.FC_E_INVALID
    assert lib.fc_prune_rmsd_perm(None, _lib.ptr(t32, C.c_int32), 0, 6, 0.5, 1.0, None, 0.0, 20, None, None) == _lib.FC_E_INVALID


def test_symmetry_with_prune_enantiomers_is_refused_and_names_the_flag():
    import firecode_amd as fc

    A = 6
    X, atoms, table = np.zeros((3, A, 3)), np.array(["C"] * A), sr.path_table(A)
    graph = _graph(A, [(a, a + 1) for a in range(A - 1)])
    for sym in (table, graph):
        for call in (lambda: fc.pruner.prune_by_rmsd(X, atoms, 0.5, prune_enantiomers=True, symmetry=sym),
                     lambda: fc.pruner.cluster_by_rmsd(X, atoms, 0.5, prune_enantiomers=True, symmetry=sym),
                     lambda: fc.ensemble.Ensemble(atoms, X, logfunction=None).similarity_pruning(
                         prune_enantiomers=True, symmetry=sym)):
            with pytest.raises(fc.FirecodeHipInputError, match="prune_enantiomers"):
                call()
    with pytest.raises(fc.FirecodeHipInputError, match="inverted"):
        fc.rmsd.rmsd_and_max_batch(X, [0], [1], inverted=True, symmetry=table)


def test_table_to_selected_indices():
    """the Python layer hands the library selected-atom indices; a permutation that leaves the selection is refused"""
    atoms = np.array(["C", "H", "C", "C", "H"])
    mask = atoms != "H"
    table = np.array([[0, 1, 2, 3, 4], [3, 1, 2, 0, 4]])
    t = S.selected_table(S.check_table(table, 5), mask)
    assert t.dtype == np.int32 and np.array_equal(t, [[0, 1, 2], [2, 1, 0]]) and np.array_equal(t, sr.selected(table, mask))
    leaves = np.array([[0, 1, 2, 3, 4], [1, 0, 2, 3, 4]])  # C0 <-> H1
    with pytest.raises(_lib.FirecodeHipInputError, match="outside the atom selection"):
        S.selected_table(S.check_table(leaves, 5), mask)
    import firecode_amd as fc

    with pytest.raises(fc.FirecodeHipInputError, match="outside the atom selection"):
        fc.pruner.prune_by_rmsd(np.zeros((3, 5, 3)), atoms, 0.5, symmetry=leaves)
    with pytest.raises(fc.FirecodeHipInputError, match="element symbols"):
        fc.rmsd.rmsd_and_max_batch(np.zeros((3, 5, 3)), [0], [1], symmetry=_graph(5, [(0, 2)]))
    with pytest.raises(fc.FirecodeHipInputError, match=r"\(K, 5\) integer table"):
        fc.pruner.prune_by_rmsd(np.zeros((3, 5, 3)), atoms, 0.5, symmetry=np.zeros((2, 4), dtype=int))


def test_no_cpu_fallback_for_the_new_calls():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    import firecode_amd as fc

    A = 6
    X, atoms, table = np.zeros((3, A, 3)), np.array(["C"] * A), sr.path_table(A)
    for call in (lambda: fc.pruner.prune_by_rmsd(X, atoms, 0.5, symmetry=table),
                 lambda: fc.pruner.cluster_by_rmsd(X, atoms, 0.5, symmetry=table),
                 lambda: fc.rmsd.rmsd_and_max_batch(X, [0], [1], center=True, symmetry=table)):
        with pytest.raises(fc.FirecodeHipDeviceError):
            call()
