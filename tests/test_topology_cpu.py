"""CPU checks of the bond-topology check (molecule_check / scramble_check, include/fc_hip.h fc_bond_changes):
the NumPy restatement against FIRECODE's own set logic on the golden cases, the drop-ins' signatures, and argument
errors raised before any device use."""

import ctypes as C
import inspect
import json
import os

import networkx as nx
import numpy as np
import pytest

from firecode_amd import _lib
import topology_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def topo():
    return np.load(os.path.join(ROOT, "tests", "golden", "topology_v1.npz"), allow_pickle=False)


def _rows(flat, off, k):
    return flat[off[k]:off[k + 1]]


def _graph(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from((int(a), int(b)) for a, b in edges)
    return g


def test_golden_cases_are_not_vacuous(topo):
    assert topo["mc_ok"].any() and (~topo["mc_ok"]).any()
    assert topo["sc_ok"].any() and (~topo["sc_ok"]).any()
    counts = np.diff(topo["sc_delta_off"])
    assert counts.min() == 0 and counts.max() >= 4
    assert set(np.unique(topo["sc_sizes"].astype(bool).sum(axis=1))) == {1, 2, 3}
    ex = topo["sc_excl"]
    assert (ex < 0).any() and any((_rows(ex, topo["sc_excl_off"], k) >= A).any() for k, A in enumerate(topo["sc_A"]))
    assert set(topo["sc_max_newbonds"].tolist()) == set(range(-1, 5))
    # self-loops in the prepared graphs (the reference drops them)
    assert (topo["mc_new_edges"][:, 0] == topo["mc_new_edges"][:, 1]).any()
    assert (topo["sc_frag_edges"][:, 0] == topo["sc_frag_edges"][:, 1]).any()


def test_restatement_matches_molecule_check(topo):
    maxes = topo["mc_max_newbonds"]
    for k, A in enumerate(topo["mc_A"]):
        delta = ref.delta_from_edges(_rows(topo["mc_new_edges"], topo["mc_new_off"], k),
                                     _rows(topo["mc_old_edges"], topo["mc_old_off"], k), int(A))
        assert np.array_equal(len(delta) <= maxes, topo["mc_ok"][k]), k


def test_restatement_matches_scramble_check(topo):
    fo = topo["sc_frag_off"]
    for k, A in enumerate(topo["sc_A"]):
        sizes = [int(s) for s in topo["sc_sizes"][k] if s > 0]
        graphs = [_graph(s, _rows(topo["sc_frag_edges"], fo, 3 * k + f)) for f, s in enumerate(sizes)]
        ref_edges, n_nodes = ref.graphs_reference(graphs)
        assert n_nodes == A
        excl = _rows(topo["sc_excl"], topo["sc_excl_off"], k)
        delta = ref.delta_from_edges(_rows(topo["sc_new_edges"], topo["sc_new_off"], k), ref_edges, int(A), excl)
        want = {(int(i), int(j)) for i, j in _rows(topo["sc_delta"], topo["sc_delta_off"], k)}
        assert delta == want, k
        assert (len(delta) <= topo["sc_max_newbonds"][k]) == topo["sc_ok"][k], k


@pytest.mark.parametrize("name", ["molecule_check", "scramble_check"])
def test_drop_in_signatures_match_the_reference(topo, name):
    from firecode_amd import utils

    want = json.loads(str(topo[f"sig_{name}"]))
    got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
           for p in inspect.signature(getattr(utils, name)).parameters.values()]
    assert got == want


def test_abi_version_stays_one():
    assert _lib.load().fc_abi_version() == 1
    for name in ("fc_bond_changes", "fc_bond_changes_list"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)


def _atoms(A):
    return np.array(["C"] * A)


def test_python_argument_errors_precede_device_use():
    from firecode_amd import refining, utils

    err = _lib.FirecodeHipInputError
    X = np.zeros((3, 4, 3))
    g2 = _graph(2, [(0, 1)])
    with pytest.raises(err):  # structures not (N, A, 3)
        utils.molecule_check_batch(_atoms(4), X[0], np.zeros((3, 4, 2)))
    with pytest.raises(err):  # reference shape differs
        utils.molecule_check_batch(_atoms(4), np.zeros((5, 3)), X)
    with pytest.raises(err):  # per-structure reference of another N
        utils.molecule_check_batch(_atoms(4), np.zeros((2, 4, 3)), X)
    with pytest.raises(err):  # atom symbols of another length
        utils.molecule_check_batch(_atoms(5), X[0], X)
    with pytest.raises(err):
        utils.molecule_check(_atoms(4), X[0], X)
    with pytest.raises(err):  # node-count mismatch: the reference's assert
        utils.scramble_check_batch(_atoms(4), X, [], [g2])
    with pytest.raises(err):
        utils.scramble_check(_atoms(4), X[0], [], [g2, g2, g2])
    with pytest.raises(err):  # ragged: per-structure exclusions for 2 of 3 structures
        utils.scramble_check_batch(_atoms(4), X, [[0], [1]], [g2, g2])
    with pytest.raises(err):  # atom indices mixed with collections
        utils.scramble_check_batch(_atoms(4), X, [0, [1], [2]], [g2, g2])
    with pytest.raises(err):  # non-integer exclusions
        utils.scramble_check_batch(_atoms(4), X, [0.5], [g2, g2])
    with pytest.raises(err):  # exit_status of another length
        refining.scramble_refining(X, _atoms(4), [g2, g2], [[0]] * 3, exit_status=[True, False])
    with pytest.raises(err):  # constrained_indices of another length
        refining.scramble_refining(X, _atoms(4), [g2, g2], [[0]] * 2)


def test_abi_argument_errors_precede_device_use():
    """fc_bond_changes refuses bad arguments with FC_E_INVALID before it initialises a device (on a machine without
    one, the same calls would otherwise end in FC_E_NODEVICE)."""
    lib = _lib.load()
    N, A = 2, 3
    X = np.zeros((N, A, 3))
    cls = np.zeros(A, dtype=np.int32)
    thr = np.array([[1.824]])
    bits = np.zeros(A, dtype=np.uint64)
    counts, ok = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.uint8)
    p32 = cls.ctypes.data_as(C.POINTER(C.c_int32))

    def call(ref_x=None, stride=0, ref_b=None, n_class=1, classes=p32, eo=None, ea=None, es=0):
        return lib.fc_bond_changes(_lib.pf(X), N, A, classes, n_class, _lib.pf(thr), _lib.pf(ref_x), stride,
                                   _lib.pw(ref_b), _lib.pi(eo), _lib.pi(ea), es, 0, _lib.pi(counts), _lib.pb(ok))

    assert call(ref_x=X[0], ref_b=bits) == _lib.FC_E_INVALID  # two references
    assert call() == _lib.FC_E_INVALID  # none
    assert call(ref_x=X[0], stride=5) == _lib.FC_E_INVALID  # stride neither 0 nor 3A
    assert call(ref_b=bits, n_class=0) == _lib.FC_E_INVALID
    bad = np.array([0, 1, 0], dtype=np.int32)  # class 1 of a 1-class table
    assert call(ref_b=bits, classes=bad.ctypes.data_as(C.POINTER(C.c_int32))) == _lib.FC_E_INVALID
    eo = np.array([0, 2, 1], dtype=np.int64)  # decreasing offsets
    assert call(ref_b=bits, eo=eo, ea=np.zeros(2, np.int64), es=2) == _lib.FC_E_INVALID
    assert call(ref_b=bits, eo=np.array([0, 1], np.int64), ea=np.zeros(1, np.int64), es=3) == _lib.FC_E_INVALID
    off = np.array([1, 1, 1], dtype=np.int64)  # list pass: offsets not starting at 0
    bonds = np.zeros((1, 3), dtype=np.int64)
    rc = lib.fc_bond_changes_list(_lib.pf(X), N, A, p32, 1, _lib.pf(thr), None, 0, _lib.pw(bits), None, None, 0,
                                  _lib.pi(off), _lib.pi(bonds))
    assert rc == _lib.FC_E_INVALID
    # N = 0 is accepted with nothing to do
    assert lib.fc_bond_changes(None, 0, A, None, 1, None, None, 0, _lib.pw(bits), None, None, 0, 0, None, None) == 0
