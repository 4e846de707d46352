"""Generate tests/golden/topology_v1.npz: FIRECODE's own molecule_check / scramble_check set logic on prepared graphs.

Run in the authoring container only (the reference never travels):

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_topology.py

Import recipe as make_golden.py (placeholder modules for the un-vendored ``prism_pruner`` that raise if called).
``firecode.utils.graphize`` is then replaced by a lookup: every "structure" passed to the reference is a token array
whose first entry names a prepared networkx graph, so only the reference's set arithmetic runs (utils.py:341-400):
bond sets from graph edges, self-loops dropped, fragment offsets, the symmetric difference, the exclusion loop, the
``max_newbonds`` test and the log line.  Nothing of this repository is imported.  Inputs are seeded.
"""

import ast
import inspect
import json
import os
import sys
import types
import typing

import networkx as nx
import numpy as np
import typing_extensions

typing.Self = typing_extensions.Self
for _name in ("prism_pruner", "prism_pruner.algebra", "prism_pruner.graph_manipulations",
              "prism_pruner.pruner", "prism_pruner.utils", "prism_pruner.rmsd",
              "prism_pruner.periodic_table"):
    _m = types.ModuleType(_name)

    def _ga(k, _n=_name):
        def _raise(*a, **kw):
            raise RuntimeError(f"placeholder {_n}.{k} called: not reference code")
        return _raise

    _m.__getattr__ = _ga
    sys.modules[_name] = _m

import firecode.utils as fu  # noqa: E402

GRAPHS = []


def _lookup(atoms, coords):
    return GRAPHS[int(coords[0][0])]


fu.graphize = _lookup


def token(graph):
    """A structure the lookup resolves to `graph` (one row per node, as the reference's length assert wants)."""
    GRAPHS.append(graph)
    return np.full((len(graph.nodes), 3), float(len(GRAPHS) - 1))


def random_graph(rng, n, p, loops):
    g = nx.Graph()
    g.add_nodes_from(range(n))  # nodes in index order, as graphize builds them
    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() < p:
                g.add_edge(i, j)
    for i in rng.choice(n, size=min(n, loops), replace=False):
        g.add_edge(int(i), int(i))
    return g


def perturbed(rng, g, flips, loops):
    """g with `flips` node pairs toggled (bonds formed or broken) and a few self-loops."""
    h = nx.Graph()
    h.add_nodes_from(range(len(g.nodes)))
    h.add_edges_from((a, b) for a, b in g.edges if a != b)
    n = len(g.nodes)
    for _ in range(flips):
        a, b = (int(v) for v in rng.choice(n, size=2, replace=False))
        if h.has_edge(a, b):
            h.remove_edge(a, b)
        else:
            h.add_edge(a, b)
    for i in rng.choice(n, size=min(n, loops), replace=False):
        h.add_edge(int(i), int(i))
    return h


def edges_of(g):
    return np.array([(a, b) for a, b in g.edges], dtype=np.int64).reshape(-1, 2)


def pack(lists, width=2):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(len(x), width) for x in lists]).reshape(-1, width)
    return flat, off


rng = np.random.default_rng(20261016)
MAXES = np.arange(-1, 5)
G = {}

# ---- molecule_check (utils.py:341-353): verdicts for max_newbonds -1..4 pin every count up to 4 -------------------
mc_A, mc_old, mc_new, mc_ok = [], [], [], []
for c in range(120):
    A = int(rng.integers(2, 41))
    old = random_graph(rng, A, float(rng.uniform(0.02, 0.3)), int(rng.integers(0, 3)))
    new = perturbed(rng, old, int(rng.integers(0, 7)), int(rng.integers(0, 3)))
    atoms = np.array(["C"] * A)
    o, n_ = token(old), token(new)
    mc_ok.append([fu.molecule_check(atoms, o, n_, max_newbonds=int(m)) for m in MAXES])
    mc_A.append(A)
    mc_old.append(edges_of(old))
    mc_new.append(edges_of(new))
G["mc_A"] = np.array(mc_A, dtype=np.int64)
G["mc_old_edges"], G["mc_old_off"] = pack(mc_old)
G["mc_new_edges"], G["mc_new_off"] = pack(mc_new)
G["mc_ok"] = np.array(mc_ok, dtype=bool)
G["mc_max_newbonds"] = MAXES

# ---- scramble_check (utils.py:356-400): 1-3 fragments, exclusions with duplicates / negatives / out of range ----------
sc = {k: [] for k in ("A", "sizes", "new", "excl", "max", "ok", "delta", "line")}
frag_lists = []
for c in range(160):
    nf = int(rng.integers(1, 4))
    sizes = [int(v) for v in rng.integers(1, 14, size=nf)]
    if sum(sizes) < 2:
        sizes[0] += 1
    A = sum(sizes)
    frags = [random_graph(rng, s, float(rng.uniform(0.05, 0.4)), int(rng.integers(0, 2))) for s in sizes]
    union = nx.Graph()
    union.add_nodes_from(range(A))
    pos = 0
    for g, s in zip(frags, sizes):
        union.add_edges_from((a + pos, b + pos) for a, b in g.edges if a != b)
        pos += s
    new = perturbed(rng, union, int(rng.integers(0, 7)), int(rng.integers(0, 3)))
    k = int(rng.integers(0, 6))
    excl = [int(v) for v in rng.integers(-3, A + 4, size=k)]
    if k and rng.random() < 0.5:
        excl.append(excl[0])  # duplicate
    maxnb = int(rng.choice(MAXES))
    atoms = np.array(["C"] * A)
    t = token(new)
    ok = fu.scramble_check(atoms, t, excl, frags, max_newbonds=maxnb)
    lines = []
    fu.scramble_check(atoms, t, excl, frags, max_newbonds=-1, logfunction=lines.append, title=f"case{c}")
    head = f"case{c}, scramble_check - found "
    assert len(lines) == 1 and lines[0].startswith(head), lines
    count_text, rest = lines[0][len(head):].split(" extra bonds: ", 1)
    delta = ast.literal_eval(rest) if rest != "set()" else set()
    assert len(delta) == int(count_text)
    sc["A"].append(A)
    sc["sizes"].append(sizes + [0] * (3 - nf))
    frag_lists += [edges_of(g) for g in frags] + [np.zeros((0, 2), np.int64)] * (3 - nf)
    sc["new"].append(edges_of(new))
    sc["excl"].append(np.array(excl, dtype=np.int64))
    sc["max"].append(maxnb)
    sc["ok"].append(ok)
    sc["delta"].append(np.array(sorted(delta), dtype=np.int64).reshape(-1, 2))
    sc["line"].append(lines[0])
G["sc_A"] = np.array(sc["A"], dtype=np.int64)
G["sc_sizes"] = np.array(sc["sizes"], dtype=np.int64)
G["sc_frag_edges"], G["sc_frag_off"] = pack(frag_lists)
G["sc_new_edges"], G["sc_new_off"] = pack(sc["new"])
G["sc_excl"], G["sc_excl_off"] = pack(sc["excl"], width=1)
G["sc_excl"] = G["sc_excl"].reshape(-1)
G["sc_max_newbonds"] = np.array(sc["max"], dtype=np.int64)
G["sc_ok"] = np.array(sc["ok"], dtype=bool)
G["sc_delta"], G["sc_delta_off"] = pack(sc["delta"])
G["sc_line_example"] = np.array(sc["line"][int(np.argmax([len(d) for d in sc["delta"]]))])

# ---- the drop-ins' signatures: parameter names and defaults (repr) --------------------------------------------------
for name in ("molecule_check", "scramble_check"):
    sig = inspect.signature(getattr(fu, name))
    G[f"sig_{name}"] = np.array(json.dumps([[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                                            for p in sig.parameters.values()]))

out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "topology_v1.npz")
np.savez_compressed(out, **G)
print(f"wrote {out}: {len(mc_A)} molecule_check cases, {len(sc['A'])} scramble_check cases, "
      f"{sum(len(d) for d in sc['delta'])} delta bonds")
