#!/usr/bin/env python
"""Sphere-exclusion RMSD clusters (fc_rmsd_butina) beside the similarity clusters (fc_rmsd_clusters) and the
density-based ones (fc_rmsd_dbscan, min_samples = 5) on one MI355X: one JSON line per case.

  python tools/bench_butina.py             # 10^4 x 50 clustered (BASELINE configs[1]) and continuous, resident and
                                           # host arrays in; then the depth worst cases: the 3 000-vertex path and thick path
  python tools/bench_butina.py --trace     # one continuous butina call behind a warm-up, for rocprofv3 --kernel-trace --stats
                                           # (the rounds: k_bu_edges + k_bu_vertices; the finish: k_bu_finish)

What is timed, as tools/bench_dbscan.py times it.  Resident: ``DeviceEnsemble.clusters`` / ``.dbscan`` / ``.butina``
ALTERNATING on one handle in one process, windows of ``--steps`` back-to-back calls per mode, ``--windows`` windows per
mode, median and spread over the windows, every mode warmed up first; butina once per value of ``--rounds``
(FC_BUTINA_ROUNDS; "default" leaves it unset), which moves work between the grid-wide rounds and the one-workgroup
finish and never changes an output.  Host clock around a window: every call ends in the library's own stream
synchronisation.  Host arrays in: ``pruner.cluster_by_rmsd`` / ``dbscan_by_rmsd`` / ``butina_by_rmsd``, single calls."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import firecode_amd as fc  # noqa: E402
from firecode_amd import synthetic as syn  # noqa: E402

N, A, THR, M = 10_000, 50, 0.5, 5


def ensembles():
    yield "clustered", syn.synthetic_ensemble(N, A, seed=2)[0]  # BASELINE configs[1]
    yield "continuous", syn.continuous_ensemble(N, A, seed=11)


def set_rounds(value):
    if value == "default":
        os.environ.pop("FC_BUTINA_ROUNDS", None)
    else:
        os.environ["FC_BUTINA_ROUNDS"] = value


def summary(times):
    t = np.array(times)
    return {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4)}


def windows_of(calls, steps, windows):
    """calls: {mode: function}; the modes alternate window by window -> {mode: (summary, last result)}"""
    for _ in range(2):  # warm-up: code objects, pool blocks, the refine's form settles
        for f in calls.values():
            f()
    times, last = {m: [] for m in calls}, {}
    for _ in range(windows):
        for mode, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                last[mode] = f()
            times[mode].append(1e3 * (time.perf_counter() - t0) / steps)
    return {m: (summary(times[m]), last[m]) for m in calls}


def butina_call(f, rounds):
    def call():
        set_rounds(rounds)
        try:
            return f()
        finally:
            set_rounds("default")
    return call


def measure(name, X, rounds_list, steps, windows):
    atoms = np.array(["C"] * A)
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        calls = {"clusters": lambda: ens.clusters(THR, 2 * THR), "dbscan": lambda: ens.dbscan(THR, 2 * THR, M)}
        for r in rounds_list:
            calls[f"butina[{r}]"] = butina_call(lambda: ens.butina(THR, 2 * THR), r)
        res = windows_of(calls, steps, windows)
    out = {"ensemble": name, "N": N, "A": A, "max_rmsd": THR, "form": "resident", "steps_per_window": steps, "windows": windows}
    for mode, (s, last) in res.items():
        out[mode] = dict(s, edges=int(last[-1][2]), clusters=int(last[-1][5]))
        if mode.startswith("butina"):
            out[mode].update(rounds_needed=int(last[-1][6]), left_to_finish=int(last[-1][7]), largest=int(last[2].max()),
                             singletons=int((last[2] == 1).sum()), largest_degree=int(last[3].max()))
    print(json.dumps(out), flush=True)
    host = windows_of({"cluster_by_rmsd": lambda: fc.pruner.cluster_by_rmsd(X, atoms, THR, heavy_atoms_only=False),
                       "dbscan_by_rmsd": lambda: fc.pruner.dbscan_by_rmsd(X, atoms, THR, min_samples=M, heavy_atoms_only=False),
                       "butina_by_rmsd": lambda: fc.pruner.butina_by_rmsd(X, atoms, THR, heavy_atoms_only=False)},
                      1, max(windows, 5))
    print(json.dumps(dict({"ensemble": name, "form": "host arrays in"}, **{m: s for m, (s, _) in host.items()})), flush=True)


def measure_graph(name, n, ei, ej, rounds_list, steps, windows):
    pairs = (ei.astype(np.uint64) << np.uint64(32)) | ej.astype(np.uint64)
    calls = {"clusters_from_pairs": lambda: fc.pruner.clusters_from_pairs(pairs, n)}
    for r in rounds_list:
        calls[f"butina_from_pairs[{r}]"] = butina_call(lambda: fc.pruner.butina_from_pairs(pairs, n, assume_unique=True), r)
    res = windows_of(calls, steps, windows)
    out = {"graph": name, "vertices": n, "edges": int(len(pairs)), "steps_per_window": steps, "windows": windows}
    out.update({m: dict(s, clusters=int(len(last.sizes))) for m, (s, last) in res.items()})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rounds", default="default,0,2,16,64")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    rounds_list = args.rounds.split(",")
    fc.init(0)
    fc._lib.warmup()
    if args.trace:
        X = dict(ensembles())["continuous"]
        with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
            for _ in range(4):
                ens.butina(THR, 2 * THR)
        return
    for name, X in ensembles():
        measure(name, X, rounds_list, args.steps, args.windows)
    n = 3000
    measure_graph("path", n, np.arange(n - 1), np.arange(1, n), rounds_list, 20, args.windows)
    ei = np.concatenate([np.arange(n - d) for d in range(1, 11)])
    ej = np.concatenate([np.arange(d, n) for d in range(1, 11)])
    measure_graph("thick path (|i - j| <= 10)", n, ei, ej, rounds_list, 20, args.windows)


if __name__ == "__main__":
    main()
