#!/usr/bin/env python
"""Density-based RMSD clusters (fc_rmsd_dbscan, min_samples = 5) beside the similarity clusters (fc_rmsd_clusters) on one
MI355X, and the labelling of a caller's graph (fc_dbscan_from_pairs beside fc_clusters_from_pairs): one JSON line per case.

  python tools/bench_dbscan.py                # 10^4 x 50 clustered (BASELINE configs[1]) and continuous; then the graph
                                              # forms at 10^6 vertices with 2 x 10^6 and 2 x 10^7 edges
  python tools/bench_dbscan.py --trace        # one continuous dbscan call behind a warm-up, for rocprofv3 --kernel-trace
  python tools/bench_dbscan.py --no-graphs    # the resident cases only

What is timed, exactly as tools/bench_clusters.py times it.  Resident cases: ``DeviceEnsemble.clusters`` and
``DeviceEnsemble.dbscan`` ALTERNATING on one handle in one process -- windows of ``--steps`` back-to-back calls per mode
(default 300), ``--windows`` windows per mode (default 7), mean and spread over the windows, every shape warmed up
first.  The cluster call is the yardstick: the same screen, refine and union-find without the degree pass, the attach
words and the two extra result arrays.  Host clock around a window: every call ends in the library's own stream
synchronisation.  Graph cases: windows of ``--graph-steps`` calls (default 5) of the two C entry points on the same
host array of distinct pairs, alternating."""

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
GRAPH_N = 1_000_000


def ensembles():
    yield "clustered", syn.synthetic_ensemble(N, A, seed=2)[0]  # BASELINE configs[1]
    yield "continuous", syn.continuous_ensemble(N, A, seed=11)


def window(ens, dbscan, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        out = ens.dbscan(THR, 2 * THR, M) if dbscan else ens.clusters(THR, 2 * THR)
    return 1e3 * (time.perf_counter() - t0) / steps, out


def summary(times):
    t = np.array(times)
    return {"ms_per_call_mean": round(float(t.mean()), 4), "ms_per_call_min": round(float(t.min()), 4),
            "ms_per_call_max": round(float(t.max()), 4)}


def measure(name, X, steps, windows):
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        for dbscan in (False, True, False, True):  # warm-up: code objects, pool blocks, the refine's form settles
            window(ens, dbscan, 3)
        times = {False: [], True: []}
        last = {}
        for _ in range(windows):
            for dbscan in (False, True):
                ms, last[dbscan] = window(ens, dbscan, steps)
                times[dbscan].append(ms)
    _, _, csizes, cstats = last[False]
    labels, _, sizes, core, degrees, stats = last[True]
    out = {"ensemble": name, "N": N, "A": A, "max_rmsd": THR, "min_samples": M, "steps_per_window": steps, "windows": windows,
           "clusters": dict(summary(times[False]), edges=int(cstats[2]), from_bits=int(cstats[4]), clusters=int(cstats[5]),
                            largest=int(csizes.max())),
           "dbscan": dict(summary(times[True]), edges=int(stats[2]), from_bits=int(stats[4]), clusters=int(stats[5]),
                          largest=int(sizes.max()) if len(sizes) else 0, core=int(stats[6]), noise=int(stats[7]),
                          largest_degree=int(degrees.max()))}
    out["dbscan_over_clusters"] = round(out["dbscan"]["ms_per_call_mean"] / out["clusters"]["ms_per_call_mean"], 4)
    c = out["clusters"]
    out["clusters_spread"] = round((c["ms_per_call_max"] - c["ms_per_call_min"]) / c["ms_per_call_mean"], 4)
    print(json.dumps(out), flush=True)


def random_pairs(n_edges, seed):
    """distinct unordered pairs, (min, max) order"""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, GRAPH_N, size=n_edges, dtype=np.uint64)
    j = (i + rng.integers(1, GRAPH_N, size=n_edges, dtype=np.uint64)) % np.uint64(GRAPH_N)  # never i
    return np.unique((np.minimum(i, j) << np.uint64(32)) | np.maximum(i, j))


def measure_graph(n_edges, steps, windows):
    pairs = random_pairs(n_edges, seed=n_edges % 1000)
    calls = {False: lambda: fc.pruner._labels_from_graph("fc_clusters_from_pairs", pairs, GRAPH_N),
             True: lambda: fc.pruner._labels_from_graph("fc_dbscan_from_pairs", pairs, GRAPH_N, M)}
    times = {False: [], True: []}
    got = {}
    for dbscan in (False, True):  # warm-up
        calls[dbscan]()
    for _ in range(windows):
        for dbscan in (False, True):
            t0 = time.perf_counter()
            for _ in range(steps):
                got[dbscan] = calls[dbscan]()
            times[dbscan].append(1e3 * (time.perf_counter() - t0) / steps)
    out = {"graph": "random", "vertices": GRAPH_N, "edges": int(len(pairs)), "min_samples": M, "steps_per_window": steps,
           "windows": windows, "clusters": dict(summary(times[False]), clusters=int(len(got[False].sizes))),
           "dbscan": dict(summary(times[True]), clusters=int(len(got[True].sizes)), core=int(got[True].core.sum()),
                          noise=int((got[True].labels < 0).sum()))}
    out["dbscan_over_clusters"] = round(out["dbscan"]["ms_per_call_mean"] / out["clusters"]["ms_per_call_mean"], 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--graph-steps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-graphs", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    if args.trace:
        X = dict(ensembles())["continuous"]
        with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
            for dbscan in (False, True, False, True):
                window(ens, dbscan, 1)
        return
    for name, X in ensembles():
        measure(name, X, args.steps, args.windows)
    if args.no_graphs:
        return
    for n_edges in (2_000_000, 20_000_000):
        measure_graph(n_edges, args.graph_steps, args.windows)


if __name__ == "__main__":
    main()
