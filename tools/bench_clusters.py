#!/usr/bin/env python
"""RMSD similarity clusters (fc_rmsd_clusters) beside the default prune on one MI355X, and the labelling of a caller's
graph (fc_clusters_from_pairs) on its own: one JSON line per case.

  python tools/bench_clusters.py                # 10^4 x 50 clustered (BASELINE configs[1]) and continuous; then
                                                # clusters_from_pairs at 10^6 vertices with 2 x 10^6 and 2 x 10^7 edges
  python tools/bench_clusters.py --trace        # every case once, for rocprofv3 --kernel-trace --stats (no timing)
  python tools/bench_clusters.py --no-graphs    # the resident cases only

What is timed.  Resident cases: ``DeviceEnsemble.prune`` and ``DeviceEnsemble.clusters`` ALTERNATING on one handle in
one process -- windows of ``--steps`` back-to-back calls per mode (default 300), ``--windows`` windows per mode
(default 7), mean and spread over the windows, every shape warmed up first.  The prune is the yardstick because the
cluster call is the same screen and refine with the ladder replaced by the union-find.  Host clock around a window:
every call ends in the library's own stream synchronisation.  Graph cases: windows of ``--graph-steps`` calls (default
5) of the C entry point ``fc_clusters_from_pairs`` on host arrays -- its host-side check of every pair, the upload, the
kernels and the download; the NumPy checks of ``pruner.clusters_from_pairs`` in front of it are left out."""

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

N, A, THR = 10_000, 50, 0.5
GRAPH_N = 1_000_000


def ensembles():
    yield "clustered", syn.synthetic_ensemble(N, A, seed=2)[0]  # BASELINE configs[1]
    yield "continuous", syn.continuous_ensemble(N, A, seed=11)


def window(ens, clusters, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        out = ens.clusters(THR, 2 * THR) if clusters else ens.prune(THR, 2 * THR)
    return 1e3 * (time.perf_counter() - t0) / steps, out


def summary(times):
    t = np.array(times)
    return {"ms_per_call_mean": round(float(t.mean()), 4), "ms_per_call_min": round(float(t.min()), 4),
            "ms_per_call_max": round(float(t.max()), 4)}


def measure(name, X, steps, windows):
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        for clusters in (False, True, False, True):  # warm-up: code objects, pool blocks, the refine's form settles
            window(ens, clusters, 3)
        times = {False: [], True: []}
        last = {}
        for _ in range(windows):
            for clusters in (False, True):
                ms, last[clusters] = window(ens, clusters, steps)
                times[clusters].append(ms)
    mask, pstats = last[False]
    labels, reps, sizes, cstats = last[True]
    out = {"ensemble": name, "N": N, "A": A, "max_rmsd": THR, "steps_per_window": steps, "windows": windows,
           "prune": dict(summary(times[False]), similar=int(pstats[2]), survivors=int(mask.sum())),
           "clusters": dict(summary(times[True]), edges=int(cstats[2]), from_bits=int(cstats[4]), clusters=int(cstats[5]),
                            largest=int(sizes.max()))}
    out["clusters_over_prune"] = round(out["clusters"]["ms_per_call_mean"] / out["prune"]["ms_per_call_mean"], 4)
    p = out["prune"]
    out["prune_spread"] = round((p["ms_per_call_max"] - p["ms_per_call_min"]) / p["ms_per_call_mean"], 4)
    print(json.dumps(out), flush=True)


def random_pairs(n_edges, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, GRAPH_N, size=n_edges, dtype=np.uint64)
    j = (i + rng.integers(1, GRAPH_N, size=n_edges, dtype=np.uint64)) % np.uint64(GRAPH_N)  # never i
    return (i << np.uint64(32)) | j


def measure_graph(n_edges, steps, windows):
    pairs = random_pairs(n_edges, seed=n_edges % 1000)
    def label():
        return fc.pruner._labels_from_graph("fc_clusters_from_pairs", pairs, GRAPH_N)

    label()  # warm-up
    times = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(steps):
            got = label()
        times.append(1e3 * (time.perf_counter() - t0) / steps)
    print(json.dumps(dict({"graph": "random", "vertices": GRAPH_N, "edges": n_edges, "steps_per_window": steps,
                           "windows": windows, "clusters": int(len(got.sizes)), "largest": int(got.sizes.max())},
                          **summary(times))), flush=True)


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
    for name, X in ensembles():
        if args.trace:
            with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
                for clusters in (False, True, False, True):
                    window(ens, clusters, 1)
            continue
        measure(name, X, args.steps, args.windows)
    if args.no_graphs:
        return
    for n_edges in (2_000_000, 20_000_000):
        if args.trace:
            fc.pruner.clusters_from_pairs(random_pairs(n_edges, seed=n_edges % 1000), GRAPH_N)
            continue
        measure_graph(n_edges, args.graph_steps, args.windows)


if __name__ == "__main__":
    main()
