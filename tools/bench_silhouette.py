#!/usr/bin/env python
"""Silhouettes under the RMSD (fc_ensemble_silhouette) on one MI355X beside their yardstick, the unfiltered k-NN: one
JSON line per case.

  python tools/bench_silhouette.py                  # 10 000 x 50 and 600 x 80, clustered and continuous
  python tools/bench_silhouette.py --sizes 600x80   # one size only
  python tools/bench_silhouette.py --trace          # one call behind a warm-up, for rocprofv3 --kernel-trace --stats

What is timed.  The kernel pair (HIP events around k_silhouette_tile and k_silhouette_join with the clearing of the head
records, as fc_ensemble_silhouette reports them) under the ensemble's Butina labels and under ``i % 7``, ALTERNATING
window by window, on one handle in one process, with ``DeviceEnsemble.bench_knn(k=1)`` under ``FC_KNN_FILTER=0``: that
run takes the same N^2 ordered pairs through the same covariance and explicit pass and keeps a list of one; the
silhouette scans instead.  Windows of ``--steps`` calls, ``--windows`` windows per mode, median and spread over the
windows, every mode warmed up first.  Then host arrays in -> result out of ``silhouette_by_rmsd``, and one
``silhouette_scan`` of five thresholds beside five separate ``butina_by_rmsd`` + ``silhouette_by_rmsd`` calls (one
upload instead of ten)."""

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

THR = 0.5
SCAN = [0.1, 0.25, 0.5, 0.75, 1.0]


def summary(times):
    t = np.array(times)
    return {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4)}


def knn_unfiltered(ens, steps):
    os.environ["FC_KNN_FILTER"] = "0"
    try:
        return ens.bench_knn(1, reps=steps)[0]
    finally:
        os.environ.pop("FC_KNN_FILTER", None)


def silhouette_kernel(ens, steps, labels):
    return float(np.mean([ens.silhouette(labels, want_ms=True)[-1] for _ in range(steps)]))


def host_ms(f, reps):
    f()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        times.append(1e3 * (time.perf_counter() - t0))
    return summary(times), out


def measure(name, X, steps, windows):
    N, A = X.shape[:2]
    atoms = np.array(["C"] * A)
    out = {"ensemble": name, "N": N, "A": A, "steps_per_window": steps, "windows": windows}
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        butina = ens.butina(THR, 2 * THR)[0]
        mod7 = (np.arange(N) % 7).astype(np.int32)
        out["butina_groups"] = int(butina.max()) + 1
        out["butina_largest"] = int(np.bincount(butina).max())
        calls = {"knn_k1_unfiltered": lambda: knn_unfiltered(ens, steps),
                 "silhouette_butina": lambda: silhouette_kernel(ens, steps, butina),
                 "silhouette_mod7": lambda: silhouette_kernel(ens, steps, mod7)}
        for f in calls.values():
            f()
        times = {m: [] for m in calls}
        for _ in range(windows):
            for m, f in calls.items():
                times[m].append(f())
        out.update({m: summary(t) for m, t in times.items()})
        for m in ("silhouette_butina", "silhouette_mod7"):
            out[m + "_over_knn"] = round(out[m]["ms_median"] / out["knn_k1_unfiltered"]["ms_median"], 4)
        out["pairs_per_s"] = round(N * (N - 1) / (out["silhouette_mod7"]["ms_median"] * 1e-3), 0)
        out["score_butina"] = round(ens.silhouette(butina)[6], 6)
        out["score_mod7"] = round(ens.silhouette(mod7)[6], 6)
        out["silhouette_call_butina"] = host_ms(lambda: ens.silhouette(butina), windows)[0]
    print(json.dumps(out), flush=True)
    host = {"ensemble": name, "N": N, "A": A, "form": "host arrays in"}
    host["silhouette_by_rmsd_butina"] = host_ms(lambda: fc.pruner.silhouette_by_rmsd(X, atoms, butina, heavy_atoms_only=False), 5)[0]

    def separate():
        return [fc.pruner.silhouette_by_rmsd(X, atoms, fc.pruner.butina_by_rmsd(X, atoms, t, heavy_atoms_only=False).labels,
                                             heavy_atoms_only=False).score for t in SCAN]

    s_scan, recs = host_ms(lambda: fc.pruner.silhouette_scan(X, atoms, SCAN, heavy_atoms_only=False), 3)
    s_sep, scores = host_ms(separate, 3)
    host["silhouette_scan_5"] = dict(s_scan, clusters=[r.n_clusters for r in recs])
    host["separate_calls_5"] = dict(s_sep, same_scores=bool(np.array_equal([r.score for r in recs], scores, equal_nan=True)))
    print(json.dumps(host), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="10000x50,600x80")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    if args.trace:
        with fc.DeviceEnsemble(syn.continuous_ensemble(10_000, 50, seed=11), center=True) as ens:
            for _ in range(4):
                ens.silhouette(np.arange(10_000) % 7)
        return
    for size in args.sizes.split(","):
        N, A = (int(v) for v in size.split("x"))
        measure("clustered", syn.synthetic_ensemble(N, A, seed=2)[0], args.steps, args.windows)
        measure("continuous", syn.continuous_ensemble(N, A, seed=11), args.steps, args.windows)


if __name__ == "__main__":
    main()
