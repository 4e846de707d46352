#!/usr/bin/env python
"""Medoids and k-medoids under the RMSD (fc_ensemble_medoids, fc_ensemble_kmedoids) on one MI355X beside their
yardstick, the unfiltered k-NN: one JSON line per case.

  python tools/bench_medoids.py            # 10 000 x 50 (clustered and continuous) and 600 x 80 (continuous)
  python tools/bench_medoids.py --trace    # one whole-ensemble medoid call behind a warm-up, for rocprofv3 --kernel-trace --stats

What is timed.  The sums kernel (HIP events around k_group_sums and the zeroing of its outputs, as fc_ensemble_medoids
reports them) for the whole ensemble as one group, ALTERNATING window by window, on one handle in one process, with
``DeviceEnsemble.bench_knn(k=1)`` under ``FC_KNN_FILTER=0``: that run takes N^2 ordered pairs through the same
covariance and explicit pass, the medoid takes N (N - 1) / 2 and keeps no lists.  Windows of ``--steps`` calls,
``--windows`` windows per mode, median and spread over the windows, both modes warmed up first.  Then, at 10 000 x 50:
the medoids under the ensemble's Butina labels (kernel and host time of the call), k-medoids with n = 100 (host time of
the call, its assignments, time per assignment), and host arrays in -> result out beside the host route
(``rmsd_values`` plus NumPy: the N x N matrix on the host)."""

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


def summary(times):
    t = np.array(times)
    return {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4)}


def knn_unfiltered(ens, steps):
    os.environ["FC_KNN_FILTER"] = "0"
    try:
        return ens.bench_knn(1, reps=steps)[0]
    finally:
        os.environ.pop("FC_KNN_FILTER", None)


def medoid_kernel(ens, steps, labels=None):
    return float(np.mean([ens.medoids(labels, want_ms=True)[-1] for _ in range(steps)]))


def host_ms(f, reps):
    f()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        times.append(1e3 * (time.perf_counter() - t0))
    return summary(times), out


def measure(name, X, steps, windows, extras):
    N, A = X.shape[:2]
    atoms = np.array(["C"] * A)
    out = {"ensemble": name, "N": N, "A": A, "steps_per_window": steps, "windows": windows}
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        calls = {"knn_k1_unfiltered": lambda: knn_unfiltered(ens, steps), "medoid_one_group": lambda: medoid_kernel(ens, steps)}
        for f in calls.values():
            f()
        times = {m: [] for m in calls}
        for _ in range(windows):
            for m, f in calls.items():
                times[m].append(f())
        out.update({m: summary(t) for m, t in times.items()})
        out["medoid_over_knn"] = round(out["medoid_one_group"]["ms_median"] / out["knn_k1_unfiltered"]["ms_median"], 4)
        out["pairs_per_s"] = round(N * (N - 1) / 2 / (out["medoid_one_group"]["ms_median"] * 1e-3), 0)
        if extras:
            bu = ens.butina(THR, 2 * THR)
            labels = bu[0]
            out["butina_medoids"] = dict(summary([medoid_kernel(ens, steps, labels) for _ in range(windows)]), kernel=True,
                                         groups=int(labels.max()) + 1, largest=int(np.bincount(labels[labels >= 0]).max()))
            out["butina_medoids_call"] = host_ms(lambda: ens.medoids(labels), windows)[0]
            s, km = host_ms(lambda: ens.kmedoids(100), 3)
            out["kmedoids_n100"] = dict(s, n_iter=km[4], ms_per_assignment=round(s["ms_median"] / max(km[4], 1), 4),
                                        cost=round(km[3] * 2.0 ** -32, 6))
            s0, km0 = host_ms(lambda: ens.kmedoids(100, max_iter=0), 3)
            out["kmedoids_n100_start_only"] = dict(s0, cost=round(km0[3] * 2.0 ** -32, 6))
    print(json.dumps(out), flush=True)
    host = {"ensemble": name, "form": "host arrays in"}
    host["medoids_by_rmsd"] = host_ms(lambda: fc.pruner.medoids_by_rmsd(X, atoms, heavy_atoms_only=False), 5)[0]
    if extras:
        def host_route():
            with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as e:
                D = e.rmsd_values()[0]
            D = np.triu(D, 1)
            return int(np.argmin(D.sum(axis=0) + D.sum(axis=1)))

        s, m_host = host_ms(host_route, 2)
        host["rmsd_values_plus_numpy"] = dict(s, medoid=m_host, same_medoid=bool(
            m_host == fc.pruner.medoids_by_rmsd(X, atoms, heavy_atoms_only=False).medoids[0]))
        host["kmedoids_by_rmsd_n100"] = host_ms(lambda: fc.pruner.kmedoids_by_rmsd(X, atoms, 100, heavy_atoms_only=False), 2)[0]
    print(json.dumps(host), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    if args.trace:
        with fc.DeviceEnsemble(syn.continuous_ensemble(10_000, 50, seed=11), center=True) as ens:
            for _ in range(4):
                ens.medoids()
        return
    measure("clustered", syn.synthetic_ensemble(10_000, 50, seed=2)[0], args.steps, args.windows, True)  # BASELINE configs[1]
    measure("continuous", syn.continuous_ensemble(10_000, 50, seed=11), args.steps, args.windows, False)
    measure("continuous", syn.continuous_ensemble(600, 80, seed=680), args.steps, args.windows, False)


if __name__ == "__main__":
    main()
