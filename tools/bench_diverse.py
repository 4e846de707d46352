#!/usr/bin/env python
"""RMSD-diverse selection (fc_ensemble_select_diverse) on one MI355X: one JSON line per workload.

  python tools/bench_diverse.py              # the sizes of DESIGN.md section 10 (10^4 x 50 at n = 100 / 1 000,
                                             # 10^5 x 50 at n = 1 000, the stop_rmsd = 0.5 cover of 10^4 x 50)
  python tools/bench_diverse.py --lanes      # both step-kernel forms (FC_DIVERSE_LANES=1 / 8) over N: the crossover
  python tools/bench_diverse.py --trace      # the 10^4 / n = 1 000 and 10^5 / n = 1 000 selections once each, for
                                             # rocprofv3 --kernel-trace --stats (no timing of its own)
  python tools/bench_diverse.py --summary KERNEL_TRACE.csv   # kernel time against launch gaps per selection

Device time: HIP events on the library's stream from the first step's launch to the end of the last (a warm-up
selection first, then the mean of 3).  The NumPy oracle's time for the same alignments is EXTRAPOLATED from a timed
sample of its stacked form (oracle.cpu_ref.rmsd_and_max_batch) and labelled so.
"""

import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import firecode_amd as fc  # noqa: E402
from firecode_amd import synthetic as syn  # noqa: E402

A = 50
_oracle_s_per_alignment = None


def oracle_rate():
    """seconds per alignment of the NumPy oracle at A = 50, timed on a sample of 20 000 pairs"""
    global _oracle_s_per_alignment
    if _oracle_s_per_alignment is None:
        from oracle import cpu_ref as o

        X = syn.continuous_ensemble(2000, A, seed=5)
        P, Q = X[np.arange(20000) % 2000], X[(np.arange(20000) * 7 + 1) % 2000]
        t0 = time.perf_counter()
        o.rmsd_and_max_batch(P, Q, center=True)
        _oracle_s_per_alignment = (time.perf_counter() - t0) / 20000
    return _oracle_s_per_alignment


def measure(name, X, n, stop_rmsd=None, reps=3, with_oracle=True):
    N = X.shape[0]
    ens = fc.DeviceEnsemble(X, atom_mask=np.ones(X.shape[1], bool), center=True)
    try:
        ens.bench_select_diverse(n, stop_rmsd=stop_rmsd, reps=1)  # warm-up: code objects, pool blocks
        dev, host, idx, lanes = ens.bench_select_diverse(n, stop_rmsd=stop_rmsd, reps=reps)
        Npad = -(-N // 64) * 64  # Xs is [(a*3+c)*Npad + n]: one atom pass reads 3 A Npad doubles
    finally:
        ens.close()
    K = len(idx)
    aligned = N * K - K * (K - 1) // 2  # step k skips the k representatives selected before it
    out = {"workload": name, "N": N, "A": X.shape[1], "n_max": n, "stop_rmsd": stop_rmsd, "selected": K,
           "lanes_per_conformer": lanes,
           "ms_device": round(dev, 4), "ms_host_call": round(host, 4), "us_per_step": round(1e3 * dev / K, 3),
           "alignments": aligned, "alignments_per_s": aligned / (dev * 1e-3),
           "xs_bytes_per_atom_pass": 3 * X.shape[1] * Npad * 8}
    out["xs_first_pass_TBps"] = out["xs_bytes_per_atom_pass"] * K / (dev * 1e-3) / 1e12
    if with_oracle:
        out["numpy_oracle_s_EXTRAPOLATED"] = round(aligned * oracle_rate(), 2)
        out["speedup_vs_oracle_extrapolated"] = round(aligned * oracle_rate() / (dev * 1e-3), 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    fc.init(0)
    fc._lib.warmup()
    X4 = syn.continuous_ensemble(10_000, A, seed=11)
    X5 = syn.continuous_ensemble(100_000, A, seed=12)
    if "--trace" in sys.argv:
        for X, n in ((X4, 1000), (X5, 1000)):
            with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
                ens.select_diverse(n)
        return
    if "--lanes" in sys.argv:
        for N in (1000, 3000, 10_000, 30_000, 100_000):
            X = X5[:N]
            for lanes in ("1", "8"):
                os.environ["FC_DIVERSE_LANES"] = lanes
                measure(f"lanes {lanes}", X, 200, with_oracle=False)
        os.environ.pop("FC_DIVERSE_LANES", None)
        return
    measure("10^4 x 50, n = 100", X4, 100)
    measure("10^4 x 50, n = 1 000", X4, 1000)
    measure("10^5 x 50, n = 1 000", X5, 1000)
    measure("10^4 x 50 cover, stop_rmsd = 0.5", X4, 10_000, stop_rmsd=0.5)


def summary(path):
    """per selection in a kernel trace (k_diverse_step launches grouped where the gap exceeds 1 ms): launches, span,
    summed kernel time and the idle gaps between consecutive launches"""
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))
                if "k_diverse_step" in r["Kernel_Name"])
    runs, cur = [], [ev[0]]
    for e in ev[1:]:
        if e[0] - cur[-1][1] > 1_000_000:
            runs.append(cur)
            cur = []
        cur.append(e)
    runs.append(cur)
    for r in runs:
        busy = sum(e - s for s, e in r)
        span = r[-1][1] - r[0][0]
        dur = np.array([e - s for s, e in r]) / 1e3
        print(json.dumps({"launches": len(r), "span_ms": span / 1e6, "kernel_ms": busy / 1e6,
                          "gap_ms": (span - busy) / 1e6, "kernel_share": busy / span,
                          "kernel_us_median": float(np.median(dur)), "gap_us_median":
                          float(np.median([r[i + 1][0] - r[i][1] for i in range(len(r) - 1)] or [0]) / 1e3)}))


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(sys.argv[sys.argv.index("--summary") + 1])
    else:
        main()
