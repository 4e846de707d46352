#!/usr/bin/env python
"""Enantiomer-aware RMSD prune (fc_prune_rmsd_enant) beside the default prune on one MI355X: one JSON line per ensemble.

  python tools/bench_enant.py                # the four ensembles of DESIGN.md section 12: 10^4 x 50 clustered
                                             # (BASELINE configs[1]) and continuous, each as it is and with a random
                                             # half of the conformers reflected
  python tools/bench_enant.py --trace        # every ensemble pruned once per mode, for rocprofv3 --kernel-trace --stats
                                             # (no timing of its own)

What is timed: the resident prune call (DeviceEnsemble.prune: screen, exact refine, ladder, one host wait), default
and enantiomer-aware ALTERNATING on the same handle in one process -- windows of ``--steps`` back-to-back calls per
mode (default 300: a good fraction of a second), ``--windows`` windows per mode (default 7), mean and spread over
the windows, every shape warmed up first.  Host clock around a window: every call ends in the library's own stream
synchronisation, so a window is device time plus the same launch and wait overhead in both modes.  The enantiomer-aware
prune has no pipelined (twin-workspace) form, so the pipelined default step of bench.py is printed beside it for
reference only (``pipelined_default_ms``); the comparison that means something is between the two call times.
"""

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


def ensembles():
    clustered, _, _ = syn.synthetic_ensemble(N, A, seed=2)  # BASELINE configs[1]
    continuous = syn.continuous_ensemble(N, A, seed=11)
    for name, X, axis in (("clustered", clustered, 0), ("continuous", continuous, 2)):
        yield name, X
        Y = X.copy()
        Y[np.random.default_rng(100).random(N) < 0.5, :, axis] *= -1.0
        yield name + ", half reflected", Y


def window(ens, enant, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        mask, stats = ens.prune(THR, 2 * THR, prune_enantiomers=enant)
    return 1e3 * (time.perf_counter() - t0) / steps, mask, stats


def measure(name, X, steps, windows):
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        for enant in (False, True, False, True):  # warm-up: code objects, pool blocks, the refine's form settles
            window(ens, enant, 3)
        times = {False: [], True: []}
        last = {}
        for _ in range(windows):
            for enant in (False, True):
                ms, mask, stats = window(ens, enant, steps)
                times[enant].append(ms)
                last[enant] = (int(mask.sum()), [int(s) for s in stats])
        kind = fc._lib.screen_last_kind()
        _, pipelined, _, _ = ens.bench_prune(THR, 2 * THR, reps=steps, want_mask=False)
    out = {"ensemble": name, "N": N, "A": A, "max_rmsd": THR, "steps_per_window": steps, "windows": windows,
           "screen_kind": kind, "pipelined_default_ms": round(pipelined, 4)}
    for enant, key in ((False, "default"), (True, "enant")):
        t = np.array(times[enant])
        survivors, stats = last[enant]
        out[key] = {"ms_per_call_mean": round(float(t.mean()), 4), "ms_per_call_min": round(float(t.min()), 4),
                    "ms_per_call_max": round(float(t.max()), 4), "candidates": stats[1], "similar": stats[2],
                    "grey": stats[3], "survivors": survivors}
    out["enant_over_default"] = round(out["enant"]["ms_per_call_mean"] / out["default"]["ms_per_call_mean"], 4)
    spread = (out["default"]["ms_per_call_max"] - out["default"]["ms_per_call_min"]) / out["default"]["ms_per_call_mean"]
    out["default_spread"] = round(spread, 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    for name, X in ensembles():
        if args.trace:
            with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
                for enant in (False, True, False, True):
                    ens.prune(THR, 2 * THR, prune_enantiomers=enant)
            continue
        measure(name, X, args.steps, args.windows)


if __name__ == "__main__":
    main()
