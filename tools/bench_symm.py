#!/usr/bin/env python
"""Symmetry-aware RMSD prune (fc_prune_rmsd_perm) beside the default prune on one MI355X: one JSON line per ensemble and K.

  python tools/bench_symm.py                 # the ensembles of DESIGN.md section 14: 10^4 x 50 clustered (BASELINE
                                             # configs[1]) and continuous, at K = 1, 2 and 6 permutations; for K > 1 a
                                             # random half of the conformers is relabelled by a random non-identity row
  python tools/bench_symm.py --trace         # every ensemble pruned once per mode, for rocprofv3 --kernel-trace --stats

What is timed: the resident prune call (DeviceEnsemble.prune: for the default the screen, exact refine and ladder; for
symmetry= the one all-pairs kernel and the ladder; one host wait each), default and symmetry-aware ALTERNATING on the same
handle in one process -- windows of ``--steps`` back-to-back calls per mode, ``--windows`` windows per mode, mean and
spread over the windows, every shape warmed up first.  Host clock around a window, as tools/bench_enant.py.

Two yardsticks are printed beside every measured value: the default prune of the same ensemble, and the kernel's
arithmetic floor -- K N^2/2 A 9 fp64 multiply-adds at 64 per CU and clock, at ``--clock-mhz`` (give the clock the chip
held during the run; the default is the 2400 MHz peak, so the floor printed is a lower bound of the floor)."""

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
FMA_PER_CU_CLOCK = 64  # fp64 vector multiply-adds of one CU per clock (4 SIMDs x 16 lanes)


def tables():
    ident = np.arange(A)
    yield 1, ident[None]
    yield 2, np.stack([ident, ident[::-1]])
    import itertools

    rows = []
    for order in itertools.permutations(range(3)):  # three runs of 16 atoms exchanged as wholes, two atoms fixed
        row = ident.copy()
        for m, src in enumerate(order):
            row[1 + 16 * m:17 + 16 * m] = np.arange(1 + 16 * src, 17 + 16 * src)
        rows.append(row)
    yield 6, np.array(rows)


def ensembles():
    clustered, _, _ = syn.synthetic_ensemble(N, A, seed=2)  # BASELINE configs[1]
    continuous = syn.continuous_ensemble(N, A, seed=11)
    for name, X in (("clustered", clustered), ("continuous", continuous)):
        for K, table in tables():
            Y = X.copy()
            if K > 1:
                rng = np.random.default_rng(100)
                for n in np.flatnonzero(rng.random(N) < 0.5):
                    Y[n] = Y[n][table[rng.integers(1, K)]]
            yield f"{name}, K = {K}" + (", half relabelled" if K > 1 else ""), Y, table


def window(ens, table, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        mask, stats = ens.prune(THR, 2 * THR, symmetry=table)
    return 1e3 * (time.perf_counter() - t0) / steps, mask, stats


def measure(name, X, table, steps, windows, clock_mhz, n_cu):
    K = len(table)
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        for mode in (None, table, None, table):  # warm-up: code objects, pool blocks, the refine's form settles
            window(ens, mode, 2)
        times = {False: [], True: []}
        last = {}
        for _ in range(windows):
            for sym in (False, True):
                ms, mask, stats = window(ens, table if sym else None, steps)
                times[sym].append(ms)
                last[sym] = (int(mask.sum()), [int(s) for s in stats])
    floor_ms = 1e3 * K * (N * (N - 1) / 2) * A * 9 / (FMA_PER_CU_CLOCK * n_cu * clock_mhz * 1e6)
    out = {"ensemble": name, "N": N, "A": A, "K": K, "max_rmsd": THR, "steps_per_window": steps, "windows": windows,
           "arithmetic_floor_ms": round(floor_ms, 4), "clock_mhz": clock_mhz, "n_cu": n_cu}
    for sym, key in ((False, "default"), (True, "symmetry")):
        t = np.array(times[sym])
        survivors, stats = last[sym]
        out[key] = {"ms_per_call_mean": round(float(t.mean()), 4), "ms_per_call_min": round(float(t.min()), 4),
                    "ms_per_call_max": round(float(t.max()), 4), "candidates": stats[1], "similar": stats[2],
                    "grey": stats[3], "survivors": survivors}
    out["symmetry_over_default"] = round(out["symmetry"]["ms_per_call_mean"] / out["default"]["ms_per_call_mean"], 3)
    out["symmetry_over_floor"] = round(out["symmetry"]["ms_per_call_mean"] / floor_ms, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    n_cu = int(fc.device_info()["n_cu"])
    for name, X, table in ensembles():
        if args.trace:
            with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
                for mode in (None, table, None, table):
                    ens.prune(THR, 2 * THR, symmetry=mode)
            continue
        measure(name, X, table, args.steps, args.windows, args.clock_mhz, n_cu)


if __name__ == "__main__":
    main()
