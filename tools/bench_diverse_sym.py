#!/usr/bin/env python
"""Symmetry- and mirror-aware RMSD-diverse selection (fc_ensemble_select_diverse_perm) beside the default selection on one
MI355X: one JSON line per ensemble size, K and mirror flag.

  python tools/bench_diverse_sym.py                   # 10^4 x 50 and 10^5 x 50 (continuous), K = 1,
                                                      # 2 and 6 permutations, each with and without mirror images; for
                                                      # K > 1 a random half of the conformers is relabelled by a random
                                                      # non-identity row, with the flag a random half is reflected
  python tools/bench_diverse_sym.py --sizes 10000     # one size

What is timed: ``--picks`` selection steps from conformer 0 (no radius stop: all steps enqueued at once, one host wait),
HIP events on the library's stream from the first step's launch to the end of the last (fc_bench_select_diverse[_perm]),
default and symmetry-aware ALTERNATING on one handle in one process -- windows of ``--steps`` selections per mode,
``--windows`` windows per mode, mean and spread over the windows, both shapes warmed up first.  The yardstick printed beside
every value is the default step of the same run; K x H times it (H = 2 with mirror images) is what K x H default
selections would cost.  ``explicit_share``: the (permutation, handedness) combinations that went on to the rotation and
the explicit deviation pass, of those whose eigenvalue was formed (counted in a selection of its own, not a timed one)."""

import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import firecode_amd as fc  # noqa: E402
from firecode_amd import synthetic as syn  # noqa: E402

A = 50


def tables():
    ident = np.arange(A)
    yield ident[None]
    yield np.stack([ident, ident[::-1]])
    rows = []
    for order in itertools.permutations(range(3)):  # three runs of 16 atoms exchanged as wholes, two atoms fixed
        row = ident.copy()
        for m, src in enumerate(order):
            row[1 + 16 * m:17 + 16 * m] = np.arange(1 + 16 * src, 17 + 16 * src)
        rows.append(row)
    yield np.array(rows)


def ensemble(X, table, mirror):
    Y, rng = X.copy(), np.random.default_rng(100)
    if len(table) > 1:
        for n in np.flatnonzero(rng.random(len(Y)) < 0.5):
            Y[n] = Y[n][table[rng.integers(1, len(table))]]
    if mirror:
        Y[rng.random(len(Y)) < 0.5, :, 0] *= -1.0
    return Y


def measure(X, table, mirror, picks, steps, windows):
    N, K = len(X), len(table)
    kw = {"symmetry": table, "prune_enantiomers": mirror}
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        for _ in range(2):  # warm-up: code objects, pool blocks
            ens.bench_select_diverse(picks, reps=1)
            ens.bench_select_diverse(picks, reps=1, **kw)
        us = {False: [], True: []}
        for _ in range(windows):
            for sym in (False, True):
                dev, _, idx, last = ens.bench_select_diverse(picks, reps=steps, **(kw if sym else {}))
                us[sym].append(1e3 * dev / len(idx))
        formed, explicit = last if K > 1 or mirror else (0, 0)
    out = {"N": N, "A": A, "K": K, "mirror": bool(mirror), "picks": picks, "steps_per_window": steps, "windows": windows,
           "lanes_per_conformer": 8 if N <= 10_000 else 1}
    for sym, key in ((False, "default"), (True, "symmetry")):
        t = np.array(us[sym])
        out[key] = {"us_per_pick_mean": round(float(t.mean()), 3), "us_per_pick_min": round(float(t.min()), 3),
                    "us_per_pick_max": round(float(t.max()), 3), "us_per_pick_std": round(float(t.std()), 3)}
    d = out["default"]["us_per_pick_mean"]
    out["K_times_default_us"] = round(K * d, 3)
    out["KH_times_default_us"] = round(K * (2 if mirror else 1) * d, 3)
    out["symmetry_over_default"] = round(out["symmetry"]["us_per_pick_mean"] / d, 3)
    out["explicit_share"] = round(explicit / formed, 4) if formed else None
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--picks", type=int, default=200)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    for N in args.sizes:
        X = syn.continuous_ensemble(N, A, seed=11 if N <= 10_000 else 12)
        for table in tables():
            for mirror in (False, True):
                measure(ensemble(X, table, mirror), table, mirror, args.picks, args.steps, args.windows)


if __name__ == "__main__":
    main()
