#!/usr/bin/env python
"""Symmetry- and mirror-aware medoid sums and silhouettes (fc_ensemble_medoids_perm, fc_ensemble_silhouette_perm) on one
MI355X beside their two yardsticks: one JSON line per (ensemble, table).

  python tools/bench_medoids_sym.py                                  # 10 000 x 50 and 600 x 80, clustered and continuous
  python tools/bench_medoids_sym.py --sizes 600x80 --tables K6m      # one size, one table
  python tools/bench_medoids_sym.py --trace                          # one call of each behind a warm-up, for a kernel trace
  python tools/bench_medoids_sym.py --filter-study --tables K2,K6m --steps 5 --windows 3
                                                                     # filter on / off, disguised ensemble / as it comes

What is timed.  HIP events around the kernels, as the entry points report them (``want_ms``): k_group_sums_sym with the
zeroing of its outputs over ONE group of all conformers (the whole upper triangle), and k_silhouette_tile_sym with
k_silhouette_join under the labels ``i % 7`` (the full square).  Beside them, ALTERNATING window by window on one handle in
one process, every mode warmed up first:
  (a) the plain kernels (``medoids`` / ``silhouette``) on the same ensemble and labels;
  (b) ``DeviceEnsemble.bench_knn(k=1, symmetry=, prune_enantiomers=)`` under ``FC_KNN_FILTER=0``: the same N^2 ordered
      pairs with every (permutation, handedness) through the covariance and the explicit pass, and a list of one.
Windows of ``--steps`` calls (their mean), ``--windows`` windows per mode, median (min - max) over the windows.  The two
counters of one call -- (pair, p, h) whose eigenvalue was formed, and those taken through the explicit pass -- go with
every line.  The ensembles: ``synthetic_ensemble`` / ``continuous_ensemble`` with a random half of the conformers
relabelled by a random row of the table and, with the flag, a random half reflected.  Tables: K2 (a path's reversal),
K6 (three blocks of (A - 1) // 3 atoms permuted as wholes), K6m (K6 with the flag)."""

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


def table(kind, A):
    if kind == "K2":
        return np.stack([np.arange(A), np.arange(A)[::-1]])
    size, rows = (A - 1) // 3, []
    for order in itertools.permutations(range(3)):
        row = np.arange(A)
        for m, src in enumerate(order):
            row[1 + m * size:1 + (m + 1) * size] = np.arange(1 + src * size, 1 + (src + 1) * size)
        rows.append(row)
    return np.array(rows)


def disguised(X, t, mirror, seed=3):
    """a random half relabelled by a random non-identity row of the table, a random half reflected with the flag"""
    rng = np.random.default_rng(seed)
    Y = np.array(X, dtype=np.float64)
    for n in np.flatnonzero(rng.random(len(Y)) < 0.5):
        Y[n] = Y[n][t[rng.integers(1, len(t))]]
    if mirror:
        Y[rng.random(len(Y)) < 0.5, :, 0] *= -1.0
    return np.ascontiguousarray(Y)


def summary(times):
    t = np.array(times)
    return {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4)}


def knn_unfiltered(ens, steps, kw):
    os.environ["FC_KNN_FILTER"] = "0"
    try:
        return ens.bench_knn(1, reps=steps, **kw)[0]
    finally:
        os.environ.pop("FC_KNN_FILTER", None)


def mean_ms(call, steps, at):
    return float(np.mean([call()[at] for _ in range(steps)]))


def measure(name, X0, kind, steps, windows):
    N, A = X0.shape[:2]
    mirror = kind.endswith("m")
    t = table(kind[:2], A)
    X = disguised(X0, t, mirror)
    kw = dict(symmetry=t, prune_enantiomers=mirror)
    out = {"ensemble": name, "N": N, "A": A, "table": kind, "K": len(t), "mirror": mirror, "steps_per_window": steps,
           "windows": windows}
    mod7 = (np.arange(N) % 7).astype(np.int32)
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        calls = {"knn_k1_sym_unfiltered": lambda: knn_unfiltered(ens, steps, kw),
                 "medoids_plain": lambda: mean_ms(lambda: ens.medoids(None, want_ms=True), steps, 6),
                 "medoids_sym": lambda: mean_ms(lambda: ens.medoids_sym(None, want_ms=True, **kw), steps, 6),
                 "silhouette_plain": lambda: mean_ms(lambda: ens.silhouette(mod7, want_ms=True), steps, 7),
                 "silhouette_sym": lambda: mean_ms(lambda: ens.silhouette_sym(mod7, want_ms=True, **kw), steps, 7)}
        for f in calls.values():
            f()
        times = {m: [] for m in calls}
        for _ in range(windows):
            for m, f in calls.items():
                times[m].append(f())
        out.update({m: summary(v) for m, v in times.items()})
        b = out["knn_k1_sym_unfiltered"]["ms_median"]
        for m in ("medoids", "silhouette"):
            out[m + "_sym_over_knn"] = round(out[m + "_sym"]["ms_median"] / b, 4)
            out[m + "_sym_over_plain"] = round(out[m + "_sym"]["ms_median"] / out[m + "_plain"]["ms_median"], 4)
        formed, explicit = ens.medoids_sym(None, want_ms=True, **kw)[7]
        out["medoids_formed"], out["medoids_explicit"] = formed, explicit
        formed, explicit = ens.silhouette_sym(mod7, want_ms=True, **kw)[8]
        out["silhouette_formed"], out["silhouette_explicit"] = formed, explicit
        out["knn_formed_explicit"] = list(ens.bench_knn(1, reps=1, **kw)[3])
        out["score_mod7_sym"] = round(ens.silhouette_sym(mod7, **kw)[6], 6)
        out["score_mod7_plain"] = round(ens.silhouette(mod7)[6], 6)
    print(json.dumps(out), flush=True)


def filter_study(name, X0, kind, steps, windows):
    """the two kernels with the filter on (the default) and off (FC_MEDOID_SYM_FILTER=0), on the disguised ensemble and on
    the ensemble as it comes -- one labelling, one handedness: the case the filter is for; the outputs must not differ"""
    N, A = X0.shape[:2]
    mirror = kind.endswith("m")
    t = table(kind[:2], A)
    kw = dict(symmetry=t, prune_enantiomers=mirror)
    mod7 = (np.arange(N) % 7).astype(np.int32)
    for disguise in (True, False):
        X = disguised(X0, t, mirror) if disguise else np.ascontiguousarray(X0)
        out = {"study": "filter", "ensemble": name, "N": N, "A": A, "table": kind, "disguised": disguise}
        with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
            first = None
            for flt in ("on", "off"):
                if flt == "off":
                    os.environ["FC_MEDOID_SYM_FILTER"] = "0"
                try:
                    ens.medoids_sym(None, **kw), ens.silhouette_sym(mod7, **kw)  # (warm)
                    tm = [mean_ms(lambda: ens.medoids_sym(None, want_ms=True, **kw), steps, 6) for _ in range(windows)]
                    ts = [mean_ms(lambda: ens.silhouette_sym(mod7, want_ms=True, **kw), steps, 7) for _ in range(windows)]
                    m, s = ens.medoids_sym(None, want_ms=True, **kw), ens.silhouette_sym(mod7, want_ms=True, **kw)
                finally:
                    os.environ.pop("FC_MEDOID_SYM_FILTER", None)
                out["medoids_" + flt], out["silhouette_" + flt] = summary(tm), summary(ts)
                out["medoids_explicit_over_formed_" + flt] = round(m[7][1] / m[7][0], 4)
                out["silhouette_explicit_over_formed_" + flt] = round(s[8][1] / s[8][0], 4)
                bits = (m[4], m[5], s[1], s[2], s[3])
                first = bits if first is None else first
                out["same_bits"] = all(np.array_equal(x, y) for x, y in zip(bits, first))
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="10000x50,600x80")
    ap.add_argument("--tables", default="K2,K6,K6m")
    ap.add_argument("--ensembles", default="clustered,continuous")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--filter-study", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    if args.trace:
        X0 = syn.continuous_ensemble(10_000, 50, seed=11)
        t = table("K6", 50)
        with fc.DeviceEnsemble(disguised(X0, t, True), center=True) as ens:
            for _ in range(2):
                ens.medoids_sym(None, symmetry=t, prune_enantiomers=True)
                ens.silhouette_sym(np.arange(10_000) % 7, symmetry=t, prune_enantiomers=True)
        return
    for size in args.sizes.split(","):
        N, A = (int(v) for v in size.split("x"))
        for name in args.ensembles.split(","):
            X0 = syn.synthetic_ensemble(N, A, seed=2)[0] if name == "clustered" else syn.continuous_ensemble(N, A, seed=11)
            for kind in args.tables.split(","):
                (filter_study if args.filter_study else measure)(name, X0, kind, args.steps, args.windows)


if __name__ == "__main__":
    main()
