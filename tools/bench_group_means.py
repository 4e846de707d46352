#!/usr/bin/env python
"""Group means under the RMSD (fc_ensemble_group_means) on one MI355X beside two baselines measured in the same run:
one JSON line per case.

  python tools/bench_group_means.py            # 10 000 x 50: one group, the Butina clusters, the continuous ensemble
  python tools/bench_group_means.py --trace    # one call per case behind a warm-up, for rocprofv3 --kernel-trace --stats

What is timed, per case, on one handle in one process:
  * the kernels of a call (HIP events from the first launch to the last, as fc_ensemble_group_means reports them) at
    ``tol=1e-9, max_iter=50``, with the turns the groups took;
  * the kernels per turn: calls at a fixed count (``tol=0``), ``(ms(8 turns) - ms(0 turns)) / 8`` -- every group turns
    all 8 times, so this is the cost of a turn over the WHOLE ensemble: align and rotate, chunk sums, combine;
  * the arithmetic floor of a turn: one step of ``select_diverse`` at the same size (``bench_select_diverse``: one
    alignment of all N conformers against one structure, no rotated coordinates written, nothing reduced), taken as
    ``(ms(65 steps) - ms(1 step)) / 64``;
  * host arrays in -> results out (``group_means_by_rmsd``, the upload and the downloads included; with
    ``aligned=True``: the superposed block as well);
  * the host route: the same turns as a NumPy loop of stacked SVDs (``tests/group_mean_ref.py`` is the per-member
    form; this one is vectorised per group, the fastest NumPy can do), one run.
Medians over ``--windows`` windows, the spread beside them."""

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


def host_ms(f, reps):
    f()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append(1e3 * (time.perf_counter() - t0))
    return summary(times)


def numpy_group_means(Xp, labels, max_iter, tol):
    """the contract's turns on the host: stacked SVDs per group -> (turns per group, milliseconds)"""
    t0 = time.perf_counter()
    turns = []
    for g in range(int(labels.max()) + 1):
        mem = Xp[labels == g]
        if len(mem) < 2:
            turns.append(0)
            continue
        M, n = mem[0].copy(), 0
        for n in range(1, max_iter + 1):
            B = np.einsum("ai,naj->nij", M, mem)
            u, _, vh = np.linalg.svd(B)
            flip = np.linalg.det(u @ vh) < 0
            u[flip, :, -1] *= -1.0
            M_new = np.einsum("nij,naj->ai", u @ vh, mem) / len(mem)
            c = np.sqrt(((M_new - M) ** 2).sum() / M.shape[0])
            M = M_new
            if c <= tol:
                break
        turns.append(n)
    return turns, 1e3 * (time.perf_counter() - t0)


def measure(name, X, labels, windows):
    N, A = X.shape[:2]
    atoms = np.array(["C"] * A)
    lab = np.zeros(N, dtype=np.int32) if labels is None else labels
    sizes = np.bincount(lab[lab >= 0])
    out = {"case": name, "N": N, "A": A, "groups": int((sizes > 0).sum()), "largest": int(sizes.max()), "windows": windows}
    with fc.DeviceEnsemble(X, atom_mask=np.ones(A, bool), center=True) as ens:
        kernel = lambda **kw: ens.group_means(labels, want_ms=True, **kw)  # noqa: E731
        kernel()
        call = [kernel() for _ in range(windows)]
        out["kernels_per_call"] = summary([c[7] for c in call])
        out["turns_max"], out["turns_mean"] = int(call[0][5].max()), round(float(call[0][5][sizes >= 2].mean()), 2)
        per_turn = [(kernel(max_iter=8, tol=0.0)[7] - kernel(max_iter=0)[7]) / 8 for _ in range(windows)]
        out["kernels_per_turn"] = summary(per_turn)
        out["final_pass"] = summary([kernel(max_iter=0)[7] for _ in range(windows)])
        step = [(ens.bench_select_diverse(65, reps=1)[0] - ens.bench_select_diverse(1, reps=1)[0]) / 64 for _ in range(windows)]
        out["select_diverse_step"] = summary(step)
        out["turn_over_step"] = round(out["kernels_per_turn"]["ms_median"] / out["select_diverse_step"]["ms_median"], 2)
        out["resident_call"] = host_ms(lambda: ens.group_means(labels), windows)
    out["host_arrays_in"] = host_ms(lambda: fc.pruner.group_means_by_rmsd(X, atoms, labels, heavy_atoms_only=False), 3)
    out["host_arrays_in_aligned"] = host_ms(
        lambda: fc.pruner.group_means_by_rmsd(X, atoms, labels, heavy_atoms_only=False, aligned=True), 3)
    turns, ms = numpy_group_means(X - X.mean(axis=1, keepdims=True), lab, 50, 1e-9)
    out["numpy_loop"] = {"ms": round(ms, 1), "turns_max": int(max(turns))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    fc.init(0)
    fc._lib.warmup()
    clustered = syn.synthetic_ensemble(10_000, 50, seed=2)[0]  # BASELINE configs[1]
    continuous = syn.continuous_ensemble(10_000, 50, seed=11)
    with fc.DeviceEnsemble(clustered, center=True) as ens:
        butina = ens.butina(THR, 2 * THR)[0]
    cases = (("one group (clustered ensemble)", clustered, None), ("butina clusters", clustered, butina),
             ("one group (continuous ensemble)", continuous, None))
    if args.trace:
        for _, X, labels in cases:
            with fc.DeviceEnsemble(X, center=True) as ens:
                for _ in range(3):
                    ens.group_means(labels)
        return
    for name, X, labels in cases:
        measure(name, X, labels, args.windows)


if __name__ == "__main__":
    main()
