#!/usr/bin/env python
"""Bond-topology check (fc_bond_changes: molecule_check / scramble_check batched) on one MI355X: one JSON line per
workload, the table of DESIGN.md section 11.

  python tools/bench_topology.py                  # host arrays in -> mask out, the bound, the CPU baselines
  python tools/bench_topology.py --trace NAME     # warm-up + 10 calls of one workload and nothing else, for
                                                  # rocprofv3 --kernel-trace --stats (kernel time)
  python tools/bench_topology.py --summary DIR    # the bond kernels of the *_kernel_stats.csv files under DIR
  python tools/bench_topology.py --json OUT.json  # also write the lines to a file

Workloads: 10 000 perturbed catalysts (85 atoms, sigma 0.05) in molecule mode (shared reference), in molecule mode with
one reference per structure, and in scramble mode (two fragment graphs, the atoms of the bonds across the cut
excluded); 100 000 x 50 and 16 x 6 900 synthetic clouds in molecule mode.  Host time: a warm-up call, then mean and
spread of 5.  The bound counts from the shapes: A(A-1)/2 distance tests per structure (twice with per-structure
references), 8 fp64 operations each (3 sub, 3 mul, 2 add: the square root is replaced by a squared threshold);
N A 24 B in (twice with per-structure references) + N 9 B out; peaks 78.6 TFLOP/s fp64 and 8 TB/s HBM as in
DESIGN.md.  CPU baselines on this host, one process: the reference form (graphize + Python sets, firecode/utils.py:
341-400) timed on 200 structures and EXTRAPOLATED to N, and the vectorised NumPy restatement (tests/topology_ref.py)
timed on up to 10 000 structures (extrapolated beyond, and labelled so).
"""

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import firecode_amd as fc  # noqa: E402
from firecode_amd import utils  # noqa: E402
from firecode_amd.torsion_perception import graphize  # noqa: E402

PEAK_F64, PEAK_HBM = 78.6e12, 8.0e12
FLOP_PER_TEST = 8
ELEMENTS = np.array(["C", "H", "N", "O", "S"])
BOND_KERNELS = ("k_bond_changes", "k_bond_counts", "k_excl_bits", "k_bond_tile_offsets")


def workloads():
    g = np.load(os.path.join(ROOT, "tests", "golden", "intree_v1.npz"))
    atoms, X0 = g["fx_catalyst_atoms"], g["fx_catalyst_coords"][0]
    X = X0[None] + np.random.default_rng(7).normal(scale=0.05, size=(10_000,) + X0.shape)
    Xr = X0[None] + np.random.default_rng(8).normal(scale=0.05, size=X.shape)
    cut = 40
    graphs = [graphize(atoms[:cut], X0[:cut]), graphize(atoms[cut:], X0[cut:])]
    crossing = sorted({int(v) for a, b in graphize(atoms, X0).edges if a < cut <= b for v in (a, b)})
    rng = np.random.default_rng(5)
    c50 = rng.uniform(0, (50 / 0.08) ** (1 / 3), size=(50, 3))
    a50 = rng.choice(ELEMENTS, size=50)
    c6900 = rng.uniform(0, (6900 / 0.08) ** (1 / 3), size=(6900, 3))
    a6900 = rng.choice(ELEMENTS, size=6900)
    return {
        "catalyst_10k_molecule": dict(mode="molecule", atoms=atoms, X=X, ref=X0),
        "catalyst_10k_molecule_per_structure": dict(mode="molecule", atoms=atoms, X=X, ref=Xr),
        "catalyst_10k_scramble": dict(mode="scramble", atoms=atoms, X=X, graphs=graphs, excl=crossing),
        "synthetic_100k_x50": dict(mode="molecule", atoms=a50, ref=c50,
                                   X=c50[None] + rng.normal(scale=0.05, size=(100_000, 50, 3))),
        "synthetic_16_x6900": dict(mode="molecule", atoms=a6900, ref=c6900,
                                   X=c6900[None] + rng.normal(scale=0.05, size=(16, 6900, 3))),
    }


def run(w):
    if w["mode"] == "molecule":
        return utils.molecule_check_batch(w["atoms"], w["ref"], w["X"])
    return utils.scramble_check_batch(w["atoms"], w["X"], w["excl"], w["graphs"])


def reference_form(w, n):
    """firecode/utils.py:341-400 as written: graphize + Python sets, one structure at a time (first n structures)"""
    t0 = time.perf_counter()
    if w["mode"] == "molecule":
        shared = w["ref"].ndim == 2
        for k in range(n):
            old = {(a, b) for a, b in graphize(w["atoms"], w["ref"] if shared else w["ref"][k]).edges if a != b}
            new = {(a, b) for a, b in graphize(w["atoms"], w["X"][k]).edges if a != b}
            _ = len((old | new) - (old & new)) <= 0
    else:
        bonds, pos = set(), 0
        for gr in w["graphs"]:
            bonds |= {tuple(sorted((a + pos, b + pos))) for a, b in gr.edges if a != b}
            pos += len(gr.nodes)
        for k in range(n):
            new = {tuple(sorted((a, b))) for a, b in graphize(w["atoms"], w["X"][k]).edges if a != b}
            delta = (bonds | new) - (bonds & new)
            for bond in delta.copy():
                for a in w["excl"]:
                    if a in bond:
                        delta -= {bond}
            _ = len(delta) <= 0
    return (time.perf_counter() - t0) / n


def restatement(w, n):
    import topology_ref as ref

    t0 = time.perf_counter()
    if w["mode"] == "molecule":
        R = w["ref"] if w["ref"].ndim == 2 else w["ref"][:n]
        ref.bond_changes(w["atoms"], w["X"][:n], ref_X=R)
    else:
        edges, _ = ref.graphs_reference(w["graphs"])
        ref.bond_changes(w["atoms"], w["X"][:n], ref_bonds=ref.ref_bits_from_edges(edges, w["X"].shape[1]),
                         excluded=w["excl"])
    return (time.perf_counter() - t0) / n


def measure(name, w, reps=5):
    N, A = w["X"].shape[:2]
    run(w)  # warm-up: code objects, pool blocks
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ok, cnt = run(w)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    per_struct_ref = w["mode"] == "molecule" and w["ref"].ndim == 3
    pairs = N * A * (A - 1) // 2
    tests = pairs * (2 if per_struct_ref else 1)
    bytes_ = N * A * 24 * (2 if per_struct_ref else 1) + N * 9
    t_flop, t_hbm = tests * FLOP_PER_TEST / PEAK_F64, bytes_ / PEAK_HBM
    n_ref = min(N, 200)
    n_vec = min(N, 10_000)
    s_ref, s_vec = reference_form(w, n_ref), restatement(w, n_vec)
    return {"workload": name, "mode": w["mode"], "N": N, "A": A, "pairs": pairs, "distance_tests": tests,
            "bytes_in_out": bytes_, "changed_structures": int((~ok).sum()), "changed_bonds": int(cnt.sum()),
            "host_ms_mean": ts.mean(), "host_ms_std": ts.std(), "host_ms_min": ts.min(), "host_ms_max": ts.max(),
            "host_pairs_per_s": pairs / (ts.mean() / 1e3),
            "binding": "fp64" if t_flop >= t_hbm else "hbm",
            "bound_ms": max(t_flop, t_hbm) * 1e3, "host_frac_of_bound": max(t_flop, t_hbm) / (ts.mean() / 1e3),
            "cpu_reference_form_s": s_ref * N, "cpu_reference_form_extrapolated_from": n_ref,
            "cpu_restatement_s": s_vec * N, "cpu_restatement_extrapolated_from": n_vec if n_vec < N else None}


def summary(path, lines):
    """kernel time per call from the rocprofv3 stats of one --trace run per workload (DIR/NAME/**/*kernel_stats.csv)"""
    out = []
    for name in sorted(os.listdir(path)):
        files = glob.glob(os.path.join(path, name, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        main, total, calls = 0.0, 0.0, 0
        for f in files:
            for r in csv.DictReader(open(f)):
                if any(k in r["Name"] for k in BOND_KERNELS):
                    total += float(r["TotalDurationNs"])
                    if "k_bond_changes" in r["Name"]:
                        main += float(r["TotalDurationNs"])
                        calls += int(r["Calls"])
        rec = {"workload": name, "calls": calls, "kernel_ms_per_call": main / calls / 1e6,
               "bond_kernels_ms_per_call": total / calls / 1e6}
        base = lines.get(name)
        if base:
            t = rec["kernel_ms_per_call"] / 1e3
            rec["kernel_pairs_per_s"] = base["pairs"] / t
            rec["kernel_frac_of_bound"] = base["bound_ms"] / 1e3 / t
            rec["kernel_frac_of_fp64_peak"] = base["distance_tests"] * FLOP_PER_TEST / t / PEAK_F64
            rec["kernel_frac_of_hbm_peak"] = base["bytes_in_out"] / t / PEAK_HBM
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None)
    ap.add_argument("--summary", default=None)
    ap.add_argument("--lines", default=None, help="the JSON file of a plain run, for rates and fractions in --summary")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.summary:
        lines = {r["workload"]: r for r in json.load(open(a.lines))} if a.lines else {}
        for rec in summary(a.summary, lines):
            print(json.dumps(rec))
        return
    fc.init(0)
    W = workloads()
    if a.trace:
        w = W[a.trace]
        for _ in range(11):
            run(w)
        return
    out = []
    for name, w in W.items():
        rec = measure(name, w)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
