#!/usr/bin/env python
"""k nearest neighbours under the RMSD (fc_ensemble_knn, fc_ensemble_knn_cross and their symmetry-aware forms) on one MI355X: one JSON line per workload.

  python tools/bench_knn.py              # the sizes of DESIGN.md section 18: continuous and clustered ensembles at
                                         # 10^4 x 50 and 10^5 x 50, k = 8 and 64; then, at 10^4 x 50, host arrays in ->
                                         # lists out against the matrix route (rmsd_values + argpartition on the host)
  python tools/bench_knn.py --small      # the 10^4 x 50 workloads and the comparison only
  python tools/bench_knn.py --filter     # the eigenvalue filter against FC_KNN_FILTER=0, alternating, at both sizes
  python tools/bench_knn.py --strips     # the strip count (FC_KNN_STRIPS) over N at k = 8
  python tools/bench_knn.py --trace      # one 10^4 x 50 call at k = 8, for rocprofv3 --kernel-trace --stats
  python tools/bench_knn.py --cross      # fc_ensemble_knn_cross: queries x references at
                                         # 10^4 x 10^4, 10^3 x 10^5 and 10^2 x 10^6, k = 1 and 8, without a cap and with
                                         # the cap at the duplicate threshold; the self form at 10^4, k = 8 beside it;
                                         # then host arrays in -> lists out at 5 000 x 5 000 against the matrix of the
                                         # concatenated 10 000 on the host
  python tools/bench_knn.py --cross --small   # without the 10^2 x 10^6 workload
  python tools/bench_knn.py --symmetry K [--mirror] [--cross]
                                         # fc_ensemble_knn_perm / fc_ensemble_knn_cross_perm at
                                         # 10^4 x 50 (--cross: 10^4 x 10^4 x 50) under a table of K permutations
                                         # (1, 2, 6 or a power of two up to 64) and, --mirror, both handednesses, k = 1 and
                                         # 8 (--cross: without a cap and with the cap at the duplicate threshold): the
                                         # device ms, the default form's ms from the same run alternating on one handle,
                                         # K H times that (the cost of the covariance loops alone), the ratio, and the
                                         # share of (pair, p, h) taken through the explicit pass

Device time: HIP events on the library's stream from the first launch to the end of the merge (a warm-up call first,
then 3 calls: mean and range).  Rates: ordered alignments (N (N - 1): the full square, whether or not a pair's explicit
pass ran) per second; the fp64 flops an unfiltered kernel would spend on them at 2 400 per explicit alignment, the
figure of DESIGN.md section 10, against the vector peak (the kernel's own only with FC_KNN_FILTER=0); first-pass bytes
of the conformer-minor copy (N^2 A 24 / 4: one column load serves the 4 rows of a wavefront) against 8 TB/s.
"""

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
FLOPS_PER_ALIGNMENT = 2400.0
FP64_VECTOR_PEAK = 78.6e12
HBM_PEAK = 8.0e12
ROWS_PER_WAVE = 4


def ensemble(kind, N, seed):
    if kind == "clusters":
        return syn.synthetic_ensemble(N, A, seed=seed)[0]
    return syn.continuous_ensemble(N, A, seed=seed)


def measure(name, X, k, reps=3):
    N = X.shape[0]
    with fc.DeviceEnsemble(X, atom_mask=np.ones(X.shape[1], bool), center=True) as ens:
        ens.bench_knn(k, reps=1)  # warm-up: code objects, pool blocks
        runs = [ens.bench_knn(k, reps=1) for _ in range(reps)]
    dev = np.array([r[0] for r in runs])
    aligned = N * (N - 1)
    s = dev.mean() * 1e-3
    out = {"workload": name, "N": N, "A": X.shape[1], "k": k, "strips": runs[0][2],
           "ms_device_mean": round(float(dev.mean()), 3), "ms_device_min": round(float(dev.min()), 3),
           "ms_device_max": round(float(dev.max()), 3), "ms_host_call_mean": round(float(np.mean([r[1] for r in runs])), 3),
           "ordered_alignments": aligned, "alignments_per_s": aligned / s,
           "unfiltered_fp64_share_of_vector_peak": aligned * FLOPS_PER_ALIGNMENT / s / FP64_VECTOR_PEAK,
           "xs_first_pass_TBps": N * N * X.shape[1] * 24 / ROWS_PER_WAVE / s / 1e12}
    out["xs_share_of_hbm_peak"] = out["xs_first_pass_TBps"] * 1e12 / HBM_PEAK
    print(json.dumps(out), flush=True)
    return out


def matrix_route(X, k):
    """the only route without fc_ensemble_knn: the whole fp64 matrix to the host, argpartition + sort per row"""
    with fc.DeviceEnsemble(X, atom_mask=np.ones(X.shape[1], bool), center=True) as ens:
        R, _ = ens.rmsd_values()
    np.fill_diagonal(R, np.inf)
    part = np.argpartition(R, k - 1, axis=1)[:, :k]
    d = np.take_along_axis(R, part, axis=1)
    order = np.lexsort((part, d), axis=1)
    return np.take_along_axis(part, order, axis=1).astype(np.int32), np.take_along_axis(d, order, axis=1)


def end_to_end(X, k, reps=3):
    """host arrays in -> lists out, the two routes alternating in one process"""
    atoms = np.array(["C"] * X.shape[1])
    fc.pruner.knn_by_rmsd(X, atoms, k), matrix_route(X, k)  # warm-up of both
    t_new, t_old, same = [], [], True
    for _ in range(reps):
        t0 = time.perf_counter()
        nb = fc.pruner.knn_by_rmsd(X, atoms, k)
        t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        idx, _ = matrix_route(X, k)
        t_old.append(time.perf_counter() - t0)
        same = same and bool(np.array_equal(idx, nb.indices))
    print(json.dumps({"workload": f"end to end, {X.shape[0]} x {X.shape[1]}, k = {k}",
                      "knn_by_rmsd_ms": [round(1e3 * t, 2) for t in t_new],
                      "matrix_route_ms": [round(1e3 * t, 2) for t in t_old],
                      "knn_by_rmsd_ms_mean": round(1e3 * float(np.mean(t_new)), 2),
                      "matrix_route_ms_mean": round(1e3 * float(np.mean(t_old)), 2),
                      "same_indices": same}), flush=True)


def split(N_q, N_r, seed):
    """queries and references drawn from one continuous ensemble, shuffled"""
    X = ensemble("continuous", N_q + N_r, seed)
    p = np.random.default_rng(seed).permutation(N_q + N_r)
    return np.ascontiguousarray(X[p[:N_q]]), np.ascontiguousarray(X[p[N_q:]])


def measure_cross(name, q, r, Nq, Nr, k, cap, reps=3):
    q.bench_knn_against(r, k, max_rmsd=cap, reps=1)  # warm-up: code objects, pool blocks
    runs = [q.bench_knn_against(r, k, max_rmsd=cap, reps=1) for _ in range(reps)]
    dev = np.array([x[0] for x in runs])
    s = dev.mean() * 1e-3
    idx, _ = q.knn_against(r, k, max_rmsd=cap)
    out = {"workload": name, "Nq": Nq, "Nr": Nr, "A": A, "k": k, "max_rmsd": cap, "strips": runs[0][2],
           "ms_device_mean": round(float(dev.mean()), 3), "ms_device_min": round(float(dev.min()), 3),
           "ms_device_max": round(float(dev.max()), 3), "ms_host_call_mean": round(float(np.mean([x[1] for x in runs])), 3),
           "ordered_alignments": Nq * Nr, "alignments_per_s": Nq * Nr / s,
           "rows_with_an_entry": int((idx[:, 0] >= 0).sum()), "entries": int((idx >= 0).sum())}
    print(json.dumps(out), flush=True)
    return out


def matrix_route_cross(Q, R, k):
    """the one route without fc_ensemble_knn_cross: the fp64 matrix of the concatenated sets to the host, the block of
    the queries against the references cut out of it, argpartition + sort per row"""
    X = np.concatenate([Q, R])
    with fc.DeviceEnsemble(X, atom_mask=np.ones(X.shape[1], bool), center=True) as ens:
        M, _ = ens.rmsd_values()
    B = M[:len(Q), len(Q):]
    part = np.argpartition(B, k - 1, axis=1)[:, :k]
    d = np.take_along_axis(B, part, axis=1)
    order = np.lexsort((part, d), axis=1)
    return np.take_along_axis(part, order, axis=1).astype(np.int32), np.take_along_axis(d, order, axis=1)


def end_to_end_cross(Q, R, k, reps=3):
    """host arrays in -> lists out, the two routes alternating in one process"""
    atoms = np.array(["C"] * Q.shape[1])
    fc.pruner.knn_by_rmsd_against(Q, R, atoms, k), matrix_route_cross(Q, R, k)  # warm-up of both
    t_new, t_old, same = [], [], True
    for _ in range(reps):
        t0 = time.perf_counter()
        nb = fc.pruner.knn_by_rmsd_against(Q, R, atoms, k)
        t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        idx, _ = matrix_route_cross(Q, R, k)
        t_old.append(time.perf_counter() - t0)
        same = same and bool(np.array_equal(idx, nb.indices))
    print(json.dumps({"workload": f"end to end, {len(Q)} x {len(R)} x {Q.shape[1]}, k = {k}",
                      "knn_by_rmsd_against_ms": [round(1e3 * t, 2) for t in t_new],
                      "matrix_route_ms": [round(1e3 * t, 2) for t in t_old],
                      "knn_by_rmsd_against_ms_mean": round(1e3 * float(np.mean(t_new)), 2),
                      "matrix_route_ms_mean": round(1e3 * float(np.mean(t_old)), 2),
                      "same_indices": same}), flush=True)


def sym_table(K):
    """K permutations of the 50 atoms, the identity first, closed under inverse: the reversal (2), three runs of 16 atoms
    behind atom 0 permuted as wholes (6), or the group of log2 K disjoint transpositions"""
    import itertools

    ident = np.arange(A)
    if K == 1:
        return ident[None]
    if K == 2:
        return np.stack([ident, ident[::-1]])
    if K == 6:
        rows = []
        for order in itertools.permutations(range(3)):
            row = ident.copy()
            for m, src in enumerate(order):
                row[1 + 16 * m:1 + 16 * (m + 1)] = np.arange(1 + 16 * src, 1 + 16 * (src + 1))
            rows.append(row)
        return np.stack(rows)
    n = K.bit_length() - 1
    if K != 1 << n or K > 64:
        raise SystemExit("--symmetry K: 1, 2, 6 or a power of two up to 64")
    rows = []
    for bits in itertools.product((0, 1), repeat=n):
        row = ident.copy()
        for m, on in enumerate(bits):
            if on:
                row[[2 * m, 2 * m + 1]] = row[[2 * m + 1, 2 * m]]
        rows.append(row)
    return np.stack(rows)


def sym_ensemble(N, table, mirror, seed):
    """a continuous ensemble with a random half relabelled by a random row of the table and -- mirror -- a random half
    reflected: the ensembles the aware forms are for"""
    X = ensemble("continuous", N, seed)
    rng = np.random.default_rng(seed)
    rows = np.where(rng.random(N) < 0.5, rng.integers(0, len(table), size=N), 0)
    X = np.take_along_axis(X, table[rows][:, :, None], axis=1)
    if mirror:
        X[rng.random(N) < 0.5, :, 0] *= -1.0
    return np.ascontiguousarray(X)


def symmetry(K, mirror, crossed, reps=3):
    table, H = sym_table(K), 2 if mirror else 1
    dup = fc.pruner.CONVENTIONS["default_max_rmsd"]
    N = 10_000
    X = sym_ensemble(2 * N if crossed else N, table, mirror, 21)
    mask = np.ones(A, bool)
    kw = dict(symmetry=table, prune_enantiomers=mirror)
    with fc.DeviceEnsemble(X[:N], atom_mask=mask, center=True) as q, fc.DeviceEnsemble(X[-N:], atom_mask=mask, center=True) as r:
        for k in (1, 8):
            for cap in ((None, dup) if crossed else (None,)):
                if crossed:
                    aware = lambda: q.bench_knn_against(r, k, max_rmsd=cap, reps=1, **kw)  # noqa: E731
                    plain = lambda: q.bench_knn_against(r, k, max_rmsd=cap, reps=1)  # noqa: E731
                else:
                    aware = lambda: q.bench_knn(k, reps=1, **kw)  # noqa: E731
                    plain = lambda: q.bench_knn(k, reps=1)  # noqa: E731
                aware(), plain()  # warm-up of both: code objects, pool blocks
                a, b = [], []
                for _ in range(reps):  # alternating on one handle
                    a.append(aware())
                    b.append(plain())
                ms, ms0 = np.array([x[0] for x in a]), np.array([x[0] for x in b])
                formed, explicit = (a[-1][3] if len(a[-1]) > 3 else (0, 0))  # (K = 1 without the flag is the default form)
                out = {"workload": f"{'cross' if crossed else 'self'} {N}{f' x {N}' if crossed else ''} x {A}, K = {K}, "
                                   f"mirror = {int(mirror)}, k = {k}, {'no cap' if cap is None else f'cap {cap}'}",
                       "K": K, "H": H, "k": k, "max_rmsd": cap, "strips": a[0][2],
                       "ms_device_mean": round(float(ms.mean()), 3), "ms_device_min": round(float(ms.min()), 3),
                       "ms_device_max": round(float(ms.max()), 3),
                       "default_ms_device_mean": round(float(ms0.mean()), 3), "default_ms_device_min": round(float(ms0.min()), 3),
                       "default_ms_device_max": round(float(ms0.max()), 3),
                       "default_ms_times_KH": round(float(ms0.mean()) * K * H, 3),
                       "ratio_to_default_times_KH": round(float(ms.mean() / (ms0.mean() * K * H)), 3),
                       "p_h_formed": int(formed), "p_h_explicit": int(explicit),
                       "explicit_share": round(explicit / formed, 4) if formed else None}
                print(json.dumps(out), flush=True)


def cross():
    dup = fc.pruner.CONVENTIONS["default_max_rmsd"]  # the duplicate threshold of prune_by_rmsd
    sizes = [(10_000, 10_000), (1_000, 100_000)] + ([] if "--small" in sys.argv else [(100, 1_000_000)])
    mask = np.ones(A, bool)
    for Nq, Nr in sizes:
        Q, R = split(Nq, Nr, 13)
        with fc.DeviceEnsemble(Q, atom_mask=mask, center=True) as q, fc.DeviceEnsemble(R, atom_mask=mask, center=True) as r:
            for k in (1, 8):
                for cap in (None, dup):
                    measure_cross(f"cross {Nq} x {Nr} x {A}, k = {k}, {'no cap' if cap is None else f'cap {cap}'}", q, r,
                                  Nq, Nr, k, cap)
        if (Nq, Nr) == (10_000, 10_000):  # the self form on the references, in the same process: N (N - 1) against N^2
            measure(f"self form, continuous {Nr} x {A}, k = 8", R, 8)
        del Q, R
    Q, R = split(5_000, 5_000, 14)
    end_to_end_cross(Q, R, 8)


def main():
    fc.init(0)
    fc._lib.warmup()
    if "--symmetry" in sys.argv:
        symmetry(int(sys.argv[sys.argv.index("--symmetry") + 1]), "--mirror" in sys.argv, "--cross" in sys.argv)
        return
    if "--cross" in sys.argv:
        cross()
        return
    if "--trace" in sys.argv:
        with fc.DeviceEnsemble(ensemble("continuous", 10_000, 11), atom_mask=np.ones(A, bool), center=True) as ens:
            ens.knn(8)
        return
    if "--strips" in sys.argv:
        X5 = ensemble("continuous", 30_000, 12)
        for N in (1000, 3000, 10_000, 30_000):
            for strips in ("1", "2", "4", "8", "16", None):
                if strips is None:
                    os.environ.pop("FC_KNN_STRIPS", None)
                else:
                    os.environ["FC_KNN_STRIPS"] = strips
                measure(f"strips {strips or 'default'}", X5[:N], 8)
        return
    if "--filter" in sys.argv:
        for N in (10_000, 100_000):
            X = ensemble("continuous", N, 11 if N == 10_000 else 12)
            for k in (8, 64):
                for flag in ("0", None):
                    if flag is None:
                        os.environ.pop("FC_KNN_FILTER", None)
                    else:
                        os.environ["FC_KNN_FILTER"] = flag
                    measure(f"continuous {N} x {A}, k = {k}, filter {'off' if flag else 'on'}", X, k)
        return
    sizes = (10_000,) if "--small" in sys.argv else (10_000, 100_000)
    for N in sizes:
        for kind in ("continuous", "clusters"):
            X = ensemble(kind, N, 11 if N == 10_000 else 12)
            for k in (8, 64):
                measure(f"{kind} {N} x {A}, k = {k}", X, k)
    X4 = ensemble("continuous", 10_000, 11)
    for k in (8, 64):
        end_to_end(X4, k)


if __name__ == "__main__":
    main()
