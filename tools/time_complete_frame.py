"""tools/time_complete_frame.py -- the two arms of the shared frame that bench.py cannot show, on the library
FC_LIB_PATH selects (run it once per build, interleaved):
  clouds: 10 000 x 50 unrelated Gaussian clouds (scale 3 A) -- no wave certifies column 0: every sub-tile pays the
          certificate and then the general form; kernel ms of `reps` passes on the resident ensemble;
  first:  ONE complete-alignment call on a fresh handle of the bench ensemble (frame + row tiles + pass), host wall clock
          around fc_ensemble_rmsd_and_max_all without the matrices, and the kernel's own ms of that call.
Usage: python tools/time_complete_frame.py [clouds|first] [n_conf] [n_atoms] [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import firecode_amd as fc  # noqa: E402
from firecode_amd import synthetic as syn  # noqa: E402

arm = sys.argv[1] if len(sys.argv) > 1 else "clouds"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
a = int(sys.argv[3]) if len(sys.argv) > 3 else 50
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
fc.init(0)
out = {"arm": arm, "n": n, "a": a}
if arm == "clouds":
    X = np.random.default_rng(5).normal(scale=3.0, size=(n, a, 3))
    with fc.DeviceEnsemble(X, center=True) as ens:
        ens.bench_rmsd_and_max_all(2)
        k, t, st = ens.bench_rmsd_and_max_all(reps)
        out.update(kernel_ms=k, total_ms_per_pass=t / reps, fixup_pairs=int(st[1]), general_form_subtiles=None if os.environ.get("FC_LIB_PATH") else int(st[3]))  # (a build before the counter leaves the word 0)
else:
    X, _, _ = syn.synthetic_ensemble(n, a, seed=2)
    with fc.DeviceEnsemble(X[:256], center=True) as warm:  # (code objects loaded, allocator warm: not part of the first call)
        warm.rmsd_and_max_all(want_matrices=False)
    calls = []
    for _ in range(reps):
        with fc.DeviceEnsemble(X, center=True) as ens:
            t0 = time.perf_counter()
            _, _, k = ens.rmsd_and_max_all(want_matrices=False)
            calls.append((1e3 * (time.perf_counter() - t0), k))
    out.update(first_call_ms_median=float(np.median([c[0] for c in calls])), first_call_ms_range=[min(c[0] for c in calls), max(c[0] for c in calls)],
               events_around_the_launches_ms_median=float(np.median([c[1] for c in calls])))
print(json.dumps(out))
