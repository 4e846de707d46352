#!/usr/bin/env python
"""Records what the restatement gives on the largest case of tests/test_gpu_diverse_sym.py (600 conformers x 80 atoms,
the path's reversal, mirror images): the cover at 0.5 A under d_sym (tests/diverse_sym_ref.py: 120 picks, each a row of
600 x 4 alignments -- 11 s of NumPy) and the default prune's mask of the same coordinates (7 s).  The test builds the
ensemble with the same call and compares the device with these arrays; tests/test_diverse_sym_cpu.py recomputes a few of
the recorded rows.  No device, no input but the seed:

    python tests/golden/make_golden_diverse_sym.py        # writes tests/golden/diverse_sym_v1.npz
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import diverse_ref as dr  # noqa: E402
import diverse_sym_ref as ds  # noqa: E402
from oracle import cpu_ref as o  # noqa: E402

CASE = ("clusters", 600, 80, "path", True)


def main():
    X, atoms, table, _ = ds.ensemble(*CASE)
    idx, lab, dist, rad, rec = dr.select_diverse(X, len(X), stop_rmsd=0.5, row=ds.sym_row(table, True))
    mask = o.prune_by_rmsd(X, atoms, 0.5)[1]
    np.savez_compressed(os.path.join(HERE, "diverse_sym_v1.npz"), cover_indices=idx, cover_labels=lab, cover_distances=dist,
                        cover_radii=rad, cover_min_gap=np.float64(rec.min_gap), prune_mask=np.asarray(mask, dtype=bool))
    print(f"{len(idx)} picks, smallest gap {rec.min_gap:.3g}, the default prune keeps {int(np.sum(mask))}")


if __name__ == "__main__":
    main()
