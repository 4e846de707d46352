"""tools/complete_items_timeline.py -- per-item time stamps of ONE complete all-pairs pass (k_simbits_screen_mfma mode 2):
fill time per item, spread of the workgroups' end times, length of the drain.

Needs a tuning build with the stamps (fc_tuning.h):
    make -C firecode_amd/csrc BUILD=build_tl OUT=../libfc_hip_tl.so EXTRA="-DFC_TUNING_BUILD -DFC_TIMELINE"
    FC_LIB_PATH=firecode_amd/libfc_hip_tl.so python tools/complete_items_timeline.py OUT.json [n_conf] [n_atoms]
The item shapes follow FC_COMPLETE_ROW_CHUNK / FC_SCREEN_TAIL_SLOTS / FC_COMPLETE_TAIL_ORDER as in the product build
(FC_COMPLETE_ROW_CHUNK=1: single row blocks).  The stamps cost time themselves: compare timelines with timelines only."""
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

out_path = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
a = int(sys.argv[3]) if len(sys.argv) > 3 else 50
raw = os.path.join(tempfile.mkdtemp(), "timeline.bin")
os.environ["FC_TIMELINE_OUT"] = raw

import firecode_amd as fc  # noqa: E402
from firecode_amd import synthetic as syn  # noqa: E402

fc.init(0)
X, _, _ = syn.synthetic_ensemble(n, a, seed=2, cluster_size=5 if a <= 200 else max(5, n // 8))
with fc.DeviceEnsemble(X, center=True) as ens:
    ens.bench_rmsd_and_max_all(2)            # warm (every pass rewrites the file; the last one is kept)
    k_ms, _, _ = ens.bench_rmsd_and_max_all(1)

w = np.fromfile(raw, dtype=np.uint64)
n_items, has_table = int(w[0]), bool(w[1])   # then the stamps (4 per item), then the item table when there is one
st = w[2:2 + 4 * n_items].reshape(n_items, 4).astype(np.int64)
table = w[2 + 4 * n_items:] if has_table else None
ran = st[:, 2] > 0
t0 = st[ran, 0].min()
start, filled, end = [(st[ran, c] - t0) / 100.0 for c in range(3)]  # us (the stamps tick at 100 MHz)
fill, dur = filled - start, end - start
# the drain: from the first workgroup that ends with no item left to start -- the first idle slot -- to the kernel's end
last_start = start.max()
first_idle = end[end >= last_start].min()


def pct(x, qs=(5, 25, 50, 75, 95)):
    return {f"p{q}": float(np.percentile(x, q)) for q in qs}


res = {
    "n_conformers": n, "n_atoms": a, "device": fc.device_info()["name"], "items": int(n_items), "items_run": int(ran.sum()),
    "env": {k: os.environ.get(k) for k in ("FC_COMPLETE_ROW_CHUNK", "FC_SCREEN_TAIL_SLOTS", "FC_COMPLETE_TAIL_ORDER")},
    "kernel_ms_with_stamps": k_ms, "span_us": float(end.max()),
    "fill_us": dict(pct(fill), mean=float(fill.mean()), total_ms=float(fill.sum() / 1e3)),
    "item_us": dict(pct(dur), mean=float(dur.mean()), max=float(dur.max())),
    "end_times_us": dict(pct(end, (50, 90, 99)), max=float(end.max())),
    # spread of the end times of the last workgroup of each of the slots: the latest 512 (or fewer) item ends
    "last_ends_spread_us": float(np.sort(end)[-min(512, len(end)):].max() - np.sort(end)[-min(512, len(end)):].min()),
    "last_item_start_us": float(last_start), "first_idle_slot_us": float(first_idle),
    "drain_us": float(end.max() - first_idle), "drain_in_median_items": float((end.max() - first_idle) / np.median(dur)),
}
if table is not None:
    blocks = ((table[ran] >> np.uint64(58)) & np.uint64(15)).astype(np.int64) + 1
    half = ((table[ran] >> np.uint64(31)) & np.uint64(1)) | ((table[ran] >> np.uint64(63)) & np.uint64(1))
    res["by_shape"] = {}
    for b in np.unique(blocks):
        for h in (0, 1):
            m = (blocks == b) & (half == h)
            if m.any():
                res["by_shape"][f"{b}_row_blocks{'_half' if h else ''}"] = {
                    "items": int(m.sum()), "fill_us_median": float(np.median(fill[m])), "item_us_median": float(np.median(dur[m]))}
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
