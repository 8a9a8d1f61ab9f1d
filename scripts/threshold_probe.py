"""Threshold neighbourhoods (cms_threshold_neighbors) beside the top-k of the
same query rows (cms_top_k_rows), in one process on the config-2-shaped table
(100K owners x 5 x 4096 from the 50M-pair Zipf stream):

  threshold             found by bisection on the count-only call, so that the
                        lists of the first `rows` owner rows average ~100 entries
  threshold_neighbors   IDs and scores, ascending-ID order
  threshold_counts_only out_ids == NULL
  top_k_rows_100        cms_top_k_rows(h, 0, rows, 100): the same slab producer,
                        the existing selection

  Each: wall time and the library's timing scopes (kernel time), warm, the
  median of 5.  Expected from bytes: the selection reads 8 bytes per pair and
  is a minor share beside the slab's MFMA work.  A figure to
  record, not a condition.

    python scripts/threshold_probe.py [out.json] [rows]
"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "threshold_probe.json"
Q = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
n, d, w = 100_000, 5, 4096
SCOPES = ["threshold_select", "cosine_mfma", "cosine_mfma_multi", "cosine_mfma_limbs", "top_k"]

items, users = zipf_stream_torch(1_000_000, n, 50_000_000, seed=20261015, device=torch.device("cuda", 0))
t = SketchTable(n, depth=d, width=w, seed=42, device=0)
t.ingest_device_rows(items, users, None, int(items.numel()))
t.finalize()
t.synchronize()
del items, users
ids = np.arange(Q, dtype=np.int64)
t.top_k_rows(0, Q, 100)  # the first all-pairs call prepares the operand images

lo, hi = 0.0, 1.0
for _ in range(14):
    mid = 0.5 * (lo + hi)
    if t.threshold_neighbor_counts(ids, mid).mean() > 100:
        lo = mid
    else:
        hi = mid
thr = 0.5 * (lo + hi)
cnt = t.threshold_neighbor_counts(ids, thr)
t.set_timing(True, 2)


def measure(fn, reps=5):
    runs = []
    for r in range(reps + 1):  # the first is the warm-up
        t.reset_timing()
        t.synchronize()
        t0 = time.perf_counter()
        fn()
        rec = {"wall_ms": (time.perf_counter() - t0) * 1e3}
        for s in SCOPES:
            rec[s + "_ms"], rec[s + "_launches"] = t.timing(s)
        if r:
            runs.append(rec)
    return {k: float(np.median([x[k] for x in runs])) for k in runs[0]}


res = {"owners": n, "depth": d, "width": w, "rows": Q, "threshold": thr, "mean_len": float(cnt.mean()),
       "max_len": int(cnt.max()),
       "threshold_neighbors": measure(lambda: t.threshold_neighbors(ids, thr)),
       "threshold_counts_only": measure(lambda: t.threshold_neighbor_counts(ids, thr)),
       "top_k_rows_100": measure(lambda: t.top_k_rows(0, Q, 100))}
t.close()
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
