"""Pairs taken out of a live table (cms_retract_device_rows) on the config-2
shaped table (100K owners, d = 5, w = 4096, the 50M-pair Zipf stream of the
bench seed), each figure beside two yardsticks taken in the same process:

  (a) 1,000 pairs over 1,000 owners      one pair of each of 1,000 distinct owners
  (b) 1M pairs of the stream's own distribution   the stream's first 1M pairs

  retract_check / retract_apply / widen_rows   the library's timing scopes of the
                        retraction (retract_check spans the two read-backs of
                        the rules' verdicts, which the host waits for)
  yardstick 1           cms_ingest_device_rows of the very same batch into the
                        very same table (existing code): its scopes partition,
                        ingest_sorted, ingest_atomic, widen_rows.  The retract
                        does the ingest's counter work twice (a read-only pass
                        and a write pass) plus the grouping: the expectation is
                        check + apply <= 2 x the ingest, 1.25 x on top as margin
  yardstick 2           the same pairs through a second handle of the full
                        shape, save_device() and subtract_device(): wall time
                        end to end, with and without creating the handle

Median of 7 calls after 2 warm-ups; the table is restored by re-ingesting the
batch (and finalized, so every call meets the same table state).  Beside it
the wall time of case (a) on the config-3 shaped table (1M owners, w = 8192):
the call's cost does not grow with num_owners x d x w.

    python scripts/retract_probe.py [out.json] [config-3 build pairs, 0 = skip]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "retract_probe.json"
c3_pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000_000
SEED = 20261015
WARM, REPS = 2, 7
INGEST_SCOPES = ("partition", "ingest_sorted", "ingest_atomic", "widen_rows")
RETRACT_SCOPES = ("retract_check", "retract_apply", "widen_rows")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def build(n, d, w, n_users, pairs):
    t = SketchTable(n, depth=d, width=w, seed=42, device=0)
    items, users = zipf_stream_torch(n_users, n, pairs, seed=SEED, device="cuda")
    t.ingest_device_rows(items, users, None, pairs)
    t.finalize()
    torch.cuda.synchronize()
    return t, items, users


def one_pair_per_owner(items, users, count):
    """`count` of the stream's own pairs, each of another owner."""
    head = items[:4_000_000].cpu().numpy()
    _, first = np.unique(head, return_index=True)
    idx = torch.from_numpy(np.sort(first[:count])).to(items.device)
    assert idx.numel() == count
    return items[idx].contiguous(), users[idx].contiguous()


def scopes(t, names):
    return {s + "_ms": t.timing(s)[0] for s in names}


def med(rows, key):
    return statistics.median(r[key] for r in rows)


def measure(t, label, rows, keys, delta_shape=None):
    m = int(rows.numel())
    sample = [0, 1, t.num_owners // 2, t.num_owners - 1] + rows[:4].tolist()
    pre = [t.read_counters_device(r, 1).clone() for r in sample]
    t.set_timing(True, level=2)
    runs = []
    for it in range(WARM + REPS):
        t.reset_timing()
        r = {"retract_wall_ms": wall(lambda: t.retract_device_rows(rows, keys, None, m))}
        r.update({"retract_" + k: v for k, v in scopes(t, RETRACT_SCOPES).items()})
        t.finalize()
        t.reset_timing()
        r["ingest_wall_ms"] = wall(lambda: t.ingest_device_rows(rows, keys, None, m))
        r.update({"ingest_" + k: v for k, v in scopes(t, INGEST_SCOPES).items()})
        t.finalize()
        if it >= WARM:
            runs.append(r)
    res = {"case": label, "pairs": m, "owners": int(torch.unique(rows).numel())}
    for k in runs[0]:
        res[k] = med(runs, k)
    res["retract_kernel_ms"] = res["retract_retract_check_ms"] + res["retract_retract_apply_ms"]
    res["ingest_kernel_ms"] = sum(res["ingest_" + s + "_ms"] for s in INGEST_SCOPES)
    res["retract_over_ingest_kernel"] = res["retract_kernel_ms"] / res["ingest_kernel_ms"]
    res["within_2x_1p25"] = res["retract_over_ingest_kernel"] <= 2.5
    res["retract_over_ingest_wall"] = res["retract_wall_ms"] / res["ingest_wall_ms"]
    if delta_shape:  # yardstick 2: the image route, end to end
        n, d, w = delta_shape
        route = []
        for it in range(WARM + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            delta = SketchTable(n, depth=d, width=w, seed=42, device=0)
            t1 = time.perf_counter()
            delta.ingest_device_rows(rows, keys, None, m)
            delta.finalize()
            image = delta.save_device()
            t.subtract_device(image)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            delta.close()
            del image
            t.finalize()
            t.ingest_device_rows(rows, keys, None, m)
            t.finalize()
            if it >= WARM:
                route.append({"image_route_wall_ms": (t2 - t0) * 1e3, "image_route_without_create_ms": (t2 - t1) * 1e3})
        for k in route[0]:
            res[k] = med(route, k)
        res["image_route_over_retract_wall"] = res["image_route_wall_ms"] / res["retract_wall_ms"]
        res["image_route_without_create_over_retract_wall"] = res["image_route_without_create_ms"] / res["retract_wall_ms"]
    res["restored_sample"] = bool(all(torch.equal(x, t.read_counters_device(r, 1)) for x, r in zip(pre, sample)))
    t.set_timing(False)
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


results = {"device": torch.cuda.get_device_name(0), "warmups": WARM, "reps": REPS, "cases": []}
n, d, w = 100_000, 5, 4096
t, items, users = build(n, d, w, 1_000_000, 50_000_000)
results["config2"] = {"shape": [n, d, w], "pairs": 50_000_000, "table_bytes": t.stats()["table_bytes"],
                      "stored_bytes": t.stats()["stored_bytes"]}
ra, ka = one_pair_per_owner(items, users, 1000)
results["cases"].append(measure(t, "(a) 1,000 pairs over 1,000 owners", ra, ka, (n, d, w)))
rb, kb = items[:1_000_000].contiguous(), users[:1_000_000].contiguous()
results["cases"].append(measure(t, "(b) 1M pairs of the stream's distribution", rb, kb, (n, d, w)))
t.close()
del items, users, ra, ka, rb, kb, t
torch.cuda.empty_cache()
if c3_pairs > 0:
    n, d, w = 1_000_000, 5, 8192
    t, items, users = build(n, d, w, 10_000_000, c3_pairs)
    results["config3"] = {"shape": [n, d, w], "pairs": c3_pairs, "table_bytes": t.stats()["table_bytes"],
                          "stored_bytes": t.stats()["stored_bytes"]}
    ra, ka = one_pair_per_owner(items, users, 1000)
    del items, users
    results["cases"].append(measure(t, "(a) on the config-3 table: 1,000 pairs over 1,000 owners", ra, ka))
    t.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
print(json.dumps({"written": out_path}))
