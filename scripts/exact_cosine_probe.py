"""Times the exact cosine's top-k (cms_exact_top_k_rows) next to the sketch's
(cms_top_k_rows) and reports the sketch's accuracy, on the config-2-shaped
DataModel transposed: 100K item owners keyed by 1M users, a (5, 4096) table
with the model attached, in one process.

    python scripts/exact_cosine_probe.py [--out FILE.json]   (default: profiles/r21/exact_cosine_probe.json)

The model: bench.py's config-2 stream (Zipf, 50M interactions), an item's
preference for a user = how often the pair occurs (integers, s = 0).  One JSON
document:
  exact      exact_top_k_rows of 1,024 consecutive owner rows from a seeded start
             (item IDs are a seeded permutation of the popularity ranks, so the
             block is a popularity sample) at k = 100: wall ms and the library
             scopes exact_tile / exact_pairs / top_k per call, median of --repeats
             calls after --warmup, every run listed
  sketch     top_k_rows of the same rows on the sketch table, the same way
             (scopes "cosine*" are not split: wall ms and top_k only)
  copy       a device-to-device copy of as many bytes as the tile pass must read
             at least once per query -- the posting lists (owner row + unit, 8 B an
             entry) of every query's items -- measured on a buffer of up to 2 GiB
             and scaled to the byte count (marked as derived)
  accuracy   sketch_accuracy on those rows: recall@100 (mean, min, quartiles)
             and the error figures; again on the table folded to width 2048
A measurement, not a test: nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCOPES = ("exact_tile", "exact_pairs", "top_k")


def timed(table, fn, warmup, repeats, scopes):
    for _ in range(warmup):
        fn()
    runs = []
    for _ in range(repeats):
        table.reset_timing()
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        runs.append({"wall_ms": round(wall, 3), **{s: round(table.timing(s)[0], 3) for s in scopes}})
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    spread = {k: [min(r[k] for r in runs), max(r[k] for r in runs)] for k in runs[0]}
    return {"median": med, "min_max": spread, "runs": runs}


def brief(rep):
    r = rep["recall_at_k"]
    return {"recall_at_k": {"mean": float(r.mean()), "min": float(r.min()),
                            "quartiles": [float(x) for x in np.percentile(r, [25, 50, 75])]},
            "exact_lists_shorter_than_k": int((rep["exact_counts"] < rep["exact_ids"].shape[1]).sum()),
            "sketch_list": rep["sketch_list"], "exact_list": rep["exact_list"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "exact_cosine_probe.json"))
    a = ap.parse_args()

    import torch

    from mahout_amd import SketchTable
    from mahout_amd.accuracy import sketch_accuracy
    from mahout_amd.synth import zipf_stream_torch

    d, w, n = 5, 4096, a.items
    dev = torch.device("cuda", 0)
    items, users = zipf_stream_torch(a.users, a.items, a.pairs, device=dev)
    # the transposed DataModel: owner = item, key = user (ascending within an item), value = occurrences
    pair, cnt = torch.unique(items * (1 << 32) + users, return_counts=True)  # sorted by item, then user
    del items, users
    owner = (pair >> 32).cpu().numpy()
    keys = (pair & ((1 << 32) - 1)).cpu().numpy()
    vals = cnt.to(torch.float32).cpu().numpy()
    del pair, cnt
    torch.cuda.empty_cache()
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=off[1:])
    del owner
    out = {"shape": {"owners": n, "keys": a.users, "interactions": a.pairs, "preferences": int(keys.size),
                     "depth": d, "width": w, "queries": a.queries, "k": a.k,
                     "longest_owner": int(np.diff(off).max())},
           "device": torch.cuda.get_device_name(0)}

    rng = np.random.default_rng(21)
    r0 = int(rng.integers(0, n - a.queries))
    rows = np.arange(r0, r0 + a.queries)
    user_len = np.bincount(keys, minlength=a.users)
    read_bytes = int(8 * sum(int(user_len[keys[off[r]:off[r + 1]]].sum()) for r in rows))
    out["queries"] = {"first_row": r0, "preferences": int(off[r0 + a.queries] - off[r0]),
                      "posting_list_bytes": read_bytes}

    t = SketchTable(n, depth=d, width=w, seed=42, device=0)
    try:
        t0 = time.perf_counter()
        t.ingest_csr(off, keys, vals)
        t.finalize()
        out["ingest_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        t.attach_exact(off, keys, vals)
        out["attach_s"] = round(time.perf_counter() - t0, 3)
        t.set_timing(True, 2)
        out["exact"] = timed(t, lambda: t.exact_top_k_rows(rows, a.k), a.warmup, a.repeats, SCOPES)
        out["sketch"] = timed(t, lambda: t.top_k_rows(r0, a.queries, a.k), a.warmup, a.repeats, ("top_k",))
        t.set_timing(False)

        nb = max(1 << 20, min(read_bytes, 2 << 30))
        src = torch.empty(nb, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        del src, dst
        torch.cuda.empty_cache()
        med = float(np.median(ms))
        out["copy"] = {"buffer_bytes": nb, "ms": round(med, 4), "min_max_ms": [round(min(ms), 4), round(max(ms), 4)],
                       "gb_per_s_read_plus_write": round(2 * nb / med / 1e6, 1),
                       "derived_ms_for_posting_list_bytes": round(med * read_bytes / nb, 3)}

        t0 = time.perf_counter()
        out["accuracy"] = {"width_%d" % w: brief(sketch_accuracy(t, rows, a.k))}
        out["accuracy_s"] = round(time.perf_counter() - t0, 3)
        f = t.folded(w // 2)
        try:
            f.finalize()
            f.attach_exact(off, keys, vals)
            out["accuracy"]["folded_%d" % (w // 2)] = brief(sketch_accuracy(f, rows, a.k))
        finally:
            f.close()
    finally:
        t.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
