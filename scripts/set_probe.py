"""Times the set similarities' top-k (cms_set_top_k, log-likelihood) next to the
co-rated similarities' (cms_common_top_k, Euclidean: the existing tile kernel
with the fewest LDS atomics), on common_probe.py's model, in one process.

    python scripts/set_probe.py [--out FILE.json]   (default: profiles/r24/set_probe.json)

The model: bench.py's config-2 stream (Zipf, 50M interactions) transposed --
100K item owners keyed by 1M users, an item's preference for a user = how often
the pair occurs -- attached to a minimal handle.  The queries: the same 4,096
consecutive owner rows from a seeded start for both, owner side, k = 100.  The
calls alternate: after --warmup calls of each, --repeats rounds of one call
of each, every call ending in the library's stream synchronise.  One JSON
document:
  loglikelihood  set_top_k: wall ms and the scopes set_tile / top_k per call,
                 the median, the extremes and every run
  tanimoto       the same kernel with an ending of one division: what the
                 log-likelihood ending's logarithms cost
  euclidean      common_top_k, the same way, with common_tile / common_pairs / top_k
  ratio          the set_tile median over the common_tile median, beside the
                 yardstick's own spread over its median (the margin), what the
                 two kernels do per posting entry, and the posting entries
                 set_tile walks per second (counted on the host from the model)
A measurement, not a test: nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "set_probe.json"))
    a = ap.parse_args()

    import torch

    from mahout_amd import SketchTable
    from mahout_amd.synth import zipf_stream_torch

    n = a.items
    dev = torch.device("cuda", 0)
    items, users = zipf_stream_torch(a.users, a.items, a.pairs, device=dev)
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
    rng = np.random.default_rng(21)
    r0 = int(rng.integers(0, n - a.queries))
    rows = np.arange(r0, r0 + a.queries)
    # what either tile kernel walks: for every preference of a query, the posting list of its key
    walked = int(np.bincount(keys, minlength=a.users)[keys[off[r0]:off[r0 + a.queries]]].sum())
    out = {"shape": {"owners": n, "keys": a.users, "interactions": a.pairs, "preferences": int(keys.size),
                     "queries": a.queries, "query_preferences": int(off[r0 + a.queries] - off[r0]), "k": a.k,
                     "first_row": r0, "posting_entries_walked": walked},
           "device": torch.cuda.get_device_name(0)}

    calls = {"loglikelihood": (lambda t: t.set_top_k(rows, a.k, "loglikelihood", "owner"), ("set_tile", "top_k")),
             "tanimoto": (lambda t: t.set_top_k(rows, a.k, "tanimoto", "owner"), ("set_tile", "top_k")),
             "euclidean": (lambda t: t.common_top_k(rows, a.k, "euclidean", "owner"),
                           ("common_tile", "common_pairs", "top_k"))}
    runs = {name: [] for name in calls}
    t = SketchTable(n, depth=1, width=32, device=0)  # owner IDs are the rows
    try:
        t.attach_exact(off, keys, vals)  # the values serve the yardstick; the set kernels read none
        t.set_timing(True, 2)
        for r in range(a.warmup + a.repeats):
            for name, (fn, scopes) in calls.items():
                t.reset_timing()
                t0 = time.perf_counter()
                fn(t)
                wall = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    runs[name].append({"wall_ms": round(wall, 3), **{s: round(t.timing(s)[0], 3) for s in scopes}})
        t.set_timing(False)
    finally:
        t.close()
    for name, rs in runs.items():
        out[name] = {"median": {k: float(np.median([r[k] for r in rs])) for k in rs[0]},
                     "min_max": {k: [min(r[k] for r in rs), max(r[k] for r in rs)] for k in rs[0]}, "runs": rs}
    base = out["euclidean"]["median"]["common_tile"]
    lo, hi = out["euclidean"]["min_max"]["common_tile"]
    out["ratio"] = {"set_tile_over_common_tile": round(out["loglikelihood"]["median"]["set_tile"] / base, 3),
                    "yardstick_spread_over_median": round((hi - lo) / base, 3),
                    "set_tile_posting_entries_per_s": round(walked / (out["loglikelihood"]["median"]["set_tile"] * 1e-3)),
                    "per_posting_entry": {"set_tile": {"lds_atomics": 1, "global_bytes": 4},
                                          "common_tile_euclidean": {"lds_atomics": 2, "global_bytes": 8}},
                    "tiles_per_query": {"set_tile": -(-n // 16384), "common_tile_euclidean": -(-n // 5440)}}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
