"""Times the co-rated similarities' top-k (cms_common_top_k: uncentered cosine,
Pearson, Euclidean) next to the exact cosine's (cms_exact_top_k_rows), on
exact_cosine_probe.py's model and query rows, in one process.

    python scripts/common_probe.py [--out FILE.json]   (default: profiles/r23/common_probe.json)

The model: bench.py's config-2 stream (Zipf, 50M interactions) transposed --
100K item owners keyed by 1M users, an item's preference for a user = how often
the pair occurs (integers, s = 0) -- attached to a minimal handle.  The queries:
the same 1,024 consecutive owner rows from the same seeded start, k = 100.  One
JSON document:
  exact      exact_top_k_rows: wall ms and the scopes exact_tile / exact_pairs /
             top_k per call, median of --repeats calls after --warmup, every run
  <measure>  common_top_k on the owner side, the same way, with the scopes
             common_tile / common_pairs / top_k
  ratios     per measure, the common_tile median over the same run's exact_tile
             median, beside the LDS atomics per posting entry (2, 4 or 6 to the
             exact kernel's 1) and that multiple times 1.25
A measurement, not a test: nothing is asserted."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ATOMICS = {"euclidean": 2, "uncentered_cosine": 4, "pearson": 6}  # per posting entry; k_exact_tile: 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "common_probe.json"))
    a = ap.parse_args()

    import torch

    from exact_cosine_probe import timed
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
    out = {"shape": {"owners": n, "keys": a.users, "interactions": a.pairs, "preferences": int(keys.size),
                     "queries": a.queries, "k": a.k, "first_row": r0},
           "device": torch.cuda.get_device_name(0)}

    t = SketchTable(n, depth=1, width=32, device=0)  # owner IDs are the rows
    try:
        t.attach_exact(off, keys, vals)
        t.set_timing(True, 2)
        out["exact"] = timed(t, lambda: t.exact_top_k_rows(rows, a.k), a.warmup, a.repeats,
                             ("exact_tile", "exact_pairs", "top_k"))
        for measure in ATOMICS:
            out[measure] = timed(t, lambda: t.common_top_k(rows, a.k, measure, "owner"), a.warmup, a.repeats,
                                 ("common_tile", "common_pairs", "top_k"))
        t.set_timing(False)
    finally:
        t.close()
    base = out["exact"]["median"]["exact_tile"]
    out["ratios"] = {m: {"common_tile_over_exact_tile": round(out[m]["median"]["common_tile"] / base, 3),
                         "lds_atomics_per_entry": ATOMICS[m], "bound_with_margin": ATOMICS[m] * 1.25}
                     for m in ATOMICS}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
