"""Times the all-lists top-k of the set similarities on the dense route
(cms_set_top_k_all: the side's bit matrix through k_set_bits_mfma) next to the
posting-list walk (cms_set_top_k over every ID, k_set_tile), log-likelihood,
k = 100, in one process.

    python scripts/set_bits_probe.py [--model a|b] [--out FILE.json]

Model a: 943 users x 1,682 items at 6 % (the shape of MovieLens 100K), seeded,
key side -- 1,682 item lists over 943 users.  Model b: set_probe.py's config-2
model (100K item lists over 1M users), owner side; its whole job is long, so
--repeats 1 --warmup 0 is the practical setting.  The calls alternate: after
--warmup calls of each, --repeats rounds of one call of each, every call ending
in the library's stream synchronise.  The bit matrix is built by the first
dense call, which is timed apart (pack).  One JSON document:
  walk    set_top_k over all IDs: wall ms and the scopes set_tile / top_k
  dense   set_top_k_all: wall ms and the scopes set_bits_mfma / top_k
  pack    the first dense call's set_bits_pack scope and the matrix bytes
  ratio   the set_tile median over the set_bits_mfma median, the walk's spread
          over its median (the margin), and the MFMA scope as a fraction of the
          fp4 peak: 2 * lists^2 * padded K operations at 10 POPS
A measurement, not a test: nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_a():
    rng = np.random.Generator(np.random.PCG64(100))
    A = rng.random((943, 1682)) < 0.06
    A[np.arange(1682) % 943, np.arange(1682)] = True  # every item is held
    off = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64)
    return 943, off, np.nonzero(A)[1].astype(np.int64), "key", 1682, 943


def model_b(users=1_000_000, items=100_000, pairs=50_000_000):
    import torch

    from mahout_amd.synth import zipf_stream_torch
    it, us = zipf_stream_torch(users, items, pairs, device=torch.device("cuda", 0))
    pair = torch.unique(it * (1 << 32) + us)  # sorted by item, then user
    del it, us
    owner, keys = (pair >> 32).cpu().numpy(), (pair & ((1 << 32) - 1)).cpu().numpy()
    del pair
    torch.cuda.empty_cache()
    off = np.zeros(items + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=items), out=off[1:])
    return items, off, keys, "owner", items, int(np.unique(keys).size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("a", "b"), default="a")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mahout_amd import SketchTable

    owners, off, keys, side, lists, num = model_a() if a.model == "a" else model_b()
    stage = 256  # kBitsStage (cms_set_bits.h)
    padded_k = max(1, -(-num // stage)) * stage
    out = {"shape": {"model": a.model, "side": side, "lists": lists, "cross_indices": num, "preferences": int(keys.size),
                     "density": keys.size / (lists * num), "k": a.k, "padded_k": padded_k,
                     "matrix_bytes": -(-lists // 128) * 128 * padded_k // 8}}
    t = SketchTable(owners, depth=1, width=32, device=0)  # owner IDs are the rows
    try:
        t.attach_sets(off, keys)
        ids = np.arange(owners) if side == "owner" else np.unique(keys)
        t.set_timing(True, 2)
        calls = {"walk": (lambda: t.set_top_k(ids, a.k, "loglikelihood", side), ("set_tile", "top_k")),
                 "dense": (lambda: t.set_top_k_all(a.k, "loglikelihood", side), ("set_bits_mfma", "top_k"))}
        t0 = time.perf_counter()
        t.set_similarity_block(ids[:1], ids[:1], "loglikelihood", side)  # builds the matrix
        out["pack"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "set_bits_pack": round(t.timing("set_bits_pack")[0], 3)}
        runs = {name: [] for name in calls}
        for r in range(a.warmup + a.repeats):
            for name, (fn, scopes) in calls.items():
                t.reset_timing()
                t0 = time.perf_counter()
                fn()
                wall = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    runs[name].append({"wall_ms": round(wall, 3), **{s: round(t.timing(s)[0], 3) for s in scopes}})
        t.set_timing(False)
    finally:
        t.close()
    for name, rs in runs.items():
        out[name] = {"median": {k: float(np.median([r[k] for r in rs])) for k in rs[0]},
                     "min_max": {k: [min(r[k] for r in rs), max(r[k] for r in rs)] for k in rs[0]}, "runs": rs}
    walk, mfma = out["walk"]["median"]["set_tile"], out["dense"]["median"]["set_bits_mfma"]
    lo, hi = out["walk"]["min_max"]["set_tile"]
    out["ratio"] = {"set_tile_over_set_bits_mfma": round(walk / mfma, 3), "walk_spread_over_median": round((hi - lo) / walk, 3),
                    "wall_walk_over_dense": round(out["walk"]["median"]["wall_ms"] / out["dense"]["median"]["wall_ms"], 3),
                    "mfma_fraction_of_fp4_peak": 2.0 * lists * lists * padded_k / (mfma * 1e-3) / 1e16}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
