"""Times GenericItemBasedRecommender.recommend_all (cms_item_recommend_batch:
one device batch of estimates) against what a caller had before it -- one
similarities(candidate, preferred items) call per candidate item and a numpy
reduction -- on the ML-100K-shaped model at config 1's depth and width
(d = 4, w = 1024, item sketches keyed by user), in one process.

    python scripts/item_recommend_probe.py [--out FILE.json]

One JSON document: (a) ms per recommend_all call over all 943 users (how_many
10, the default strategy) and per user, median of --repeats after --warmup;
(b) the baseline's ms per user over a fixed sample of 32 users; the library
scopes item_estimate / item_block (cms_get_timing) of one more call, and the
estimate epilogue's share, taken as the difference between the estimate launch
and block launches over the same pairs.  (The pair_cosine scope of the same
pairs is not formed: cms_similarities runs on a reader's stream, which is
never timed.)  A measurement, not a test: nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(x, 3) for x in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from mahout_amd import taste
    from mahout_amd.datamodel import GenericDataModel
    from mahout_amd.synth import movielens_like

    d, w, how = 4, 1024, 10
    users, items, ratings = movielens_like()
    uid = np.unique(users)
    rows = np.searchsorted(uid, users)
    order = np.lexsort((items, rows))
    rows, items, ratings = rows[order], items[order], ratings[order]
    off = np.zeros(uid.size + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=uid.size), out=off[1:])
    model = GenericDataModel.from_csr(uid, off, items, ratings)
    sim = taste.CosineCM(model.transposed(), taste.FixedShapeConfig(d, w), taste.HashFunctionBuilder(42))
    out = {"shape": {"users": int(uid.size), "items": model.getNumItems(), "ratings": int(items.size), "depth": d,
                     "width": w, "how_many": how},
           "device": torch.cuda.get_device_name(0)}
    try:
        t = sim.table
        rec = taste.GenericItemBasedRecommender(model, sim)
        capper = taste.build_capper(model)

        # (a) every user in one native call
        ms, runs = median_ms(lambda: rec.recommend_all(uid, how), a.warmup, a.repeats)
        out["recommend_all"] = {"ms_per_call": round(ms, 3), "ms_per_user": round(ms / uid.size, 5), "runs_ms": runs}

        # (b) the parent commit's route for a fixed sample: one similarities() per candidate, numpy reduction
        sample = uid[np.random.default_rng(11).choice(uid.size, a.sample, replace=False)]
        cands = {}
        whole = rec.recommend_all(sample, model.getNumItems() + 1)  # every candidate with an estimate
        for u, ranking in zip(sample.tolist(), whole):  # (the candidate sets are not part of the timed baseline)
            keys, vals = model.getPreferencesFromUser(u)
            cands[u] = (keys, vals, sorted(i for i, _ in ranking))
        out["sample"] = {"users": int(sample.size), "candidates": int(sum(len(c[2]) for c in cands.values())),
                         "pairs": int(sum(len(c[2]) * c[0].size for c in cands.values()))}

        def baseline():
            res = []
            for u in sample.tolist():
                keys, vals, cand = cands[u]
                v = vals.astype(np.float64)
                est = np.full(len(cand), np.nan, np.float32)
                for i, c in enumerate(cand):
                    s = t.similarities(c, keys)
                    ok = ~np.isnan(s)
                    if ok.sum() > 1:
                        est[i] = np.float32(min(max((s[ok] * v[ok]).sum() / s[ok].sum(), capper[0]), capper[1]))
                res.append(taste.get_top_items(how, cand, est))
            return res

        ms_b, runs_b = median_ms(baseline, 1, 3)
        out["baseline"] = {"ms_per_user": round(ms_b / sample.size, 4), "runs_ms": runs_b,
                           "spread_ms_per_user": round((max(runs_b) - min(runs_b)) / sample.size, 4)}
        ms_s, runs_s = median_ms(lambda: rec.recommend_all(sample, how), a.warmup, a.repeats)
        out["recommend_all_sample"] = {"ms_per_user": round(ms_s / sample.size, 5), "runs_ms": runs_s}

        # device scopes of one more call of each (timed calls run on the handle's stream)
        po = np.concatenate([[0], np.cumsum([cands[u][0].size for u in sample.tolist()])])
        co = np.concatenate([[0], np.cumsum([len(cands[u][2]) for u in sample.tolist()])])
        pi = np.concatenate([cands[u][0] for u in sample.tolist()])
        pv = np.concatenate([cands[u][1] for u in sample.tolist()])
        ci = np.concatenate([np.asarray(cands[u][2], np.int64) for u in sample.tolist()])
        t.set_timing(True, 2)
        scopes = {}
        t.reset_timing()
        rec.recommend_all(uid, how)
        scopes["recommend_all_943"] = {s: dict(zip(("ms", "launches"), t.timing(s))) for s in ("item_estimate", "item_block")}
        t.reset_timing()
        t.item_estimates_batch(po, pi, pv, co, ci, capper)
        scopes["estimates_sample"] = {"item_estimate": dict(zip(("ms", "launches"), t.timing("item_estimate")))}
        t.reset_timing()
        for u in sample.tolist():  # the same pairs as blocks: the kernel without the ordered fp64 tail
            t.similarity_block(cands[u][2], cands[u][0])
        scopes["blocks_sample"] = {"item_block": dict(zip(("ms", "launches"), t.timing("item_block")))}
        t.set_timing(False)
        out["scopes"] = scopes
        e, b = scopes["estimates_sample"]["item_estimate"]["ms"], scopes["blocks_sample"]["item_block"]["ms"]
        out["estimate_tail_share"] = None if not e else round(max(e - b, 0.0) / e, 3)
        out["expectation_a_below_b"] = out["recommend_all"]["ms_per_user"] < (
            out["baseline"]["ms_per_user"] - out["baseline"]["spread_ms_per_user"])
        same = [[(i, float(v)) for i, v in x] for x in rec.recommend_all(sample[:4], how)]
        base = [[(i, float(v)) for i, v in x] for x in baseline()[:4]]
        out["top_items_equal_baseline_items"] = [[i for i, _ in x] for x in same] == [[i for i, _ in x] for x in base]
    finally:
        sim.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
