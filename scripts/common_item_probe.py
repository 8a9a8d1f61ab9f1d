"""Times GenericItemBasedRecommender.recommend_all over PearsonCorrelationSimilarity
(cms_common_item_recommend_batch: one k_common_item_estimate launch) next to the host route it replaces and to
k_common_tile over the same (user, preferred item) queries, in one process.

    python scripts/common_item_probe.py [--out FILE.json]   (default: profiles/r26/common_item_probe.json)

The model: the ML-100K-shaped one with its integer ratings (943 users, 1,682 items); Pearson, weighted kind, the
default strategy, how_many 10.  After --warmup rounds, --repeats rounds of one call of each, alternating:
  a  recommend_all for all users by the device route: wall ms, per user, and the scope common_item_estimate
  b  the host route for a fixed sample of users: one itemSimilarities call (a k_common_pairs launch, a copy back, a
     stream synchronise) per candidate, item_estimate and get_top_items; the candidate sets are formed before the
     clock starts, as in set_item_probe.py
  c  common_top_k on the key side with every user's preferred items as the queries, on a second handle created with
     CMS_COMMON_TILE equal to the estimate tile: k_common_tile walks the same posting entries with the same
     searches, entry after entry
with medians, extremes and every run, a per user against b per user less b's spread, and the ratio
common_item_estimate / common_tile, whatever it is; then
  d  the common_item_estimate scope of recommend_all for the one user with the most preferences among those that
     have a candidate left, alone -- one workgroup per tile, the serial chain of preferred items -- and for all
     users of at most 256 preferences
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "common_item_probe.json"))
    a = ap.parse_args()

    import torch

    from mahout_amd import SketchTable, taste
    from mahout_amd.datamodel import GenericDataModel
    from mahout_amd.synth import movielens_like

    how, tile = 10, 1024  # Pearson, weighted: the default tile
    users, items, ratings = movielens_like()
    uid = np.unique(users)
    rows = np.searchsorted(uid, users)
    order = np.lexsort((items, rows))
    rows, items, ratings = rows[order], items[order], np.asarray(ratings, np.float32)[order]
    off = np.zeros(uid.size + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=uid.size), out=off[1:])
    model = GenericDataModel.from_csr(uid, off, items, ratings)
    out = {"shape": {"users": int(uid.size), "items": model.getNumItems(), "preferences": int(items.size),
                     "measure": "pearson", "kind": "weighted", "how_many": how, "tile": tile},
           "device": torch.cuda.get_device_name(0)}
    sim = taste.PearsonCorrelationSimilarity(model, device=0)
    os.environ["CMS_COMMON_TILE"] = str(tile)  # read at cms_create: the yardstick's handle alone
    yard = SketchTable(uid.size, depth=1, width=32, device=0, owner_ids=uid)
    del os.environ["CMS_COMMON_TILE"]
    try:
        yard.attach_exact(model)
        rec = taste.GenericItemBasedRecommender(model, sim)
        capper = taste.build_capper(model)
        sample = uid[np.random.default_rng(11).choice(uid.size, a.sample, replace=False)]
        whole = rec.recommend_all(sample, model.getNumItems() + 1)  # every candidate with an estimate
        cands = {u: sorted(i for i, _ in r) for u, r in zip(sample.tolist(), whole)}
        out["sample"] = {"users": int(sample.size), "candidates": int(sum(len(c) for c in cands.values()))}

        def host_route():
            res = []
            for u in sample.tolist():
                keys, vals = model.getPreferencesFromUser(u)
                est = [taste.item_estimate(sim.itemSimilarities(c, keys), vals, capper) for c in cands[u]]
                res.append(taste.get_top_items(how, cands[u], est))
            return res

        calls = {"a_device_all_users": (sim.table, lambda: rec.recommend_all(uid, how), ("common_item_estimate",)),
                 "b_host_route_sample": (sim.table, host_route, ("common_pairs",)),
                 "c_common_tile_yardstick": (yard, lambda: yard.common_top_k(items, how, "pearson", "key"),
                                             ("common_tile", "common_pairs", "top_k"))}
        runs = {name: [] for name in calls}
        sim.table.set_timing(True, 2)
        yard.set_timing(True, 2)
        for r in range(a.warmup + a.repeats):
            for name, (t, fn, scopes) in calls.items():
                t.reset_timing()
                t0 = time.perf_counter()
                fn()
                wall = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    runs[name].append({"wall_ms": round(wall, 3), **{s: round(t.timing(s)[0], 3) for s in scopes},
                                       "launches": t.timing(scopes[0])[1]})
        for name, rs in runs.items():
            out[name] = {"median": {k: float(np.median([r[k] for r in rs])) for k in rs[0]},
                         "min_max": {k: [min(r[k] for r in rs), max(r[k] for r in rs)] for k in rs[0]}, "runs": rs}
        pa = out["a_device_all_users"]["median"]["wall_ms"] / uid.size
        pb = out["b_host_route_sample"]["median"]["wall_ms"] / sample.size
        lo, hi = out["b_host_route_sample"]["min_max"]["wall_ms"]
        alo, ahi = out["a_device_all_users"]["min_max"]["wall_ms"]
        est = out["a_device_all_users"]["median"]["common_item_estimate"]
        ylo, yhi = out["c_common_tile_yardstick"]["min_max"]["common_tile"]
        ymed = out["c_common_tile_yardstick"]["median"]["common_tile"]
        out["compare"] = {"a_ms_per_user": round(pa, 5), "a_spread_ms_per_user": round((ahi - alo) / uid.size, 5),
                          "b_ms_per_user": round(pb, 4), "b_spread_ms_per_user": round((hi - lo) / sample.size, 4),
                          "b_over_a": round(pb / pa, 1), "a_below_b_less_spread": pa < pb - (hi - lo) / sample.size,
                          "common_item_estimate_over_common_tile": round(est / ymed, 3),
                          "yardstick_spread_over_median": round((yhi - ylo) / ymed, 3)}
        npref = np.diff(off)
        heavy = uid[np.argmax(np.where(npref < model.getNumItems(), npref, 0))]  # (all items held: no candidate, no tile)
        out["d_by_preference_count"] = {"preferences_median_mean_max": [float(np.median(npref)), float(npref.mean()),
                                                                        int(npref.max())],
                                        "users_holding_every_item": int((npref == model.getNumItems()).sum())}
        for name, part in (("heaviest_with_candidates", np.array([heavy])), ("at_most_256", uid[npref <= 256])):
            ms = []
            for _ in range(a.warmup + a.repeats):
                sim.table.reset_timing()
                rec.recommend_all(part, how)
                ms.append(round(sim.table.timing("common_item_estimate")[0], 3))
            ms = ms[a.warmup:]
            out["d_by_preference_count"][name] = {
                "users": int(part.size), "most_preferences": int(npref[np.searchsorted(uid, part)].max()),
                "common_item_estimate_ms": float(np.median(ms)), "min_max": [min(ms), max(ms)]}
        same = rec.recommend_all(sample[:4], how)
        out["device_lists_equal_host_route"] = [[(i, float(v)) for i, v in x] for x in same] == \
            [[(i, float(v)) for i, v in x] for x in host_route()[:4]]
    finally:
        yard.close()
        sim.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
