"""Times k_nb_estimate (cms_neighbor.hip) next to k_exact_estimate (cms_exact.hip) on the same batch, in one process.

    python scripts/nb_estimate_probe.py [--out FILE.json]   (default: profiles/r27/nb_estimate_probe.json)

The model: the ML-100K-shaped one (943 users, 1,682 items).  The neighbourhoods: NearestNUserNeighborhood over
PearsonCorrelationSimilarity at n = 10 and n = 50.  The candidates: recommend_all's, the neighbours' items less the
user's own.  For each n, after --warmup rounds, --repeats rounds of one call of each, alternating:
  exact  cms_exact_estimate_preferences_batch: scope exact_estimate (k_exact_estimate, a barrier per neighbour)
  nb     cms_neighbor_estimate_preferences_batch, Pearson, generic kind: scope nb_estimate (k_nb_estimate, two
         barriers per chunk of 16 neighbours)
with the device-synchronised scopes of both, medians, extremes and every run.  Both kernels add the same data points
when neither measure is NaN on a neighbourhood; the NaN similarities of both are counted.  The yardstick:
nb_estimate no slower than exact_estimate beyond exact_estimate's own spread (max - min) in this call.
Then recommend_all per user, end to end, for GenericUserBasedRecommender over Pearson and for
GenericBooleanPrefUserBasedRecommender over LogLikelihoodSimilarity on the same lists without values, at n = 10.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "nb_estimate_probe.json"))
    a = ap.parse_args()

    import torch

    from mahout_amd import taste
    from mahout_amd.datamodel import GenericDataModel
    from mahout_amd.synth import movielens_like

    users, items, ratings = movielens_like()
    uid = np.unique(users)
    rows = np.searchsorted(uid, users)
    order = np.lexsort((items, rows))
    rows, items, ratings = rows[order], items[order], np.asarray(ratings, np.float32)[order]
    off = np.zeros(uid.size + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=uid.size), out=off[1:])
    model = GenericDataModel.from_csr(uid, off, items, ratings)
    out = {"shape": {"users": int(uid.size), "items": model.getNumItems(), "preferences": int(items.size)},
           "device": torch.cuda.get_device_name(0)}
    sim = taste.PearsonCorrelationSimilarity(model, device=0)
    try:
        t = sim.table
        t.set_timing(True, 2)
        capper = (model.getMinPreference(), model.getMaxPreference())
        for n in (10, 50):
            nbo, nb = taste.NearestNUserNeighborhood(n, sim, model).getUserNeighborhoods(uid)
            nbr = np.searchsorted(uid, nb)
            cands = [np.setdiff1d(np.concatenate([items[off[r]:off[r + 1]] for r in nbr[nbo[u]:nbo[u + 1]]] +
                                                 [np.zeros(0, np.int64)]), items[off[u]:off[u + 1]])
                     for u in range(uid.size)]
            ito = np.zeros(uid.size + 1, np.int64)
            np.cumsum([c.size for c in cands], out=ito[1:])
            keys = np.concatenate(cands)
            pair_user = np.repeat(uid, np.diff(nbo))
            calls = {"exact": (lambda: t.exact_estimate_preferences_batch(uid, nbo, nb, ito, keys, capper),
                               ("exact_estimate", "exact_pairs")),
                     "nb": (lambda: t.neighbor_estimate_preferences_batch(uid, nbo, nb, ito, keys, "pearson", "generic",
                                                                          capper), ("nb_estimate", "nb_pairs"))}
            runs = {name: [] for name in calls}
            est = {}
            for r in range(a.warmup + a.repeats):
                for name, (fn, scopes) in calls.items():
                    t.reset_timing()
                    t0 = time.perf_counter()
                    est[name] = fn()
                    wall = (time.perf_counter() - t0) * 1e3
                    if r >= a.warmup:
                        runs[name].append({"wall_ms": round(wall, 3), **{s: round(t.timing(s)[0], 4) for s in scopes}})
            res = {"neighbours": int(nb.size), "candidates": int(keys.size),
                   "nan_similarities": {"exact": int(np.isnan(t.exact_pairs(pair_user, nb)).sum()),
                                        "pearson": int(np.isnan(t.common_pairs(pair_user, nb, "pearson")).sum())},
                   "same_nan_estimates": bool(np.array_equal(np.isnan(est["exact"]), np.isnan(est["nb"])))}
            for name, rs in runs.items():
                res[name] = {"median": {k: float(np.median([x[k] for x in rs])) for k in rs[0]},
                             "min_max": {k: [min(x[k] for x in rs), max(x[k] for x in rs)] for k in rs[0]}, "runs": rs}
            ex, new = res["exact"]["median"]["exact_estimate"], res["nb"]["median"]["nb_estimate"]
            lo, hi = res["exact"]["min_max"]["exact_estimate"]
            res["compare"] = {"nb_estimate_over_exact_estimate": round(new / ex, 3),
                              "exact_estimate_spread_ms": round(hi - lo, 4),
                              "nb_no_slower_beyond_spread": new <= ex + (hi - lo)}
            out[f"n_{n}"] = res
    finally:
        sim.close()

    # end to end: recommend_all per user for the two recommender classes
    out["recommend_all"] = {}
    boolean = GenericDataModel.from_csr(uid, off, items, None)
    for name, cls, dm, sim_cls in (
            ("generic_pearson", taste.GenericUserBasedRecommender, model, taste.PearsonCorrelationSimilarity),
            ("boolean_loglikelihood", taste.GenericBooleanPrefUserBasedRecommender, boolean, taste.LogLikelihoodSimilarity)):
        sim = sim_cls(dm, device=0)
        try:
            rec = cls(dm, taste.NearestNUserNeighborhood(10, sim, dm), sim)
            ms = []
            for r in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                lists = rec.recommend_all(uid, 10)  # ends in the library's stream synchronise
                ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            ms = ms[a.warmup:]
            out["recommend_all"][name] = {"users": int(uid.size), "lists_with_10": int(sum(len(x) == 10 for x in lists)),
                                          "wall_ms_median": float(np.median(ms)), "min_max": [min(ms), max(ms)],
                                          "ms_per_user": round(float(np.median(ms)) / uid.size, 5)}
        finally:
            sim.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
