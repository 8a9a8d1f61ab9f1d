"""Times SketchTable.anonymous_most_similar against the only other way to the
same answer -- twin owners ingested into the table, similarities(twin, every
ID) per query and a host top-k -- on a config-2-shaped table (100K owners,
w = 4096, d = 5; bench.py's stream generator), for Q = 1, 64 and 1024
profiles of 100 keys, k = 100.

    python scripts/anonymous_probe.py [--pairs 50000000] [--out FILE.json]

One JSON document: ms per call and per profile for each Q (median of
--repeats after --warmup), the baseline's ms per query, the per-scope device
times (cms_get_timing) of one more call of each, and whether the two ways
agree on the lists.  A measurement, not a test: nothing is asserted."""
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
    return float(np.median(ts)), [round(x, 4) for x in ts]


def host_top_k(ids, sims, k):
    """(similarity descending, ID ascending), NaN excluded: TopItems.getTopUsers' order."""
    ok = ~np.isnan(sims)
    i, s = ids[ok], sims[ok]
    if i.size > k:  # keep every entry that can tie with the k-th
        kth = np.partition(s, s.size - k)[s.size - k]
        keep = s >= kth
        i, s = i[keep], s[keep]
    order = np.lexsort((i, -s))[:k]
    return i[order], s[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--keys", type=int, default=100, help="keys per profile")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-queries", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bench
    from mahout_amd import SketchTable
    from mahout_amd.synth import zipf_stream_torch

    n, d, w, qmax = 100_000, 5, 4096, 1024
    dev = torch.device("cuda", 0)
    c2 = argparse.Namespace(n_users=1_000_000, n_items=n, pairs=a.pairs)
    items, users = bench.rank_stream(c2, 0, 1, dev)
    _, pk = zipf_stream_torch(c2.n_users, qmax, qmax * a.keys, seed=77, device=dev)
    prof_keys = pk.reshape(qmax, a.keys).contiguous()
    twin_rows = (n + torch.arange(qmax, device=dev)).repeat_interleave(a.keys)
    rows = torch.cat([items, twin_rows])
    keys = torch.cat([users, prof_keys.reshape(-1)])
    out = {"shape": {"owners": n, "twins": qmax, "depth": d, "width": w, "pairs": int(rows.numel()),
                     "keys_per_profile": a.keys, "k": a.k},
           "device": torch.cuda.get_device_name(0)}
    with SketchTable(n + qmax, depth=d, width=w, seed=42, device=0) as t:
        t.ingest_device_rows(rows, keys, None, int(rows.numel()))
        t.finalize()
        t.synchronize()
        del rows, keys, items, users
        st = t.stats()
        out["table"] = {k_: st[k_] for k_ in ("stored_bytes", "list_rows", "hot_rows", "u8_rows", "nibble_rows",
                                              "crumb_rows", "bit_rows")}
        out["batch"] = {"u16": t.anonymous_batch(2), "u32": t.anonymous_batch(4)}
        all_ids = np.arange(n + qmax, dtype=np.int64)
        hk = prof_keys.cpu().numpy()
        off_all = np.arange(qmax + 1, dtype=np.int64) * a.keys

        def new_call(q):
            return t.anonymous_most_similar((off_all[:q + 1], hk[:q].reshape(-1), None), a.k)

        out["new"] = {}
        for q in (1, 64, 1024):
            ms, runs = median_ms(lambda: new_call(q), a.warmup, a.repeats if q < 1024 else max(3, a.repeats // 2))
            out["new"][str(q)] = {"ms_per_call": round(ms, 4), "ms_per_profile": round(ms / q, 5), "runs_ms": runs}

        nb = a.baseline_queries

        def base_call():
            for q in range(nb):
                host_top_k(all_ids, t.similarities(n + q, all_ids), a.k)

        ms, runs = median_ms(base_call, 1, 3)
        out["baseline"] = {"queries": nb, "ms_per_query": round(ms / nb, 5), "runs_ms": runs}
        sims_only, _ = median_ms(lambda: [t.similarities(n + q, all_ids) for q in range(nb)], 1, 3)
        out["baseline"]["ms_per_query_similarities_only"] = round(sims_only / nb, 5)

        # per-scope device times of one more call of each
        t.set_timing(True, 2)
        scopes = {}
        for label, fn in (("new_q64", lambda: new_call(64)), ("new_q1024", lambda: new_call(1024)),
                          ("baseline_64", base_call)):
            t.reset_timing()
            fn()
            scopes[label] = {s: dict(zip(("ms", "launches"), t.timing(s)))
                             for s in ("anon_sketch", "anon_cosine", "top_k", "pair_cosine")}
        t.set_timing(False)
        out["scopes"] = scopes

        ids, sc, cnt = new_call(8)
        same = True
        for q in range(8):
            bi, bs = host_top_k(all_ids, t.similarities(n + q, all_ids), a.k)
            same = same and cnt[q] == bi.size and ids[q, :cnt[q]].tolist() == bi.tolist() \
                and sc[q, :cnt[q]].tolist() == bs.tolist()
        out["lists_equal_baseline"] = bool(same)
    out["acceptance_q64_per_profile_below_baseline"] = \
        out["new"]["64"]["ms_per_profile"] < out["baseline"]["ms_per_query"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
