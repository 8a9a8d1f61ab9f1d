"""Subtracting a saved table from a live one (cms_subtract_table_device) on
the tables of scripts/merge_probe.py, each figure beside two yardsticks taken
in the same process:

  streamed - delta      the table after 20 streamed batches of 10M pairs
                        receives the image of 20 further batches (a merge: the
                        add's figures) and then loses it again
  config 3 - config 3   a fresh config-3 table (1M x 5 x 8192 from the 500M-pair
                        Zipf stream) receives a second fresh config-3 table and
                        loses it again; and a table built fresh from both
                        streams at once, list rows and all, loses the second

  ckpt_verify / ckpt_subcheck / ckpt_sub / widen_rows   the library's timing
                        scopes (kernel time) of the subtraction: ckpt_subcheck
                        is k_ckpt_apply<kCheck> and k_ckpt_check_rows,
                        ckpt_sub k_ckpt_apply<kSub> and k_ckpt_apply_lists<kSub>
  (a) memory-bound      a device-to-device copy of the image's bytes plus a
                        read-and-write pass over the live table's stored bytes
                        (ckpt_sub); the copy plus a read pass over them
                        (ckpt_subcheck, which stores nothing)
  (b) ckpt_add          of the very same image into the very same table, one
                        step earlier

    python scripts/subtract_probe.py [out.json] [stream batches] [owners] [build pairs]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "subtract_probe.json"
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
build_pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 500_000_000
d, w = 5, 8192
FORM_KEYS = ("hot_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows", "list_rows")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pairs_of(seeds):
    its, uss = zip(*[zipf_stream_torch(10_000_000, n, build_pairs, seed=s, device="cuda") for s in seeds])
    return (its[0], uss[0]) if len(seeds) == 1 else (torch.cat(its), torch.cat(uss))


def build(seeds):
    t = SketchTable(n, depth=d, width=w, seed=42, device=0)
    it_, us = pairs_of(seeds)
    t.ingest_device_rows(it_, us, None, int(it_.numel()))
    t.finalize()
    torch.cuda.synchronize()
    return t


def stream(t, seed0):
    for b in range(nb):
        it_, us = zipf_stream_torch(10_000_000, n, 10_000_000, seed=seed0 + b, device="cuda")
        t.ingest_device_rows(it_, us, None, int(it_.numel()))
        del it_, us
    torch.cuda.synchronize()


def forms(stats):
    return {k: stats[k] for k in FORM_KEYS}


def measure(label, live, image, merge_first):
    """merge_first: the image is merged into `live` first (the add's figures);
    else `live` already holds the image's stream."""
    res = {"case": label, "image_bytes": int(image.numel())}
    live.set_timing(True, level=2)
    if merge_first:
        live.reset_timing()
        res["merge_wall_ms"] = wall(lambda: live.merge_device(image))
        res["ckpt_add_ms"] = live.timing("ckpt_add")[0]
        res["merge_widen_rows_ms"] = live.timing("widen_rows")[0]
    before = live.stats()
    res["stored_bytes_before"], res["table_bytes_before"] = before["stored_bytes"], before["table_bytes"]
    res["forms_before"] = forms(before)
    live.reset_timing()
    res["subtract_wall_ms"] = wall(lambda: live.subtract_device(image))
    for scope in ("ckpt_verify", "ckpt_subcheck", "ckpt_sub", "widen_rows"):
        res[scope + "_ms"] = live.timing(scope)[0]
    res["finalize_wall_ms"] = wall(live.finalize)
    after = live.stats()
    res["stored_bytes_after"], res["table_bytes_after"] = after["stored_bytes"], after["table_bytes"]
    res["forms_after"] = forms(after)
    res["pairs_ingested_after"] = after["pairs_ingested"]
    # (a): the image copied device to device; the live table's stored bytes read, and read and written, once
    twin = torch.empty_like(image)
    twin.copy_(image)
    res["dtod_image_ms"] = min(event_ms(lambda: twin.copy_(image)) for _ in range(5))
    del twin
    words = int(max(before["stored_bytes"], after["stored_bytes"])) // 8
    dst = torch.zeros(words, dtype=torch.int64, device=image.device)
    dst.add_(1)
    res["rw_live_ms"] = min(event_ms(lambda: dst.add_(1)) for _ in range(5))
    res["read_live_ms"] = min(event_ms(lambda: dst.sum()) for _ in range(5))
    del dst
    res["sub_yardstick_ms"] = res["dtod_image_ms"] + res["rw_live_ms"]
    res["check_yardstick_ms"] = res["dtod_image_ms"] + res["read_live_ms"]
    res["sub_over_yardstick"] = res["ckpt_sub_ms"] / res["sub_yardstick_ms"]
    res["check_over_yardstick"] = res["ckpt_subcheck_ms"] / res["check_yardstick_ms"]
    res["check_over_sub"] = res["ckpt_subcheck_ms"] / res["ckpt_sub_ms"]
    if merge_first:  # (b)
        res["sub_over_add"] = res["ckpt_sub_ms"] / res["ckpt_add_ms"]
        res["check_over_add"] = res["ckpt_subcheck_ms"] / res["ckpt_add_ms"]
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def same_rows(a, b):
    rows = [0, 1, n // 2, n - 1]
    return bool(all(torch.equal(a.read_counters_device(r, 1), b.read_counters_device(r, 1)) for r in rows))


results = {"shape": [n, d, w], "build_pairs": build_pairs, "stream_batches": nb, "cases": []}
S1, S2 = 20261015, 20261016
other = build([S2])
image = other.save_device()
live = build([S1])
results["cases"].append(measure("config 3 + config 3 - config 3", live, image, True))
both = build([S1, S2])  # fresh from both streams at once: its list rows lose the image's entries
results["cases"].append(measure("fresh config 3 of both streams - config 3", both, image, False))
results["fresh_equals_merged_then_subtracted_sample"] = same_rows(live, both)
both.close()
live.close()
del image
# `other` becomes the streamed table; the delta is built in a handle of its own
stream(other, 555_000)
other.finalize()
delta = SketchTable(n, depth=d, width=w, seed=42, device=0)
stream(delta, 777_000)
delta.finalize()
image = delta.save_device()
delta.close()
pre = [other.read_counters_device(r, 1).clone() for r in (0, 1, n // 2, n - 1)]
results["cases"].append(measure("streamed + delta of %d batches - delta" % nb, other, image, True))
results["streamed_restored_sample"] = bool(all(
    torch.equal(x, other.read_counters_device(r, 1)) for x, r in zip(pre, (0, 1, n // 2, n - 1))))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
print(json.dumps({"written": out_path}))
