"""Merging a saved table into a live one (cms_merge_table_device) on the
headline table (config 3: 1M x 5 x 8192 built from the 500M-pair Zipf stream)
and on that table after 20 streaming batches of 10M pairs, each beside its
memory-bound yardstick taken in the same process:

  config 3 + config 3   a second config-3 table (another stream) merged into
                        the first: every row receives, list rows meet lists
  streamed + delta      the table after 20 streamed batches receives the
                        image of 20 further batches built in a handle of their
                        own -- and, for comparison, the only alternative
                        without a merge: the same 20 batches re-ingested into
                        a restored copy of the live table

  ckpt_verify / ckpt_add  the library's timing scopes (kernel time):
                          k_ckpt_unpack<false>; k_ckpt_apply<kAdd> and
                          k_ckpt_apply_lists<kAdd>
  yardstick               a device-to-device copy of the image's bytes plus a
                          read-and-write pass over as many bytes as the live
                          table stores after the merge (the rows it touched)

    python scripts/merge_probe.py [out.json] [stream batches] [owners] [build pairs]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "merge_probe.json"
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


def build(seed):
    t = SketchTable(n, depth=d, width=w, seed=42, device=0)
    it_, us = zipf_stream_torch(10_000_000, n, build_pairs, seed=seed, device="cuda")
    ms = wall(lambda: (t.ingest_device_rows(it_, us, None, int(it_.numel())), t.finalize()))
    return t, ms


def stream(t, seed0):
    ms = 0.0
    for b in range(nb):
        it_, us = zipf_stream_torch(10_000_000, n, 10_000_000, seed=seed0 + b, device="cuda")
        ms += wall(lambda: t.ingest_device_rows(it_, us, None, int(it_.numel())))
        del it_, us
    return ms


def measure(label, live, image):
    res = {"case": label, "image_bytes": int(image.numel())}
    before = live.stats()
    res["stored_bytes_before"], res["table_bytes_before"] = before["stored_bytes"], before["table_bytes"]
    res["forms_before"] = {k: before[k] for k in FORM_KEYS}
    live.set_timing(True, level=2)
    live.reset_timing()
    res["merge_wall_ms"] = wall(lambda: live.merge_device(image))
    for scope in ("ckpt_verify", "ckpt_add", "widen_rows"):
        res[scope + "_ms"] = live.timing(scope)[0]
    res["finalize_wall_ms"] = wall(live.finalize)
    after = live.stats()
    res["stored_bytes_after"], res["table_bytes_after"] = after["stored_bytes"], after["table_bytes"]
    res["forms_after"] = {k: after[k] for k in FORM_KEYS}
    res["pairs_ingested_after"] = after["pairs_ingested"]
    # the yardstick: the image copied device to device, the touched rows' bytes read and written once
    twin = torch.empty_like(image)
    twin.copy_(image)
    res["dtod_image_ms"] = min(event_ms(lambda: twin.copy_(image)) for _ in range(5))
    del twin
    dst = torch.zeros(int(after["stored_bytes"]) // 8, dtype=torch.int64, device=image.device)
    dst.add_(1)
    res["rw_dest_ms"] = min(event_ms(lambda: dst.add_(1)) for _ in range(5))
    del dst
    yard = res["dtod_image_ms"] + res["rw_dest_ms"]
    res["yardstick_ms"] = yard
    res["add_over_yardstick"] = res["ckpt_add_ms"] / yard
    res["verify_over_dtod"] = res["ckpt_verify_ms"] / res["dtod_image_ms"]  # (the verify pass only reads)
    res["wall_over_yardstick"] = res["merge_wall_ms"] / yard
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


results = {"shape": [n, d, w], "build_pairs": build_pairs, "stream_batches": nb, "cases": []}
live, results["build_wall_ms"] = build(20261015)
other, _ = build(20261016)
image = other.save_device()
results["cases"].append(measure("config 3 + config 3", live, image))
del image
live.close()
# `other` becomes the streamed table; the delta is built in a handle of its own
results["stream_wall_ms"] = stream(other, 555_000)
other.finalize()
pre = other.save_device()  # the live table before the merge, for the re-ingest alternative
delta = SketchTable(n, depth=d, width=w, seed=42, device=0)
results["delta_build_wall_ms"] = stream(delta, 777_000)
delta.finalize()
image = delta.save_device()
delta.close()
results["cases"].append(measure("streamed + delta of %d batches" % nb, other, image))
del image
# the alternative a caller has without a merge: the second stream again, into the live table
again = SketchTable(n, depth=d, width=w, seed=42, device=0)
again.load_device(pre)
again.finalize()
del pre
results["reingest_wall_ms"] = stream(again, 777_000)
results["reingest_finalize_wall_ms"] = wall(again.finalize)
rows = [0, 1, n // 2, n - 1]
results["merge_equals_reingest_sample"] = bool(all(
    torch.equal(other.read_counters_device(r, 1), again.read_counters_device(r, 1)) for r in rows))
results["reingest_over_merge_wall"] = results["reingest_wall_ms"] / results["cases"][1]["merge_wall_ms"]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
print(json.dumps({"written": out_path}))
