"""Folding a live table to a narrower width (cms_fold_table_device) beside a
plain save of the same table and a device copy of its stored bytes, taken in
one process on the same table:

  config 3              a fresh config-3 table (1M x 5 x 8192 from the 500M-pair
                        Zipf stream)
  config 3 + 20 batches the same table after 20 streamed 10M-pair batches (the
                        in-place writers have widened and moved rows)

  fold_scan / fold_pack the library's timing scopes (kernel time) of the two
                        kernels, for a fold to w / 2 and to w / 4
  ckpt_pack             of save_device() on the same table: it reads and writes
                        the stored bytes once
  d2d copy              stored_bytes copied device to device

  Expected: the fold reads the stored bytes twice and writes less than it
  reads, at most 1.5 x ckpt_pack's traffic, so scan + pack within 2 x ckpt_pack
  (1.5 with a 1.25 x margin and some slack for the strided group walk).  Past
  that a cause is to be looked for.  A figure to record, not a condition.

    python scripts/fold_probe.py [out.json] [owners] [build pairs] [batches]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable, checkpoint as ck  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r16/fold_probe.json"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
build_pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 500_000_000
batches = int(sys.argv[4]) if len(sys.argv) > 4 else 20
d, w = 5, 8192
FORM_KEYS = ("hot_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows", "list_rows")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def state(t):
    s = t.stats()
    out = {"stored_bytes": s["stored_bytes"], "table_bytes": s["table_bytes"], "pairs_ingested": s["pairs_ingested"]}
    out.update({k: s[k] for k in FORM_KEYS})
    return out


def image_forms(image):
    """Rows by form and payload bytes of a device image, from its header and directory alone."""
    hd = np.frombuffer(image[:ck.HEADER_BYTES].cpu().numpy().tobytes(), ck.HEADER)[0]
    lo, hi = int(hd["dir_off"]), int(hd["dir_off"]) + int(hd["dir_bytes"])
    forms = np.frombuffer(image[lo:hi].cpu().numpy().tobytes(), ck.DIR_ENTRY)["form"]
    counts = np.bincount(forms, minlength=len(ck.ROW_FORMS))
    return {"stored_bytes": int(hd["payload_bytes"]), "rows": {ck.ROW_FORMS[f]: int(c) for f, c in enumerate(counts) if c}}


def measure(t):
    res = {"source": state(t)}
    t.set_timing(True, level=2)
    t.reset_timing()
    held = []
    res["save_wall_ms"] = wall(lambda: held.append(t.save_device()))
    res["ckpt_pack_ms"] = t.timing("ckpt_pack")[0]
    res["image_bytes"] = int(held[0].numel())
    held.clear()
    stored = res["source"]["stored_bytes"]
    a = torch.empty(stored, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    wall(lambda: b.copy_(a))  # (first touch)
    res["d2d_copy_ms"] = min(wall(lambda: b.copy_(a)) for _ in range(3))
    del a, b
    for div in (2, 4):
        t.reset_timing()
        res_w = {"width": w // div}
        res_w["fold_wall_ms"] = wall(lambda: held.append(t.fold_device(w // div)))  # (fold_size + the fold: two scans)
        scan_ms, scans = t.timing("fold_scan")
        res_w["fold_scan_ms"] = scan_ms / max(scans, 1)
        res_w["fold_pack_ms"] = t.timing("fold_pack")[0]
        res_w["scan_plus_pack_ms"] = res_w["fold_scan_ms"] + res_w["fold_pack_ms"]
        res_w["ratio_to_ckpt_pack"] = res_w["scan_plus_pack_ms"] / res["ckpt_pack_ms"] if res["ckpt_pack_ms"] else None
        res_w["folded"] = image_forms(held[0])
        held.clear()
        res["w/%d" % div] = res_w
    t.set_timing(False)
    return res


res = {"owners": n, "depth": d, "width": w, "build_pairs": build_pairs, "batches": batches}
with SketchTable(n, depth=d, width=w, seed=42, device=0) as t:
    it_, us = zipf_stream_torch(10_000_000, n, build_pairs, seed=20261015, device="cuda")
    t.ingest_device_rows(it_, us, None, int(it_.numel()))
    t.finalize()
    del it_, us
    res["config3"] = measure(t)
    print(json.dumps(res["config3"]), file=sys.stderr, flush=True)
    for b in range(batches):
        it_, us = zipf_stream_torch(10_000_000, n, 10_000_000, seed=555_000 + b, device="cuda")
        t.ingest_device_rows(it_, us, None, int(it_.numel()))
        del it_, us
    t.finalize()
    res["streamed"] = measure(t)

print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
