"""Compacting a live table (cms_compact_table) after the README's sliding
window has widened it, beside the parent route's rewrite of the same rows,
taken in the same process on the same pre-compaction table:

  config 3 + config 3 - config 3   a fresh config-3 table (1M x 5 x 8192 from
                        the 500M-pair Zipf stream) receives the image of a
                        second config-3 stream and loses it again: the counters
                        are the fresh table's, the forms are not; then compact()

  compact_scan / compact_pack   the library's timing scopes (kernel time) of
                        k_fold_scan / k_fold_pack at the table's own width;
                        ckpt_verify / ckpt_unpack the
                        restore's
  yardstick             save_device() (ckpt_pack) + reset() + load_device()
                        (ckpt_unpack) of the pre-compaction table: the same rows
                        rewritten in the forms they have.  Expected: scan + pack
                        within 2 x ckpt_pack + ckpt_unpack (they read the same
                        bytes twice and write fewer); past 2 x 1.25 a cause is
                        to be looked for.  A figure to record, not a condition.

    python scripts/compact_probe.py [out.json] [owners] [build pairs]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "compact_probe.json"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
build_pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 500_000_000
d, w = 5, 8192
FORM_KEYS = ("hot_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows", "list_rows")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def build(seed):
    t = SketchTable(n, depth=d, width=w, seed=42, device=0)
    it_, us = zipf_stream_torch(10_000_000, n, build_pairs, seed=seed, device="cuda")
    t.ingest_device_rows(it_, us, None, int(it_.numel()))
    t.finalize()
    torch.cuda.synchronize()
    return t


def state(t):
    s = t.stats()
    out = {"stored_bytes": s["stored_bytes"], "table_bytes": s["table_bytes"], "pairs_ingested": s["pairs_ingested"]}
    out.update({k: s[k] for k in FORM_KEYS})
    return out


def sample(t, rows):
    return torch.stack([t.read_counters_device(int(r), 1)[0] for r in rows])


res = {"owners": n, "depth": d, "width": w, "build_pairs": build_pairs}
with build(20261015) as second:
    image = second.save_device().clone()
res["image_bytes"] = int(image.numel())
with build(20261016) as t:
    rows = torch.randint(0, n, (64,), generator=torch.Generator().manual_seed(3)).tolist()
    res["fresh"] = state(t)
    want = sample(t, rows)
    t.merge_device(image)
    t.subtract_device(image)
    t.finalize()
    del image
    res["before"] = state(t)
    assert torch.equal(sample(t, rows), want)

    # the yardstick first, on the pre-compaction table: its rows rewritten as they are
    t.set_timing(True, level=2)
    t.reset_timing()
    snap = None

    def save():
        global snap
        snap = t.save_device()

    res["yard_save_wall_ms"] = wall(save)
    res["yard_load_wall_ms"] = wall(lambda: (t.reset(), t.load_device(snap)))
    res["yard_ckpt_pack_ms"] = t.timing("ckpt_pack")[0]
    res["yard_ckpt_unpack_ms"] = t.timing("ckpt_unpack")[0]
    res["yardstick_ms"] = res["yard_ckpt_pack_ms"] + res["yard_ckpt_unpack_ms"]
    snap = None
    t.finalize()
    res["restored"] = state(t)  # (defragmented, every form kept)
    assert torch.equal(sample(t, rows), want)

    t.reset_timing()
    changed = []
    res["compact_wall_ms"] = wall(lambda: changed.append(t.compact()))
    res["rows_changed"] = changed[0]
    for scope in ("compact_scan", "compact_pack", "ckpt_dir", "ckpt_verify", "ckpt_unpack"):
        res[scope + "_ms"] = t.timing(scope)[0]
    res["scan_plus_pack_ms"] = res["compact_scan_ms"] + res["compact_pack_ms"]
    res["ratio_to_yardstick"] = res["scan_plus_pack_ms"] / res["yardstick_ms"] if res["yardstick_ms"] else None
    res["after"] = state(t)
    assert torch.equal(sample(t, rows), want)
    res["second_compact_wall_ms"] = wall(lambda: changed.append(t.compact()))
    res["second_rows_changed"] = changed[1]

print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
