"""Checkpoint / restore on the headline table (config 3: 1M x 5 x 8192 built
from the 500M-pair Zipf stream) and on that table after 20 streaming batches
of 10M pairs (moved rows, a fragmented arena).  Every figure sits beside the
plain copy of the same byte count it was measured against, taken in the same
process:

  device path  k_ckpt_pack / k_ckpt_unpack kernel time (the library's timing
               scopes) against torch's device-to-device copy, 5 repeats
  file path    save / load wall time to a tmpfs file against a pinned D2H /
               H2D copy of the same bytes (1 GiB pinned buffer, 3 repeats)
  sizes        image bytes against stored_bytes; table_bytes before the save
               and after the restore; the build's own wall time for context

    python scripts/checkpoint_probe.py [out.json] [stream batches] [owners] [build pairs]
"""
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
from mahout_amd import SketchTable  # noqa: E402
from mahout_amd.synth import zipf_stream_torch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "checkpoint_probe.json"
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
build_pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 500_000_000
d, w = 5, 8192
PIN = 1 << 30
shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
path = os.path.join(shm, "mahout_ckpt_probe_%d.bin" % os.getpid())


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


def chunked_copy(dst_of, src_of, nbytes):
    for o in range(0, nbytes, PIN):
        k = min(PIN, nbytes - o)
        dst_of(o, k).copy_(src_of(o, k), non_blocking=True)


def measure(label, t, spare):
    """spare: an empty handle of the same shape that takes the restores."""
    res = {"case": label}
    st = t.stats()
    t.set_timing(True, level=1)
    t.reset_timing()
    image = t.save_device()
    nbytes = int(image.numel())
    res["image_bytes"], res["stored_bytes"], res["table_bytes_before"] = nbytes, st["stored_bytes"], st["table_bytes"]
    res["image_over_stored"] = nbytes / st["stored_bytes"]
    res["pack_kernel_ms"], res["dir_kernel_ms"] = t.timing("ckpt_pack")[0], t.timing("ckpt_dir")[0] / 2  # (size + save)
    res["save_device_wall_ms"] = wall(lambda: t.save_device())
    # the plain device-to-device copy of the same bytes
    twin = torch.empty_like(image)
    twin.copy_(image)
    res["dtod_ms"] = [event_ms(lambda: twin.copy_(image)) for _ in range(5)]
    del twin
    best = min(res["dtod_ms"])
    res["pack_over_dtod"] = res["pack_kernel_ms"] / best
    res["pack_gb_s"], res["dtod_gb_s"] = 2e-6 * nbytes / res["pack_kernel_ms"], 2e-6 * nbytes / best  # read + write
    # restore from the device image
    spare.set_timing(True, level=1)
    spare.reset_timing()
    res["load_device_wall_ms"] = wall(lambda: spare.load_device(image))
    res["unpack_kernel_ms"] = spare.timing("ckpt_unpack")[0]
    res["unpack_over_dtod"] = res["unpack_kernel_ms"] / best
    spare.finalize()
    res["table_bytes_after"] = spare.stats()["table_bytes"]
    res["restored_image_equal"] = bool(torch.equal(spare.save_device(), image))
    spare.reset()
    # the file path, to tmpfs
    res["file_dir"] = shm
    t.reset_timing()
    res["save_file_wall_ms"] = wall(lambda: t.save(path))
    res["save_file_io_scope_ms"] = t.timing("ckpt_io")[0]
    res["file_bytes"] = os.path.getsize(path)
    spare.reset_timing()
    res["load_file_wall_ms"] = wall(lambda: spare.load(path))
    res["load_file_io_scope_ms"] = spare.timing("ckpt_io")[0]
    spare.finalize()
    res["file_restored_image_equal"] = bool(torch.equal(spare.save_device(), image))
    spare.reset()
    os.remove(path)
    # plain pinned copies of the same bytes
    pin = torch.empty(PIN, dtype=torch.uint8, pin_memory=True)
    d2h = lambda: chunked_copy(lambda o, k: pin[:k], lambda o, k: image[o:o + k], nbytes)  # noqa: E731
    h2d = lambda: chunked_copy(lambda o, k: image[o:o + k], lambda o, k: pin[:k], nbytes)  # noqa: E731
    wall(d2h)
    res["pinned_d2h_ms"] = [wall(d2h) for _ in range(3)]
    res["pinned_h2d_ms"] = [wall(h2d) for _ in range(3)]
    del pin  # (the H2D repeats overwrote the image: it is not used again)
    chunks = max(1, -(-nbytes // (64 << 20)))
    res["pipeline_chunks"] = chunks
    res["expected_margin"] = (chunks + 1) / chunks
    res["save_over_d2h"] = res["save_file_wall_ms"] / min(res["pinned_d2h_ms"])
    res["load_over_h2d"] = res["load_file_wall_ms"] / min(res["pinned_h2d_ms"])
    res["forms"] = {k: st[k] for k in ("hot_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows", "list_rows")}
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


t = SketchTable(n, depth=d, width=w, seed=42, device=0)
spare = SketchTable(n, depth=d, width=w, seed=42, device=0)
it_, us = zipf_stream_torch(10_000_000, n, build_pairs, seed=20261015, device="cuda")
build_ms = wall(lambda: (t.ingest_device_rows(it_, us, None, int(it_.numel())), t.finalize()))
del it_, us
results = {"shape": [n, d, w], "build_pairs": build_pairs, "build_wall_ms": build_ms, "cases": []}
results["cases"].append(measure("config 3 table", t, spare))
stream_ms = 0.0
for b in range(nb):
    it_, us = zipf_stream_torch(10_000_000, n, 10_000_000, seed=555_000 + b, device="cuda")
    stream_ms += wall(lambda: t.ingest_device_rows(it_, us, None, int(it_.numel())))
    del it_, us
t.finalize()
results["stream_batches"], results["stream_wall_ms"] = nb, stream_ms
results["cases"].append(measure("after %d streaming batches" % nb, t, spare))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
print(json.dumps({"written": out_path}))
