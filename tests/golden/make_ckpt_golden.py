"""Writes tests/golden/ckpt_v1_small.bin: a checkpoint (format version 1) of a
tiny table -- n = 64, d = 4, w = 128 -- holding at least one row of every
form a row build and later batches leave side by side at this shape (list,
1-, 2-, 4-, 8-, 16-bit and u32 rows; owners on the shared zero row exist only
in tables no row build has laid out, which hold no list rows).  Run once on
the GPU:

    python tests/golden/make_ckpt_golden.py

tests/test_checkpoint_host.py decodes the file with the pure-numpy reader
(mahout_amd.checkpoint) and compares it with the oracle's build_table of
golden_stream() below, which pins the format for later changes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ckpt_v1_small.bin")
N, D, W, SEED, N_KEYS = 64, 4, 128, 42, 5000


def golden_stream():
    """[(owners, keys, weights or None for unit increments)]: a row build,
    then a first-touch batch.

    Batch 1 (>= 262144 pairs: the row build): owners 0-1 pass mass 2^16 (u32
    hot rows), owners 2-7 are wide narrow rows, owners 8-23 have 1..7 distinct
    keys (list rows).  Batch 2 (small: first touches by weight): owners 32-55
    become 1-, 2-, 4-, 8- and 16-bit rows.  Owners 24-31 and 56-63 have no
    keys (the row build gives them 1-bit rows of zeros)."""
    rng = np.random.Generator(np.random.PCG64(2024))
    rows, keys = [], []
    for o, cnt in ((0, 90000), (1, 70000), (2, 40000), (3, 30000), (4, 20000), (5, 8000), (6, 3000), (7, 1200)):
        rows.append(np.full(cnt, o, np.int64))
        keys.append(rng.integers(0, N_KEYS, cnt, dtype=np.int64))
    for o in range(8, 24):
        m = 1 + (o - 8) % 7
        rows.append(np.full(m, o, np.int64))
        keys.append(rng.choice(N_KEYS, m, replace=False).astype(np.int64))
    r1, k1 = np.concatenate(rows), np.concatenate(keys)
    perm = rng.permutation(r1.size)
    r1, k1 = r1[perm], k1[perm]
    assert r1.size >= 262144
    r2 = np.arange(32, 56, dtype=np.int64)
    k2 = (r2 * 37 + 11) % N_KEYS
    w2 = np.array([1, 2, 10, 200, 1000], np.float32)[np.arange(r2.size) % 5]
    return [(r1, k1, None), (r2, k2, w2)]  # (list rows need unit increments without a value array)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from mahout_amd import SketchTable
    from mahout_amd.checkpoint import read_checkpoint, ROW_FORMS

    with SketchTable(N, depth=D, width=W, seed=SEED) as t:
        for r, k, v in golden_stream():
            t.ingest(r, k, v)
        t.finalize()
        t.save(OUT)
    c = read_checkpoint(OUT)
    print(c.form_counts(), os.path.getsize(OUT), "bytes")
    assert set(c.form_counts()) == set(ROW_FORMS) - {"f64", "zero"}, c.form_counts()
    assert os.path.getsize(OUT) < 100 * 1024
