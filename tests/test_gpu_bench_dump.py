"""GPU: a plain bench.py run (no --full) at a small shape, in this process.

--dump-outputs writes what the last timed step computed: the sampled counters
and similarities equal the oracle's for the same seeded stream bit for bit,
two runs with the same arguments write identical files, and the result line
holds the headline keys and none of the --full measurements."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, USERS, PAIRS, D, W = 600, 20_000, 200_000, 5, 1024
NAMES = ("counter_rows", "counters", "similarity_queries", "similarity_candidates", "similarities")


def _run(bench, capsys, outdir, steps):
    bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--n-items", str(N), "--n-users", str(USERS),
                "--pairs", str(PAIRS), "--depth", str(D), "--width", str(W), "--dump-outputs", str(outdir)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return line, {k: np.load(os.path.join(str(outdir), k + ".npy")) for k in NAMES}


def test_plain_run_dumps_the_last_step(oracle, capsys, tmp_path):
    import bench
    line, got = _run(bench, capsys, tmp_path / "a", steps=2)
    _, again = _run(bench, capsys, tmp_path / "b", steps=3)

    # the line: the headline's keys, --steps timed steps, nothing that --full measures
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(PAIRS / (line["ms_per_step"] * 1e-3))
    for k in ("cpu_baseline", "cosines_per_s", "breakdown_ms_per_step", "config2", "config1"):
        assert k not in line, k
    assert "cfg2_updates_per_s" not in line["summary"] and "cfg4_wall_s" not in line["summary"]

    # the files: float64, within the size limit, the same from run to run
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT_BYTES == 64_000_000
    for k in NAMES:
        assert got[k].dtype == np.float64, k
        assert np.array_equal(got[k], again[k], equal_nan=True), k

    # ... and they hold the finished table of the seeded stream
    import torch
    items, users = bench.config3_shard(N, USERS, PAIRS, 0, 1, "cuda:0")
    items, users = items.cpu().numpy(), users.cpu().numpy()
    torch.cuda.empty_cache()
    a, b = oracle.hash_params(42, D)
    exp = oracle.build_table(N, D, W, a, b, items, users)
    rows = got["counter_rows"].astype(np.int64)
    assert rows.size >= 8 and got["counters"].shape == (rows.size, D, W)
    assert set(np.argsort(-np.bincount(items, minlength=N), kind="stable")[:8]) <= set(rows)
    assert np.array_equal(got["counters"], exp[rows])
    cands = got["similarity_candidates"].astype(np.int64)
    queries = got["similarity_queries"].astype(np.int64)
    assert got["similarities"].shape == (queries.size, cands.size)
    for qi, q in enumerate(queries):
        ref = oracle.similarities_row(exp, int(q))
        ref[q] = oracle.cosine_cm(exp[q], exp[q])
        assert np.array_equal(got["similarities"][qi], ref[cands], equal_nan=True), q
