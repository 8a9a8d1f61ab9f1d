"""CPU: what k_set_item_estimate shares with the host (cms_set_item_plan.h and the two estimates of cms_ref.h, built as
tests/cpp/set_item_host_shim.hip) against tests/set_item_ref.py: the batch plan on unknown, repeated and unsorted
candidates at T = 64, the estimates fed point by point, and the designed order models."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import set_item_ref as I

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "set_item_host_shim.hip")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("cms_set_item_plan.h", "cms_exact_plan.h", "cms_ref.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libset_item_host_shim.so")
KINDS = ("weighted", "boolean")
p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.sih_estimate.restype = ctypes.c_float
    lib.sih_estimate.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                 ctypes.c_float, ctypes.c_float]
    return lib


def shim_estimate(shim, kind, sims, prefs, capper=None):
    s, v = np.asarray(sims, np.float64), np.asarray(prefs if prefs is not None else np.zeros(len(sims)), np.float32)
    lo, hi = capper or (0.0, 0.0)
    return np.float32(shim.sih_estimate(KINDS.index(kind), p(s), p(v), s.size, int(capper is not None), lo, hi))


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_plan(shim, n):
    """User 0: every item, shuffled, one repeated and one unknown key; user 1: the last item alone; user 2: nothing."""
    T, ids = 64, np.arange(n, dtype=np.int64) * 7 + 5
    first = np.concatenate([np.random.Generator(np.random.PCG64(n)).permutation(ids), [ids[3], 4]])
    keys = np.concatenate([first, ids[-1:]])
    off = np.array([0, first.size, keys.size, keys.size], np.int64)
    slot, pos = np.zeros(keys.size, np.int32), np.zeros(keys.size, np.int64)
    tiles, counts = np.zeros((keys.size, 4), np.int64), np.zeros(2, np.int64)
    shim.sih_plan(p(ids), ctypes.c_int64(n), ctypes.c_int64(3), p(off), p(keys), T, p(slot), p(pos), p(tiles), p(counts))
    S, nt = counts.tolist()
    assert S == n + 1 and pos[-2] == -1 and (np.delete(pos, -2) >= 0).all()  # the repeat is folded, the unknown unplaced
    assert (ids[slot[np.delete(pos, -2)]] == np.delete(keys, -2)).all()
    assert (np.diff(slot[:n]) > 0).all()  # a user's slots ascend strictly
    tiles = tiles[:nt]
    assert tiles[:, 0].tolist() == [0] * -(-n // T) + [1]  # only tiles that hold a candidate; none for user 2
    assert tiles[:, 3].tolist() == list(range(-(-n // T))) + [(n - 1) // T]
    assert tiles[0, 1] == 0 and (tiles[1:, 1] == tiles[:-1, 1] + tiles[:-1, 2]).all() and tiles[-1, 1:3].sum() == S
    for _, lo, ln, t in tiles.tolist():
        assert ln >= 1 and (slot[lo:lo + ln] // T == t).all()


@pytest.mark.parametrize("kind", KINDS)
def test_estimates_point_by_point(shim, kind):
    rng = np.random.Generator(np.random.PCG64(7))
    for m in (0, 1, 2, 3, 17):
        for nan_rate, capper in ((0.0, None), (0.4, (1.0, 5.0)), (1.0, None)):
            sims = np.where(rng.random(m) < nan_rate, np.nan, rng.random(m))
            prefs = rng.integers(1, 11, m) / np.float32(2)
            exp = I.estimate(kind, sims.tolist(), prefs, capper if kind == "weighted" else None)
            got = shim_estimate(shim, kind, sims, prefs, capper)
            assert got.view(np.int32) == exp.view(np.int32) or (math.isnan(got) and math.isnan(exp)), (m, got, exp)


@pytest.mark.parametrize("kind", KINDS)
def test_order_models(shim, kind):
    """The designed models' estimates differ between ascending and reversed preference order in the restatement
    itself -- boolean in the fp64 sum's bits, weighted in the float32 estimate -- and the shim gives the ascending."""
    lists, vals, sizes = I.order_model(kind)
    m, iu, sims = len(sizes), I.item_users(lists), [1.0 / s for s in sizes]
    assert [len(iu[i]) for i in range(m)] == list(sizes) and iu[m] == {1} and all(1 in iu[i] for i in range(m))
    if kind == "boolean":
        assert m >= 3 and np.float64(sum(sims)).view(np.int64) != np.float64(sum(sims[::-1])).view(np.int64)
    asc, rev = I.estimate(kind, sims, vals), I.estimate(kind, sims[::-1], vals and vals[::-1])
    assert kind == "boolean" or asc.view(np.int32) != rev.view(np.int32)
    assert I.estimates("tanimoto", kind, lists, range(m), vals, [m])[0].view(np.int32) == asc.view(np.int32)
    assert shim_estimate(shim, kind, sims, vals).view(np.int32) == asc.view(np.int32)
