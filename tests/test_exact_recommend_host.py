"""CPU: the host side of the exact user-based recommender and its reference.

  - the plan of an estimate batch (cms_exact_plan.h, built for the host in
    tests/cpp/exact_rec_host_shim.hip): keys the model lacks, repeated and
    unsorted candidate keys, the position -> slot map, tile cuts at T = 64 for
    63, 64, 65 and 136 candidates, CMS_EXACT_EST_TILE's rounding;
  - the reference itself (tests/exact_rec_ref.py): a neighbourhood whose two
    orders give estimates that differ in their bits, so that a GPU test passing
    on it cannot be summing in another order; the 0.0 data point; and the
    reference's arithmetic against ItemEstimate fed one data point at a time,
    as k_exact_estimate feeds it.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exact_rec_ref as X
import exact_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "exact_rec_host_shim.hip")
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("cms_exact.h", "cms_exact_plan.h", "cms_ref.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libexact_rec_host_shim.so")

vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.er_tile_for.restype = ctypes.c_int
    lib.er_tile_for.argtypes = [ctypes.c_int]
    lib.er_plan.restype = i64
    lib.er_plan.argtypes = [vp, i64, i64, vp, vp, ctypes.c_int, vp, vp, ctypes.POINTER(i64), vp, vp, vp, i64]
    lib.er_estimate.restype = ctypes.c_float
    lib.er_estimate.argtypes = [vp, vp, i64, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    return lib


def _p(a):
    return a.ctypes.data_as(vp)


def _plan(shim, ids, cands, T):
    """The plan of the users' candidate lists `cands` over the model's sorted
    unique keys `ids`: (pos_slot, slot_item, [(user, lo, len)])."""
    ids = np.ascontiguousarray(ids, np.int64)
    off = np.zeros(len(cands) + 1, np.int64)
    np.cumsum([len(c) for c in cands], out=off[1:])
    keys = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int64) for c in cands] + [np.zeros(0, np.int64)]))
    Q = int(off[-1])
    pos_slot = np.full(Q, -7, np.int64)
    slot_item = np.full(Q, -7, np.int32)
    cap = Q + len(cands)
    tu, tl, tn = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    slots = i64()
    nt = shim.er_plan(_p(ids), ids.size, len(cands), _p(off), _p(keys), T, _p(pos_slot), _p(slot_item),
                      ctypes.byref(slots), _p(tu), _p(tl), _p(tn), cap)
    assert nt <= cap
    return pos_slot, slot_item[:slots.value], list(zip(tu[:nt].tolist(), tl[:nt].tolist(), tn[:nt].tolist()))


def _check_plan(ids, cands, T, pos_slot, slot_item, tiles):
    """The plan's own invariants, from Python alone."""
    ids = [int(x) for x in ids]
    dense = {k: i for i, k in enumerate(ids)}
    pos = 0
    lo = 0
    exp_tiles = []
    for u, c in enumerate(cands):
        known = sorted({dense[int(k)] for k in c if int(k) in dense})
        assert slot_item[lo:lo + len(known)].tolist() == known  # sorted, unique, the user's own
        for k in c:
            s = int(pos_slot[pos])
            if int(k) in dense:
                assert lo <= s < lo + len(known) and slot_item[s] == dense[int(k)]
            else:
                assert s == -1
            pos += 1
        exp_tiles += [(u, t, min(T, lo + len(known) - t)) for t in range(lo, lo + len(known), T)]
        lo += len(known)
    assert lo == slot_item.size and tiles == exp_tiles


def test_tile_rule(shim):
    assert shim.er_tile_for(0) == 2048 and shim.er_tile_for(-3) == 2048
    assert shim.er_tile_for(64) == 64 and shim.er_tile_for(65) == 128 and shim.er_tile_for(1) == 64
    assert shim.er_tile_for(2048) == 2048 and shim.er_tile_for(5000) == 2048


def test_plan_unknown_repeated_unsorted(shim):
    ids = [-50, 3, 7, 8, 100, 2 ** 40]
    cands = [[8, 3, 8, 999, 7, 3, -50, -51],   # repeated, unsorted, two the model lacks
             [],                                # no candidate
             [5, 6],                            # only keys the model lacks: no slot, no tile
             [2 ** 40, -50]]
    pos_slot, slot_item, tiles = _plan(shim, ids, cands, 64)
    _check_plan(ids, cands, 64, pos_slot, slot_item, tiles)
    assert slot_item.tolist() == [0, 1, 2, 3, 0, 5]
    assert pos_slot.tolist() == [3, 1, 3, -1, 2, 1, 0, -1, -1, -1, 5, 4]
    assert tiles == [(0, 0, 4), (3, 4, 2)]


@pytest.mark.parametrize("count", [63, 64, 65, 136])
def test_plan_tile_cuts(shim, count):
    rng = np.random.Generator(np.random.PCG64(count))
    ids = np.arange(400) * 3 + 1
    first = rng.permutation(ids)[:count]
    cands = [first, rng.permutation(ids)[:5], np.concatenate([first, first[:9], [2, 5]])]  # the third repeats the first
    pos_slot, slot_item, tiles = _plan(shim, ids, cands, 64)
    _check_plan(ids, cands, 64, pos_slot, slot_item, tiles)
    lens = [n for u, _, n in tiles if u == 0]
    assert lens == {63: [63], 64: [64], 65: [64, 1], 136: [64, 64, 8]}[count]
    assert [n for u, _, n in tiles if u == 2] == lens and [n for u, _, n in tiles if u == 1] == [5]
    # at the default tile everything of a user is one tile
    _, _, tiles = _plan(shim, ids, cands, shim.er_tile_for(0))
    assert [n for _, _, n in tiles] == [count, 5, count]


# ---- the reference ----

def test_reference_order_matters():
    M = X.order_model()
    sims = M.similarities_row(0)
    assert sims[1] == -sims[2] and sims[3] == -sims[4] and sims[1] > 0 and sims[3] > 0
    e1 = X.estimate(M, sims, 0, [1, 2, 3, 4], 9)
    e2 = X.estimate(M, sims, 0, [1, 3, 4, 2], 9)
    e3 = X.estimate(M, sims, 0, [2, 3, 4, 1], 9)
    assert np.isposinf(e1) and np.isfinite(e2) and np.isfinite(e3) and e2 > 1e15 and e3 < -1e15
    assert not X.same_bits32(e1, e2) and not X.same_bits32(e2, e3)
    # the capper turns them into the bounds
    assert X.estimate(M, sims, 0, [1, 2, 3, 4], 9, (0.5, 5.0)) == np.float32(5.0)
    assert X.estimate(M, sims, 0, [2, 3, 4, 1], 9, (0.5, 5.0)) == np.float32(0.5)


def test_reference_zero_is_a_data_point_and_absent_is_not():
    M = R.Model.from_lists([[(0, 1.0), (1, 2.0)],
                            [(0, 1.0), (1, 1.0), (5, 4.0)],
                            [(0, 2.0), (1, 1.0), (5, 0.0)],      # holds item 5 with 0.0
                            [(0, 2.0), (1, 3.0)],                # lacks item 5
                            [(0, 0.0), (5, 3.0)],                # the common item's value is 0.0: similarity 0.0
                            [(5, 2.0)], []])
    sims = M.similarities_row(0)
    assert sims[4] == 0.0 and sims[5] == 0.0 and np.isnan(sims[6])
    one = X.estimate(M, sims, 0, [1, 3], 5)          # one data point
    two = X.estimate(M, sims, 0, [1, 2, 3], 5)       # the 0.0 is the second
    assert np.isnan(one) and two == np.float32(sims[1] * 4.0 / (sims[1] + sims[2]))
    assert np.isnan(X.estimate(M, sims, 0, [0, 1, 0], 5))   # the user itself is skipped
    assert np.isnan(X.estimate(M, sims, 0, [1, 6], 5))      # an empty neighbour: no data point
    assert np.isnan(X.estimate(M, sims, 0, [], 5))
    assert np.isnan(X.estimate(M, sims, 0, [1, 2], 77))     # an item nobody holds
    # a neighbour named twice counts twice, as the loop walks the array
    assert X.estimate(M, sims, 0, [1, 1], 5) == np.float32(4.0)


def test_reference_arithmetic_is_item_estimate_one_point_at_a_time(shim):
    M = X.order_model()
    sims = M.similarities_row(0)
    for nb in ([1, 2, 3, 4], [1, 3, 4, 2], [2, 3, 4, 1], [3, 1], [4]):
        for capper in (None, (0.5, 5.0)):
            s = np.ascontiguousarray([sims[r] for r in nb], np.float64)
            p = np.ascontiguousarray([M._rows[r][1][M._rows[r][2][9]] for r in nb], np.float32)
            lo, hi = capper if capper else (0.0, 0.0)
            got = np.float32(shim.er_estimate(_p(s), _p(p), len(nb), int(capper is not None), lo, hi))
            assert X.same_bits32(got, X.estimate(M, sims, 0, nb, 9, capper)), (nb, capper)
