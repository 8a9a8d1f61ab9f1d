"""CPU: what the co-rated similarity kernels share with the host (cms_common.h,
built as tests/cpp/common_host_shim.hip) against the plain-Python restatement
(tests/common_ref.py), bit for bit, NaN matching NaN: the merge join and the
endings by the sequential route (k_common_pairs) and, where the pair is
eligible, from the integer cells (k_common_tile); eligibility at U = 2^51 - 1
and 2^51; the pair at U_x = U_y = 2^51 - 1 with opposite signs, whose sum of
squared differences, 4 U, must be exact in the integer cell."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import common_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "common_host_shim.hip")
DEPS = [SRC] + [os.path.join(HERE, "..", "mahout_amd", "csrc", f) for f in ("cms_common.h", "cms_exact.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libcommon_host_shim.so")


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.ch_finish.restype = ctypes.c_double
    return lib


def _routes(shim, measure, x, y, num, weighted):
    """(the sequential route's value, the integer route's or None when not eligible, U_x, U_y, the cells as sums)"""
    xk, yk = (np.ascontiguousarray(a[0], np.int64) for a in (x, y))
    xv, yv = (np.ascontiguousarray(a[1], np.float32) for a in (x, y))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    i64 = ctypes.c_int64
    lists = (p(xk), p(xv), i64(xk.size), p(yk), p(yv), i64(yk.size))
    finish = lambda s: shim.ch_finish(measure, p(s), i64(xk.size), i64(yk.size), i64(num), int(weighted))  # noqa: E731
    seq, cells, U, both = np.zeros(7), np.zeros(7), np.zeros(2, np.uint64), np.concatenate([xv, yv])
    shim.ch_merge_join(*lists, p(seq))
    ok = shim.ch_cells(*lists, shim.ch_shift(p(both), i64(both.size)), p(U), p(cells))
    return finish(seq), (finish(cells) if ok else None), int(U[0]), int(U[1]), cells


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


DESIGNED = {
    "disjoint": (([1, 3, 5], [1.0, 2.0, 3.0]), ([2, 4, 6], [4.0, 5.0, 6.0])),
    "x_empty": (([], []), ([2, 4], [4.0, 5.0])),
    "one_common": (([1, 3, 5], [1.0, 2.0, 3.0]), ([3, 4], [4.5, 5.0])),
    "constant_over_common": (([1, 2, 3, 9], [3.0, 3.0, 3.0, 1.0]), ([1, 2, 3, 8], [1.0, 4.5, 2.0, 3.0])),
    "negatives": (([1, 2, 3, 7], [1.5, -2.0, 3.0, 1.0]), ([1, 2, 3], [-1.0, 2.5, -0.5])),
    "half_stars": (([1, 2, 3, 4, 10], [0.5, 4.5, 3.0, 2.5, 5.0]), ([2, 3, 4, 5], [1.0, 3.5, 0.5, 2.0])),
    "thirds": (([1, 2, 3], [1.0 / 3.0, -2.0 / 3.0, 0.7]), ([1, 3, 4], [0.9, -1.0 / 3.0, 0.5])),  # s = 25
    "tenths": (([4, 5, 6], [0.1, 0.8, 0.3]), ([4, 5, 6], [0.3, 0.1, 0.8])),  # s = 27: 0.8's unit squared passes 2^51
    "no_shift": (([1, 2, 3], [1.0 / 3.0, -1.0 / 768.0, 0.7]), ([1, 2, 4], [0.9, -1.0 / 3.0, 2.0])),
    "nan_value": (([1, 2], [float("nan"), 1.0]), ([1, 2], [1.0, 1.0])),
    "interleaved": ((list(range(0, 60, 2)), [((7 * i) % 11 - 5) / 2 for i in range(30)]),
                    (list(range(0, 60, 3)), [((5 * i) % 9 - 4) / 4 for i in range(20)])),
}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("measure", range(3))
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_pairs_both_routes_both_orders(shim, name, measure, weighted):
    for x, y in (DESIGNED[name], DESIGNED[name][::-1]):
        for num in (7, 60):  # normalizeWeightResult's num is the caller's, not the lists'
            exp = R.similarity(R.MEASURES[measure], x, y, num, weighted)
            seq, cells = _routes(shim, measure, x, y, num, weighted)[:2]
            assert _same(seq, exp), (name, seq, exp)
            if name in ("tenths", "no_shift", "nan_value"):
                assert cells is None  # the sequential route only
            else:
                assert cells is not None and _same(cells, exp), (name, cells, exp)


def _squares_summing_to(total):
    """float32-representable integers whose squares sum to `total`: greedily the
    largest 24-bit-mantissa integer whose square still fits."""
    out, rem = [], total
    while rem:
        v = math.isqrt(rem)
        drop = max(0, v.bit_length() - 24)
        out.append((v >> drop) << drop)
        rem -= out[-1] ** 2
    return out


def test_eligibility_turns_at_two_to_the_51_and_the_bound_holds(shim):
    below, at = _squares_summing_to(2 ** 51 - 1), _squares_summing_to(2 ** 51)
    keys = list(range(len(below)))
    x, y = (keys, below), (keys, [-v for v in below])  # U_x = U_y = 2^51 - 1, opposite signs
    for m in range(3):
        seq, cells, Ux, Uy, sums = _routes(shim, m, x, y, 9, False)
        assert (Ux, Uy) == (2 ** 51 - 1, 2 ** 51 - 1) and cells is not None
        assert _same(cells, R.similarity(R.MEASURES[m], x, y, 9)) and _same(cells, seq)
    assert [shim.ch_tile_for(m, a) for m in range(3) for a in (0, 65, 10 ** 6)] == [2304, 128, 2304, 1472, 128, 1472, 5440, 128, 5440]
    # the sum of squared differences is 4 U = 2^53 - 4: exact in the integer cell, and the sequential loop's
    assert sums[5] == float(4 * (2 ** 51 - 1)) == R.sums(keys, [float(v) for v in below], keys, [-float(v) for v in below])[5]
    assert sums[0] == -float(2 ** 51 - 1) and sums[3] == sums[4] == float(2 ** 51 - 1) and sums[6] == len(below)
    _, cells, Ux, Uy, _ = _routes(shim, 0, (list(range(len(at))), at), x, 9, False)
    assert (Ux, Uy) == (2 ** 51, 2 ** 51 - 1) and cells is None
