"""CPU: what the exact-cosine kernels share with the host (cms_exact.h), built
for the host (tests/cpp/exact_host_shim.hip), against the plain-Python
restatement of CosineSimilarity.userSimilarity (tests/exact_ref.py).

  - the attach rules: the chosen shift s, the units, the eligibility flag at
    U = 2^53 - 1 and at 2^53, the refusal of unsorted and repeated keys and of
    offsets that decrease;
  - exact_finish and the merge join on designed vectors: disjoint lists (0.0,
    not NaN), one empty list, all-zero values, -0.0 products, negative dots
    under the weighting, a result the clamp touches -- by the sequential route
    (what k_exact_pairs computes) and, where the pair is eligible, by the
    integer route (what k_exact_tile computes), bit for bit, NaN matching NaN.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import exact_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "exact_host_shim.hip")
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("cms_exact.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libexact_host_shim.so")

vp, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.eh_shift.restype = ctypes.c_int
    lib.eh_shift.argtypes = [vp, i64]
    lib.eh_unit.restype = ctypes.c_int32
    lib.eh_unit.argtypes = [ctypes.c_float, ctypes.c_int]
    lib.eh_owner.restype = ctypes.c_int
    lib.eh_owner.argtypes = [vp, i64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(dbl),
                             ctypes.POINTER(dbl)]
    lib.eh_valid_csr.restype = ctypes.c_int
    lib.eh_valid_csr.argtypes = [i64, vp, vp]
    lib.eh_merge_join.restype = dbl
    lib.eh_merge_join.argtypes = [vp, vp, i64, vp, vp, i64]
    lib.eh_finish.restype = dbl
    lib.eh_finish.argtypes = [dbl, dbl, dbl, i64, i64, ctypes.c_int]
    lib.eh_similarity_seq.restype = dbl
    lib.eh_similarity_seq.argtypes = [vp, vp, i64, vp, vp, i64, ctypes.c_int]
    lib.eh_similarity_int.restype = dbl
    lib.eh_similarity_int.argtypes = [vp, vp, i64, vp, vp, i64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.eh_tile_for.restype = ctypes.c_int
    lib.eh_tile_for.argtypes = [ctypes.c_int]
    return lib


def _p(a):
    return a.ctypes.data_as(vp)


def _f32(v):
    return np.ascontiguousarray(v, np.float32)


def _i64(v):
    return np.ascontiguousarray(v, np.int64)


def _shift(shim, vals):
    v = _f32(vals)
    return shim.eh_shift(_p(v), v.size)


def _owner(shim, vals, s):
    v = _f32(vals)
    U, s2, root = ctypes.c_uint64(), dbl(), dbl()
    ok = shim.eh_owner(_p(v), v.size, s, ctypes.byref(U), ctypes.byref(s2), ctypes.byref(root))
    return ok, U.value, s2.value, root.value


# ---- attach rules ----

@pytest.mark.parametrize("vals,s", [
    ([1, 2, 5], 0), ([1.5, 4.0, 0.5], 1), ([0.25, 3.0], 2), ([0.1], 27), ([0.1, 0.8, 0.3], 27), ([-2.5, 3.0], 1),
    ([-0.0, 0.0], 0), ([], 0), ([1e8], 0), ([2147483520.0], 0), ([-2147483520.0, 0.5], -1),  # 2^31 - 128, then doubled
    ([2147483648.0], -1), ([2.0 ** -30], 30), ([2.0 ** -31], -1), ([float("nan")], -1),
    ([1.0, float("inf")], -1), ([1.0, 2.0 ** -30, 4.0], -1),  # 4 * 2^30 is no i32
    # every float32 is dyadic: 1/3 rounds to 11184811 * 2^-25, so thirds alone do have a shift ...
    ([1.0 / 3.0], 25), ([-1.0 / 3.0, 2.0], 25), ([-2.0 / 3.0, 0.7], 24),
    # ... and a 256th of one needs 33 fractional bits
    ([1.0 / 3.0, 1.0 / 768.0], -1),
])
def test_shift_is_the_smallest_that_makes_every_value_an_i32(shim, vals, s):
    assert _shift(shim, vals) == s
    if s >= 0:  # the rule itself, restated: integers below 2^31 at s, and not at s - 1
        v = np.asarray(vals, np.float32).astype(np.float64)
        x = np.ldexp(v, s)
        assert np.all(x == np.floor(x)) and np.all(np.abs(x) < 2.0 ** 31)
        if s > 0:
            y = np.ldexp(v, s - 1)
            assert not np.all(y == np.floor(y))
        for a in np.asarray(vals, np.float32):
            assert shim.eh_unit(float(a), s) == int(np.ldexp(float(a), s))


def _squares_summing_to(total):
    """float32-representable integers whose squares sum to `total`: greedily the
    largest 24-bit-mantissa integer whose square still fits."""
    out, rem = [], total
    while rem:
        v = math.isqrt(rem)
        drop = max(0, v.bit_length() - 24)
        v = (v >> drop) << drop
        assert float(np.float32(v)) == float(v)
        out.append(v)
        rem -= v * v
    return out


def test_eligibility_turns_at_two_to_the_53(shim):
    below = _squares_summing_to(2 ** 53 - 1)
    at = _squares_summing_to(2 ** 53)
    assert sum(v * v for v in below) == 2 ** 53 - 1 and sum(v * v for v in at) == 2 ** 53
    ok, U, s2, root = _owner(shim, below, 0)
    assert (ok, U) == (1, 2 ** 53 - 1)
    ok, U, s2, root = _owner(shim, at, 0)
    assert (ok, U) == (0, 2 ** 53)
    # at a shift: 0.8f is 13421773 * 2^-24, its unit at s = 27 is 13421773 * 8, and one such preference passes 2^53
    assert _shift(shim, [0.1, 0.8]) == 27
    ok, U, _, _ = _owner(shim, [0.8], 27)
    assert (ok, U) == (0, (13421773 * 8) ** 2) and U >= 2 ** 53
    ok, U, _, _ = _owner(shim, [0.1] * 40, 27)
    assert (ok, U) == (1, 40 * 13421773 ** 2)
    # saturation, and no shift at all
    ok, U, _, _ = _owner(shim, [2147483520.0] * 5, 0)
    assert (ok, U) == (0, 2 ** 64 - 1)
    ok, U, _, _ = _owner(shim, [1.0], -1)
    assert (ok, U) == (0, 2 ** 64 - 1)


def test_owner_sums_are_the_sequential_fp64_sums(shim):
    rng = np.random.Generator(np.random.PCG64(7))
    for vals in ([0.1, 0.8, 0.3, 0.7], rng.random(50).astype(np.float32) * 5, [1e8, 3.0, 1e-3], [-0.0], []):
        v = _f32(vals)
        s2 = 0.0
        for x in v:
            s2 += float(x) * float(x)
        _, _, got2, root = _owner(shim, v, -1)
        assert got2 == s2 and root == math.sqrt(s2)


def test_csr_validation(shim):
    def valid(off, keys):
        off, keys = _i64(off), _i64(keys)
        return shim.eh_valid_csr(off.size - 1, _p(off), _p(keys))

    assert valid([0, 2, 2, 5], [3, 9, -4, 0, 7]) == 1
    assert valid([0, 0, 0], []) == 1
    assert valid([0, 2, 5], [9, 3, 1, 2, 3]) == 0   # unsorted
    assert valid([0, 2, 5], [3, 9, 1, 1, 3]) == 0   # a key twice
    assert valid([1, 2, 5], [3, 9, 1, 2, 3]) == 0   # does not start at 0
    assert valid([0, 3, 2], [1, 2, 3]) == 0         # decreasing
    assert valid([0, 2, 4], [5, 6, 5, 6]) == 1      # ascending within each row only


def test_tile_tunable_rounds_to_64_and_stops_at_the_default(shim):
    assert [shim.eh_tile_for(a) for a in (0, -5, 1, 64, 65, 200, 8192, 8193, 10 ** 6)] == \
        [8192, 8192, 64, 64, 128, 256, 8192, 8192, 8192]


# ---- exact_finish and the merge join on designed vectors ----

def _seq(shim, x, y, weighted):
    xk, xv, yk, yv = _i64(x[0]), _f32(x[1]), _i64(y[0]), _f32(y[1])
    return shim.eh_similarity_seq(_p(xk), _p(xv), xk.size, _p(yk), _p(yv), yk.size, int(weighted))


def _int(shim, x, y, weighted):
    xk, xv, yk, yv = _i64(x[0]), _f32(x[1]), _i64(y[0]), _f32(y[1])
    s = _shift(shim, np.concatenate([xv, yv]))
    ok = ctypes.c_int()
    r = shim.eh_similarity_int(_p(xk), _p(xv), xk.size, _p(yk), _p(yv), yk.size, s, int(weighted), ctypes.byref(ok))
    return r if ok.value == 1 else None


def _bits(a):
    return np.float64(a).view(np.int64)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or _bits(a) == _bits(b)


DESIGNED = {
    "disjoint": (([1, 3, 5], [1.0, 2.0, 3.0]), ([2, 4, 6], [4.0, 5.0, 6.0])),
    "x_empty": (([], []), ([2, 4], [4.0, 5.0])),
    "y_empty": (([1, 2], [4.0, 5.0]), ([], [])),
    "x_all_zero": (([1, 2, 3], [0.0, 0.0, 0.0]), ([1, 2, 3], [1.0, 2.0, 3.0])),
    "both_all_zero": (([1], [0.0]), ([1], [-0.0])),
    "neg_zero_products": (([1, 2, 9], [-0.0, 0.0, 2.0]), ([1, 2, 8], [3.0, -4.0, 1.0])),
    "neg_zero_only_common": (([1, 9], [-0.0, 2.0]), ([1, 8], [3.0, 1.0])),
    "negative_dot": (([1, 2, 3, 7], [1.5, -2.0, 3.0, 1.0]), ([1, 2, 3], [-1.0, 2.5, -0.5])),
    "small_negative_dot": (([1, 2], [1.0, 5.0]), ([1, 3], [-0.5, 4.0])),
    "identical": (([4, 5, 6], [0.1, 0.8, 0.3]), ([4, 5, 6], [0.1, 0.8, 0.3])),
    # sqrt(sumX2)^2 rounds below sumX2: the quotient passes 1.0 and the clamp brings it back
    "clamped": (([1, 2, 3, 4], [0.8, 0.3, 0.6, 0.2]), ([1, 2, 3, 4], [0.8, 0.3, 0.6, 0.2])),
    "clamped_negative": (([1, 2, 3, 4], [0.8, 0.3, 0.6, 0.2]), ([1, 2, 3, 4], [-0.8, -0.3, -0.6, -0.2])),
    "clamped_half_stars": (([1, 2, 3, 4, 5], [4.0, 5.0, 0.5, 4.0, 1.5]), ([1, 2, 3, 4, 5], [4.0, 5.0, 0.5, 4.0, 1.5])),
    "half_stars": (([1, 2, 3, 4, 10], [0.5, 4.5, 3.0, 2.5, 5.0]), ([2, 3, 4, 5], [1.0, 3.5, 0.5, 2.0])),
    "big_value": (([1, 2], [1e8, 3.0]), ([1, 2], [2.0, 5.0])),
    "thirds": (([1, 2, 3], [1.0 / 3.0, -2.0 / 3.0, 0.7]), ([1, 3, 4], [0.9, -1.0 / 3.0, 2.0])),  # s = 25
    "no_shift": (([1, 2, 3], [1.0 / 3.0, -1.0 / 768.0, 0.7]), ([1, 2, 4], [0.9, -1.0 / 3.0, 2.0])),
    "nan_value": (([1, 2], [float("nan"), 1.0]), ([1, 2], [1.0, 1.0])),
    "inf_value": (([1, 2], [float("inf"), 1.0]), ([3], [1.0])),
    "interleaved": ((list(range(0, 60, 2)), [((7 * i) % 11 - 5) / 2 for i in range(30)]),
                    (list(range(0, 60, 3)), [((5 * i) % 9 - 4) / 4 for i in range(20)])),
}


def test_designed_set_holds_what_it_claims(shim):
    """The cases are what their names say, judged by the restatement alone."""
    assert R.user_similarity(*DESIGNED["disjoint"][0], *DESIGNED["disjoint"][1]) == 0.0
    assert math.isnan(R.user_similarity(*DESIGNED["x_empty"][0], *DESIGNED["x_empty"][1]))
    assert math.isnan(R.user_similarity(*DESIGNED["x_all_zero"][0], *DESIGNED["x_all_zero"][1]))
    assert _bits(R.user_similarity(*DESIGNED["neg_zero_only_common"][0], *DESIGNED["neg_zero_only_common"][1])) == 0
    assert R.user_similarity(*DESIGNED["negative_dot"][0], *DESIGNED["negative_dot"][1], weighted=True) < 0
    for name in ("clamped", "clamped_negative", "clamped_half_stars"):  # the quotient passes 1.0 before the clamp
        s2 = 0.0
        for v in np.asarray(DESIGNED[name][0][1], np.float32):
            s2 += float(v) * float(v)
        assert s2 / (math.sqrt(s2) * math.sqrt(s2)) > 1.0
        assert abs(R.user_similarity(*DESIGNED[name][0], *DESIGNED[name][1])) == 1.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_pairs_both_routes_both_orders(shim, name, weighted):
    for x, y in (DESIGNED[name], DESIGNED[name][::-1]):
        exp = R.user_similarity(x[0], x[1], y[0], y[1], weighted=weighted)
        got = _seq(shim, x, y, weighted)
        assert _same(got, exp), (name, got, exp)
        gi = _int(shim, x, y, weighted)
        # ("identical" holds 0.8 at s = 27: one such unit squared passes 2^53)
        if name in ("no_shift", "nan_value", "inf_value", "big_value", "identical"):
            assert gi is None  # no shift, or an owner at or past 2^53: the sequential route only
        else:
            assert gi is not None and _same(gi, exp), (name, gi, exp)


def test_merge_join_and_finish_apart(shim):
    (xk, xv), (yk, yv) = DESIGNED["interleaved"]
    xk_, xv_, yk_, yv_ = _i64(xk), _f32(xv), _i64(yk), _f32(yv)
    exp = 0.0
    y_at = dict(zip(yk, yv_))
    for k, v in zip(xk, xv_):
        if k in y_at:
            exp += float(v) * float(y_at[k])
    assert shim.eh_merge_join(_p(xk_), _p(xv_), xk_.size, _p(yk_), _p(yv_), yk_.size) == exp
    nan = float("nan")
    assert math.isnan(shim.eh_finish(1.0, 2.0, 3.0, 0, 4, 0)) and math.isnan(shim.eh_finish(1.0, 2.0, 3.0, 4, 0, 0))
    assert math.isnan(shim.eh_finish(0.0, 0.0, 3.0, 1, 1, 0)) and math.isnan(shim.eh_finish(nan, 2.0, 3.0, 1, 1, 1))
    assert _bits(shim.eh_finish(0.0, 2.0, 3.0, 1, 1, 0)) == 0          # no common item: 0.0 / den
    assert shim.eh_finish(7.0, 2.0, 3.0, 1, 1, 0) == 1.0               # the clamp
    assert shim.eh_finish(-7.0, 2.0, 3.0, 1, 1, 1) == -1.0
    from oracle import oracle as O
    for r, nx, ny in [(0.3, 2, 5), (-0.3, 2, 5), (0.0, 1, 1), (-0.999, 40, 2)]:
        assert shim.eh_finish(r * 6.0, 2.0, 3.0, nx, ny, 1) == O.normalize_weight_result(r * 6.0 / 6.0, nx + ny, nx + ny, True)
