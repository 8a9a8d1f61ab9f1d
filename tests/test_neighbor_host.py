"""CPU: what k_nb_estimate shares with the host (tests/cpp/nb_host_shim.hip)
against the restatement tests/user_est_ref.py: BoolUserEstimate point by point
(a NaN similarity is a NaN estimate, no data point is NaN), an order model per
kind whose two neighbourhood orders differ in the restatement itself, the
ascending-bit fold of a chunk's mask equal to the sequential loop."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import common_ref as C
import user_est_ref as U
from exact_rec_ref import same_bits32

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "nb_host_shim.hip")
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("cms_neighbor.h", "cms_ref.h", "cms_exact.h", "cms_exact_plan.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libnb_host_shim.so")
vp, i64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.nb_generic.restype = lib.nb_boolean.restype = f32
    lib.nb_generic.argtypes = [vp, vp, i64, ctypes.c_int, ctypes.c_int, f32, f32]
    lib.nb_boolean.argtypes = [vp, i64, ctypes.c_int]
    return lib


def _run(shim, kind, sims, prefs, by_mask, capper=None):
    """The struct of `kind` fed the data points (sims[i], prefs[i]) in order."""
    s = np.ascontiguousarray(sims, np.float64)
    if kind == "boolean":
        return np.float32(shim.nb_boolean(s.ctypes.data_as(vp), s.size, by_mask))
    p = np.ascontiguousarray(prefs, np.float32)
    lo, hi = capper or (0.0, 0.0)
    return np.float32(shim.nb_generic(s.ctypes.data_as(vp), p.ctypes.data_as(vp), s.size, by_mask, int(capper is not None),
                                      lo, hi))


def _ref(kind, sims, prefs, capper=None):
    """The restatement over the same data points: neighbour i + 1 holds item 0 with prefs[i]; row 0 is the user."""
    rows = [{}] + [{0: float(p)} for p in prefs]
    return U.estimate(kind, rows, [np.nan] + list(sims), 0, list(range(1, len(sims) + 1)), 0, capper)


def test_boolean_struct_point_by_point(shim):
    for sims in ([0.25], [0.1, 0.7, -0.3], [1.0, 2.0 ** -24, 2.0 ** -24, -1.0], [0.5, np.nan, 0.25], [1e39, 1e39], []):
        assert same_bits32(_run(shim, "boolean", sims, None, 0), _ref("boolean", sims, [1.0] * len(sims))), sims
    assert np.isnan(_run(shim, "boolean", [0.5, np.nan, 0.25], None, 0))  # NaN is not skipped
    assert np.isnan(_run(shim, "boolean", [], None, 0)) and np.isposinf(_run(shim, "boolean", [1e39, 1e39], None, 0))


def test_order_models_differ_in_the_restatement(shim):
    M = C.Model(U.GENERIC_ORDER_PREFS)
    sims = M.row("pearson", "owner", 0)
    assert 0.99 < sims[1] == -sims[2] and 0 < sims[3] == -sims[4] < 0.99
    rows = [dict(p) for p in U.GENERIC_ORDER_PREFS]
    g = [U.estimate("generic", rows, sims, 0, nb, 9) for nb in U.GENERIC_ORDERS]
    assert np.isinf(g[0]) and np.isfinite(g[1]) and not same_bits32(g[0], g[1])
    held = [{9: 1.0} for _ in U.BOOLEAN_ORDER_SIMS]
    b = [U.estimate("boolean", held, U.BOOLEAN_ORDER_SIMS, 0, nb, 9) for nb in U.BOOLEAN_ORDERS]
    assert b[0] == 0.0 and b[1] == np.float32(2.0 ** -23)
    for nb, eg in zip(U.GENERIC_ORDERS, g):  # the structs give the same bits, order by order
        assert same_bits32(_run(shim, "generic", sims[nb], [rows[r][9] for r in nb], 0), eg)
    for nb, eb in zip(U.BOOLEAN_ORDERS, b):
        assert same_bits32(_run(shim, "boolean", [U.BOOLEAN_ORDER_SIMS[r] for r in nb], None, 0), eb)


@pytest.mark.parametrize("kind", ["generic", "boolean"])
@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 33, 65])
def test_ascending_bit_fold_is_the_sequential_loop(shim, kind, m):
    rng = np.random.Generator(np.random.PCG64(m))
    sims = rng.uniform(-1, 1, m)
    sims[rng.integers(m)] = np.nan if m > 2 else sims[0]
    prefs = rng.integers(1, 11, m) * np.float32(0.5)
    seq = _run(shim, kind, sims, prefs, 0, (1.0, 4.0))
    assert same_bits32(_run(shim, kind, sims, prefs, 1, (1.0, 4.0)), seq)
    assert same_bits32(seq, _ref(kind, sims, prefs, (1.0, 4.0)))
