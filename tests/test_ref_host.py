"""CPU: the reference's scalar query semantics (mahout_amd/csrc/cms_ref.h:
sketch_get, estimate_one, cosine_finish -- the functions k_point_query,
k_estimate and the pair-cosine kernels call) compiled for the host with the
fixed-shape fp64 accessor over host arrays, and compared bit for bit with the
oracle's restatement of DoubleCountMinSketch.get (:94-103),
GenericUserBasedRecommender.doEstimatePreference (:134-184) and
normalizeWeightResult (AbstractSimilarity.java:313-330).

The input is small but reaches every branch of the estimate: the user's own
row among the neighbours, an empty neighbour (every point query 0), NaN and
negative similarities, items with fewer than two data points (NaN), and
estimates below, inside and above the capper's range."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "ref_host_shim.hip")
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("cms_ref.h", "cms_hash.h", "cms_internal.h", "cms_forms.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libref_host_shim.so")

N, D, W = 12, 3, 16
USER = 2
NEIGHBOURS = np.array([5, 2, 11, 0, 7, 9, 3], np.int64)
ITEMS = np.arange(-2, 40, dtype=np.int64)
CAPPER = (1.0, 4.0)
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    vp, ll, i, f = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float
    lib.rh_sketch_get.restype = None
    lib.rh_sketch_get.argtypes = [vp, i, i, vp, vp, ll, vp, ll, vp]
    lib.rh_estimate.restype = None
    lib.rh_estimate.argtypes = [vp, i, i, vp, vp, ll, vp, vp, ll, vp, ll, i, f, f, vp]
    lib.rh_cosine_finish.restype = ctypes.c_double
    lib.rh_cosine_finish.argtypes = [ctypes.c_double, i]
    return lib


@pytest.fixture(scope="module")
def model(oracle):
    rng = np.random.Generator(np.random.PCG64(3))
    rows = rng.integers(0, 11, 70)  # owner 11 stays empty
    keys = rng.integers(0, 24, 70)
    vals = np.round(rng.normal(0, 2.5, 70), 1).astype(np.float32)
    a, b = oracle.hash_params(42, D)
    table = oracle.build_table(N, D, W, a, b, rows, keys, vals)
    return a, b, table, oracle.similarities_row(table, USER)


def same_bits(got, exp):
    """Bit equality, any NaN equal to any NaN."""
    got, exp = np.asarray(got), np.asarray(exp)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(got) & np.isnan(exp)
    return got.dtype == exp.dtype and got.shape == exp.shape and bool(np.all(nan | (got.view(bits) == exp.view(bits))))


def _p(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def test_estimate_one_equals_the_oracle(shim, oracle, model):
    a, b, table, sims = model
    nb_sims = np.ascontiguousarray(sims[NEIGHBOURS])
    others = nb_sims[NEIGHBOURS != USER]
    assert np.isnan(others).sum() >= 1 and (others < 0).sum() >= 1
    plain = np.array([oracle.estimate_preference(table, a, b, USER, NEIGHBOURS, int(k)) for k in ITEMS], np.float32)
    capped = np.array([oracle.estimate_preference(table, a, b, USER, NEIGHBOURS, int(k), capper=CAPPER)
                       for k in ITEMS], np.float32)
    # the expected values themselves reach every branch
    assert np.isnan(plain).any()
    assert (plain < CAPPER[0]).any() and (plain > CAPPER[1]).any()
    assert ((plain >= CAPPER[0]) & (plain <= CAPPER[1])).any()
    assert (capped == np.float32(CAPPER[0])).any() and (capped == np.float32(CAPPER[1])).any()
    for use_capper, exp in ((0, plain), (1, capped)):
        got = np.zeros(ITEMS.size, np.float32)
        shim.rh_estimate(_p(table), D, W, _p(a), _p(b), USER, _p(NEIGHBOURS), _p(nb_sims), NEIGHBOURS.size, _p(ITEMS),
                         ITEMS.size, use_capper, CAPPER[0], CAPPER[1], _p(got))
        assert same_bits(got, exp), (use_capper, got, exp)


def test_sketch_get_equals_the_oracle(shim, oracle, model):
    a, b, table, _ = model
    zeros = 0
    for row in (USER, 7, 11):  # 11: the empty owner
        exp = np.array([oracle.sketch_get(table[row], a, b, int(k)) for k in ITEMS], np.float64)
        got = np.zeros(ITEMS.size, np.float64)
        shim.rh_sketch_get(_p(table), D, W, _p(a), _p(b), row, _p(ITEMS), ITEMS.size, _p(got))
        assert same_bits(got, exp), row
        zeros += int((exp == 0).sum())
        if row == 11:
            assert not exp.any()
        else:
            assert exp.any()
    assert zeros > ITEMS.size  # the "no data point" branch of the estimates is well fed


def test_cosine_finish_equals_the_oracle(shim, oracle):
    one_up = np.nextafter(1.0, 2.0)  # 1.0000000000000002
    for weighted in (False, True):
        assert np.isnan(shim.rh_cosine_finish(DBL_MAX, int(weighted)))  # no row qualified
        for v in (0.0, 0.5, 1.0, one_up):
            for r in (v, -v):
                got = np.array([shim.rh_cosine_finish(r, int(weighted))])
                exp = np.array([oracle.normalize_weight_result(r, weighted=weighted)])
                assert same_bits(got, exp), (r, weighted, got, exp)
