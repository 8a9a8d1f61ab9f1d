"""CPU: the host side of the item-based recommender.

  - the library's candidate strategies (cms_recommend.cpp ItemCandidates:
    PreferredItemsNeighborhoodCandidateItemsStrategy over the transposed CSR,
    AllUnknownItemsCandidateItemsStrategy) built for the host, against the
    taste.FastIDSet restatements, on models that force rehashes, repeated
    raters and removals.  The library skips a rater it has already added
    (every key present) but keeps what such an add() can still do -- the table
    rebuild that precedes the lookup; the models here include users for whom
    dropping that rebuild changes the iteration order, and the test asserts so;
  - item_estimate_one (cms_ref.h, the kernel's estimate epilogue) built for
    the host against taste.item_estimate on designed similarity vectors;
  - FullRunningAverage and the multi-item estimator;
  - GenericDataModel.transposed().
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from mahout_amd import taste
from mahout_amd.datamodel import GenericDataModel

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "item_host_shim.hip")
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
LIB_SRC = os.path.join(CSRC, "cms_recommend.cpp")
DEPS = [SRC, LIB_SRC] + [os.path.join(CSRC, f) for f in ("cms_ref.h", "cms_hash.h", "cms_internal.h", "cms_forms.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libitem_host_shim.so")

vp = ctypes.c_void_p
i64 = ctypes.c_int64


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, LIB_SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.ih_candidates.restype = i64
    lib.ih_candidates.argtypes = [i64, vp, vp, i64, ctypes.c_int, ctypes.c_int, vp, i64]
    lib.ih_raters.restype = i64
    lib.ih_raters.argtypes = [i64, vp, vp, i64, vp, i64]
    lib.ih_item_estimate.restype = ctypes.c_float
    lib.ih_item_estimate.argtypes = [vp, vp, i64, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    lib.ih_item_estimate_pieces.restype = ctypes.c_float
    lib.ih_item_estimate_pieces.argtypes = [vp, vp, i64, i64, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    return lib


def _p(a):
    return a.ctypes.data_as(vp)


# ---- candidate strategies ----

def _model(seed, n_users=40, n_items=400, mean=18):
    """A user -> {item: value} model with scattered, negative and large item
    IDs (the FastIDSet hash is the low 31 bits), and a few empty users."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(n_items * 50, n_items, replace=False).astype(np.int64) * 7919 - 10 ** 6
    prefs = {}
    for u in range(n_users):
        m = 0 if u % 13 == 5 else int(rng.integers(1, 2 * mean))
        prefs[3 * u + 1] = {int(i): float(rng.integers(1, 6)) for i in rng.choice(ids, m, replace=False)}
    return GenericDataModel(prefs)


def _skipping_without_rebuild(model, side, preferred):
    """The candidate order if a rater met again were skipped outright."""
    possible = taste.FastIDSet()
    seen = set()
    for item in preferred:
        for u in side.getPreferencesFromUser(item)[0].tolist():
            if u in seen:
                continue
            seen.add(u)
            keys = model.getPreferencesFromUser(u)[0]
            s = taste.FastIDSet(len(keys))
            for k in keys.tolist():
                s.add(k)
            possible.addAll(s)
    for item in preferred:
        possible.remove(item)
    return possible.toList()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_candidate_strategies_in_fastidset_order(shim, seed):
    m = _model(seed)
    side = m.transposed()
    out = np.zeros(m.getNumItems() + 8, np.int64)
    strategies = (taste.PreferredItemsNeighborhoodCandidateItemsStrategy(), taste.AllUnknownItemsCandidateItemsStrategy())
    repeats = rebuild_matters = 0
    for row, user in enumerate(m.getUserIDs().tolist()):
        keys, vals = m.getPreferencesFromUser(user)
        for strat in strategies:
            for known in (0, 1):
                n = shim.ih_candidates(m.getNumUsers(), _p(m.offsets), _p(m.keys), row, strat.native, known, _p(out),
                                       out.size)
                want = strat.getCandidateItems(user, (keys, vals), m, bool(known)).toList()
                assert out[:n].tolist() == want, (user, strat.native, known)
                if not known:
                    assert not set(want) & set(keys.tolist())  # the removals
        raters = [u for k in keys.tolist() for u in side.getPreferencesFromUser(k)[0].tolist()]
        repeats += len(raters) - len(set(raters))
        want = strategies[0].getCandidateItems(user, (keys, vals), m, False).toList()
        rebuild_matters += _skipping_without_rebuild(m, side, keys.tolist()) != want
    assert repeats > 100  # raters met again
    print("users whose order needs the repeated add's rebuild:", rebuild_matters)


def test_repeated_add_rebuild_is_kept(shim):
    """A model built so that the LAST new key fills the table to its load
    limit and only repeated raters follow: FastIDSet.add rebuilds the table on
    the next add even though the key is present, which changes the iteration
    order.  Skipping the repeated rater outright would miss it."""
    # a new FastIDSet() has 5 slots (nextTwinPrime(3)) and add() starts with a
    # rebuild once numSlotsUsed * 1.5 >= the slots: it grows to 13 slots on the
    # 5th key and is due again with 9 keys in -- so 9 distinct items in all
    found = None
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        items = rng.choice(5000, 9, replace=False).astype(np.int64)
        # user 1 prefers items[0], items[1]; user 2 holds both plus the rest -> met twice
        prefs = {1: {int(items[0]): 1.0, int(items[1]): 2.0},
                 2: {int(i): 3.0 for i in items}}
        m = GenericDataModel(prefs)
        side = m.transposed()
        keys = m.getPreferencesFromUser(1)[0]
        want = taste.PreferredItemsNeighborhoodCandidateItemsStrategy().getCandidateItems(1, (keys, None), m, False).toList()
        if _skipping_without_rebuild(m, side, keys.tolist()) != want:
            found = (m, want)
            break
    assert found is not None, "no model in the search needs the rebuild"
    m, want = found
    out = np.zeros(32, np.int64)
    n = shim.ih_candidates(m.getNumUsers(), _p(m.offsets), _p(m.keys), 0, 0, 0, _p(out), out.size)
    assert out[:n].tolist() == want


def test_raters_ascend_and_repeat_once(shim):
    m = _model(7)
    side = m.transposed()
    out = np.zeros(m.getNumUsers() + 1, np.int64)
    for item in m.getItemIDs().tolist()[::5]:
        n = shim.ih_raters(m.getNumUsers(), _p(m.offsets), _p(m.keys), item, _p(out), out.size)
        want = np.searchsorted(m.getUserIDs(), side.getPreferencesFromUser(item)[0])
        assert out[:n].tolist() == want.tolist()
    assert shim.ih_raters(m.getNumUsers(), _p(m.offsets), _p(m.keys), 123456789, _p(out), out.size) == 0
    # a CSR that repeats a (user, item) pair: getPreferencesForItem holds the user once
    off = np.array([0, 3, 5], np.int64)
    keys = np.array([4, 4, 9, 4, 9], np.int64)
    assert shim.ih_raters(2, _p(off), _p(keys), 4, _p(out), out.size) == 2 and out[:2].tolist() == [0, 1]


# ---- the estimate ----

NAN = float("nan")
ESTIMATE_CASES = {
    "all_nan": ([NAN, NAN, NAN], [1.0, 2.0, 3.0]),
    "one_point": ([NAN, 0.5, NAN], [1.0, 4.0, 3.0]),          # exactly one non-NaN: NaN
    "two_points": ([0.25, NAN, 0.75], [1.0, 5.0, 4.0]),
    "total_zero_nan": ([0.0, 0.0], [3.0, 4.0]),                # 0 / 0
    "total_zero_inf": ([0.5, -0.5], [5.0, 1.0]),               # 2 / 0 = +inf: the capper's upper edge
    "total_zero_minus_inf": ([0.5, -0.5], [1.0, 5.0]),         # -2 / 0 = -inf: the lower edge
    "above_max": ([1.0, -0.5], [5.0, 1.0]),                    # 4.5 / 0.5 = 9
    "below_min": ([1.0, -0.5], [1.0, 5.0]),                    # -1.5 / 0.5 = -3
    "on_the_edges": ([0.5, 0.5], [5.0, 5.0]),
    "empty": ([], []),
    "rounding": ([1 / 3, 1e-17, 2 / 3, 0.1, NAN, 0.7], [4.5, 1.0, 3.5, 2.0, 5.0, 0.5]),
}


def _same_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


@pytest.mark.parametrize("name", sorted(ESTIMATE_CASES))
@pytest.mark.parametrize("capper", [None, (1.0, 5.0)])
def test_item_estimate_one_against_restatement(shim, name, capper):
    sims = np.array(ESTIMATE_CASES[name][0], np.float64)
    prefs = np.array(ESTIMATE_CASES[name][1], np.float32)
    lo, hi = capper or (0.0, 0.0)
    got = shim.ih_item_estimate(_p(sims), _p(prefs), sims.size, int(capper is not None), lo, hi)
    want = taste.item_estimate(sims, prefs, capper)
    assert _same_f32(got, want), (got, want)
    finite = int((~np.isnan(sims)).sum())
    if finite <= 1:
        assert math.isnan(got)
    if name == "two_points":
        assert got == np.float32((0.25 * 1.0 + 0.75 * 4.0) / 1.0)
    if capper and name in ("total_zero_inf", "above_max"):
        assert got == 5.0
    if capper and name in ("total_zero_minus_inf", "below_min"):
        assert got == 1.0
    if not capper and name == "total_zero_inf":
        assert got == math.inf
    for piece in (1, 2, 4):  # fed in pieces, as the kernel's tiles feed it
        assert _same_f32(shim.ih_item_estimate_pieces(_p(sims), _p(prefs), sims.size, piece, int(capper is not None),
                                                      lo, hi), want)


def test_item_estimate_random_orders(shim):
    """fp64 sums are order-dependent: long random vectors, and the same ones reversed."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        m = int(rng.integers(2, 300))
        sims = rng.uniform(-1, 1, m)
        sims[rng.random(m) < 0.2] = np.nan
        prefs = rng.integers(1, 11, m).astype(np.float32) / 2
        a = shim.ih_item_estimate(_p(sims), _p(prefs), m, 0, 0.0, 0.0)
        assert _same_f32(a, taste.item_estimate(sims, prefs))
        rs, rp = np.ascontiguousarray(sims[::-1]), np.ascontiguousarray(prefs[::-1])
        b = shim.ih_item_estimate(_p(rs), _p(rp), m, 0, 0.0, 0.0)
        assert _same_f32(b, taste.item_estimate(rs, rp))
    # a vector on which the order decides the float result: forward the sums
    # are (2^60 + 1 -> 2^60) - 2^60 + 1 = 1, backward 1 is lost twice and 0 / 0 is left
    sims = np.array([2.0 ** 60, 1.0, -2.0 ** 60, 1.0])
    prefs = np.ones(4, np.float32)
    rs = np.ascontiguousarray(sims[::-1])
    a = shim.ih_item_estimate(_p(sims), _p(prefs), 4, 0, 0.0, 0.0)
    b = shim.ih_item_estimate(_p(rs), _p(prefs), 4, 0, 0.0, 0.0)
    assert a == 1.0 and math.isnan(b)
    assert _same_f32(a, taste.item_estimate(sims, prefs)) and _same_f32(b, taste.item_estimate(rs, prefs))


# ---- running average and the multi-item estimator ----

def test_full_running_average():
    avg = taste.FullRunningAverage()
    assert math.isnan(avg.getAverage()) and avg.getCount() == 0
    data = [0.63, -0.99, 0.71, -0.93, 0.46]
    want = None
    for c, x in enumerate(data, 1):
        avg.addDatum(x)
        want = x if c == 1 else want * (c - 1) / c + x / c  # the incremental formula, not sum / count
        assert avg.getAverage() == want and avg.getCount() == c
    assert want != sum(data) / len(data)  # (the two differ in the last bit here)


def test_multi_most_similar_estimate():
    est = taste.multi_most_similar_estimate
    assert est([0.5, 0.25]) == 0.5 * 1 / 2 + 0.25 / 2
    assert math.isnan(est([0.5, NAN, 0.25], True))          # NaN enters the average
    assert est([0.5, NAN, 0.25], False) == est([0.5, 0.25])  # ... or is left out
    assert math.isnan(est([NAN, NAN], False))                # nothing averaged: NaN
    assert math.isnan(est([], True))
    assert math.isnan(est([0.0, 0.0], True))                 # an average of 0 becomes NaN
    assert math.isnan(est([0.5, -0.5], False))
    assert est([-0.5, -0.25], True) == -0.5 * 1 / 2 + -0.25 / 2


# ---- the transposed model ----

def test_transposed_round_trip():
    m = _model(11, n_users=30, n_items=120, mean=10)
    t = m.transposed()
    assert np.array_equal(t.getUserIDs(), m.getItemIDs())
    assert np.array_equal(t.getItemIDs(), np.unique(np.repeat(m.user_ids, np.diff(m.offsets))))
    for item in t.getUserIDs().tolist():
        users, vals = t.getPreferencesFromUser(item)
        assert np.all(np.diff(users) > 0)  # keys ascending per owner
        for u, v in zip(users.tolist(), vals.tolist()):
            assert m.getPreferenceValue(u, item) == v
    assert t.keys.size == m.keys.size
    back = t.transposed()
    keep = np.diff(m.offsets) > 0  # users without preferences have no place in the transpose
    assert np.array_equal(back.user_ids, m.user_ids[keep]) and (~keep).any()
    assert np.array_equal(back.offsets, np.concatenate([[0], np.cumsum(np.diff(m.offsets)[keep])]))
    assert np.array_equal(back.keys, m.keys) and np.array_equal(back.values, m.values)
    assert back.values.dtype == np.float32
    nv = GenericDataModel.from_csr(m.user_ids, m.offsets, m.keys, None).transposed()
    assert nv.values is None and np.array_equal(nv.keys, t.keys)
