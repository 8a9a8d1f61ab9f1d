"""CPU: what the retraction kernels share with the host
(mahout_amd/csrc/cms_retract.h: the batch validation and the per-owner,
per-sketch-row step "sum the decrements per bucket, compare each sum with the
live counter" -- the functions k_retract_validate, k_retract_wave and
k_retract_image call) compiled for the host and compared
with numpy, and the Python side of the feature, which needs no library:
datamodel.preference_delta and FileDataModel's update files
(T/impl/model/file/FileDataModel.java:239-334, 493-527)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mahout_amd.datamodel import FileDataModel, GenericDataModel, preference_delta

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "retract_host_shim.hip")
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("cms_retract.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libretract_host_shim.so")

OK, E_PARAM, E_VALUE = 0, 1, 5  # include/mahout_cms.h


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.rh_validate.restype = i
    lib.rh_validate.argtypes = [vp, vp, ll, ll, i]
    lib.rh_dec.restype = None
    lib.rh_dec.argtypes = [vp, ll, i, vp, vp]
    lib.rh_combine.restype = None
    lib.rh_combine.argtypes = [vp, vp, i, vp, vp]
    lib.rh_check_run.restype = ll
    lib.rh_check_run.argtypes = [vp, vp, i, vp, i]
    lib.rh_wave_run.restype = i
    lib.rh_wave_run.argtypes = []
    return lib


def _p(arr):
    return None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)


# ---- the shared validation: an ingest's rule ----

def _ingest_takes(v, fb):
    """load_inc (cms_device.h), restated: val * 2^fb is a non-negative integer below 2^32."""
    x = np.ldexp(np.float64(np.float32(v)), fb)
    return bool(x >= 0 and x == np.floor(x) and x < 2.0 ** 32)


VALUES = [0.0, 1.0, 2.5, 0.5, 0.25, 3.0, -1.0, -0.5, 1.1, 2.0 ** 31, 2.0 ** 31 - 128, 2.0 ** 32, 2.0 ** 33, 1e30,
          float("nan"), float("inf"), float("-inf"), -0.0]


@pytest.mark.parametrize("fb", [0, 1])
def test_values_are_validated_as_an_ingest_validates_them(shim, fb):
    vals = np.array(VALUES, np.float32)
    dec = np.zeros(vals.size, np.uint32)
    ok = np.zeros(vals.size, np.uint8)
    shim.rh_dec(_p(vals), vals.size, fb, _p(dec), _p(ok))
    for v, d, o in zip(VALUES, dec, ok):
        assert bool(o) == _ingest_takes(v, fb), (v, fb)
        assert int(d) == (int(np.ldexp(np.float64(np.float32(v)), fb)) if o else 0), (v, fb)
        one = np.array([v], np.float32)
        assert shim.rh_validate(None, _p(one), 1, 0, fb) == (OK if o else E_VALUE), (v, fb)
    # negative, non-dyadic and too large: the ingest's code at both granularities
    for bad in (-1.0, 1.1, 2.0 ** 32):
        assert shim.rh_validate(None, _p(np.array([1.0, bad], np.float32)), 2, 0, fb) == E_VALUE
    assert shim.rh_validate(None, _p(np.array([2.5], np.float32)), 1, 0, fb) == (E_VALUE if fb == 0 else OK)
    assert shim.rh_validate(None, _p(np.array([2.0 ** 31], np.float32)), 1, 0, fb) == (OK if fb == 0 else E_VALUE)
    # vals null: every value is 1.0
    shim.rh_dec(None, 3, fb, _p(dec), _p(ok))
    assert ok[:3].all() and (dec[:3] == 1 << fb).all()


def test_rows_are_validated_before_values(shim):
    rows = np.array([0, 4, 2], np.int64)
    vals = np.array([1.0, 1.0, -1.0], np.float32)
    assert shim.rh_validate(_p(rows), _p(vals), 3, 5, 0) == E_VALUE
    assert shim.rh_validate(_p(rows), _p(vals), 3, 4, 0) == E_PARAM  # row 4 of 4 owners: reported first
    assert shim.rh_validate(_p(rows), _p(vals), 2, 5, 0) == OK
    assert shim.rh_validate(_p(np.array([-1], np.int64)), None, 1, 5, 0) == E_PARAM
    assert shim.rh_validate(_p(rows), None, 0, 5, 0) == OK  # the empty batch


# ---- sum per bucket and compare ----

def _check(shim, bucket, dec, counters):
    bucket = np.ascontiguousarray(bucket, np.uint32)
    dec = np.ascontiguousarray(dec, np.uint32)
    counters = np.ascontiguousarray(counters, np.uint32)
    return shim.rh_check_run(_p(bucket), _p(dec), bucket.size, _p(counters), counters.size)


def _expected(bucket, dec, counters):
    sums = np.bincount(np.asarray(bucket, np.int64), weights=np.asarray(dec, np.float64), minlength=len(counters))
    bad = np.flatnonzero(sums > np.asarray(counters, np.float64))
    return int(bad[0]) if bad.size else -1


def test_combine_sums_every_bucket_once(shim):
    rng = np.random.Generator(np.random.PCG64(3))
    for cnt in (1, 2, 7, shim.rh_wave_run(), 200):
        bucket = rng.integers(0, 16, cnt).astype(np.uint32)
        dec = rng.integers(0, 5, cnt).astype(np.uint32)
        total = np.zeros(cnt, np.uint64)
        leader = np.zeros(cnt, np.uint8)
        shim.rh_combine(_p(bucket), _p(dec), cnt, _p(total), _p(leader))
        sums = np.bincount(bucket, weights=dec, minlength=16)
        assert np.array_equal(total.astype(np.float64), sums[bucket])
        first = np.zeros(cnt, bool)
        first[np.unique(bucket, return_index=True)[1]] = True
        assert np.array_equal(leader.astype(bool), first)


RUNS = [
    # (buckets, decrements, live counters [8], note)
    ([3, 3], [1, 1], [0, 0, 0, 2, 0, 0, 0, 0], "a duplicated pair: exact equality passes"),
    ([3, 3], [1, 1], [0, 0, 0, 1, 0, 0, 0, 0], "a duplicated pair: each copy alone would fit"),
    ([5, 5], [2, 3], [9, 9, 9, 9, 9, 5, 9, 9], "two keys in one bucket, equal to the counter"),
    ([5, 5], [2, 3], [9, 9, 9, 9, 9, 4, 9, 9], "two keys in one bucket, one over"),
    ([1, 6, 1, 6, 2], [1, 1, 1, 1, 7], [0, 2, 7, 0, 0, 0, 1, 0], "bucket 6 one over, bucket 1 and 2 exact"),
    ([7, 0], [1, 1], [0, 0, 0, 0, 0, 0, 0, 0], "two offenders: the smallest bucket is named"),
    ([4, 4, 4], [0, 0, 0], [0] * 8, "zero decrements fit an empty counter"),
    ([2], [4294967295], [0, 0, 4294967295, 0, 0, 0, 0, 0], "the largest decrement"),
    ([2, 2], [4294967295, 1], [0, 0, 4294967295, 0, 0, 0, 0, 0], "a sum past 2^32 does not wrap"),
    ([], [], [0] * 8, "the empty run"),
]


@pytest.mark.parametrize("case", range(len(RUNS)))
def test_designed_runs_against_bincount(shim, case):
    bucket, dec, counters, note = RUNS[case]
    assert _check(shim, bucket, dec, counters) == _expected(bucket, dec, counters), note


def test_designed_runs_name_the_bucket(shim):
    assert _check(shim, *RUNS[0][:3]) == -1
    assert _check(shim, *RUNS[1][:3]) == 3
    assert _check(shim, *RUNS[2][:3]) == -1
    assert _check(shim, *RUNS[3][:3]) == 5
    assert _check(shim, *RUNS[4][:3]) == 6
    assert _check(shim, *RUNS[5][:3]) == 0
    assert _check(shim, *RUNS[8][:3]) == 2


def test_random_runs_against_bincount(shim):
    rng = np.random.Generator(np.random.PCG64(11))
    seen = set()
    for _ in range(200):
        w = int(rng.integers(1, 40))
        cnt = int(rng.integers(0, 130))  # both sides of a wave's run
        bucket = rng.integers(0, w, cnt)
        dec = rng.integers(0, 4, cnt)
        counters = np.bincount(bucket, weights=dec, minlength=w).astype(np.int64)
        if rng.integers(0, 2) and w > 0:  # lower a few counters: some of them under their sums
            hit = rng.integers(0, w, 3)
            counters[hit] = np.maximum(counters[hit] - rng.integers(0, 2, 3), 0)
        got = _check(shim, bucket, dec, counters)
        assert got == _expected(bucket, dec, counters)
        seen.add(got >= 0)
    assert seen == {True, False}


# ---- preference_delta ----

def _coo(t):
    return sorted(zip(t[0].tolist(), t[1].tolist(), t[2].tolist()))


def test_preference_delta_removals_changes_additions_and_emptied_users():
    old = GenericDataModel({1: {10: 1.0, 11: 2.5, 12: 3.0}, 2: {10: 4.0}, 3: {7: 1.0, 8: 1.0}, 4: {}})
    new = GenericDataModel({1: {10: 1.0, 11: 3.5, 13: 2.0}, 2: {}, 3: {7: 1.0, 8: 1.0}, 4: {9: 0.5}})
    retract, ingest = preference_delta(old, new)
    assert _coo(retract) == [(1, 11, 2.5), (1, 12, 3.0), (2, 10, 4.0)]  # changed at the OLD value, removed, emptied
    assert _coo(ingest) == [(1, 11, 3.5), (1, 13, 2.0), (4, 9, 0.5)]    # changed at the NEW value, added
    assert retract[0].dtype == np.int64 and retract[1].dtype == np.int64 and retract[2].dtype == np.float32
    # old - retract + ingest == new, pair for pair
    pairs = {(u, k): v for u, k, v in _coo((np.repeat(old.user_ids, np.diff(old.offsets)), old.keys, old.values))}
    for u, k, v in _coo(retract):
        assert pairs.pop((u, k)) == v
    for u, k, v in _coo(ingest):
        assert (u, k) not in pairs
        pairs[(u, k)] = v
    assert pairs == {(u, k): v for u, k, v in
                     _coo((np.repeat(new.user_ids, np.diff(new.offsets)), new.keys, new.values))}


def test_preference_delta_of_equal_models_is_empty_and_other_users_are_refused():
    m = GenericDataModel({1: {10: 1.0}, 2: {11: 2.0}})
    retract, ingest = preference_delta(m, GenericDataModel({1: {10: 1.0}, 2: {11: 2.0}}))
    assert retract[0].size == 0 and ingest[0].size == 0
    with pytest.raises(ValueError):
        preference_delta(m, GenericDataModel({1: {10: 1.0}, 3: {11: 2.0}}))
    # a (user, item) pair is matched as a pair: the same item under another user is an addition
    retract, ingest = preference_delta(m, GenericDataModel({1: {10: 1.0, 11: 2.0}, 2: {}}))
    assert _coo(retract) == [(2, 11, 2.0)] and _coo(ingest) == [(1, 11, 2.0)]


def test_preference_delta_random_models():
    rng = np.random.Generator(np.random.PCG64(21))
    users = list(range(30))

    def model():
        return {u: {int(k): float(rng.integers(1, 11)) / 2 for k in rng.choice(40, size=rng.integers(0, 12), replace=False)}
                for u in users}
    a, b = model(), model()
    retract, ingest = preference_delta(GenericDataModel(a), GenericDataModel(b))
    exp_r = sorted((u, k, v) for u in users for k, v in a[u].items() if b[u].get(k) != v)
    exp_i = sorted((u, k, v) for u in users for k, v in b[u].items() if a[u].get(k) != v)
    assert _coo(retract) == exp_r and _coo(ingest) == exp_i


# ---- FileDataModel's update files ----

DATA = "1,10,1.0\n1,11,2.5\n2,10,4.0\n2,12,3.0\n3,7,1.0\n"


def _write(path, text, mtime):
    path.write_text(text)
    os.utime(path, (mtime, mtime))


def _as_dict(m):
    return {int(u): dict(zip(m.getPreferencesFromUser(u)[0].tolist(), m.getPreferencesFromUser(u)[1].tolist()))
            for u in m.getUserIDs()}


def test_update_files_delete_override_and_are_chosen_by_name_and_time(tmp_path):
    t0 = 1_700_000_000
    data = tmp_path / "prefs.csv"
    _write(data, DATA, t0)
    _write(tmp_path / "prefs.1.csv", "1,11,\n2,10,5.0\n4,9,0.5\n", t0 + 10)       # a delete, an override, a new user
    _write(tmp_path / "prefs.2.csv", "2,10,1.5\n3,7,\n", t0 + 20)                 # later: overrides the override; empties 3
    _write(tmp_path / "prefs.0.csv", "1,10,9.0\n", t0 - 10)                       # older than the data file: ignored
    _write(tmp_path / "other.1.csv", "1,10,8.0\n", t0 + 30)                       # another prefix: ignored
    (tmp_path / "prefs.d").mkdir()                                               # a directory: ignored
    plain = FileDataModel(str(data))
    assert _as_dict(plain) == {1: {10: 1.0, 11: 2.5}, 2: {10: 4.0, 12: 3.0}, 3: {7: 1.0}}
    m = FileDataModel(str(data), update_files=True)
    assert _as_dict(m) == {1: {10: 1.0}, 2: {10: 1.5, 12: 3.0}, 3: {}, 4: {9: 0.5}}  # user 3 stays, emptied
    assert m.getNumUsers() == 4
    # update_files=False is today's model, array for array
    off = FileDataModel(str(data), update_files=False)
    for x, y in ((plain.user_ids, off.user_ids), (plain.offsets, off.offsets), (plain.keys, off.keys),
                 (plain.values, off.values), (plain.item_ids, off.item_ids)):
        assert np.array_equal(x, y) and x.dtype == y.dtype


def test_update_files_are_read_in_modification_order_not_name_order(tmp_path):
    t0 = 1_700_000_000
    data = tmp_path / "prefs.csv"
    _write(data, DATA, t0)
    _write(tmp_path / "prefs.a.csv", "1,10,7.0\n", t0 + 20)  # first by name, last by time: its value wins
    _write(tmp_path / "prefs.b.csv", "1,10,6.0\n", t0 + 10)
    m = FileDataModel(str(data), update_files=True)
    assert m.getPreferenceValue(1, 10) == 7.0
    _write(tmp_path / "prefs.c.csv", "1,10,2.0\n", t0)  # a time equal to the data file's counts (>=)
    _write(tmp_path / "prefs.a.csv", "1,10,7.0\n", t0 + 20)
    assert FileDataModel(str(data), update_files=True).getPreferenceValue(1, 10) == 7.0
    os.utime(tmp_path / "prefs.c.csv", (t0 + 30, t0 + 30))
    assert FileDataModel(str(data), update_files=True).getPreferenceValue(1, 10) == 2.0


def test_refresh_rereads_everything_and_replaces_the_arrays(tmp_path):
    t0 = 1_700_000_000
    data = tmp_path / "prefs.txt"  # the prefix ends at the first period
    _write(data, DATA, t0)
    m = FileDataModel(str(data), update_files=True)
    before = (m.offsets, m.keys, m.values)
    snapshot = [x.copy() for x in before]
    _write(tmp_path / "prefs.1.txt", "1,11,\n2,12,0.5\n", t0 + 5)
    m.refresh()
    assert _as_dict(m) == {1: {10: 1.0}, 2: {10: 4.0, 12: 0.5}, 3: {7: 1.0}}
    assert all(x is not y for x, y in zip(before, (m.offsets, m.keys, m.values)))
    assert all(np.array_equal(x, y) for x, y in zip(before, snapshot))  # the old arrays are as they were
    plain = FileDataModel(str(data))
    _write(tmp_path / "prefs.2.txt", "3,7,\n", t0 + 6)
    plain.refresh()  # without update files a refresh reads the data file alone
    assert _as_dict(plain) == {1: {10: 1.0, 11: 2.5}, 2: {10: 4.0, 12: 3.0}, 3: {7: 1.0}}
