"""GPU: pairs taken out of a live sketch table (cms_retract /
cms_retract_device_rows: the grouping by owner, the mass rule and the counter
rule of k_retract_wave<false> and k_retract_image<false>, widen_rows
over the live list rows that lose entries, then the write pass).  Every
comparison is exact: counters bit for bit against the oracle's rebuild of the
remaining stream (`T/impl/common/DoubleCountMinSketch.java:72-80`),
similarities and top-k lists against a fresh handle built from that stream.

Two thresholds choose the kernels.  An owner's pairs up to WAVE_RUN = 64
(kRetractWaveRun, cms_retract.h) are one wave's run, longer runs take the LDS
image kernel; a batch below PARTITION_PAIRS = 32768 (kPartitionPairs,
cms_retract.hip) is grouped by a counting sort, a larger one by the
partition.  The inverse-of-ingest test has a batch on each side of the second
and owners on both sides of the first, and at it; the designed batch of the
first test (below PARTITION_PAIRS) has long runs behind the counting sort.

No test provokes a fault: a refused batch is refused by the checks before any
store, and is tried once.
"""
import os
from collections import Counter

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib
from mahout_amd.synth import zipf_stream

pytestmark = pytest.mark.gpu

FORMS = SketchTable.FORMS  # ("u32", "u16", "u8", "u4", "u2", "u1", "list")
WAVE_RUN = 64
PARTITION_PAIRS = 32768
LAYOUT_VARS = ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_NO_VMM")
D = 4


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _handle(n, w, env=None, d=D, **kw):
    """A handle created under the given layout variables (read once, at creation)."""
    saved = {k: os.environ.pop(k, None) for k in LAYOUT_VARS}
    os.environ.update(env or {})
    try:
        return SketchTable(n, depth=d, width=w, seed=42, **kw)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _default_layout():
    return not any(os.environ.get(v, "") not in ("", "0") for v in LAYOUT_VARS)


def _code(fn, *args):
    with pytest.raises(_lib.CmsError) as ei:
        fn(*args)
    return ei.value.code, str(ei.value)


def _csr(owners):
    off = np.zeros(len(owners) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k in owners])
    return off, np.concatenate([np.asarray(k, np.int64) for k in owners])


def _coo(owners):
    rows = np.concatenate([np.full(len(k), r, np.int64) for r, k in enumerate(owners)])
    return rows, np.concatenate([np.asarray(k, np.int64) for k in owners])


def _device(t, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", t.device))


# ---- the designed table of tests 1, 8 and 10: every stored form ----

N_DESIGNED = 40
_DESIGN = {}


def _spread_keys(oracle, a, b, w, count):
    """`count` keys no two of which share a bucket in any sketch row."""
    cand = np.arange(1000, 1000 + 60 * w, dtype=np.int64)
    hb = oracle.hash_keys(a, b, w, cand)
    used = [set() for _ in range(hb.shape[1])]
    out = []
    for k, row in zip(cand, hb):
        if all(int(x) not in u for x, u in zip(row, used)):
            out.append(int(k))
            for x, u in zip(row, used):
                u.add(int(x))
            if len(out) == count:
                return np.array(out, np.int64)
    raise AssertionError("no spread keys")


def _designed(oracle, w):
    """Per owner (all pairs, the pairs to retract): by owner % 8 a list row (3
    keys), a 1-bit row (20 spread keys), a 2-bit row (12 keys twice), a 4-bit
    row (one key 9 times), a u8 row (one key 100 times), a u16 row (one key
    1000 times), an owner of no keys, a list with a repeated key; the last
    owner is hot (one key 66000 times: mass >= 2^16).  Every owner with keys
    loses some, in every class."""
    if w in _DESIGN:
        return _DESIGN[w]
    a, b = oracle.hash_params(42, D)
    s = _spread_keys(oracle, a, b, w, 20)
    full, take = [], []
    for r in range(N_DESIGNED):
        c = r % 8
        o = 7 * r  # owners of one class differ in their keys
        if r == N_DESIGNED - 1:
            f, t = np.concatenate([s, np.full(66000, s[2])]), np.concatenate([s[::4], np.full(20000, s[2])])
        elif c == 0:
            f, t = np.array([5 + o, 77 + o, 901 + o]), np.array([77 + o])
        elif c == 1:
            f, t = s.copy(), s[::2]
        elif c == 2:
            f, t = np.concatenate([s[:12], s[:12]]), np.concatenate([s[:6], s[6:7], s[6:7]])
        elif c == 3:
            f, t = np.concatenate([s, np.full(8, s[0])]), np.concatenate([np.full(5, s[0]), s[3:4]])
        elif c == 4:
            f, t = np.concatenate([s, np.full(99, s[0])]), np.concatenate([np.full(60, s[0]), s[5:6]])
        elif c == 5:
            f, t = np.concatenate([s, np.full(1000, s[1])]), np.concatenate([np.full(700, s[1]), s[::3]])
        elif c == 6:
            f, t = np.zeros(0, np.int64), np.zeros(0, np.int64)
        else:
            f, t = np.array([3 + o, 3 + o, 40 + o, 41 + o, 42 + o]), np.array([3 + o, 41 + o])
        full.append(np.asarray(f, np.int64))
        take.append(np.asarray(t, np.int64))
    rest = []
    for f, t in zip(full, take):  # the remaining stream: the multiset difference
        left = Counter(f.tolist())
        left.subtract(t.tolist())
        assert all(c >= 0 for c in left.values())
        rest.append(np.array(sorted(left.elements()), np.int64))
    rows_t, keys_t = _coo(take)
    perm = np.random.Generator(np.random.PCG64(w)).permutation(rows_t.size)  # owners interleaved
    rows_r, keys_r = _coo(rest)
    exp = oracle.build_table(N_DESIGNED, D, w, a, b, rows_r, keys_r)
    exp.setflags(write=False)
    _DESIGN[w] = dict(full=full, rest=rest, batch=(rows_t[perm], keys_t[perm]), exp=exp)
    return _DESIGN[w]


def _check_counters(t, exp):
    got = t.read_counters()
    bad = np.flatnonzero((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, ("owners whose counters differ from the oracle", bad[:20], bad.size)


ENVS = [{}, {"CMS_NO_FORMS": "1"}, {"CMS_NO_COMPACT": "1"}, {"CMS_NO_VMM": "1"}]


# ---- 1: every stored form, the remaining stream equals the oracle ----

@pytest.mark.parametrize("w", [128, 100, 256])
@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join(e) or "default")
def test_every_stored_form_gives_the_remaining_streams_table(oracle, w, env):
    ds = _designed(oracle, w)
    with _handle(N_DESIGNED, w, env) as t, _handle(N_DESIGNED, w, env) as fresh:
        t.ingest_csr(*_csr(ds["full"]))
        t.finalize()
        form0 = [FORMS[f] for f in t.owner_forms()[0]]
        print("forms", w, env, sorted(set(form0)))
        if not env and _default_layout() and w % 128 == 0:
            assert set(form0) == set(FORMS), form0
        elif w % 32 != 0 or "CMS_NO_FORMS" in env:
            assert set(form0) <= {"u16", "u32"}, form0
        assert form0[-1] == "u32"
        n0 = t.stats()["pairs_ingested"]
        assert WAVE_RUN < 20000 < ds["batch"][0].size < PARTITION_PAIRS  # long runs behind the counting sort
        t.retract(*ds["batch"])
        assert t.stats()["pairs_ingested"] == n0 - ds["batch"][0].size
        _check_counters(t, ds["exp"])
        # dense rows keep their form; a live list that lost entries is dense now
        form1 = [FORMS[f] for f in t.owner_forms()[0]]
        for r, (f0, f1) in enumerate(zip(form0, form1)):
            assert f1 == f0 or (f0 == "list" and f1 != "list"), (r, f0, f1)
        assert _code(t.similarities, 0, np.arange(N_DESIGNED))[0] == _lib.CMS_E_STATE  # until finalize
        t.finalize()
        _check_counters(t, ds["exp"])
        fresh.ingest_csr(*_csr(ds["rest"]))
        fresh.finalize()
        for q in (0, 5, N_DESIGNED - 1):
            s, so = t.similarities(q, np.arange(N_DESIGNED)), fresh.similarities(q, np.arange(N_DESIGNED))
            assert _same(s, so), q
        for x, y in zip(t.top_k_all(5), fresh.top_k_all(5)):
            assert _same(x, y)


# ---- 2: an owner retracted to nothing ----

def test_an_owner_retracted_to_nothing():
    n, w = 16, 128
    rng = np.random.Generator(np.random.PCG64(2))
    rows, keys = rng.integers(0, n, 400), rng.integers(0, 500, 400)
    mine = rows == 3
    with _handle(n, w) as t:
        t.ingest(rows, keys)
        t.finalize()
        t.retract(rows[mine], keys[mine])
        c = t.read_counters()
        assert not c[3].any() and c[4].any()
        t.finalize()
        others = np.array([r for r in range(n) if r != 3])
        assert np.all(np.isnan(t.similarities(3, others)))
        assert t.point_query(3, int(keys[mine][0])) == 0.0
        assert not np.all(np.isnan(t.similarities(4, others)))


# ---- 3: the check is on sums ----

def test_the_check_is_on_the_sums_per_counter():
    n, w, k = 64, 16, 3
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    rng = np.random.Generator(np.random.PCG64(3))
    rows, keys = rng.integers(8, n, 3000), rng.integers(0, 200, 3000)  # owners [0, 8) are designed below
    with _handle(n, w, owner_ids=ids) as t, _handle(n, w, owner_ids=ids) as twin:
        cand = np.arange(10_000, 10_400, dtype=np.int64)
        hb = t.hash_keys(cand)
        A = int(cand[0])
        # C shares no bucket with A; B shares A's bucket in sketch row 0 and not in row 1
        C = int(cand[np.flatnonzero((hb != hb[0]).all(axis=1))[0]])
        B = int(cand[1:][np.flatnonzero((hb[1:, 0] == hb[0, 0]) & (hb[1:, 1] != hb[0, 1]))[0]])
        drow = np.array([2, 2, 5, 5])  # owner 2 holds A and C once each, owner 5 holds A twice and nothing else
        dkey = np.array([A, C, A, A])
        for x in (t, twin):
            x.ingest(ids[np.concatenate([rows, drow])], np.concatenate([keys, dkey]))
            x.finalize()
            x.top_k_refresh(k)

        def state():
            s = t.stats()
            s.pop("topk_redo")
            return t.read_counters(), t.owner_forms(), s, t.refresh_stats()

        def unchanged(before):
            now = state()
            return (np.array_equal(now[0], before[0]) and all(np.array_equal(x, y) for x, y in zip(now[1], before[1]))
                    and now[2] == before[2] and now[3] == before[3])

        before = state()
        # (a) the pair twice: each copy alone fits the counter (a per-pair comparison with the untouched
        # table would pass), and the owner's mass of 2 covers the batch: the counter rule refuses it
        code, msg = _code(t.retract, ids[[2, 2]], [A, A])
        assert code == _lib.CMS_E_OVERFLOW and "owner ID %d" % ids[2] in msg, msg
        assert unchanged(before)
        # (b) two keys that share a bucket of sketch row 0 (2 <= 2 there) and not of row 1
        code, msg = _code(t.retract, ids[[5, 5]], [A, B])
        assert code == _lib.CMS_E_OVERFLOW and "owner ID %d" % ids[5] in msg, msg
        assert unchanged(before)
        # the device variant names the row
        code, msg = _code(t.retract_device_rows, _device(t, np.array([2, 2], np.int64)),
                          _device(t, np.array([A, A], np.int64)), None, 2)
        assert code == _lib.CMS_E_OVERFLOW and "owner row 2" in msg, msg
        assert unchanged(before)
        t.similarities(ids[2], ids)  # still finalized
        for x, y in zip(t.top_k_refresh(k), twin.top_k_refresh(k)):
            assert _same(x, y)
        assert t.refresh_stats() == twin.refresh_stats()
        # what does fit is then taken out: A once from owner 2, both copies from owner 5
        t.retract(ids[[2, 5, 5]], [A, A, A])
        twin.retract(ids[[5, 2, 5]], [A, A, A])
        assert np.array_equal(t.read_counters(), twin.read_counters())
        assert not t.read_counters()[5].any()


# ---- 4: the mass rule ----

def test_the_mass_rule_and_the_empty_handle():
    n, w = 32, 128
    with _handle(n, w) as t:
        code, msg = _code(t.retract, [3], [17])  # a batch against an empty handle
        assert code == _lib.CMS_E_OVERFLOW
        assert t.stats()["pairs_ingested"] == 0 and not t.read_counters().any()
        t.retract([], [])  # n == 0: nothing, not even an error
        t.retract([3], [17], [0.0])  # a zero value is a no-op
        t.ingest([3, 3, 3, 4], [10, 11, 12, 10])
        t.finalize()
        before = t.read_counters()
        # four unit pairs against a mass of three: no single pair exceeds it
        code, msg = _code(t.retract, [3, 3, 3, 3], [10, 11, 12, 10])
        assert code == _lib.CMS_E_OVERFLOW and "owner row 3" in msg and "mass" in msg, msg
        assert np.array_equal(t.read_counters(), before)
        t.similarities(3, [4])  # the refusal left the handle finalized
        t.retract([], [])
        t.retract([3], [10], [0.0])
        t.similarities(3, [4])  # ... and so do the empty batch and the zero value
        t.retract([3, 3, 3], [10, 11, 12])
        assert not t.read_counters()[3].any()


# ---- 5: values and IDs ----

def test_values_and_ids(oracle):
    n, w = 24, 128
    ids = np.arange(n, dtype=np.int64) * 5 + 100
    a, b = oracle.hash_params(42, D)
    rng = np.random.Generator(np.random.PCG64(5))
    rows, keys = rng.integers(0, n, 600), rng.integers(0, 300, 600)
    vals = (rng.integers(0, 11, 600) / 2).astype(np.float32)  # half stars, 2.5 among them, and zeros
    vals[:4] = 2.5
    out = np.zeros(600, bool)
    out[::3] = True
    with _handle(n, w, owner_ids=ids, frac_bits=1) as t:
        t.ingest(ids[rows], keys, vals)
        t.finalize()
        t.retract(ids[rows[out]], keys[out], vals[out])
        rest = oracle.build_table(n, D, w, a, b, rows[~out], keys[~out], vals[~out])
        assert np.array_equal(t.read_counters(), rest)
        before = t.read_counters()
        good_r, good_k = ids[rows[~out][:5]], keys[~out][:5]
        for bad in (-1.0, 0.25, 1.1):  # negative, and non-dyadic at frac_bits = 1
            code, _ = _code(t.retract, np.append(good_r, ids[0]), np.append(good_k, 1), np.append(vals[~out][:5], bad))
            assert code == _lib.CMS_E_VALUE, bad
        # one bad pair at the end of a good batch writes nothing: an unknown ID, a row equal to n
        code, _ = _code(t.retract, np.append(good_r, 99), np.append(good_k, 1), np.append(vals[~out][:5], 1.0))
        assert code == _lib.CMS_E_NO_SUCH_ID
        code, _ = _code(t.retract_device_rows, _device(t, np.append(rows[~out][:5], n)),
                        _device(t, np.append(good_k, 1)), _device(t, np.append(vals[~out][:5], np.float32(1.0))), 6)
        assert code == _lib.CMS_E_PARAM
        assert np.array_equal(t.read_counters(), before)
    with _handle(n, w) as t, _handle(n, w) as u:  # 2^31 at frac_bits = 0: as the ingest answers it, or the mass rule
        t.ingest([1], [2])
        u.ingest([1], [2])
        big = np.array([2.0 ** 31], np.float32)
        try:
            u.ingest([1], [3], big)
            ingest_code = 0
        except _lib.CmsError as e:
            ingest_code = e.code
        code, _ = _code(t.retract, [1], [3], big)
        assert code in (_lib.CMS_E_VALUE, _lib.CMS_E_OVERFLOW) and ingest_code in (0, code, _lib.CMS_E_OVERFLOW)
        assert t.read_counters()[1].sum() == D


# ---- 6: states ----

def test_states():
    n, w = 40, 128
    with _handle(n, w, counters="f64") as t:
        t.ingest([0, 1], [5, 6], np.array([1, 2], np.float32))
        t.finalize()
        code, msg = _code(t.retract, [0], [5])
        assert code == _lib.CMS_E_STATE and "fp64" in msg
        code, _ = _code(t.retract_device_rows, _device(t, np.array([0], np.int64)), _device(t, np.array([5], np.int64)), None, 1)
        assert code == _lib.CMS_E_STATE
        assert t.stats()["pairs_ingested"] == 2
    with SketchTable.per_owner_shapes(n) as t:
        assert _code(t.retract, [0], [5])[0] == _lib.CMS_E_STATE
    from mahout_amd import transport
    with _handle(n, w, collective_single_rank=True) as t:
        def allgather(send, recv, nbytes):
            host = np.empty(nbytes, np.uint8)
            transport._d2h(host, send, nbytes)
            transport._h2d(recv, host, nbytes)
        t.comm_init_transport(0, 1, lambda ptr, count: None, allgather)
        t.ingest([0, 1, 2, 2], [5, 6, 7, 7])
        t.finalize()
        before = t.read_counters()
        code, msg = _code(t.retract, [2], [7])
        assert code == _lib.CMS_E_STATE and "communicator" in msg
        assert np.array_equal(t.read_counters(), before)
    with _handle(n, w) as t, _handle(n, w) as u:  # before the first finalize
        t.ingest([0, 1, 2, 2], [5, 6, 7, 7])
        t.retract([2, 0], [7, 5])
        u.ingest([1, 2], [6, 7])
        assert np.array_equal(t.read_counters(), u.read_counters())
        assert t.stats()["pairs_ingested"] == 2
        assert _code(t.similarities, 1, [2])[0] == _lib.CMS_E_STATE
        t.finalize()
        u.finalize()
        assert _same(t.similarities(1, np.arange(n)), u.similarities(1, np.arange(n)))
        t.retract([1], [6])
        assert _code(t.similarities, 1, [2])[0] == _lib.CMS_E_STATE  # after a retract, until finalize
        t.finalize()
        assert np.all(np.isnan(t.similarities(1, [2])))


# ---- 7: the inverse of the ingest, on both run classes ----

def _base_2000(w):
    n = 2000
    items, users = zipf_stream(4000, n, 120_000, seed=w)
    order = np.argsort(items, kind="stable")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(items, minlength=n))
    return n, off, users[order].astype(np.int64)


def test_retract_is_the_inverse_of_ingest_on_both_run_classes():
    w = 256
    n, off, keys = _base_2000(w)
    rng = np.random.Generator(np.random.PCG64(7))
    # short runs only: 300 pairs over 300 owners
    short = (rng.choice(n, size=300, replace=False), rng.integers(0, 4000, 300))
    # 70,000 pairs: one owner has 40,000 (a long run), owners with exactly WAVE_RUN and WAVE_RUN + 1 pairs, the rest spread
    spread = 70_000 - 40_000 - (2 * WAVE_RUN + 1)
    rows = np.concatenate([np.full(40_000, 11), np.full(WAVE_RUN, 12), np.full(WAVE_RUN + 1, 13),
                           rng.integers(20, n, spread)])
    mixed = (rows, rng.integers(0, 4000, rows.size))
    perm = rng.permutation(rows.size)
    mixed = (mixed[0][perm], mixed[1][perm])
    counts = np.bincount(mixed[0], minlength=n)
    assert counts[12] == WAVE_RUN and counts[13] == WAVE_RUN + 1 and counts.max() == 40_000
    assert np.bincount(short[0]).max() == 1
    assert short[0].size < PARTITION_PAIRS <= mixed[0].size
    with _handle(n, w) as t:
        t.ingest_csr(off, keys)
        t.finalize()
        before = t.read_counters()
        pairs = t.stats()["pairs_ingested"]
        for batch in (short, mixed):
            t.ingest(*batch)
            assert not np.array_equal(t.read_counters(), before)
            t.retract(*batch)
            assert np.array_equal(t.read_counters(), before)
            assert t.stats()["pairs_ingested"] == pairs
        # the same with the retract after a finalize, and weighted pairs
        vals = rng.integers(0, 4, mixed[0].size).astype(np.float32)
        t.ingest(mixed[0], mixed[1], vals)
        t.finalize()
        t.retract(mixed[0], mixed[1], vals)
        assert np.array_equal(t.read_counters(), before)


# ---- 8: the device variant ----

@pytest.mark.parametrize("w", [128, 100])
def test_the_device_variant_equals_the_host_variant(oracle, w):
    ds = _designed(oracle, w)
    rows, keys = ds["batch"]
    with _handle(N_DESIGNED, w) as t:
        t.ingest_csr(*_csr(ds["full"]))
        t.finalize()
        n0 = t.stats()["pairs_ingested"]
        d_row, d_key = _device(t, rows), _device(t, keys)
        t.retract_device_rows(d_row, d_key, None, rows.size)
        # blocking: the call has returned with the table changed, before any synchronize()
        assert t.stats()["pairs_ingested"] == n0 - rows.size
        _check_counters(t, ds["exp"])
        t.finalize()
        _check_counters(t, ds["exp"])


# ---- 9: the refresh stays incremental ----

def test_refresh_stays_incremental_after_a_retract():
    n, w, k = 2000, 128, 5
    items, users = zipf_stream(4000, n, 120_000, seed=77)
    rng = np.random.Generator(np.random.PCG64(9))
    touched = rng.choice(np.unique(items), size=n * 3 // 100, replace=False)  # 3 % of the owners
    pick = np.concatenate([np.flatnonzero(items == r)[:2] for r in touched])  # up to two of each one's own pairs
    with _handle(n, w) as t:
        t.ingest(items, users)
        t.finalize()
        t.top_k_refresh(k)  # the whole job: the kept lists
        assert t.refresh_stats()[2] == 1
        t.retract(items[pick], users[pick])
        t.finalize()
        got = t.top_k_refresh(k)
        n_touched, _, full = t.refresh_stats()
        assert full == 1, "the retract dropped the kept lists: the refresh was a whole job"
        assert n_touched == np.unique(items[pick]).size == touched.size
        for x, y in zip(got, t.top_k_all(k)):
            assert _same(x, y)


# ---- 10: agrees with the image route ----

def test_retract_agrees_with_the_image_route(oracle):
    w = 128
    ds = _designed(oracle, w)
    with _handle(N_DESIGNED, w) as t, _handle(N_DESIGNED, w) as u, _handle(N_DESIGNED, w) as delta:
        for x in (t, u):
            x.ingest_csr(*_csr(ds["full"]))
            x.finalize()
        delta.ingest(*ds["batch"])
        delta.finalize()
        u.subtract_device(delta.save_device())
        t.retract(*ds["batch"])
        assert np.array_equal(t.read_counters(), u.read_counters())
        assert t.stats()["pairs_ingested"] == u.stats()["pairs_ingested"]
        t.finalize()
        u.finalize()
        for x, y in zip(t.top_k_all(5), u.top_k_all(5)):
            assert _same(x, y)


# ---- 11: the taste route ----

def test_cosinecm_refresh_applies_update_files_in_place(tmp_path):
    from mahout_amd.datamodel import FileDataModel, preference_delta
    from mahout_amd.taste import CosineCM, FixedShapeConfig, HashFunctionBuilder
    rng = np.random.Generator(np.random.PCG64(11))
    users = list(range(1, 41))
    prefs = {u: {int(i): float(rng.integers(1, 11)) / 2 for i in rng.choice(60, size=rng.integers(3, 15), replace=False)}
             for u in users}
    t0 = 1_700_000_000
    data = tmp_path / "ratings.csv"
    data.write_text("".join("%d,%d,%s\n" % (u, i, v) for u in users for i, v in prefs[u].items()))
    os.utime(data, (t0, t0))

    def build(model):
        return CosineCM(model, FixedShapeConfig(4, 128), HashFunctionBuilder(42))

    def agree(sim, fresh):
        assert np.array_equal(sim.table.read_counters(), fresh.table.read_counters())
        assert sim.table.stats()["pairs_ingested"] == fresh.table.stats()["pairs_ingested"]
        for u in (1, 2, 7, 20, 40):
            assert np.array_equal(sim.mostSimilarUserIDs(u, 5), fresh.mostSimilarUserIDs(u, 5)), u

    model = FileDataModel(str(data), update_files=True)
    sim = build(model)
    table0, pairs0 = sim.table, sim.table.stats()["pairs_ingested"]
    old = FileDataModel(str(data), update_files=True)
    # deletes (user 7 is emptied), changed values and additions for known users
    lines = ["%d,%d,\n" % (7, i) for i in prefs[7]]
    lines += ["%d,%d,\n" % (u, next(iter(prefs[u]))) for u in (1, 2, 3)]
    lines += ["%d,%d,%s\n" % (u, list(prefs[u])[1], prefs[u][list(prefs[u])[1]] + 0.5) for u in (4, 5, 20)]
    lines += ["%d,%d,%s\n" % (u, 100 + u, 2.5) for u in (6, 40)]
    up = tmp_path / "ratings.1.csv"
    up.write_text("".join(lines))
    os.utime(up, (t0 + 10, t0 + 10))
    model.refresh()
    sim.refresh()
    (ru, _, _), (au, _, _) = preference_delta(old, model)
    assert ru.size == len(prefs[7]) + 3 + 3 and au.size == 3 + 2
    assert sim.table is table0, "the table was rebuilt"
    assert sim.table.stats()["pairs_ingested"] == pairs0 - ru.size + au.size
    fresh = build(FileDataModel(str(data), update_files=True))
    agree(sim, fresh)
    assert np.all(np.isnan(sim.table.similarities(7, [1, 2, 3])))
    fresh.close()
    # a new user changes the ID universe: the rebuild, which still matches
    up2 = tmp_path / "ratings.2.csv"
    up2.write_text("77,5,3.0\n77,6,1.5\n1,5,4.0\n")
    os.utime(up2, (t0 + 20, t0 + 20))
    model.refresh()
    sim.refresh()
    assert sim.table is not table0
    fresh = build(FileDataModel(str(data), update_files=True))
    agree(sim, fresh)
    assert sim.mostSimilarUserIDs(77, 3).size > 0
    # setDataModel: another model object over the same users is applied in place
    table1 = sim.table
    up3 = tmp_path / "ratings.3.csv"
    up3.write_text("77,5,\n2,%d,5.0\n" % list(prefs[2])[2])
    os.utime(up3, (t0 + 30, t0 + 30))
    newer = FileDataModel(str(data), update_files=True)
    sim.setDataModel(newer)
    sim.refresh()
    assert sim.table is table1
    agree(sim, build(newer))
    sim.close()
