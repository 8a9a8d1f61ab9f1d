"""GPU: the streamed mid-class owners of a fresh build (cms_build.hip:
k_build_classes' cached and streamed lists, the one-pass u8-image kernel
k_build_mid<2, D, 512> and its hand-back to the row-at-a-time u16 rows).

An owner of more than 1024 keys and at most the split threshold is built in
one key pass on a [d][w] u8 image when the increments are units; it is stored
as u8 rows where no counter passes 255 and handed back for u16 rows where one
does or where the owner starts at u16 (more than CMS_MID_U8_KEYS keys).  Every
case is compared bit for bit with the oracle through read_counters(); norms
and maxima through similarities() and top_k_all() against a CMS_NO_FORMS=1
handle built from the same pairs.  The stored form of every owner is pinned
from the rule (u8 iff the oracle's largest counter is at most 255).

The cases go through ingest_csr (a CSR batch always takes the row build;
a COO batch does so only from 262144 pairs on), each under 200K pairs.  The one
exception is the token case: the u32 tokens and their escapes to the key array
exist only behind the COO partition, so that case ingests 286720 pairs.
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable

pytestmark = pytest.mark.gpu

CACHED = 1024  # keys k_build_mid caches in registers: more are streamed
U32, U16, U8 = 0, 1, 2  # SketchTable.FORMS


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _handle(n, d, w, env=None):
    """A handle created under the given tunables (read once, at creation)."""
    env = env or {}
    names = ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_MID_U8_KEYS")
    saved = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(env)
    try:
        return SketchTable(n, depth=d, width=w, seed=42)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _csr(owners):
    off = np.zeros(len(owners) + 1, np.int64)
    off[1:] = np.cumsum([k.size for k in owners])
    return off, np.concatenate(owners).astype(np.int64)


def _pairs(owners):
    rows = np.concatenate([np.full(k.size, i, np.int64) for i, k in enumerate(owners)])
    return rows, np.concatenate(owners).astype(np.int64)


def _distinct(rng, m, span=1 << 20, base=0):
    return base + rng.permutation(span)[:m].astype(np.int64)


def _expected_forms(exp, counts, split, u8_keys, forms=True):
    """The form of every streamed or split owner by the parent's rule (-1: a
    cached owner, whose form -- a list row where that is smaller -- is not
    this file's subject)."""
    mx = exp.max(axis=(1, 2))
    out = np.full(len(counts), -1)
    for i, m in enumerate(counts):
        if m > split:
            out[i] = U32
        elif not forms:
            out[i] = U16
        elif m > CACHED:
            out[i] = U8 if m <= u8_keys and mx[i] <= 255 else U16
    return out


def _check(oracle, t, plain, d, w, owners, exp, want_forms):
    n = len(owners)
    assert np.array_equal(t.read_counters(), exp)
    form, bound = t.owner_forms()
    pinned = want_forms >= 0
    assert np.array_equal(form[pinned], want_forms[pinned]), (form, want_forms)
    mx = exp.max(axis=(1, 2))
    narrow = pinned & (want_forms != U32)
    assert np.array_equal(bound[narrow & (want_forms == U8)], mx[narrow & (want_forms == U8)].astype(np.uint32))
    ids = np.arange(n)
    for q in range(n):
        s = t.similarities(q, ids)
        assert _same(s, plain.similarities(q, ids)), q
        ref = oracle.similarities_row(exp, q)
        ref[q] = oracle.cosine_cm(exp[q], exp[q])
        assert _same(s, ref), q
    got = t.top_k_all(min(5, n - 1))
    want = plain.top_k_all(min(5, n - 1))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, want))


# (d, w): the bench instantiation, the other unrolled depth, the generic depth
# at a width that is no power of two (bucket_exact), and a shape whose u8 image
# (128 KB) exceeds the LDS budget, which builds without forms
@pytest.mark.parametrize("d,w,layout", [(5, 8192, "compact"), (5, 8192, "slots"), (4, 1024, "compact"),
                                        (3, 96, "compact"), (8, 16384, "compact")])
def test_streamed_key_counts(oracle, d, w, layout):
    """Key counts on either side of the cached / streamed boundary (1024,
    1025), one that is no multiple of the kernel's 1024-key step, either side
    of the u16 start (CMS_MID_U8_KEYS) and either side of the split threshold
    (the neighbour class, k_build_slices)."""
    rng = np.random.Generator(np.random.PCG64(d * 100003 + w))
    env = {"CMS_NO_COMPACT": "1"} if layout == "slots" else {}
    if w >= 8192:
        split, u8_keys = 16384, 12288  # the defaults
    else:
        split, u8_keys = 8192, 4096    # the split threshold of narrower sketches is below the default u16 start
        env["CMS_MID_U8_KEYS"] = str(u8_keys)
    counts = [CACHED, CACHED + 1, 1500, 2 * CACHED, 2 * CACHED + 1, u8_keys, u8_keys + 1, split, split + 1]
    owners = [_distinct(rng, m) for m in counts]
    n = len(owners)
    off, keys = _csr(owners)
    assert keys.size < 200_000
    a, b = oracle.hash_params(42, d)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    forms = d * w <= 64 * 1024
    want = _expected_forms(exp, counts, split, u8_keys, forms)
    with _handle(n, d, w, env) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        _check(oracle, t, plain, d, w, owners, exp, want)
        st = t.stats()
        assert st["hot_rows"] == 1, st
        if forms:  # (the cached owner may be a u8 row too)
            assert int(np.sum(want == U8)) <= st["u8_rows"] <= int(np.sum(want == U8)) + 1, (st, want)


def _free_key(oracle, a, b, w, taken, start):
    """The first key from `start` whose buckets are all outside `taken`
    ([d] sets of buckets), and its buckets."""
    for k in range(start, start + 100000):
        bk = oracle.hash_keys(a, b, w, np.array([k]))[0]
        if all(int(bk[r]) not in taken[r] for r in range(len(bk))):
            return k, bk
    raise AssertionError("no free key")


def test_streamed_counter_widths(oracle):
    """A streamed owner whose one key repeats 255 times stays u8; one whose
    key repeats 256 times leaves through the hand-back as u16; and both again
    with a second key in the same packed LDS word of sketch row 0 (a counter at
    255, or passing it, next to a non-zero neighbour: the carry case)."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(7))
    a, b = oracle.hash_params(42, d)
    base = _distinct(rng, 1100, span=1 << 16)
    hb = oracle.hash_keys(a, b, w, base)
    taken = [set(hb[:, r].tolist()) for r in range(d)]
    rep, rb = _free_key(oracle, a, b, w, taken, 1 << 17)
    for r in range(d):
        taken[r].add(int(rb[r]))
    # a neighbour: row-0 bucket in the same 4-byte word as rep's, another byte,
    # and no bucket shared with the base keys or with rep
    cand = np.arange(1 << 18, (1 << 18) + 400000, dtype=np.int64)
    cb = oracle.hash_keys(a, b, w, cand)
    ok = ((cb[:, 0] >> 2) == (int(rb[0]) >> 2)) & (cb[:, 0] != int(rb[0]))
    nb = None
    for i in np.flatnonzero(ok):
        if all(int(cb[i, r]) not in taken[r] for r in range(d)):
            nb = int(cand[i])
            break
    assert nb is not None
    owners = [np.concatenate([base, np.full(255, rep)]),
              np.concatenate([base, np.full(256, rep)]),
              np.concatenate([base, np.full(255, rep), np.full(3, nb)]),
              np.concatenate([base, np.full(256, rep), np.full(3, nb)]),
              np.concatenate([np.full(200, rep), base, np.full(200, rep)])]  # 400 in one counter, spread over the pass
    owners = [rng.permutation(k) for k in owners]
    n = len(owners)
    off, keys = _csr(owners)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    assert [int(x) for x in exp.max(axis=(1, 2))] == [255, 256, 255, 256, 400]
    want = np.array([U8, U16, U8, U16, U16])
    with _handle(n, d, w) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        _check(oracle, t, plain, d, w, owners, exp, want)
        for q in range(n):
            for key in (rep, nb, int(base[0])):
                assert t.point_query(q, key) == oracle.sketch_get(exp[q], a, b, key)


def _wide_keys(rng, m):
    """Keys below 2^31, in [2^31, 2^32), at and above 2^32, and negative."""
    q = m // 4
    return rng.permutation(np.concatenate([
        _distinct(rng, m - 3 * q),
        _distinct(rng, q, base=1 << 31), np.array([1 << 31, (1 << 32) - 1])[: min(q, 2)],
        _distinct(rng, q, base=1 << 32), np.array([1 << 32, (1 << 62) + 5])[: min(q, 2)],
        -1 - _distinct(rng, q)]))


def test_streamed_wide_keys_csr(oracle):
    """int64 keys at and above 2^31 and 2^32 (the hash's route for keys that
    do not fit 32 bits) in streamed owners of a CSR batch."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(11))
    counts = [1025, 3000, 5001]
    owners = [_wide_keys(rng, m) for m in counts]
    n = len(owners)
    off, keys = _csr(owners)
    a, b = oracle.hash_params(42, d)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    want = _expected_forms(exp, [k.size for k in owners], 16384, 12288)
    with _handle(n, d, w) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        _check(oracle, t, plain, d, w, owners, exp, want)


def test_streamed_wide_keys_tokens(oracle):
    """The same keys behind the COO partition: a key in [0, 2^31) travels as
    its own u32 token, any other as an index into the batch's keys."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(13))
    counts = [7168] * 40  # 286720 pairs: the smallest COO batches that take the row build have 262144
    owners = [_wide_keys(rng, m) for m in counts]
    n = len(owners)
    rows, keys = _pairs(owners)
    order = rng.permutation(rows.size)
    a, b = oracle.hash_params(42, d)
    exp = oracle.build_table(n, d, w, a, b, rows[order], keys[order])
    want = _expected_forms(exp, [k.size for k in owners], 16384, 12288)
    assert np.all(want == U8)
    with _handle(n, d, w) as t:
        t.ingest(rows[order], keys[order])
        t.finalize()
        assert np.array_equal(t.read_counters(), exp)
        form, _ = t.owner_forms()
        assert np.array_equal(form, want)
        ids = np.arange(n)
        for q in (0, n - 1):
            ref = oracle.similarities_row(exp, q)
            ref[q] = oracle.cosine_cm(exp[q], exp[q])
            assert _same(t.similarities(q, ids), ref), q


def _streamed_only(rng):
    """Owners that are all streamed or split: their forms do not depend on
    whether the increments are implicit (list rows need implicit units)."""
    counts = [1025, 1500, 4096, 4097, 9000, 12288, 12289, 16384, 16385]
    return counts, [_distinct(rng, m, span=1 << 15) for m in counts]


def test_streamed_weighted_takes_row_passes(oracle):
    """A weighted ingest with streamed owners is built row at a time (the
    one-pass kernel counts units only): counters equal the oracle's."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(17))
    counts, owners = _streamed_only(rng)
    n = len(owners)
    off, keys = _csr(owners)
    vals = rng.integers(1, 4, keys.size).astype(np.float32)
    a, b = oracle.hash_params(42, d)
    rows, _ = _pairs(owners)
    exp = oracle.build_table(n, d, w, a, b, rows, keys, vals)
    with _handle(n, d, w) as t:
        t.ingest_csr(off, keys, vals)
        t.finalize()
        assert np.array_equal(t.read_counters(), exp)
        ids = np.arange(n)
        for q in (0, 3, n - 1):
            ref = oracle.similarities_row(exp, q)
            ref[q] = oracle.cosine_cm(exp[q], exp[q])
            assert _same(t.similarities(q, ids), ref), q


def test_streamed_stats_equal_row_passes(oracle):
    """stats() of the one-pass build equal those of the same stream built row
    at a time: explicit increments of 1.0 disable the one-pass kernel and give
    the same counters (every owner here is streamed or split, so no form
    depends on the increments being implicit)."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(19))
    counts, owners = _streamed_only(rng)
    # one owner a counter sends back to u16
    owners[2] = np.concatenate([owners[2][:-300], np.full(300, int(owners[2][0]))])
    n = len(owners)
    off, keys = _csr(owners)
    a, b = oracle.hash_params(42, d)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    want = _expected_forms(exp, counts, 16384, 12288)
    assert want[2] == U16 and np.sum(want == U8) >= 4
    with _handle(n, d, w) as t, _handle(n, d, w) as rowwise:
        t.ingest_csr(off, keys)
        rowwise.ingest_csr(off, keys, np.ones(keys.size, np.float32))
        for x in (t, rowwise):
            x.finalize()
            assert np.array_equal(x.read_counters(), exp)
            assert np.array_equal(x.owner_forms()[0], want)
        st, sr = t.stats(), rowwise.stats()
        for f in ("stored_bytes", "hot_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows", "list_rows"):
            assert st[f] == sr[f], (f, st, sr)
        assert st["u8_rows"] == int(np.sum(want == U8)) and st["hot_rows"] == 1
