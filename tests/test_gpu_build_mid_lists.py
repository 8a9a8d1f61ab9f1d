"""GPU: the cached mid-class list rows of a fresh build (cms_build.hip:
k_build_mid_lists<2, D>, the wave-per-owner kernel of the owners mid_list_row
makes list rows, and mid_rows, which builds them wherever that kernel does not
exist -- another depth, a width that is no power of two -- and the owners it
sends back).

A cached mid owner (256 to 1024 keys with unit increments) is a list row when
d m <= 8192 and its list (2 + 2 d m bytes) is smaller than the 4-bit row, as
long as no counter passes 255; past that it is a u16 row.  Every case is
compared bit for bit with the oracle through read_counters(); norms and maxima
through similarities() and top_k_all() against a CMS_NO_FORMS=1 handle built
from the same pairs; the stored form of every owner is pinned from the rule.

The cases go through ingest_csr (a CSR batch always takes the row build), each
under 200K pairs, with two exceptions: the token case (the u32 tokens and their
escapes exist only behind the COO partition, which takes the row build from
262144 pairs on) and the many-owners case (a wave of the resident grid takes a
second owner only past some 5000 owners of at least 256 keys each).
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable

pytestmark = pytest.mark.gpu

U32, U16, U8, U4, U2, U1, LIST = range(7)  # SketchTable.FORMS
BYTE_KEYS = 256        # the byte class: at most this many keys and a mass bound below 256
LIST_KEYS = 256        # CMS_LIST_KEYS, the byte class's list rows
CACHED_KEYS = 1024     # cached mid owners (and the most keys of a mid list row)
MID_U4_KEYS, MID_U8_KEYS = 768, 12288  # the default tunables: the first dense form of a mid owner


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _handle(n, d, w, env=None):
    """A handle created under the given tunables (read once, at creation)."""
    env = env or {}
    names = ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_LIST_KEYS", "CMS_MID_U4_KEYS", "CMS_MID_U8_KEYS")
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


def _pairs(owners, rows=None):
    rows = range(len(owners)) if rows is None else rows
    own = np.concatenate([np.full(owners[r].size, i, np.int64) for i, r in enumerate(rows)])
    return own, np.concatenate([owners[r] for r in rows]).astype(np.int64)


def _distinct(rng, m, span=1 << 20, base=0):
    return base + rng.choice(span, size=m, replace=False).astype(np.int64)


def _mid_list(m, d, w):
    """mid_list_row for unit increments."""
    return m <= CACHED_KEYS and d * m <= 8192 and 2 + 2 * d * m < d * w // 2


def _byte_list(m, d, w):
    """nib_list_row for unit increments at the default tunables."""
    first = 1 if m <= 64 and w % 128 == 0 else 2 if m <= 256 and w % 64 == 0 else 4
    return m <= LIST_KEYS and 2 + 2 * d * m <= d * w * first // 8


def _expected_form(m, mx, d, w):
    """The form of a unit-increment owner of m keys and largest counter mx by
    the rules (-1: a dense byte-class row, not this file's subject)."""
    if m < BYTE_KEYS:
        return LIST if _byte_list(m, d, w) else -1
    if m <= CACHED_KEYS and _mid_list(m, d, w):
        return LIST if mx <= 255 else U16
    if m <= MID_U4_KEYS and mx <= 15:
        return U4
    assert m <= MID_U8_KEYS
    return U8 if mx <= 255 else U16


def _expected_forms(mx, counts, d, w):
    return np.array([_expected_form(m, mx[i], d, w) for i, m in enumerate(counts)])


def _row0(oracle, a, b, w, start, count):
    cand = np.arange(start, start + count, dtype=np.int64)
    return cand, oracle.hash_keys(a, b, w, cand)[:, 0]


def _colliding(oracle, a, b, w, count=3, start=1 << 21):
    """`count` distinct keys that share one bucket of sketch row 0."""
    cand, b0 = _row0(oracle, a, b, w, start, 40 * w)
    for bk in np.unique(b0):
        hit = cand[b0 == bk]
        if hit.size >= count:
            return hit[:count]
    raise AssertionError("no colliding keys")


def _neighbours(oracle, a, b, w, start=1 << 22):
    """Two keys whose row-0 buckets are different counters of one 32-bit word
    of a u8 image (buckets 4 j and 4 j + 1)."""
    cand, b0 = _row0(oracle, a, b, w, start, 40 * w)
    first = {}
    for k, bk in zip(cand, b0):
        first.setdefault(int(bk), int(k))
    for bk, k in first.items():
        if bk % 4 == 0 and bk + 1 in first:
            return np.array([k, first[bk + 1]], np.int64)
    raise AssertionError("no neighbouring keys")


def _wide_keys(rng, m):
    """Keys below 2^31, in [2^31, 2^32), at and above 2^32, and negative."""
    q = m // 4
    return rng.permutation(np.concatenate([
        _distinct(rng, m - 3 * q),
        _distinct(rng, q - 2, base=1 << 31), np.array([1 << 31, (1 << 32) - 1]),
        _distinct(rng, q - 2, base=1 << 32), np.array([1 << 32, (1 << 62) + 5]),
        -1 - _distinct(rng, q)]))


def _repeated(rng, m, times, key=None):
    """An owner of m keys, one of them `times` times."""
    k = _distinct(rng, m - times + 1)
    rep = k[0] if key is None else key
    return rng.permutation(np.concatenate([k[1:], np.full(times, rep, np.int64)]))


SLOT_EDGES = (255, 256, 257, 319, 320, 321, 639, 640, 641, 1023, 1024, 1025)
REPEATS = (15, 16, 255, 256)


def _kinds(rng, oracle, a, b, w):
    """Key counts at the edges of the 64-key slots and of the groups of four
    slots, with the byte-class (255) and streamed (1025) neighbours; one key
    15, 16, 255 and 256 times in an owner of 300; three keys in one bucket;
    two keys in neighbouring counters of one LDS word, one of them 255 times;
    wide keys in owners of about 300 and 1000 keys."""
    owners = [_distinct(rng, m) for m in SLOT_EDGES]
    owners += [_repeated(rng, 300, t) for t in REPEATS]
    owners.append(np.concatenate([_colliding(oracle, a, b, w), _distinct(rng, 297)]))
    nb = _neighbours(oracle, a, b, w)
    owners.append(np.concatenate([np.full(255, nb[0]), np.full(3, nb[1]), _distinct(rng, 42)]))
    owners.append(_wide_keys(rng, 300))
    owners.append(_wide_keys(rng, 1000))
    return owners


def _check(oracle, t, plain, d, w, owners, exp, want_forms):
    n = len(owners)
    assert np.array_equal(t.read_counters(), exp)
    form, bound = t.owner_forms()
    pinned = want_forms >= 0
    assert np.array_equal(form[pinned], want_forms[pinned]), (form, want_forms)
    mx = exp.max(axis=(1, 2))
    lists = pinned & (want_forms == LIST)
    assert np.array_equal(bound[lists], mx[lists].astype(np.uint32))
    assert t.stats()["list_rows"] == int(np.sum(form == LIST))
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


def _run(oracle, d, w, owners, env=None, coo=None):
    """Builds the owners (CSR, or the COO pairs given) in a handle under env
    and in a CMS_NO_FORMS=1 handle, checks both ways; returns (forms, mx)."""
    n = len(owners)
    counts = [k.size for k in owners]
    a, b = oracle.hash_params(42, d)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    mx = exp.max(axis=(1, 2))
    want = _expected_forms(mx, counts, d, w)
    with _handle(n, d, w, env) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            if coo is None:
                off, keys = _csr(owners)
                assert keys.size < 200_000
                x.ingest_csr(off, keys)
            else:
                x.ingest(*coo)
            x.finalize()
        _check(oracle, t, plain, d, w, owners, exp, want)
        return want, mx


@pytest.mark.parametrize("layout", ["compact", "slots"])
def test_mid_list_owner_kinds(oracle, layout):
    """Slot edges, repeats and wide keys at the bench shape, in both layouts."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(901))
    a, b = oracle.hash_params(42, d)
    owners = _kinds(rng, oracle, a, b, w)
    counts = [k.size for k in owners]
    env = {"CMS_NO_COMPACT": "1"} if layout == "slots" else {}
    want, mx = _run(oracle, d, w, owners, env)
    ne = len(SLOT_EDGES)
    # every cached key count is a list row here; 255 is the byte class's list, 1025 a streamed u8 row
    assert all(want[i] == LIST for i, m in enumerate(SLOT_EDGES) if m <= CACHED_KEYS)
    assert want[SLOT_EDGES.index(1025)] == U8
    rep = want[ne:ne + len(REPEATS)]
    assert [int(mx[ne + i]) for i in range(len(REPEATS))] == list(REPEATS)
    assert list(rep) == [LIST, LIST, LIST, U16]  # 256 of one key: sent back for u16 rows
    assert mx[ne + 4] == 3 and want[ne + 4] == LIST      # three keys in one bucket
    assert mx[ne + 5] == 255 and want[ne + 5] == LIST    # 255 beside 3 in one LDS word
    assert counts[ne + 6] == 300 and counts[ne + 7] == 1000 and want[ne + 6] == LIST and want[ne + 7] == LIST


def test_mid_list_point_queries(oracle):
    """Point queries of the repeated, colliding and neighbouring keys."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(902))
    a, b = oracle.hash_params(42, d)
    owners = _kinds(rng, oracle, a, b, w)[len(SLOT_EDGES):]
    n = len(owners)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    with _handle(n, d, w) as t:
        t.ingest_csr(*_csr(owners))
        t.finalize()
        for q in range(n):
            vals, cnt = np.unique(owners[q], return_counts=True)
            for key in (vals[np.argmax(cnt)], owners[q][0], owners[q][-1]):
                assert t.point_query(q, int(key)) == oracle.sketch_get(exp[q], a, b, int(key)), (q, key)


# shapes that move the rule: the other unrolled depth; widths at which the
# largest cached owners are no list rows; a shape without any cached list row;
# a depth that is not unrolled and a width that is no power of two (both
# through mid_rows)
@pytest.mark.parametrize("d,w", [(4, 8192), (5, 4096), (5, 2048), (4, 1024), (3, 8192), (5, 6144)])
def test_mid_list_rule_shapes(oracle, d, w):
    rng = np.random.Generator(np.random.PCG64(d * 100003 + w))
    counts = (255, 256, 300, 511, 512, 513, 767, 768, 769, 1000, 1023, 1024, 1025)
    owners = [_distinct(rng, m) for m in counts]
    owners += [_repeated(rng, 300, t) for t in (16, 256)] + [_repeated(rng, 1000, 16), _wide_keys(rng, 500)]
    want, mx = _run(oracle, d, w, owners)
    by_m = {m: want[i] for i, m in enumerate(counts)}
    if (d, w) == (5, 4096):
        assert by_m[1023] == LIST and by_m[1024] == U8
    if (d, w) == (5, 2048):
        assert by_m[511] == LIST and by_m[512] != LIST and by_m[1024] == U8
    if (d, w) == (4, 1024):
        assert not any(want[i] == LIST for i, k in enumerate(owners) if k.size >= BYTE_KEYS)
    if w >= 6144:
        assert all(by_m[m] == LIST for m in counts if m <= CACHED_KEYS)
        assert want[len(counts) + 1] == U16  # one key 256 times


def test_mid_list_owners_weighted(oracle):
    """The same key counts with explicit increments: no list rows."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(903))
    a, b = oracle.hash_params(42, d)
    owners = [_distinct(rng, m) for m in (255, 256, 300, 640, 1023, 1024, 1025)] + [_repeated(rng, 300, 16)]
    n = len(owners)
    off, keys = _csr(owners)
    vals = rng.integers(1, 3, keys.size).astype(np.float32)
    rows, _ = _pairs(owners)
    exp = oracle.build_table(n, d, w, a, b, rows, keys, vals)
    with _handle(n, d, w) as t:
        t.ingest_csr(off, keys, vals)
        t.finalize()
        assert np.array_equal(t.read_counters(), exp)
        form, _ = t.owner_forms()
        assert not np.any(form == LIST) and t.stats()["list_rows"] == 0
        ids = np.arange(n)
        for q in range(n):
            ref = oracle.similarities_row(exp, q)
            ref[q] = oracle.cosine_cm(exp[q], exp[q])
            assert _same(t.similarities(q, ids), ref), q


def test_mid_list_rows_tokens(oracle):
    """The same behind the COO partition: a key in [0, 2^31) travels as its
    own u32 token, any other as an index into the batch's keys."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(904))
    owners = []
    for i in range(40):
        m = int(rng.integers(256, 1025))
        owners.append(_wide_keys(rng, m) if i % 2 == 0 else _distinct(rng, m))
    owners += [_wide_keys(rng, 300), _wide_keys(rng, 1000), _repeated(rng, 300, 256), _distinct(rng, 255)]
    have = sum(k.size for k in owners)
    while have < 266_000:  # streamed owners fill the batch up to the row build's smallest COO size
        owners.append(_distinct(rng, 4000) if len(owners) % 2 else _wide_keys(rng, 4000))
        have += 4000
    rows, keys = _pairs(owners)
    assert 262144 <= keys.size < 300_000
    order = rng.permutation(rows.size)
    want, _ = _run(oracle, d, w, owners, coo=(rows[order], keys[order]))
    assert np.sum(want == LIST) >= 43 and np.sum(want == U16) >= 1


MANY = 11_000     # more than twice the waves of the resident grid (256 CUs x 5 workgroups x 4 waves at the most)
STREAMED = 300


def test_many_mid_list_owners(oracle):
    """More cached list rows than the resident grid has waves, so a wave takes
    several owners in turn (the prefetched spans, places and first keys), with
    owners that k_build_mid_lists and the one-pass streamed kernel both send
    back to the cached list in one build.  About 3.6M pairs: the smallest
    batch in which a wave walks its list."""
    import torch
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(905))
    a, b = oracle.hash_params(42, d)
    counts = rng.integers(256, 290, MANY)
    counts[rng.choice(MANY, 600, replace=False)] = rng.integers(290, 1025, 600)
    counts[:4] = (1024, 256, 1023, 257)
    counts[-4:] = (256, 1024, 641, 1000)
    counts = np.concatenate([counts, rng.integers(1025, 1200, STREAMED)])
    n = counts.size
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(counts)
    # Zipf-repeated keys: the popular keys repeat inside an owner, the most
    # popular past 255 times in some of the larger owners
    keys = (rng.zipf(1.25, int(off[-1])) % (1 << 20)).astype(np.int64)
    # every third streamed owner repeats one key 300 times (the streamed kernel sends it back)
    for r in range(MANY, n, 3):
        keys[off[r]:off[r] + 300] = 7_000_000 + r
    # and some cached owners one key 256 times (k_build_mid_lists sends them back)
    sent = rng.choice(np.arange(4, MANY - 4), 200, replace=False)
    for r in sent:
        keys[off[r]:off[r] + 256] = 8_000_000 + r
    owners = [keys[off[r]:off[r + 1]] for r in range(n)]
    with _handle(n, d, w) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        # the whole table against the handle without forms, and every owner's largest counter
        mx = np.zeros(n, np.int64)
        for r0 in range(0, n, 512):
            rc = min(512, n - r0)
            got = t.read_counters_device(r0, rc)
            ref = plain.read_counters_device(r0, rc)
            assert bool(torch.equal(got, ref)), r0
            mx[r0:r0 + rc] = ref.reshape(rc, -1).max(dim=1).values.cpu().numpy()
        form, bound = t.owner_forms()
        want = _expected_forms(mx, counts, d, w)
        assert np.array_equal(form, want), np.nonzero(form != want)[0][:20]
        assert np.all(want[sent] == U16) and np.all(want[np.arange(MANY, n, 3)] == U16)
        assert np.sum(want == LIST) > 2 * 5120 and np.sum(want[:MANY] == U16) >= 200
        lists = want == LIST
        assert np.array_equal(bound[lists], mx[lists].astype(np.uint32))
        # sampled owners against the oracle: both ends of the table, owners sent back, streamed ones
        sel = np.unique(np.concatenate([np.arange(6), np.arange(MANY - 6, MANY + 6), np.arange(n - 3, n), sent[:6],
                                        rng.choice(n, 12, replace=False)]))
        exp = oracle.build_table(sel.size, d, w, a, b, *_pairs(owners, sel))
        for i, r in enumerate(sel):
            assert np.array_equal(t.read_counters(int(r), 1)[0], exp[i]), r
        for qi in range(0, sel.size, 5):
            s = t.similarities(int(sel[qi]), sel)
            assert _same(s, plain.similarities(int(sel[qi]), sel)), qi
            ref = np.array([oracle.cosine_cm(exp[qi], exp[j]) for j in range(sel.size)])
            assert _same(s, ref), qi
