"""GPU: the byte-class list rows of a fresh build (cms_build.hip:
k_build_lists<2, D>, the depth-unrolled kernel of the owners nib_list_row
makes list rows, and k_build_nibbles, which builds them wherever that kernel
does not exist: another depth, a width that is no power of two, weighted
increments).

An owner of at most 255 keys whose list (2 + 2 d m bytes) is no larger than
the dense row it would take first is stored as a list row.  Every case is
compared bit for bit with the oracle through read_counters(); norms and
maxima through similarities() and top_k_all() against a CMS_NO_FORMS=1 handle
built from the same pairs; the stored form of every byte-class owner and the
row counts and stored bytes of stats() are pinned from the rule.

The cases go through ingest_csr (a CSR batch always takes the row build; a
COO batch does so only from 262144 pairs on), each under 200K pairs.  The one
exception is the token case: the u32 tokens and their escapes to the key array
exist only behind the COO partition, so that case ingests about 287K pairs.
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable

pytestmark = pytest.mark.gpu

U32, U16, U8, U4, U2, U1, LIST = range(7)  # SketchTable.FORMS
BYTE_KEYS = 256  # the byte class: at most this many keys and a mass bound below 256
BIT_KEYS, CRUMB_KEYS, LIST_KEYS = 64, 256, 256  # the default tunables


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _handle(n, d, w, env=None):
    """A handle created under the given tunables (read once, at creation)."""
    env = env or {}
    names = ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_LIST_KEYS", "CMS_BIT_KEYS", "CMS_CRUMB_KEYS")
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


def _first_bits(m, w):
    return 1 if m <= BIT_KEYS and w % 128 == 0 else 2 if m <= CRUMB_KEYS and w % 64 == 0 else 4


def _is_list(m, d, w, weighted=False):
    """nib_list_row: unit increments, at most CMS_LIST_KEYS keys, the list no
    larger than the dense row the owner would take first."""
    return not weighted and m <= LIST_KEYS and 2 + 2 * d * m <= d * w * _first_bits(m, w) // 8


def _expected_forms(mx, counts, d, w):
    """The form of every byte-class owner by the rule (-1: another class's
    owner, whose form is not this file's subject): a list row where
    nib_list_row says so, whatever its counters; else the narrowest of the
    1-, 2-, 4- and 8-bit rows, from the one its key count starts at, that
    holds its largest counter."""
    out = np.full(len(counts), -1)
    for i, m in enumerate(counts):
        if m >= BYTE_KEYS:
            continue
        if _is_list(m, d, w):
            out[i] = LIST
            continue
        first = _first_bits(m, w)
        out[i] = (U1 if first == 1 and mx[i] <= 1 else U2 if first <= 2 and mx[i] <= 3 else U4 if mx[i] <= 15 else U8)
    return out


def _colliding(oracle, a, b, w, count=3, start=1 << 21):
    """`count` distinct keys that share one bucket of sketch row 0."""
    cand = np.arange(start, start + 40 * w, dtype=np.int64)
    b0 = oracle.hash_keys(a, b, w, cand)[:, 0]
    for bk in np.unique(b0):
        hit = cand[b0 == bk]
        if hit.size >= count:
            return hit[:count]
    raise AssertionError("no colliding keys")


def _wide_keys(rng, m):
    """Keys below 2^31, in [2^31, 2^32), at and above 2^32, and negative."""
    q = m // 4
    return rng.permutation(np.concatenate([
        _distinct(rng, m - 3 * q),
        _distinct(rng, q - 2, base=1 << 31), np.array([1 << 31, (1 << 32) - 1]),
        _distinct(rng, q - 2, base=1 << 32), np.array([1 << 32, (1 << 62) + 5]),
        -1 - _distinct(rng, q)]))


def _special(rng, oracle, a, b, w):
    """The owners at the edges: key counts at the edges of the four 64-key
    slots, the mid-class neighbour (256 keys), one key 15 times (still
    4-bit-countable) and 16 times (sent to k_build_bytes), three keys in one
    bucket, and wide keys."""
    owners = [_distinct(rng, m) for m in (0, 1, 63, 64, 65, 128, 129, 192, 193, 255, 256)]
    owners.append(np.full(15, 777, np.int64))
    owners.append(np.full(16, 778, np.int64))
    owners.append(_colliding(oracle, a, b, w))
    owners.append(np.concatenate([_colliding(oracle, a, b, w, start=1 << 22), _distinct(rng, 30)]))
    owners.append(_wide_keys(rng, 40))
    owners.append(_wide_keys(rng, 100))
    return owners


def _small(rng, count):
    """Random small owners: mostly a few keys, some empty, some up to 255,
    a repeated key now and then."""
    out = []
    for _ in range(count):
        kind = rng.integers(0, 10)
        m = 0 if kind == 0 else int(rng.integers(1, 256)) if kind == 1 else int(rng.integers(1, 40))
        k = _distinct(rng, m, span=1 << 16)
        if kind == 2 and m > 2:
            k[1:3] = k[0]
        out.append(k)
    return out


def _mixed(rng, oracle, a, b, w, nsmall):
    """The special owners among random small ones, in random order, with a
    special owner in the first and in the last row."""
    sp = _special(rng, oracle, a, b, w)
    rest = sp[1:-1] + _small(rng, nsmall)
    return [sp[0]] + [rest[i] for i in rng.permutation(len(rest))] + [sp[-1]]


def _check_stats(t, form, counts, d, w):
    """stats() row counts and stored bytes from the forms and the list rule."""
    st = t.stats()
    dw = d * w
    cnt = [int(np.sum(form == f)) for f in range(7)]
    assert (st["hot_rows"], st["u8_rows"], st["nibble_rows"], st["crumb_rows"], st["bit_rows"], st["list_rows"]) == \
        (cnt[U32], cnt[U8], cnt[U4], cnt[U2], cnt[U1], cnt[LIST]), (st, cnt)
    list_bytes = sum(2 + 2 * d * m for m, f in zip(counts, form) if f == LIST)
    want = 4 * cnt[U32] * dw + 2 * cnt[U16] * dw + cnt[U8] * dw + cnt[U4] * dw // 2 + cnt[U2] * dw // 4 + \
        cnt[U1] * dw // 8 + list_bytes
    assert st["stored_bytes"] == want, (st, cnt, list_bytes)


def _check(oracle, t, plain, d, w, owners, exp, want_forms):
    n = len(owners)
    counts = [k.size for k in owners]
    assert np.array_equal(t.read_counters(), exp)
    form, bound = t.owner_forms()
    pinned = want_forms >= 0
    assert np.array_equal(form[pinned], want_forms[pinned]), (form, want_forms)
    mx = exp.max(axis=(1, 2))
    lists = pinned & (want_forms == LIST)
    assert np.array_equal(bound[lists], mx[lists].astype(np.uint32))
    _check_stats(t, form, counts, d, w)
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


# (d, w): the bench instantiation in both layouts, the other instantiation at
# the smallest width with byte-class lists, the generic depth and a width that
# is no power of two (both through k_build_nibbles)
@pytest.mark.parametrize("d,w,layout", [(5, 8192, "compact"), (5, 8192, "slots"), (4, 1024, "compact"),
                                        (3, 1024, "compact"), (5, 96, "compact")])
def test_list_owner_kinds(oracle, d, w, layout):
    """Every kind of byte-class owner among a few hundred random small ones."""
    rng = np.random.Generator(np.random.PCG64(d * 100003 + w))
    a, b = oracle.hash_params(42, d)
    owners = _mixed(rng, oracle, a, b, w, 200)
    n = len(owners)
    counts = [k.size for k in owners]
    off, keys = _csr(owners)
    assert keys.size < 200_000
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    mx = exp.max(axis=(1, 2))
    assert sorted(int(mx[i]) for i, m in enumerate(counts) if m in (15, 16) and np.all(owners[i] == owners[i][0])) \
        == [15, 16]
    assert any(m == 3 and mx[i] == 3 for i, m in enumerate(counts))  # the three colliding keys
    want = _expected_forms(mx, counts, d, w)
    assert np.sum(want == LIST) > 100
    if w >= 8192:
        assert np.all(want[np.array(counts) < BYTE_KEYS] == LIST)
    env = {"CMS_NO_COMPACT": "1"} if layout == "slots" else {}
    with _handle(n, d, w, env) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        _check(oracle, t, plain, d, w, owners, exp, want)
        for q, m in enumerate(counts):
            if m in (3, 15, 16):
                assert t.point_query(q, int(owners[q][0])) == oracle.sketch_get(exp[q], a, b, int(owners[q][0]))


def test_list_owners_weighted_take_the_generic_kernel(oracle):
    """The same owners with explicit increments: no list rows, the oracle's
    table through k_build_nibbles."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(23))
    a, b = oracle.hash_params(42, d)
    # (a weighted owner's mass bound, not its key count, decides its class)
    owners = [k for k in _mixed(rng, oracle, a, b, w, 100)]
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
        for q in (0, n // 2, n - 1):
            ref = oracle.similarities_row(exp, q)
            ref[q] = oracle.cosine_cm(exp[q], exp[q])
            assert _same(t.similarities(q, ids), ref), q


STRIDE_ROWS = 12288  # more rows than a resident grid has waves (256 CUs x 8 workgroups x 4 waves, one more workgroup allowed for)
EDGE = 300           # rows checked at either end of the table


def _strided(rng, oracle, a, b, w):
    """Enough owners that a wave of k_build_lists' resident grid takes a
    second row: the mixed owners at both ends of the table (the rows a wave
    prefetches from, and the rows it prefetches), tiny owners between."""
    head = _mixed(rng, oracle, a, b, w, EDGE - 17)
    tail = _mixed(rng, oracle, a, b, w, EDGE - 17)
    assert len(head) == EDGE and len(tail) == EDGE
    mid = [_distinct(rng, int(m), span=1 << 16) for m in rng.integers(0, 12, STRIDE_ROWS - 2 * EDGE)]
    return head + mid + tail


def _check_edges(oracle, t, d, w, a, b, owners, stream=None):
    """Counters, forms and similarities of the first and the last EDGE rows
    against the oracle's table of those rows."""
    n = len(owners)
    sel = list(range(EDGE)) + list(range(n - EDGE, n))
    counts = [owners[r].size for r in sel]
    own, keys = _pairs(owners, sel) if stream is None else stream(sel)
    exp = oracle.build_table(len(sel), d, w, a, b, own, keys)
    got = np.concatenate([t.read_counters(0, EDGE), t.read_counters(n - EDGE, EDGE)])
    assert np.array_equal(got, exp)
    mx = exp.max(axis=(1, 2))
    want = _expected_forms(mx, counts, d, w)
    form, bound = t.owner_forms()
    fs, bs = form[sel], bound[sel]
    pinned = want >= 0
    assert np.array_equal(fs[pinned], want[pinned]), (fs, want)
    lists = pinned & (want == LIST)
    assert np.array_equal(bs[lists], mx[lists].astype(np.uint32))
    ids = np.array(sel)
    for qi in list(range(0, 2 * EDGE, 37)) + [EDGE - 1, EDGE, 2 * EDGE - 1]:
        ref = np.array([oracle.cosine_cm(exp[qi], exp[j]) for j in range(len(sel))])
        assert _same(t.similarities(sel[qi], ids), ref), qi
    return form


@pytest.mark.parametrize("d,w", [(5, 8192), (4, 1024)])
def test_list_rows_beyond_the_resident_grid(oracle, d, w):
    """More owners than the resident grid has waves: a wave walks rows g,
    g + G, ... and loads the next owner's spans and first keys ahead."""
    rng = np.random.Generator(np.random.PCG64(29 + d))
    a, b = oracle.hash_params(42, d)
    owners = _strided(rng, oracle, a, b, w)
    n = len(owners)
    counts = [k.size for k in owners]
    off, keys = _csr(owners)
    assert keys.size < 200_000
    with _handle(n, d, w) as t:
        t.ingest_csr(off, keys)
        t.finalize()
        form = _check_edges(oracle, t, d, w, a, b, owners)
        assert np.all(form[EDGE:n - EDGE] == LIST)  # at most 11 keys each
        _check_stats(t, form, counts, d, w)
        sel = [EDGE, EDGE + 3, n // 2, n - EDGE - 1]  # and a few of the tiny owners between
        exp = oracle.build_table(len(sel), d, w, a, b, *_pairs(owners, sel))
        for i, r in enumerate(sel):
            assert np.array_equal(t.read_counters(r, 1)[0], exp[i]), r


def test_list_rows_tokens(oracle):
    """The same behind the COO partition: a key in [0, 2^31) travels as its
    own u32 token, any other as an index into the batch's keys."""
    d, w = 5, 8192
    rng = np.random.Generator(np.random.PCG64(31))
    a, b = oracle.hash_params(42, d)
    owners = _strided(rng, oracle, a, b, w)
    n = len(owners)
    # tiny owners with wide keys between, up to about 287K pairs: the smallest
    # COO batches that take the row build have 262144
    have = sum(k.size for k in owners)
    for r in range(EDGE, n - EDGE):
        if have >= 286720:
            break
        extra = _wide_keys(rng, 24) if r % 3 == 0 else _distinct(rng, 24, span=1 << 16)
        have += extra.size
        owners[r] = np.concatenate([owners[r], extra])
    rows, keys = _pairs(owners)
    assert 262144 <= keys.size < 300_000
    order = rng.permutation(rows.size)
    rows, keys = rows[order], keys[order]

    def stream(sel):
        remap = np.full(n, -1, np.int64)
        remap[sel] = np.arange(len(sel))
        keep = remap[rows] >= 0
        return remap[rows[keep]], keys[keep]

    with _handle(n, d, w) as t:
        t.ingest(rows, keys)
        t.finalize()
        form = _check_edges(oracle, t, d, w, a, b, owners, stream)
        _check_stats(t, form, [k.size for k in owners], d, w)
        sel = [EDGE, EDGE + 3, n // 2, n - EDGE - 1]
        own, ks = stream(sel)
        exp = oracle.build_table(len(sel), d, w, a, b, own, ks)
        for i, r in enumerate(sel):
            assert np.array_equal(t.read_counters(r, 1)[0], exp[i]), r
