"""GPU: a live sketch table compacted (cms_compact_table: k_fold_scan at the
table's own width, the host's ckpt::compact_form, k_fold_pack, then the
loader's verify pass and restore_layout / k_ckpt_unpack).  Every comparison is
bit for bit against the no-GPU specification checkpoint.compact_checkpoint of
the table's own image before the call, and the counters against what they were.

Tables are installed with load_device(build_checkpoint(...)), every row in a
form and place class wider than its counters need.  The shapes are the
smallest at which each path can go wrong: (48, 4, 128) has every form;
(40, 5, 96) forms but no 1-/2-bit rows; (24, 3, 100) no forms and rows that
are no multiple of 16 bytes; (8, 5, 8192) 160 KB hot rows; (4, 2, 32768) the
widest sketch row; (16, 4, 1024) lists at the limit m = 256 / 257.

The file also passes under CMS_NO_COMPACT=1, CMS_NO_VMM=1 and CMS_NO_FORMS=1:
the specification is given the handle's forms and list limit, and what a
handle cannot hold (a row without storage, a place narrower than a slot) is
not asserted of it.  No test provokes a fault: every image is the writer's own.
(tests/test_gpu_compact.py is about the compact row layout, not this call.)
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib, checkpoint as ck
from mahout_amd.synth import zipf_stream

pytestmark = pytest.mark.gpu

SHAPES = [(48, 4, 128), (40, 5, 96), (24, 3, 100), (8, 5, 8192), (4, 2, 32768), (16, 4, 1024)]
LAYOUT_VARS = ("CMS_NO_COMPACT", "CMS_NO_VMM", "CMS_NO_FORMS")
LIST_KEYS = int(os.environ.get("CMS_LIST_KEYS", "256"))
F = {name: i for i, name in enumerate(ck.ROW_FORMS)}
CAP = {"u1": 1, "u2": 3, "u4": 15, "u8": 255, "u16": 65535, "u32": 2 ** 32 - 1}
SOURCES = ("u32", "u16", "list", "u8", "u4", "u2", "u1", "zero")  # widest first: small tables keep the wide sources
N_KEYS = 20000


def _flag(name):
    return os.environ.get(name, "") not in ("", "0")


def _layout(w):
    """(forms, compact) of a handle created now at width w (cms_create)."""
    forms = w % 32 == 0 and not _flag("CMS_NO_FORMS")
    return forms, forms and not _flag("CMS_NO_COMPACT")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _device(t, data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", t.device))


def _image(t):
    return bytes(t.save_device().cpu().numpy().tobytes())


def _code(fn, *args):
    with pytest.raises(_lib.CmsError) as ei:
        fn(*args)
    return ei.value.code, str(ei.value)


def _spec(image, w):
    forms, _ = _layout(w)
    return ck.compact_checkpoint(image, list_keys=LIST_KEYS, forms=forms)


def _assert_image(got, spec, w):
    """The handle's image after compact() against the specification's."""
    g, s = ck.Checkpoint(got), ck.Checkpoint(spec)
    _, compact = _layout(w)
    assert np.array_equal(g.masses, s.masses) and g.pairs_ingested == s.pairs_ingested
    assert np.array_equal(g.a, s.a) and np.array_equal(g.b, s.b) and g.seed == s.seed
    assert (g.owner_ids is None) == (s.owner_ids is None)
    assert g.owner_ids is None or np.array_equal(g.owner_ids, s.owner_ids)
    assert np.array_equal(g.counters(), s.counters())
    assert np.array_equal(g.bounds, s.bounds), np.flatnonzero(g.bounds != s.bounds)
    if compact:
        assert np.array_equal(g.forms, s.forms), [(r, ck.ROW_FORMS[g.forms[r]], ck.ROW_FORMS[s.forms[r]])
                                                  for r in np.flatnonzero(g.forms != s.forms)[:10]]
        assert np.array_equal(g.classes, s.classes), np.flatnonzero(g.classes != s.classes)
        assert got == spec  # byte for byte: directory, sorted list entries, pad bytes, checksum
        return
    # without the compact layout every narrow row keeps a whole u16 slot, a row of zeros included
    zero = s.forms == F["zero"]
    assert np.array_equal(g.forms[~zero], s.forms[~zero])
    assert np.all(g.forms[zero] == F["u16"])
    narrow = g.forms != F["u32"]
    assert np.all(g.classes[narrow] == 5) and np.all(g.classes[~narrow] == 0)
    for r in np.flatnonzero(s.forms == F["list"]).tolist():
        assert np.array_equal(g.list_entries(r), s.list_entries(r))


# ---- designed tables: one owner per (source form, counters) ----

def _patterns(d, w):
    """(name, counters [d][w]) -- the counters that make each target form."""
    rng = np.random.Generator(np.random.PCG64(1000 * d + w))

    def ragged(v):  # sketch row i holds 2 + i buckets of v: the row sums disagree, so never a list
        c = np.zeros((d, w), np.uint64)
        for i in range(d):
            c[i, rng.permutation(w)[:2 + i]] = v
        return c

    def even(k, v):  # k buckets of v in every sketch row: the sums agree
        c = np.zeros((d, w), np.uint64)
        for i in range(d):
            c[i, rng.permutation(w)[:k]] = v
        return c

    short = even(2, 1)
    for i in range(d):
        short[i, np.flatnonzero(short[i])[0]] = 2  # m = 3 with a repeated bucket
    full = np.zeros((d, w), np.uint64)
    full[np.arange(d), rng.integers(0, w, d)] = 256  # 256 keys of one bucket: the sums agree, yet never a list
    pats = [("stay_u32", ragged(70000)), ("u16", ragged(300)), ("zero", np.zeros((d, w), np.uint64)), ("full256", full),
            ("ones", even(min(w, w // 16 + 8), 1)), ("list", short), ("cap1", ragged(1)),
            # sums that agree, yet the list would be longer than the 2-bit / 4-bit row: a list source of those targets
            ("twos", even(w // 8, 2)), ("fours", even(w // 8, 4)), ("cap255", ragged(255))]
    if w == 1024:  # the list limit: 256 keys are a list, 257 are not
        m257 = even(8, 32)
        m257[:, 0] += 1
        pats += [("m256", even(8, 32)), ("m257", m257)]
    return pats


def _list_entries(c, w):
    """The row as an unsorted list (descending buckets), or None when it is none."""
    d = c.shape[0]
    sums = c.sum(axis=1)
    m = int(sums[0])
    if np.any(sums != m) or m > ck.LIST_MAX_KEYS or d * m > ck.LIST_MAX_ENTRIES or 2 + 2 * d * m > 2 * d * w:
        return None
    return np.stack([np.repeat(np.arange(w), c[i].astype(np.int64))[::-1] for i in range(d)]).reshape(d, m)


def _designed(n, d, w):
    """(counters [n][d][w], per-row source form names, build_checkpoint keywords)."""
    forms_h, _ = _layout(w)
    combos = []
    for pi, (name, c) in enumerate(_patterns(d, w)):
        cmax = int(c.max())
        for si, src in enumerate(SOURCES):
            if src == "zero":
                ok = cmax == 0
            elif src == "list":
                ok = forms_h and ck.shape_has_form("list", d, w) and _list_entries(c, w) is not None
            else:
                ok = ck.shape_has_form(src, d, w) and (forms_h or src in ("u16", "u32")) and cmax <= CAP[src]
            if ok:
                combos.append((si, pi, src, c))
    combos.sort(key=lambda x: (x[0], x[1]))
    combos = combos[:n]
    counters = np.zeros((n, d, w), np.uint64)
    forms, classes, lists = ["zero"] * n, [0] * n, {}
    for r, (_, _, src, c) in enumerate(combos):
        counters[r] = c
        forms[r] = src
        if src == "list":
            lists[r] = _list_entries(c, w)
        elif src in ("u1", "u2", "u4", "u8", "u16"):
            classes[r] = 5 if r % 2 else 1 + ("u1", "u2", "u4", "u8", "u16").index(src)  # odd owners: a whole slot
    return counters, forms, dict(forms=forms, classes=classes, lists=lists)


_HASH = {}


def _load_designed(oracle, n, d, w):
    _HASH[d] = oracle.hash_params(42, d)
    counters, sources, kw = _designed(n, d, w)
    data = ck.build_checkpoint(counters, *_HASH[d], seed=42, **kw)
    t = SketchTable(n, depth=d, width=w, seed=42)
    t.load_device(_device(t, data))
    return t, counters, sources


def _stats_match(t, image):
    fc, st = ck.Checkpoint(image).form_counts(), t.stats()
    got = {k: st[k] for k in ("hot_rows", "list_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows")}
    want = {"hot_rows": fc.get("u32", 0), "list_rows": fc.get("list", 0), "u8_rows": fc.get("u8", 0),
            "nibble_rows": fc.get("u4", 0), "crumb_rows": fc.get("u2", 0), "bit_rows": fc.get("u1", 0)}
    assert got == want


# ---- 1: every source form into every target form ----

@pytest.mark.parametrize("n,d,w", SHAPES)
def test_every_source_form_into_every_target_form(oracle, n, d, w):
    forms_h, compact = _layout(w)
    default = not any(_flag(v) for v in LAYOUT_VARS) and LIST_KEYS == 256
    t, counters, sources = _load_designed(oracle, n, d, w)
    with t:
        before = _image(t)
        spec = _spec(before, w)
        b, s = ck.Checkpoint(before), ck.Checkpoint(spec)
        held = [ck.ROW_FORMS[f] for f in b.forms]  # (a handle without forms holds narrow images as u16)
        pairs = sorted(set(zip(held, (ck.ROW_FORMS[f] for f in s.forms))))
        print("(source, target) pairs", pairs)
        if default and (n, d, w) == SHAPES[0]:  # every form on both sides, and every narrowing of a dense row
            assert {p[0] for p in pairs} == {p[1] for p in pairs} == set(ck.ROW_FORMS) - {"f64"}, pairs
            dense = ("u1", "u2", "u4", "u8", "u16", "u32")
            for i, tgt in enumerate(dense):
                for src in dense[i:]:
                    assert (src, tgt) in pairs, (src, tgt)
                assert ("list", tgt) in pairs or tgt in ("u8", "u16", "u32"), tgt  # (a list that long does not fit a row)
            for src in dense + ("list", "zero"):
                assert (src, "zero") in pairs, src
            for src in ("u32", "u16", "u8", "u4", "u2", "list"):
                assert (src, "list") in pairs, src
        if default and (n, d, w) == SHAPES[5]:  # the list limit: m = 256 is a list, m = 257 is not
            m, cmax = b.masses, counters.max(axis=(1, 2))  # (8 buckets of 32 per sketch row, and one key more)
            assert np.all(s.forms[(m == 256) & (cmax == 32)] == F["list"]) and np.any((m == 256) & (cmax == 32))
            assert np.all(s.forms[m == 257] == F["u8"]) and np.any(m == 257)
        full = (b.masses == 256) & (counters.max(axis=(1, 2)) == 256)  # a bucket of 256 is no list, however short
        assert np.any(full) and np.all(s.forms[full] == F["u16"])
        if default and (n, d, w) in (SHAPES[3], SHAPES[5]):
            assert 2 + 2 * d * 256 < 2 * d * w  # (here the list would be the shorter)
        if default and (n, d, w) in (SHAPES[3], SHAPES[4]):
            assert ("u32", "u32") in pairs and ("u32", "u16") in pairs and ("u32", "zero") in pairs
        stored0 = t.stats()["stored_bytes"]
        tab0 = t.read_counters()
        assert np.array_equal(tab0, counters)
        # the fold at the table's own width is the compaction as an image (whatever layout the handle holds)
        assert bytes(t.fold_device(w).cpu().numpy().tobytes()) == spec
        changed = t.compact()
        after = _image(t)
        _assert_image(after, spec, w)
        assert np.array_equal(t.read_counters(), tab0)
        a = ck.Checkpoint(after)
        assert changed == int(((a.forms != b.forms) | (a.classes != b.classes)).sum())
        assert changed > 0
        _stats_match(t, after)
        assert t.stats()["stored_bytes"] < stored0
        assert t.stats()["pairs_ingested"] == b.pairs_ingested
        assert t.compact() == 0
        assert _image(t) == after
        assert np.array_equal(t.read_counters(), tab0)


# ---- 2: the motivating case: merge a second table, subtract it again, compact ----

def _phases(n, d, w, live=False):
    """Table A's batches (tests/test_gpu_merge_table.py's phases, restated);
    live: the same phases with the owner index reversed and other keys."""
    built = n // 2
    items, users = zipf_stream(N_KEYS, built, 300_000, seed=d + w + (1000 if live else 0))
    fresh = np.arange(built, n - 16)  # the last 16 owners have no keys
    wts = np.array([1, 2, 10, 200, 1000], np.float32)[np.arange(fresh.size) % 5]
    wts[-1] = 70000  # one hot owner by first touch
    k1, k2 = ((17, 3), (29, 11)) if live else ((31, 5), (13, 1))
    kf = (fresh * k1[0] + k1[1]) % N_KEYS
    lift = fresh[(np.arange(fresh.size) % 5 == 2) & (np.arange(fresh.size) % 10 < 5)]
    more = fresh[(np.arange(fresh.size) % 5 == 0) & (np.arange(fresh.size) % 10 < 5)]
    a = [(items, users, None), (fresh, kf, wts),
         (np.concatenate([lift, more]), np.concatenate([(lift * k1[0] + k1[1]) % N_KEYS, (more * k2[0] + k2[1]) % N_KEYS]),
          np.concatenate([np.full(lift.size, 300), np.ones(more.size)]).astype(np.float32))]
    if live:
        a = [(n - 1 - r, k, v) for r, k, v in a]
    return a


def _table(n, d, w, phases):
    t = SketchTable(n, depth=d, width=w, seed=42)
    for r, k, v in phases:
        t.ingest(r, k, v)
        t.finalize()
    return t


def test_compact_after_a_merge_and_its_subtraction(oracle):
    n, d, w = 4096, 4, 1024
    forms_h, compact = _layout(w)
    pa, pb = _phases(n, d, w), _phases(n, d, w, live=True)
    ha, hb = oracle.hash_params(42, d)
    vals = [np.ones(x[0].size, np.float32) if x[2] is None else x[2] for x in pa]
    exp = oracle.build_table(n, d, w, ha, hb, np.concatenate([x[0] for x in pa]), np.concatenate([x[1] for x in pa]),
                             np.concatenate(vals))
    with _table(n, d, w, pb) as tb:
        image_b = tb.save_device().clone()
    with _table(n, d, w, pa) as t:
        fresh = t.stats()
        t.merge_device(image_b.to("cuda:%d" % t.device))
        t.subtract_device(image_b.to("cuda:%d" % t.device))
        wide = t.stats()
        before = _image(t)
        changed = t.compact()
        st = t.stats()
        print("stored_bytes fresh %d, after merge and subtract %d, compacted %d; table_bytes %d / %d / %d; rows changed %d"
              % (fresh["stored_bytes"], wide["stored_bytes"], st["stored_bytes"], fresh["table_bytes"], wide["table_bytes"],
                 st["table_bytes"], changed))
        got = t.read_counters()
        bad = np.flatnonzero((got != exp).any(axis=(1, 2)))
        assert bad.size == 0, ("owners whose counters differ from the oracle's table A", bad[:20], bad.size)
        _assert_image(_image(t), _spec(before, w), w)
        assert st["stored_bytes"] < wide["stored_bytes"]
        assert st["pairs_ingested"] == wide["pairs_ingested"] == fresh["pairs_ingested"]
        if forms_h and LIST_KEYS > 0:
            assert fresh["list_rows"] > 0 and st["list_rows"] > 0
            assert changed > 0
        if compact:
            assert st["table_bytes"] < wide["table_bytes"]
        # the compacted table is table A still: its norms are re-derived to the same queries
        t.finalize()
        sims = oracle.similarities_row(exp, 3)
        sims[3] = oracle.cosine_cm(exp[3], exp[3])
        assert _same(t.similarities(3, np.arange(n)), sims)


# ---- 3: queries do not move ----

def _answers(t, n):
    rows = np.arange(n)
    keys = np.array([1, 5, 17, 4242, 19999], np.int64)
    prof = [(np.array([3, 5, 17, 900]), None), (np.array([1, 2]), np.array([2.0, 1.0], np.float32))]
    out = [np.stack([t.similarities(q, rows) for q in range(n)])]
    out += list(t.top_k_all(5))
    out.append(np.array([[t.point_query(r, int(k)) for k in keys] for r in range(n)]))
    out.append(np.stack([t.estimate_preferences(u, rows[(rows != u)][:6], keys) for u in (0, 1, n // 2, n - 1)]))
    out += list(t.anonymous_most_similar(prof, 5))
    return out


@pytest.mark.parametrize("n,d,w", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_queries_do_not_move(oracle, n, d, w):
    t, counters, _ = _load_designed(oracle, n, d, w)
    with t:
        code, _ = _code(t.similarities, 0, np.arange(n))
        assert code == _lib.CMS_E_STATE  # loaded, not finalized ...
        assert t.compact() > 0
        code, _ = _code(t.similarities, 0, np.arange(n))
        assert code == _lib.CMS_E_STATE  # ... and it stays so
    t, counters, _ = _load_designed(oracle, n, d, w)
    with t:
        t.finalize()
        want = _answers(t, n)
        assert t.compact() > 0
        got = _answers(t, n)  # no finalize() in between
        for i, (x, y) in enumerate(zip(got, want)):
            assert _same(x, y), i
        t.finalize()  # ... and a new one changes nothing either
        for i, (x, y) in enumerate(zip(_answers(t, n), want)):
            assert _same(x, y), i


# ---- 4: writers continue on the compacted table ----

def _reproducible(t, n, d, w):
    s1 = t.save_device()
    with SketchTable(n, depth=d, width=w, seed=42) as back:
        back.load_device(s1)
        assert _image(back) == bytes(s1.cpu().numpy().tobytes())


@pytest.mark.parametrize("n,d,w", SHAPES)
def test_writers_continue_on_the_compacted_table(oracle, n, d, w):
    t, counters, sources = _load_designed(oracle, n, d, w)
    ha, hb = _HASH[d]
    with t:
        t.compact()
        held = ck.Checkpoint(_image(t))
        _, compact = _layout(w)
        # an owner whose 256 keys share a bucket was kept dense: the batch below adds to it like to any row
        full = (held.masses == 256) & (counters.max(axis=(1, 2)) == 256)
        assert np.any(full) and np.all(held.forms[full] == F["u16"])
        if compact:  # the batch below reaches an owner without storage and a list row
            assert np.any(held.forms == F["zero"]) and (np.any(held.forms == F["list"]) or not ck.shape_has_form("list", d, w))
        exp = counters.astype(np.float64)
        rows = np.arange(n)
        keys = (rows * 31 + 5) % N_KEYS
        inc = np.array([1, 2, 14, 250, 70000], np.float32)[(rows + rows // 5) % 5]  # each owner crosses some capacity
        t.ingest(rows, keys, inc)
        exp = exp + oracle.build_table(n, d, w, ha, hb, rows, keys, inc)
        assert np.array_equal(t.read_counters(), exp)
        _reproducible(t, n, d, w)
        part = rows[::2]
        t.retract(part, keys[part], inc[part])
        exp = exp - oracle.build_table(n, d, w, ha, hb, part, keys[part], inc[part])
        assert np.array_equal(t.read_counters(), exp)
        _reproducible(t, n, d, w)
        r2 = rows[::3]
        k2 = (r2 * 7 + 1) % N_KEYS
        small = oracle.build_table(n, d, w, ha, hb, np.repeat(r2, 2), np.concatenate([k2, k2 + 1]), np.ones(2 * r2.size, np.float32))
        image = _device(t, ck.build_checkpoint(small.astype(np.uint64), ha, hb, seed=42))
        t.merge_device(image)
        assert np.array_equal(t.read_counters(), exp + small)
        _reproducible(t, n, d, w)
        t.subtract_device(image)
        assert np.array_equal(t.read_counters(), exp)
        _reproducible(t, n, d, w)
        before = _image(t)
        t.compact()  # and once more, on what the writers left
        _assert_image(_image(t), _spec(before, w), w)
        assert np.array_equal(t.read_counters(), exp)
        _reproducible(t, n, d, w)


# ---- 5: the refresh stays incremental ----

def test_refresh_stays_incremental_after_a_compaction():
    n, d, w, k = 300, 4, 128, 10  # (kept lists need w % 128 == 0)
    items, users = zipf_stream(4000, n, 20_000, seed=77)
    rng = np.random.Generator(np.random.PCG64(5))
    touched = rng.choice(n, size=n // 20, replace=False)
    drow, dkey = touched[rng.integers(0, touched.size, 400)], rng.integers(0, 4000, 400)
    with SketchTable(n, depth=d, width=w, seed=42) as delta, SketchTable(n, depth=d, width=w, seed=42) as t:
        delta.ingest(rng.integers(0, n, 3000), rng.integers(0, 4000, 3000))
        delta.finalize()
        image = delta.save_device()
        t.ingest(items, users)
        t.finalize()
        t.merge_device(image)
        t.subtract_device(image)  # rows widened for nothing: the compaction has work to do
        t.finalize()
        t.top_k_refresh(k)  # the whole job: the kept lists
        assert t.refresh_stats()[2] == 1
        t.compact()
        t.ingest(drow, dkey)
        t.finalize()
        got = t.top_k_refresh(k)
        n_touched, _, full = t.refresh_stats()
        assert full == 1, "the compaction dropped the kept lists: the refresh was a whole job"
        assert n_touched == np.unique(drow).size < n
        for x, y in zip(got, t.top_k_all(k)):
            assert _same(x, y)


# ---- 6: refusals and no-ops ----

def test_an_fp64_handle_refuses_the_compaction():
    with SketchTable(200, depth=3, width=101, seed=42, counters="f64") as t:
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]), np.array([1, 2, 1, 1], np.float32))
        t.finalize()
        before = _image(t)
        code, msg = _code(t.compact)
        assert code == _lib.CMS_E_STATE and "fp64" in msg, msg
        assert _image(t) == before
        t.similarities(0, np.arange(3))  # still finalized


def test_a_per_owner_handle_refuses_the_compaction():
    with SketchTable.per_owner_shapes(40) as t:
        code, msg = _code(t.compact)
        assert code == _lib.CMS_E_STATE and "per-owner" in msg, msg


def test_a_handle_with_a_communicator_refuses_the_compaction():
    from mahout_amd import transport
    n, d, w = 64, 4, 128
    with SketchTable(n, depth=d, width=w, seed=42, collective_single_rank=True) as t:
        def allgather(send, recv, nbytes):
            host = np.empty(nbytes, np.uint8)
            transport._d2h(host, send, nbytes)
            transport._h2d(recv, host, nbytes)
        t.comm_init_transport(0, 1, lambda ptr, count: None, allgather)
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]))
        t.finalize()
        before, tab = _image(t), t.read_counters()
        code, msg = _code(t.compact)
        assert code == _lib.CMS_E_STATE and "communicator" in msg, msg
        assert _image(t) == before and np.array_equal(t.read_counters(), tab)


def test_an_empty_handle_compacts_to_nothing():
    with SketchTable(64, depth=4, width=128, seed=42) as t:
        assert t.compact() == 0
        assert t.stats()["pairs_ingested"] == 0 and not t.read_counters().any()
        t.ingest(np.array([0, 1]), np.array([5, 6]))
        t.reset()
        assert t.compact() == 0
        t.ingest(np.array([3]), np.array([5]))  # the handle is as it was: empty, and builds
        t.finalize()
        assert t.read_counters().sum() == 4


def test_a_pending_ingest_error_is_reported_first(oracle):
    import torch
    n, d, w = SHAPES[0]
    t, counters, _ = _load_designed(oracle, n, d, w)
    with t:
        before = ck.Checkpoint(_image(t))
        rows = torch.tensor([n], dtype=torch.int64, device="cuda:%d" % t.device)  # outside [0, n)
        keys = torch.tensor([7], dtype=torch.int64, device="cuda:%d" % t.device)
        t.ingest_device_rows(rows, keys, None, 1)
        code, msg = _code(t.compact)
        assert code == _lib.CMS_E_PARAM and "owner row" in msg, msg
        after = ck.Checkpoint(_image(t))  # nothing was re-stored
        for f in ("forms", "classes", "bounds", "masses", "lengths", "offsets"):
            assert np.array_equal(getattr(after, f), getattr(before, f)), f
        assert bytes(after.payload) == bytes(before.payload)
        assert np.array_equal(t.read_counters(), counters)
        assert t.compact() > 0  # the error was reported once; the call now goes through
        assert np.array_equal(t.read_counters(), counters)
