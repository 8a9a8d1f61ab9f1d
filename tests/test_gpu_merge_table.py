"""GPU: a saved sketch table merged into a live one (cms_merge_table /
cms_merge_table_device: k_ckpt_unpack's verify pass, then k_ckpt_apply<kAdd>
and k_ckpt_apply_lists<kAdd> after the in-place writers' promote / widen step).  Every
comparison covers the WHOLE table and is bit for bit against the oracle's
rebuild of both streams (`T/impl/common/DoubleCountMinSketch.java:72-80`) and
against the numpy specification checkpoint.sum_counters.

Table A of each shape is tests/test_gpu_checkpoint.py's: every form the shape
allows, movers and holes.  The live tables run the same phases with the owner
index reversed (r -> n - 1 - r) and other keys, so A's forms meet other live
forms: B all phases (a row build: lists, every narrow form, hot rows), Z the
first-touch and mover phases into an empty handle, which leave every untouched
owner on the shared zero row -- a row build gives every owner a place, so only
Z has such owners.  The shapes are the smallest at which each path can go
wrong: (4096, 4, 1024) reaches lists, 1-/2-bit rows and movers; (2000, 5, 96)
has forms but no 1-/2-bit rows; (300, 3, 100) has no forms and rows that are
no multiple of 16 bytes; (512, 5, 8192) has 160 KB hot rows and 4 KB list
slots.

The file also passes when the suite runs under CMS_NO_COMPACT=1, CMS_NO_VMM=1
or CMS_NO_FORMS=1: what a handle cannot hold is not asserted of it.  No test
provokes a fault: a corrupt image is refused by the checks before any kernel
indexes by its contents, and is tried once.
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib, checkpoint as ck
from mahout_amd.synth import zipf_stream

pytestmark = pytest.mark.gpu

FORMS = SketchTable.FORMS  # ("u32", "u16", "u8", "u4", "u2", "u1", "list")
CAPACITY = {"u32": 2 ** 32 - 1, "u16": 65535, "u8": 255, "u4": 15, "u2": 3, "u1": 1, "list": 0}
N_KEYS = 20000
SHAPES = [(4096, 4, 1024), (2000, 5, 96), (300, 3, 100), (512, 5, 8192)]
LAYOUT_VARS = ("CMS_NO_COMPACT", "CMS_NO_VMM", "CMS_NO_FORMS")
STAT_KEYS = ("pairs_ingested", "hot_rows", "list_rows", "u8_rows", "nibble_rows", "crumb_rows", "bit_rows",
             "stored_bytes", "table_bytes")


def _flag(name):
    return os.environ.get(name, "") not in ("", "0")


def _layout(w):
    """(forms, compact) of a handle created now at width w (cms_create)."""
    forms = w % 32 == 0 and not _flag("CMS_NO_FORMS")
    return forms, forms and not _flag("CMS_NO_COMPACT")


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _phases(n, d, w, live=False):
    """Table A's batches and the further batch of the streaming test
    (tests/test_gpu_checkpoint.py); live: the same phases with the owner index
    reversed and other keys."""
    built = n // 2
    items, users = zipf_stream(N_KEYS, built, 300_000, seed=d + w + (1000 if live else 0))
    fresh = np.arange(built, n - 16)  # the last 16 owners have no keys
    wts = np.array([1, 2, 10, 200, 1000], np.float32)[np.arange(fresh.size) % 5]
    wts[-1] = 70000  # one hot owner by first touch
    k1, k2, k3 = ((17, 3), (29, 11), (11, 2)) if live else ((31, 5), (13, 1), (7, 1))
    kf = (fresh * k1[0] + k1[1]) % N_KEYS
    lift = fresh[(np.arange(fresh.size) % 5 == 2) & (np.arange(fresh.size) % 10 < 5)]
    more = fresh[(np.arange(fresh.size) % 5 == 0) & (np.arange(fresh.size) % 10 < 5)]
    a = [(items, users, None), (fresh, kf, wts),
         (np.concatenate([lift, more]), np.concatenate([(lift * k1[0] + k1[1]) % N_KEYS, (more * k2[0] + k2[1]) % N_KEYS]),
          np.concatenate([np.full(lift.size, 300), np.ones(more.size)]).astype(np.float32))]
    rows = np.arange(0, n - 8, 3)
    more_w = np.array([1, 3, 14, 250, 900], np.float32)[np.arange(rows.size) % 5]
    extra = (rows, (rows * k3[0] + k3[1]) % N_KEYS, more_w)
    if live:
        # Reversed, A's built owner r meets a first-touch owner and A's first-touch owners meet built ones.  A's
        # list rows (the Zipf tail, just below n / 2) would so never meet a list, an untouched owner or a hot
        # row: the window W of 64 owners below n / 2 takes no first touch; its first 24 owners get 5 keys each in
        # the row build (list rows), the next one a first touch of 70000 (hot), the rest nothing (a place of no
        # keys after the build, the zero row in a table without one).
        win = np.arange(n // 2 - 64, n // 2)
        a = [(n - 1 - r, k, v) for r, k, v in a]
        for i in (1, 2):
            keep = ~np.isin(a[i][0], win)
            a[i] = (a[i][0][keep], a[i][1][keep], a[i][2][keep])
        lrow = np.repeat(win[:24], 5)
        a[0] = (np.concatenate([a[0][0], lrow]), np.concatenate([a[0][1], (lrow * 5 + np.arange(lrow.size)) % N_KEYS]), None)
        a[1] = (np.append(a[1][0], win[24]), np.append(a[1][1], 4242), np.append(a[1][2], np.float32(70000)))
    return a, extra


_REF = {}


def _oracle_table(oracle, n, d, w, batches):
    ha, hb = oracle.hash_params(42, d)
    vals = [np.ones(x[0].size, np.float32) if x[2] is None else x[2] for x in batches]
    t = oracle.build_table(n, d, w, ha, hb, np.concatenate([x[0] for x in batches]),
                           np.concatenate([x[1] for x in batches]), np.concatenate(vals))
    t.setflags(write=False)
    return t


def _reference(oracle, n, d, w):
    """Phases and oracle tables of one shape, computed once: A, the live B
    (all reversed phases) and Z (without the row build), and the further batch."""
    if (n, d, w) not in _REF:
        pa, extra = _phases(n, d, w)
        pb, _ = _phases(n, d, w, live=True)
        _REF[(n, d, w)] = dict(pa=pa, pb=pb, extra=extra, A=_oracle_table(oracle, n, d, w, pa),
                               B=_oracle_table(oracle, n, d, w, pb), Z=_oracle_table(oracle, n, d, w, pb[1:]),
                               X=_oracle_table(oracle, n, d, w, [extra]))
    return _REF[(n, d, w)]


def _table(n, d, w, phases):
    t = SketchTable(n, depth=d, width=w, seed=42)
    for r, k, v in phases:
        t.ingest(r, k, v)
        t.finalize()
    return t


def _check_counters(t, exp):
    got = t.read_counters()
    bad = np.flatnonzero((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, ("owners whose counters differ from the oracle", bad[:20], bad.size)


def _queries(n):
    return (0, 1, n // 2 + 1, n - 1)


def _default_env():
    """Context: the layout variables off (the default, compact layout)."""
    class Ctx:
        def __enter__(self):
            self.old = {v: os.environ.get(v) for v in LAYOUT_VARS}
            for v in LAYOUT_VARS:
                os.environ[v] = "0"

        def __exit__(self, *a):
            for v, x in self.old.items():
                if x is None:
                    del os.environ[v]
                else:
                    os.environ[v] = x
    return Ctx()


def _live_states(t, tmp_path, name):
    """Per owner, the live row's state before a merge: its owner_forms() form,
    or "zero" for an owner on the shared zero row (the handle's own directory
    tells them apart)."""
    path = str(tmp_path / name)
    t.save(path)
    c = ck.read_checkpoint(path)
    form, _ = t.owner_forms()
    state = np.array([FORMS[f] for f in form], dtype=object)
    state[c.forms == ck.ROW_FORMS.index("zero")] = "zero"
    return state


# ---- 1: every form into every form ----

REQUIRED_PAIRS = [("list", "list"), ("list", "zero"), ("list", "u32"), ("u32", "narrow"), ("narrow", "u32"),
                  ("u16", "u8-"), ("u1", "u16")]
NARROW = ("u16", "u8", "u4", "u2", "u1", "list")


def _has_pair(pairs, want):
    src, dst = want
    srcs = NARROW if src == "narrow" else (src,)
    dsts = NARROW if dst == "narrow" else ("u8", "u4", "u2", "u1") if dst == "u8-" else (dst,)
    return any((s, t) in pairs for s in srcs for t in dsts)


@pytest.mark.parametrize("n,d,w", SHAPES)
def test_every_form_into_every_form(oracle, tmp_path, n, d, w):
    ref = _reference(oracle, n, d, w)
    forms, compact = _layout(w)
    default = not any(_flag(v) for v in LAYOUT_VARS)
    path = str(tmp_path / "a.ckpt")
    with _table(n, d, w, ref["pa"]) as a:
        a.save(path)
    img = ck.read_checkpoint(path)
    img_form = np.array([ck.ROW_FORMS[f] for f in img.forms], dtype=object)
    adds = (img.lengths > 0) & (img.masses > 0)  # the image rows that add anything
    pairs = set()
    for name, phases in (("B", ref["pb"]), ("Z", ref["pb"][1:])):
        with _table(n, d, w, phases) as t:
            state = _live_states(t, tmp_path, name + ".ckpt")
            pairs |= set(zip(img_form[adds].tolist(), state[adds].tolist()))
            t.merge(path)
            both = ref["A"] + ref[name]
            _check_counters(t, both)
            if name == "B":  # the oracle over both tables' batches concatenated, and the numpy specification
                assert np.array_equal(both, _oracle_table(oracle, n, d, w, ref["pa"] + ref["pb"]))
                assert np.array_equal(ck.sum_counters([path, str(tmp_path / "B.ckpt")]), both)
            form, _ = t.owner_forms()
            assert not np.any((np.array(FORMS, dtype=object)[form] == "list") & adds), "a merged row stayed a list"
            assert t.stats()["pairs_ingested"] == sum(x[0].size for x in ref["pa"] + list(phases))
            if name != "B":
                continue
            # finalize: the norms, similarities and lists of one handle that ingested every batch itself
            t.finalize()
            sims = [t.similarities(q, np.arange(n)) for q in _queries(n)]
            top = t.top_k_all(10)
            with _table(n, d, w, ref["pa"] + ref["pb"]) as one:
                _check_counters(one, both)
                for q, s in zip(_queries(n), sims):
                    so = one.similarities(q, np.arange(n))
                    assert _same(s, so) and np.array_equal(np.isnan(s), np.isnan(so)), q
                for x, y in zip(top, one.top_k_all(10)):
                    assert _same(np.asarray(x, np.float64), np.asarray(y, np.float64))
    # which (image form, live state) pairs the shape covered
    have_img = {f for f in img_form[adds].tolist()}
    print("covered pairs", sorted(pairs))
    if default and forms:
        for f in have_img:  # every image form the shape has meets at least three distinct live states
            met = {t for s, t in pairs if s == f}
            assert len(met) >= 3, (f, met)
        if (n, d, w) == SHAPES[0]:
            assert have_img == set(ck.ROW_FORMS) - {"zero", "f64"}, have_img
            for want in REQUIRED_PAIRS:
                assert _has_pair(pairs, want), (want, sorted(pairs))
    elif not forms:  # whole u16 slots and hot rows are all such a handle holds
        assert {t for _, t in pairs} <= {"u16", "u32"}, pairs
        assert ("u16", "u32") in pairs and ("u16", "u16") in pairs and any(s == "u32" for s, _ in pairs), pairs


# ---- 2: capacity edges, exactly at each step ----

EDGE_SUMS = (1, 2, 3, 4, 15, 16, 255, 256, 65535, 65536)


@pytest.mark.parametrize("w", [128, 96])
def test_capacity_edges(oracle, w):
    """Owners with one key each: the live count a and the image count b give
    a + b at and one past every form's capacity, in both splits."""
    d = 4
    cases = []
    for s in EDGE_SUMS:
        cases += [(1, s - 1), (s - 1, 1)] if s > 1 else [(0, 1), (1, 0)]
    n = len(cases) + 4  # (the last owners stay empty)
    rows = np.arange(len(cases))
    keys = (rows * 37 + 11) % N_KEYS
    la = np.array([c[0] for c in cases], np.float32)
    ib = np.array([c[1] for c in cases], np.float32)
    ha, hb = oracle.hash_params(42, d)
    exp = oracle.build_table(n, d, w, ha, hb, np.concatenate([rows, rows]), np.concatenate([keys, keys]),
                             np.concatenate([la, ib]))
    with SketchTable(n, depth=d, width=w, seed=42) as src, SketchTable(n, depth=d, width=w, seed=42) as t:
        src.ingest(rows[ib > 0], keys[ib > 0], ib[ib > 0])
        src.finalize()
        image = src.save_device()
        t.ingest(rows[la > 0], keys[la > 0], la[la > 0])
        t.finalize()
        t.merge_device(image)
        _check_counters(t, exp)
        form, _ = t.owner_forms()
        for i, (a, b) in enumerate(cases):
            f = FORMS[form[i]]
            assert CAPACITY[f] >= a + b, (a, b, f)
            if a + b == 65536:
                assert f == "u32", (a, b, f)
        t.finalize()
        _check_counters(t, exp)
        assert abs(t.similarity(0, 0) - 1.0) < 1e-12


def test_a_u16_image_row_is_bounded_by_its_mass_not_its_saved_bound(oracle):
    """A u16 row in a whole slot takes in-place adds without a cbound update,
    so the image's cbound (300 here) can be far below its counters (40300):
    the live row (30000 on the same key) must still move to a u32 slot."""
    n, d, w = 8, 4, 128
    ha, hb = oracle.hash_params(42, d)
    with SketchTable(n, depth=d, width=w, seed=42) as src, SketchTable(n, depth=d, width=w, seed=42) as t:
        src.ingest(np.array([2]), np.array([77]), np.array([300], np.float32))
        src.finalize()
        src.ingest(np.array([2]), np.array([77]), np.array([40000], np.float32))
        src.finalize()
        image = src.save_device()
        t.ingest(np.array([2, 3]), np.array([77, 78]), np.array([30000, 5], np.float32))
        t.finalize()
        t.merge_device(image)
        exp = oracle.build_table(n, d, w, ha, hb, np.array([2, 2, 2, 3]), np.array([77, 77, 77, 78]),
                                 np.array([300, 40000, 30000, 5], np.float32))
        _check_counters(t, exp)
        assert FORMS[t.owner_forms()[0][2]] == "u32"


# ---- 3: algebra ----

def test_merge_algebra(oracle, tmp_path):
    import torch
    n, d, w = SHAPES[0]
    ref = _reference(oracle, n, d, w)
    pa_, pb_ = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    pairs_a = sum(x[0].size for x in ref["pa"])
    with _table(n, d, w, ref["pa"]) as a, _table(n, d, w, ref["pb"]) as b:
        a.save(pa_)
        b.save(pb_)
        image_a = a.save_device()
        a.merge(pb_)  # A.merge(B) and B.merge(A) give equal counters
        b.merge(pa_)
        ca = a.read_counters()
        assert np.array_equal(ca, b.read_counters())
        assert np.array_equal(ca, ref["A"] + ref["B"])
        forms_b = b.owner_forms()
    # the file path and merge_device(save_device()) give equal tables
    with _table(n, d, w, ref["pb"]) as b2:
        b2.merge_device(image_a)
        assert np.array_equal(b2.read_counters(), ca)
        form2, bound2 = b2.owner_forms()
        assert np.array_equal(form2, forms_b[0])
        if _layout(w)[0]:  # (cbound is maintained for form rows only: a handle without forms never reads it)
            assert np.array_equal(bound2, forms_b[1])
    # into an empty handle: the image's counters and pairs; the same image twice
    with SketchTable(n, depth=d, width=w, seed=42) as e:
        e.merge(pa_)
        _check_counters(e, ref["A"])
        assert e.stats()["pairs_ingested"] == pairs_a == ck.read_checkpoint(pa_).pairs_ingested
        e.merge_device(image_a)
        _check_counters(e, 2 * ref["A"])  # (the oracle with A's batches twice: the table is linear in its stream)
        assert e.stats()["pairs_ingested"] == 2 * pairs_a
        e.finalize()
        exp = 2 * ref["A"]
        sims = oracle.similarities_row(exp, 1)
        sims[1] = oracle.cosine_cm(exp[1], exp[1])
        assert _same(e.similarities(1, np.arange(n)), sims)
    assert isinstance(image_a, torch.Tensor)


# ---- 4: streaming continues ----

@pytest.mark.parametrize("n,d,w", SHAPES)
def test_streaming_continues_after_a_merge(oracle, tmp_path, n, d, w):
    ref = _reference(oracle, n, d, w)
    path = str(tmp_path / "a.ckpt")
    with _table(n, d, w, ref["pa"]) as a:
        a.save(path)
    with _table(n, d, w, ref["pb"]) as b:
        b.merge(path)
        b.ingest(*ref["extra"])  # cbound, masses and places are consistent for the next writer
        b.finalize()
        exp = ref["A"] + ref["B"] + ref["X"]
        _check_counters(b, exp)
        form, _ = b.owner_forms()
        top = exp.max(axis=(1, 2))
        cap = np.array([CAPACITY[FORMS[f]] for f in form], np.float64)
        lists = np.array(FORMS, dtype=object)[form] == "list"
        assert np.all((cap >= top) | lists)
        sims = oracle.similarities_row(exp, 3)
        sims[3] = oracle.cosine_cm(exp[3], exp[3])
        assert _same(b.similarities(3, np.arange(n)), sims)


# ---- 5: the incremental refresh survives a delta merge ----

def test_refresh_stays_incremental_after_a_delta_merge():
    n, d, w, k = 2000, 4, 256, 10
    items, users = zipf_stream(4000, n, 120_000, seed=77)
    rng = np.random.Generator(np.random.PCG64(5))
    touched = rng.choice(n, size=n // 20, replace=False)  # about 5 % of the owners
    drow = touched[rng.integers(0, touched.size, 3000)]
    dkey = rng.integers(0, 4000, 3000)
    with SketchTable(n, depth=d, width=w, seed=42) as delta, SketchTable(n, depth=d, width=w, seed=42) as b, \
            SketchTable(n, depth=d, width=w, seed=42) as one:
        delta.ingest(drow, dkey)
        delta.finalize()
        image = delta.save_device()
        b.ingest(items, users)
        b.finalize()
        first = b.top_k_refresh(k)  # the whole job: the kept lists
        assert b.refresh_stats()[2] == 1
        assert all(_same(np.asarray(x, np.float64), np.asarray(y, np.float64)) for x, y in zip(first, b.top_k_all(k)))
        b.merge_device(image)
        b.finalize()
        got = b.top_k_refresh(k)
        n_touched, _, full = b.refresh_stats()
        assert full == 1, "the merge dropped the kept lists: the refresh was a whole job"
        assert n_touched == np.unique(drow).size < n
        one.ingest(np.concatenate([items, drow]), np.concatenate([users, dkey]))
        one.finalize()
        for x, y in zip(got, one.top_k_all(k)):
            assert _same(np.asarray(x, np.float64), np.asarray(y, np.float64))


# ---- 6: fp64 counters ----

def test_fp64_merge(oracle, tmp_path):
    n, d, w = 200, 3, 101  # (d w odd: fp64 rows that are no multiple of 16 bytes)
    rng = np.random.Generator(np.random.PCG64(6))
    ha, hb = oracle.hash_params(42, d)
    path = str(tmp_path / "f.ckpt")
    tables, exps = [], []
    try:
        for i in range(2):
            rows = np.sort(rng.integers(0, n - 3 - i, 6000))  # (the last owners keep all-zero sketches)
            keys = rng.integers(0, 5000, 6000)
            vals = (rng.normal(0, 2, 6000) + 0.1).astype(np.float32)  # negative and non-dyadic preferences
            t = SketchTable(n, depth=d, width=w, seed=42, counters="f64")
            tables.append(t)
            t.ingest(rows, keys, vals)
            t.finalize()
            exps.append(oracle.build_table(n, d, w, ha, hb, rows, keys, vals))
            assert np.array_equal(t.read_counters().view(np.uint64), exps[i].view(np.uint64))
        a, b = tables
        assert (exps[0] < 0).any() and (exps[0] != np.round(exps[0] * 1024) / 1024).any()
        a.save(path)
        image = a.save_device()
        b.merge(path)
        want = exps[1] + exps[0]  # one correctly rounded add per counter
        got = b.read_counters()
        assert np.all((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want)))  # bitwise
        assert np.array_equal(ck.sum_counters([str(path), str(path)]), 2 * exps[0])
        b.finalize()
        assert abs(b.similarity(0, 0) - 1.0) < 1e-12
        with SketchTable(n, depth=d, width=w, seed=42, counters="f64") as e:  # an empty handle, the device image
            e.merge_device(image)
            assert np.array_equal(e.read_counters().view(np.uint64), exps[0].view(np.uint64))
            assert e.stats()["pairs_ingested"] == 6000
    finally:
        for t in tables:
            t.close()


# ---- 7: refusals leave the table untouched ----

RN, RD, RW = SHAPES[0]


@pytest.fixture(scope="module")
def a_file(oracle, tmp_path_factory):
    """Table A of the first shape as a file, saved once by a handle in the
    default layout (so it holds list and 4-bit rows whatever layout the suite
    runs under; the handles that merge it take the suite's)."""
    path = str(tmp_path_factory.mktemp("merge") / "a.ckpt")
    ref = _reference(oracle, RN, RD, RW)
    with _default_env():
        with _table(RN, RD, RW, ref["pa"]) as a:
            a.save(path)
    return path


def _snapshot(t):
    s = t.stats()
    return t.read_counters(), t.owner_forms(), {k: s[k] for k in STAT_KEYS}


def _unchanged(t, snap):
    c, (f, b), s = _snapshot(t)
    return np.array_equal(c.view(np.uint64), snap[0].view(np.uint64)) and np.array_equal(f, snap[1][0]) and \
        np.array_equal(b, snap[1][1]) and s == snap[2]


def _code(fn, *args):
    with pytest.raises(_lib.CmsError) as ei:
        fn(*args)
    return ei.value.code


def _fix_checksum(img):
    hd = np.frombuffer(bytes(img[:ck.HEADER_BYTES]), ck.HEADER)[0]
    po = int(hd["payload_off"])
    img[112:120] = np.uint64(ck.payload_checksum(bytes(img[po:]))).tobytes()


def _corruptions():
    """tests/test_gpu_checkpoint.py's set, restated."""
    def truncated(img, c):
        return img[:-16]

    def flipped_byte(img, c):  # caught by the checksum
        img[c.payload_off + int(c.offsets[np.flatnonzero(c.lengths)[0]])] ^= 0x10
        return img

    def list_entry_w(img, c):  # a list entry set to w, the checksum recomputed: the device validation
        r = int(np.flatnonzero(c.forms == ck.ROW_FORMS.index("list"))[-1])
        at = c.payload_off + int(c.offsets[r]) + int(c.lengths[r]) - 2  # its last entry
        img[at:at + 2] = np.uint16(c.width).tobytes()
        _fix_checksum(img)
        return img

    def list_wrong_m(img, c):  # a wrong leading m
        r = int(np.flatnonzero(c.forms == ck.ROW_FORMS.index("list"))[0])
        at = c.payload_off + int(c.offsets[r])
        m = int(np.frombuffer(bytes(img[at:at + 2]), "<u2")[0])
        img[at:at + 2] = np.uint16(m + 1).tobytes()
        _fix_checksum(img)
        return img

    def bad_directory(img, c):  # refused on the host: a 4-bit row claimed as u8
        r = int(np.flatnonzero(c.forms == ck.ROW_FORMS.index("u4"))[0])
        img[int(c.header["dir_off"]) + 32 * r] = ck.ROW_FORMS.index("u8")
        return img

    return [truncated, flipped_byte, list_entry_w, list_wrong_m, bad_directory]


@pytest.mark.parametrize("corrupt", _corruptions(), ids=lambda f: f.__name__)
@pytest.mark.parametrize("device_image", [False, True], ids=["file", "device"])
def test_a_bad_image_is_refused_and_the_table_is_untouched(oracle, a_file, tmp_path, corrupt, device_image):
    """With a correct library nothing is launched that indexes by these bytes
    and no counter, place, form, bound or mass changes; with an incorrect one
    the status assertion fails first."""
    import torch
    ref = _reference(oracle, RN, RD, RW)
    c = ck.read_checkpoint(a_file)
    img = corrupt(bytearray(open(a_file, "rb").read()), c)
    with _table(RN, RD, RW, ref["pb"]) as t:
        snap = _snapshot(t)
        if device_image:
            dev = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(torch.device("cuda", t.device))
            assert _code(t.merge_device, dev) == _lib.CMS_E_PARAM
        else:
            bad = tmp_path / "bad.ckpt"
            bad.write_bytes(img)
            assert _code(t.merge, str(bad)) == _lib.CMS_E_PARAM
        assert _unchanged(t, snap)
        t.merge(a_file)  # the good image then merges
        _check_counters(t, ref["A"] + ref["B"])


MISMATCH = {
    "seed": dict(seed=7),
    "depth": dict(depth=RD + 1),
    "width": dict(width=RW // 2),
    "num_owners": dict(num_owners=RN // 2),
    "counters": dict(counters="f64"),
    "frac_bits": dict(frac_bits=1),
}


@pytest.mark.parametrize("case", list(MISMATCH))
def test_an_incompatible_handle_refuses_the_merge(oracle, a_file, case):
    import torch
    args = dict(num_owners=RN, depth=RD, width=RW, counters="u32", frac_bits=0, seed=42)
    args.update(MISMATCH[case])
    n = args.pop("num_owners")
    image = torch.frombuffer(bytearray(open(a_file, "rb").read()), dtype=torch.uint8)
    with SketchTable(n, **args) as t:
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]), np.array([1, 2, 1, 1], np.float32))
        t.finalize()
        before = t.read_counters()
        pairs = t.stats()["pairs_ingested"]
        forms = None if case == "counters" else t.owner_forms()
        assert _code(t.merge, a_file) == _lib.CMS_E_PARAM
        assert _code(t.merge_device, image.to(torch.device("cuda", t.device))) == _lib.CMS_E_PARAM
        assert np.array_equal(t.read_counters().view(np.uint64), before.view(np.uint64))
        assert t.stats()["pairs_ingested"] == pairs
        if forms is not None:
            assert all(np.array_equal(x, y) for x, y in zip(t.owner_forms(), forms))


def test_installed_hash_parameters_differing_in_one_value_are_refused(oracle, a_file):
    ref = _reference(oracle, RN, RD, RW)
    ha, hb = oracle.hash_params(42, RD)
    hb2 = hb.copy()
    hb2[RD - 1] += 1
    with SketchTable(RN, depth=RD, width=RW, seed=42) as t:
        t.set_hash_params(ha, hb2)
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]))
        t.finalize()
        snap = _snapshot(t)
        assert _code(t.merge, a_file) == _lib.CMS_E_PARAM
        assert _unchanged(t, snap)
    with SketchTable(RN, depth=RD, width=RW, seed=1234) as t:  # another seed, the image's parameters installed
        t.set_hash_params(ha, hb)
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]))
        t.merge(a_file)
        exp = ref["A"] + oracle.build_table(RN, RD, RW, ha, hb, np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]),
                                            np.ones(4, np.float32))
        _check_counters(t, exp)


def test_owner_id_sections_must_agree(oracle, tmp_path):
    n, d, w = 300, 3, 100
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    other = ids.copy()
    other[n // 2] += 1  # one ID differs (still ascending)
    ha, hb = oracle.hash_params(42, d)
    rng = np.random.Generator(np.random.PCG64(8))
    rows, keys = rng.integers(0, n, 5000), rng.integers(0, 3000, 5000)
    exp = oracle.build_table(n, d, w, ha, hb, rows, keys, np.ones(rows.size, np.float32))
    with_ids, without = str(tmp_path / "ids.ckpt"), str(tmp_path / "plain.ckpt")
    with SketchTable(n, depth=d, width=w, seed=42, owner_ids=ids) as a:
        a.ingest(ids[rows], keys)
        a.finalize()
        a.save(with_ids)
    with SketchTable(n, depth=d, width=w, seed=42) as a:
        a.ingest(rows, keys)
        a.save(without)
    for live_ids, path, ok in ((None, with_ids, False), (ids, without, False), (other, with_ids, False),
                               (ids, with_ids, True), (None, without, True)):
        with SketchTable(n, depth=d, width=w, seed=42, owner_ids=live_ids) as t:
            t.ingest(rows[:100] if live_ids is None else live_ids[rows[:100]], keys[:100])
            t.finalize()
            snap = _snapshot(t)
            if ok:
                t.merge(path)
                _check_counters(t, exp + oracle.build_table(n, d, w, ha, hb, rows[:100], keys[:100],
                                                            np.ones(100, np.float32)))
            else:
                assert _code(t.merge, path) == _lib.CMS_E_PARAM
                assert _unchanged(t, snap)


def test_merge_with_a_communicator_is_refused(oracle, a_file):
    from mahout_amd import transport
    with SketchTable(RN, depth=RD, width=RW, seed=42, collective_single_rank=True) as t:
        def allgather(send, recv, nbytes):
            host = np.empty(nbytes, np.uint8)
            transport._d2h(host, send, nbytes)
            transport._h2d(recv, host, nbytes)
        t.comm_init_transport(0, 1, lambda ptr, count: None, allgather)
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]))
        t.finalize()
        before = t.read_counters()
        with pytest.raises(_lib.CmsError) as ei:
            t.merge(a_file)
        assert ei.value.code == _lib.CMS_E_STATE and "communicator" in str(ei.value)
        with pytest.raises(_lib.CmsError) as el:
            t.load(a_file)
        assert str(el.value).split(":", 1)[1] == str(ei.value).split(":", 1)[1]  # the load's wording
        assert np.array_equal(t.read_counters(), before)


def test_merge_into_a_per_owner_handle_is_refused(a_file):
    import torch
    with SketchTable.per_owner_shapes(40) as t:
        assert _code(t.merge, a_file) == _lib.CMS_E_STATE
        image = torch.frombuffer(bytearray(open(a_file, "rb").read()), dtype=torch.uint8)
        assert _code(t.merge_device, image.to(torch.device("cuda", t.device))) == _lib.CMS_E_STATE


def test_a_mass_reaching_2_32_is_refused(oracle):
    """Two owners of mass 2^31 each: the ingest's overflow rule (old + inc >=
    2^32), checked before any write."""
    n, d, w = 8, 3, 128
    big = np.array([2.0 ** 31], np.float32)
    with SketchTable(n, depth=d, width=w, seed=42) as src, SketchTable(n, depth=d, width=w, seed=42) as t:
        src.ingest(np.array([3]), np.array([9]), big)
        src.finalize()
        image = src.save_device()
        t.ingest(np.array([3, 4]), np.array([9, 9]), np.array([2.0 ** 31, 5.0], np.float32))
        t.finalize()
        snap = _snapshot(t)
        assert _code(t.merge_device, image) == _lib.CMS_E_OVERFLOW
        assert _unchanged(t, snap)
    with SketchTable(n, depth=d, width=w, seed=42) as src, SketchTable(n, depth=d, width=w, seed=42) as t:
        src.ingest(np.array([3]), np.array([9]), np.array([2.0 ** 31 - 128], np.float32))  # (a float32 below 2^31)
        image = src.save_device()
        t.ingest(np.array([3]), np.array([9]), big)
        t.merge_device(image)  # 2^32 - 128 fits
        ha, hb = oracle.hash_params(42, d)
        exp = oracle.build_table(n, d, w, ha, hb, np.array([3]), np.array([9]), np.ones(1, np.float32)) * (2.0 ** 32 - 128)
        _check_counters(t, exp)


# ---- 8: layouts ----

def _setenv(monkeypatch, on):
    for v in LAYOUT_VARS:
        monkeypatch.setenv(v, "1" if v == on else "0")


@pytest.mark.parametrize("var", LAYOUT_VARS)
def test_default_file_merges_into_every_layout(oracle, tmp_path, monkeypatch, var):
    n, d, w = SHAPES[0]
    ref = _reference(oracle, n, d, w)
    path = str(tmp_path / "a.ckpt")
    _setenv(monkeypatch, None)  # the default (compact) layout saves
    with _table(n, d, w, ref["pa"]) as a:
        a.save(path)
    _setenv(monkeypatch, var)
    with _table(n, d, w, ref["pb"]) as b:
        b.merge(path)
        both = ref["A"] + ref["B"]
        _check_counters(b, both)
        if var == "CMS_NO_FORMS":  # the same kernels into u16 slots and hot rows: no expansion detour
            assert {FORMS[f] for f in np.unique(b.owner_forms()[0])} == {"u32", "u16"}
        b.finalize()
        sims = oracle.similarities_row(both, 1)
        sims[1] = oracle.cosine_cm(both[1], both[1])
        assert _same(b.similarities(1, np.arange(n)), sims)


# ---- 9: designed images: a long list in one bucket; the one group below a byte ----

def _device(t, data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", t.device))


def _narrowest(bound, w):
    """widen_target for a row without counters of its own (cms_forms.h)."""
    if bound <= 1 and w % 128 == 0:
        return "u1"
    if bound <= 3 and w % 64 == 0:
        return "u2"
    return "u4" if bound <= 15 else "u8" if bound <= 255 else "u16"


def _masses(t, tmp_path):
    path = str(tmp_path / "masses.ckpt")
    t.save(path)
    return ck.read_checkpoint(path).masses


# (m, w): the loader takes a list only while it is shorter than the u16 row (2 + 2 d m <= 2 d w), so at d = 2 the
# longest list a build stores, m = 1024, needs w > 1024; 511 is the longest at w = 512
LONG_LISTS = [(255, 512), (256, 512), (300, 512), (511, 512), (1024, 2048)]


@pytest.mark.parametrize("m,w", LONG_LISTS)
def test_a_long_list_in_one_bucket(oracle, tmp_path, m, w):
    """Image row 0 is a list of m entries that all share bucket 5 of sketch row
    0 and bucket 7 of sketch row 1: the loader bounds a list's length, not a
    bucket's count, so a count passes 2^8.  (A u8 cell, four to a word, would
    carry from bucket 5 into bucket 6 and off the word from bucket 7.)  Merged
    into an empty table, a u8 row, a u32 row and a list row, every counter of
    every row is live + image, row 0 in the narrowest form that holds its
    bound; the subtraction of the same image gives the live table back.

    On the commit before the list rows' write pass counted in u16 cells (and
    before merge_increment bounded a list's counter by 1024, not 255) this test
    passed for m = 255 and failed for every longer list, with wrong counters
    and nothing worse.  Into the empty table, sketch row 0 / buckets 5 and 6,
    sketch row 1 / bucket 7: m = 256 gave 0, 1, 0; m = 300 gave 44, 1, 44;
    m = 511 gave 255, 1, 255; m = 1024 gave 0, 4, 0 -- m mod 256 in the bucket,
    the carry in bucket 6, and off the top of the word from bucket 7."""
    n, d = 4, 2
    ha, hb = oracle.hash_params(42, d)
    forms, _ = _layout(w)
    img = np.zeros((n, d, w), np.uint64)
    img[0, 0, 5] = img[0, 1, 7] = m
    img[1, :, 3:9] = 2
    img[2, 1, 100] = 70000  # a u32 image row
    img[3, 0, w - 1] = 1
    image = ck.build_checkpoint(img, ha, hb, seed=42, lists={0: np.array([[5] * m, [7] * m])})
    assert ck.ROW_FORMS[ck.Checkpoint(image).forms[0]] == "list"
    lives = {}
    lives["empty"] = None
    c = np.zeros((n, d, w), np.uint64)
    c[0, :, 5], c[0, :, 6], c[0, :, 7] = 3, 200, 1
    c[1, 0, 4] = 9
    lives["u8"] = (c, dict(forms=["u8", None, None, None]))
    c = np.zeros((n, d, w), np.uint64)
    c[0, :, 5], c[0, :, 6], c[0, :, 7] = 70000, 3 * 65535, 255
    c[3, :, w - 1] = 14
    lives["u32"] = (c, dict(forms=["u32", None, None, None]))
    c = np.zeros((n, d, w), np.uint64)
    c[0, :, 5] = c[0, :, 6] = c[0, :, 7] = 1
    c[2, 0, 100] = 5
    lives["list"] = (c, dict(lists={0: np.array([[5, 6, 7], [5, 6, 7]])}))
    for name, live in lives.items():
        with SketchTable(n, depth=d, width=w, seed=42) as t:
            if live is None:
                base = np.zeros((n, d, w), np.uint64)
            else:
                base = live[0]
                t.load_device(_device(t, ck.build_checkpoint(base, ha, hb, seed=42, **live[1])))
                assert not forms or FORMS[t.owner_forms()[0][0]] == name
            mass0 = _masses(t, tmp_path) if live is not None else np.zeros(n, np.uint64)
            dev = _device(t, image)
            t.merge_device(dev)
            got = t.read_counters()
            print(name, m, "row 0 buckets 4..8:", got[0, :, 4:9].tolist())
            assert np.array_equal(got, (base + img).astype(np.float64)), (name, m)
            # (the u8 row's mass is 204: with m more it passes u8 for every m here)
            want = "u32" if name == "u32" else _narrowest(int(mass0[0]) + m, w) if forms else "u16"
            assert FORMS[t.owner_forms()[0][0]] == want, (name, m, FORMS[t.owner_forms()[0][0]], want)
            assert np.array_equal(_masses(t, tmp_path), mass0 + ck.Checkpoint(image).masses)
            t.subtract_device(dev)
            assert np.array_equal(t.read_counters(), base.astype(np.float64)), (name, m)
            assert np.array_equal(_masses(t, tmp_path), mass0)


def test_u32_image_counters_out_of_a_one_bit_row(oracle, tmp_path):
    """The one group below a byte: four u32 image counters face four bits of a
    1-bit live row, the low or the high half of a byte that the neighbouring
    lane's chunk shares."""
    n, d, w = 4, 2, 512
    ha, hb = oracle.hash_params(42, d)
    live = np.zeros((n, d, w), np.uint64)
    live[1, 0, 0:8] = 1       # both halves of byte 0 of sketch row 0
    live[1, 1, 40:48] = 1     # and of byte 5 of sketch row 1
    live[1, 1, 509] = 1
    live[2, :, 7] = 3
    img = np.zeros((n, d, w), np.uint64)
    img[1, 0, [0, 1, 6, 7]] = 1
    img[1, 1, [41, 42, 44, 509]] = 1

    def image_of(c):
        return ck.build_checkpoint(c, ha, hb, seed=42, forms=[None, "u32", None, None])

    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.load_device(_device(t, ck.build_checkpoint(live, ha, hb, seed=42, forms=[None, "u1", None, None])))
        assert not _layout(w)[0] or FORMS[t.owner_forms()[0][1]] == "u1"
        dev = _device(t, image_of(img))
        t.subtract_device(dev)
        left = live - img
        assert np.array_equal(t.read_counters(), left.astype(np.float64))
        assert not _layout(w)[0] or FORMS[t.owner_forms()[0][1]] == "u1"
        assert int(_masses(t, tmp_path)[1]) == 5
        snap = _snapshot(t)
        with pytest.raises(_lib.CmsError) as ei:  # the masses allow it (5 >= 4), the counters do not
            t.subtract_device(dev)
        assert ei.value.code == _lib.CMS_E_OVERFLOW and "owner row 1" in str(ei.value), str(ei.value)
        assert _unchanged(t, snap)
        # bucket 2 (low half) is still set, bucket 6 (high half) no longer: the compare looks at the right half
        one = np.zeros((n, d, w), np.uint64)
        one[1, 0, [2, 6]] = 1
        assert _code(t.subtract_device, _device(t, image_of(one))) == _lib.CMS_E_OVERFLOW
        assert _unchanged(t, snap)
        one[1, 0, 6], one[1, 0, 5] = 0, 1  # buckets 2 and 5: both set
        t.subtract_device(_device(t, image_of(one)))
        assert np.array_equal(t.read_counters(), (left - one).astype(np.float64))
