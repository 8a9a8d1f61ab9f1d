"""GPU: a saved sketch table subtracted from a live one (cms_subtract_table /
cms_subtract_table_device: k_ckpt_unpack's verify pass, the counter check of
k_ckpt_apply<kCheck> and k_ckpt_check_rows, then widen_rows over the live
list rows and the subtraction itself, k_ckpt_apply<kSub> and
k_ckpt_apply_lists<kSub>).  Every comparison covers the WHOLE
table and is bit for bit against the oracle's rebuild of the remaining stream
(`T/impl/common/DoubleCountMinSketch.java:72-80`) and against the numpy
specification checkpoint.diff_counters.

The shapes are tests/test_gpu_merge_table.py's, the smallest at which each
path can go wrong: (4096, 4, 1024) reaches lists, 1-/2-bit rows and movers;
(2000, 5, 96) has forms but no 1-/2-bit rows; (300, 3, 100) has no forms and
rows that are no multiple of 16 bytes; (512, 5, 8192) has 160 KB hot rows.
Tables A, B and Z are built by the phases of that file, restated here.

The file also passes when the suite runs under CMS_NO_COMPACT=1, CMS_NO_VMM=1
or CMS_NO_FORMS=1: what a handle cannot hold is not asserted of it.  No test
provokes a fault: an image that is refused is refused by the checks before any
kernel indexes by its contents, and is tried once.
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
NARROW = ("u16", "u8", "u4", "u2", "u1")


def _flag(name):
    return os.environ.get(name, "") not in ("", "0")


def _layout(w):
    """(forms, compact) of a handle created now at width w (cms_create)."""
    forms = w % 32 == 0 and not _flag("CMS_NO_FORMS")
    return forms, forms and not _flag("CMS_NO_COMPACT")


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _phases(n, d, w, live=False):
    """Table A's batches and the further batch of the streaming test; live:
    the same phases with the owner index reversed and other keys, and a window
    of 64 owners below n / 2 that holds list rows, a hot row and untouched
    owners (tests/test_gpu_merge_table.py)."""
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


def _saved(t, tmp_path, name):
    path = str(tmp_path / name)
    t.save(path)
    return ck.read_checkpoint(path)


def _live_states(t, c):
    """Per owner, the live row's state: its owner_forms() form, or "zero" for
    an owner on the shared zero row (c: the handle's own saved directory)."""
    form, _ = t.owner_forms()
    state = np.array([FORMS[f] for f in form], dtype=object)
    state[c.forms == ck.ROW_FORMS.index("zero")] = "zero"
    return state


def _device(t, data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", t.device))


def _code(fn, *args):
    with pytest.raises(_lib.CmsError) as ei:
        fn(*args)
    return ei.value.code, str(ei.value)


def _snapshot(t):
    s = t.stats()
    return bytes(t.save_device().cpu().numpy().tobytes()), {k: s[k] for k in STAT_KEYS}


def _unchanged(t, snap):
    return _snapshot(t) == snap


# ---- 1: the inverse of the merge ----

@pytest.mark.parametrize("n,d,w", SHAPES)
def test_subtract_is_the_inverse_of_the_merge(oracle, tmp_path, n, d, w):
    ref = _reference(oracle, n, d, w)
    path = str(tmp_path / "a.ckpt")
    with _table(n, d, w, ref["pa"]) as a:
        a.save(path)
    data = open(path, "rb").read()
    for name, phases in (("B", ref["pb"]), ("Z", ref["pb"][1:])):
        for device_image in (False, True):
            with _table(n, d, w, phases) as t:
                if device_image:
                    image = _device(t, data)
                    t.merge_device(image)
                else:
                    t.merge(path)
                merged = _saved(t, tmp_path, "m.ckpt")
                if device_image:
                    t.subtract_device(image)
                else:
                    t.subtract(path)
                _check_counters(t, ref[name])
                spec, spec_mass = ck.diff_counters(merged, path)
                assert np.array_equal(spec, ref[name])
                after = _saved(t, tmp_path, "s.ckpt")
                assert np.array_equal(after.masses, spec_mass)
                with _table(n, d, w, phases) as one:
                    alone = _saved(one, tmp_path, "o.ckpt")
                    assert np.array_equal(after.masses, alone.masses)
                    assert t.stats()["pairs_ingested"] == one.stats()["pairs_ingested"] == sum(x[0].size for x in phases)
                    if name != "B" or device_image:
                        continue
                    t.finalize()
                    _check_counters(t, ref[name])
                    for q in _queries(n):
                        s, so = t.similarities(q, np.arange(n)), one.similarities(q, np.arange(n))
                        assert _same(s, so) and np.array_equal(np.isnan(s), np.isnan(so)), q
                    for x, y in zip(t.top_k_all(10), one.top_k_all(10)):
                        assert _same(np.asarray(x, np.float64), np.asarray(y, np.float64))


# ---- 2 and 3: every image form out of every live form, no merge first; dense live rows keep form and place ----

# Owners per group: [0, 40) meet a live list, [40, 80) a dense narrow row, the first HOT owners of [80, 120) a hot
# row; the rest of that group and [120, 160) have nothing but the image's stream; [160, 200) are not in the image.
GROUP = 40
HOT = 7
IMG_FORMS = ("list", "u1", "u2", "u4", "u8", "u16", "u32")
REQUIRED_PAIRS = [("list", "list"), ("narrow", "list"), ("u32", "list"), ("list", "narrow"), ("list", "u32"),
                  ("u32", "narrow"), ("narrow", "u32"), ("u1", "u16"), ("u16", "u8-")]


def _designed_streams(n):
    """Streams A (the image's, four unit pairs per owner of the first four
    groups) and C (what remains): unit increments only, so one row build
    stores the smallest owners as lists."""
    ra = np.repeat(np.arange(4 * GROUP), 4)
    ka = (ra * 31 + 5 + np.tile(np.arange(4), 4 * GROUP) * 977) % N_KEYS
    rc, kc = [], []
    for r in range(GROUP):  # three more keys: the owner stays a list
        rc += [r] * 3
        kc += [(r * 17 + 3 + t * 131) % N_KEYS for t in range(3)]
    for r in range(GROUP, 2 * GROUP):  # too many keys for a list (150 or 400), or one key 1000 times: a u16 row
        m = (150, 400, 1000)[r % 3]
        rc += [r] * m
        kc += [(r * 17 + 3) % N_KEYS] * m if m == 1000 else [(r * 17 + 3 + t * 131) % N_KEYS for t in range(m)]
    for r in range(2 * GROUP, 2 * GROUP + HOT):
        rc += [r] * 70000
        kc += [(r * 17 + 3) % N_KEYS] * 70000
    for r in range(4 * GROUP, 5 * GROUP):
        rc += [r] * 2
        kc += [(r * 17 + 3) % N_KEYS, (r * 17 + 4) % N_KEYS]
    items, users = zipf_stream(N_KEYS, n - 256, 300_000, seed=n)  # the bulk of the row build: owners [256, n)
    rc = np.concatenate([np.array(rc, np.int64), items + 256])
    kc = np.concatenate([np.array(kc, np.int64), users])
    return (ra, ka), (rc, kc)


def _designed_image(ca, d, w):
    """A's counters as an image whose row forms are chosen explicitly: owner r
    takes IMG_FORMS[r % 7], or the next wider one where the shape lacks the
    form or a counter does not fit it."""
    n = ca.shape[0]
    forms, lists = [None] * n, {}
    cu = ca.astype(np.uint64)
    for r in range(4 * GROUP):
        cmax = int(cu[r].max())
        for f in IMG_FORMS[r % 7:]:
            if not ck.shape_has_form(f, d, w):
                continue
            if f == "list":
                lists[r] = np.stack([np.repeat(np.arange(w), cu[r, i].astype(np.int64)) for i in range(d)])
                break
            if cmax <= CAPACITY[f]:
                forms[r] = f
                break
    return ck.build_checkpoint(cu, *_HASH[d], seed=42, forms=forms, lists=lists)


_HASH = {}


def _has_pair(pairs, want):
    src, dst = want
    srcs = NARROW if src == "narrow" else (src,)
    dsts = NARROW if dst == "narrow" else ("u8", "u4", "u2", "u1") if dst == "u8-" else (dst,)
    return any((s, t) in pairs for s in srcs for t in dsts)


def _narrowest(mass, w):
    """widen_target for a list row whose bound is its mass (cms_forms.h)."""
    if mass <= 1 and w % 128 == 0:
        return "u1"
    if mass <= 3 and w % 64 == 0:
        return "u2"
    return "u4" if mass <= 15 else "u8" if mass <= 255 else "u16"


@pytest.mark.parametrize("n,d,w", SHAPES)
@pytest.mark.parametrize("device_image", [False, True], ids=["file", "device"])
def test_every_image_form_out_of_every_live_form(oracle, tmp_path, n, d, w, device_image):
    _HASH[d] = oracle.hash_params(42, d)
    ha, hb = _HASH[d]
    forms, compact = _layout(w)
    default = not any(_flag(v) for v in LAYOUT_VARS)
    (ra, ka), (rc, kc) = _designed_streams(n)
    ca = oracle.build_table(n, d, w, ha, hb, ra, ka, np.ones(ra.size, np.float32))
    cc = oracle.build_table(n, d, w, ha, hb, rc, kc, np.ones(rc.size, np.float32))
    data = _designed_image(ca, d, w)
    img = ck.Checkpoint(data)
    assert np.array_equal(img.counters(), ca)
    img_form = np.array([ck.ROW_FORMS[f] for f in img.forms], dtype=object)
    subs = (img.lengths > 0) & (img.masses > 0)  # the image rows that subtract anything
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(np.concatenate([ra, rc]), np.concatenate([ka, kc]))  # ONE row build
        t.finalize()
        _check_counters(t, ca + cc)
        before = _saved(t, tmp_path, "l.ckpt")
        state = _live_states(t, before)
        form0, _ = t.owner_forms()
        pairs = set(zip(img_form[subs].tolist(), state[subs].tolist()))
        print("covered pairs", sorted(pairs))
        # on the CPU, from the two directories: which pairs this layout must show
        live_has = set(state[subs].tolist())
        if default and forms:
            assert "u32" in live_has and "u16" in live_has, live_has
            if d * w <= 4096:  # (at w = 8192 a list is smaller than any dense form for owners this small)
                assert live_has & {"u8", "u4", "u2", "u1"}, live_has
            if ck.shape_has_form("list", d, w):
                assert "list" in live_has, live_has
        elif not forms:
            assert live_has <= {"u16", "u32"}, live_has
        for want in REQUIRED_PAIRS:
            src, dst = want
            src_ok = any(ck.shape_has_form(f, d, w) for f in (NARROW if src == "narrow" else (src,)))
            dsts = NARROW if dst == "narrow" else ("u8", "u4", "u2", "u1") if dst == "u8-" else (dst,)
            if src_ok and live_has & set(dsts):  # (a form the shape lacks, a state the layout cannot hold)
                assert _has_pair(pairs, want), (want, sorted(pairs))
        assert np.array_equal(ck.diff_counters(before, img)[0], cc)
        if device_image:
            t.subtract_device(_device(t, data))
        else:
            p = tmp_path / "a.ckpt"
            p.write_bytes(data)
            t.subtract(str(p))
        _check_counters(t, cc)
        # 3: dense live rows keep form and place; a live list that lost entries is dense, in the narrowest form
        # that holds the mass it had
        after = _saved(t, tmp_path, "s.ckpt")
        form1, _ = t.owner_forms()
        was_list = state == "list"
        lost = was_list & subs
        assert np.array_equal(form1[~lost], form0[~lost])
        assert np.array_equal(after.classes[~lost], before.classes[~lost])
        assert np.array_equal(after.forms[~lost], before.forms[~lost])
        for r in np.flatnonzero(lost).tolist():
            assert FORMS[form1[r]] == _narrowest(int(before.masses[r]), w), (r, FORMS[form1[r]], int(before.masses[r]))
        assert np.array_equal(after.masses, before.masses - img.masses)
        assert t.stats()["pairs_ingested"] == rc.size
        t.finalize()
        _check_counters(t, cc)
        sims = oracle.similarities_row(cc, 300 % n)
        sims[300 % n] = oracle.cosine_cm(cc[300 % n], cc[300 % n])
        assert _same(t.similarities(300 % n, np.arange(n)), sims)


# ---- 4: subtracting everything ----

@pytest.mark.parametrize("n,d,w", SHAPES[:1] + SHAPES[2:3])
def test_subtracting_the_tables_own_image_leaves_zeros(oracle, n, d, w):
    ref = _reference(oracle, n, d, w)
    with _table(n, d, w, ref["pb"]) as t:
        t.subtract_device(t.save_device())
        assert not t.read_counters().any()
        assert t.stats()["pairs_ingested"] == 0
        t.finalize()
        assert np.all(np.isnan(t.similarities(0, np.arange(1, n))))
        assert not t.read_counters().any()
        t.ingest(*ref["extra"])
        t.finalize()
        _check_counters(t, ref["X"])
        sims = oracle.similarities_row(ref["X"], 3)
        sims[3] = oracle.cosine_cm(ref["X"][3], ref["X"][3])
        assert _same(t.similarities(3, np.arange(n)), sims)


def test_the_masses_are_zero_after_subtracting_everything(oracle, tmp_path):
    n, d, w = SHAPES[0]
    ref = _reference(oracle, n, d, w)
    with _table(n, d, w, ref["pb"]) as t:
        path = str(tmp_path / "b.ckpt")
        t.save(path)
        t.subtract(path)
        c = _saved(t, tmp_path, "z.ckpt")
        assert not c.masses.any() and not c.counters().any()


# ---- 5: round trip after a subtraction ----

@pytest.mark.parametrize("n,d,w", SHAPES)
def test_round_trip_after_a_subtraction(oracle, tmp_path, n, d, w):
    ref = _reference(oracle, n, d, w)
    pa, p1, p2 = (str(tmp_path / x) for x in ("a.ckpt", "s1.ckpt", "s2.ckpt"))
    with _table(n, d, w, ref["pa"]) as a:
        a.save(pa)
    with _table(n, d, w, ref["pb"]) as t:
        t.merge(pa)
        hot = np.array(FORMS, dtype=object)[t.owner_forms()[0]] == "u32"
        t.subtract(pa)
        if (n, d, w) == SHAPES[3]:  # a hot row whose mass fell below 2^16 stays a u32 row
            c = _saved(t, tmp_path, "c.ckpt")
            assert np.any(hot & (c.masses < 65536) & (c.forms == ck.ROW_FORMS.index("u32")))
        t.save(p1)
        with SketchTable.from_checkpoint(p1) as back:
            assert np.array_equal(back.read_counters(), ref["B"])
            back.save(p2)
            back.finalize()
            sims = oracle.similarities_row(ref["B"], 1)
            sims[1] = oracle.cosine_cm(ref["B"][1], ref["B"][1])
            assert _same(back.similarities(1, np.arange(n)), sims)
    assert open(p1, "rb").read() == open(p2, "rb").read()


# ---- 6: streaming continues ----

@pytest.mark.parametrize("n,d,w", SHAPES)
def test_streaming_continues_after_a_subtraction(oracle, tmp_path, n, d, w):
    ref = _reference(oracle, n, d, w)
    path = str(tmp_path / "a.ckpt")
    with _table(n, d, w, ref["pa"]) as a:
        a.save(path)
    with _table(n, d, w, ref["pb"]) as b:
        b.merge(path)
        b.subtract(path)
        b.ingest(*ref["extra"])  # cbound, masses and places are consistent for the next writer
        b.finalize()
        exp = ref["B"] + ref["X"]
        _check_counters(b, exp)
        form, _ = b.owner_forms()
        cap = np.array([CAPACITY[FORMS[f]] for f in form], np.float64)
        lists = np.array(FORMS, dtype=object)[form] == "list"
        assert np.all((cap >= exp.max(axis=(1, 2))) | lists)
        sims = oracle.similarities_row(exp, 3)
        sims[3] = oracle.cosine_cm(exp[3], exp[3])
        assert _same(b.similarities(3, np.arange(n)), sims)


# ---- 7: the incremental refresh survives a delta merge and the delta's subtraction ----

def test_refresh_stays_incremental_after_a_subtraction():
    n, d, w, k = 2000, 4, 256, 10
    items, users = zipf_stream(4000, n, 120_000, seed=77)
    rng = np.random.Generator(np.random.PCG64(5))
    touched = rng.choice(n, size=n // 20, replace=False)  # about 5 % of the owners
    drow = touched[rng.integers(0, touched.size, 3000)]
    dkey = rng.integers(0, 4000, 3000)
    with SketchTable(n, depth=d, width=w, seed=42) as delta, SketchTable(n, depth=d, width=w, seed=42) as b:
        delta.ingest(drow, dkey)
        delta.finalize()
        image = delta.save_device()
        b.ingest(items, users)
        b.finalize()
        b.top_k_refresh(k)  # the whole job: the kept lists
        assert b.refresh_stats()[2] == 1
        b.merge_device(image)
        b.finalize()
        b.top_k_refresh(k)
        assert b.refresh_stats()[2] == 1
        b.subtract_device(image)
        b.finalize()
        got = b.top_k_refresh(k)
        n_touched, _, full = b.refresh_stats()
        assert full == 1, "the subtraction dropped the kept lists: the refresh was a whole job"
        assert n_touched == np.unique(drow).size < n
        for x, y in zip(got, b.top_k_all(k)):
            assert _same(np.asarray(x, np.float64), np.asarray(y, np.float64))


# ---- 8: refusals leave the table untouched ----

RN, RD, RW = SHAPES[0]


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


@pytest.fixture(scope="module")
def a_file(oracle, tmp_path_factory):
    """Table A of the first shape as a file, saved once by a handle in the
    default layout (so it holds list and 4-bit rows whatever layout the suite
    runs under)."""
    path = str(tmp_path_factory.mktemp("subtract") / "a.ckpt")
    ref = _reference(oracle, RN, RD, RW)
    with _default_env():
        with _table(RN, RD, RW, ref["pa"]) as a:
            a.save(path)
    return path


def _fix_checksum(img):
    hd = np.frombuffer(bytes(img[:ck.HEADER_BYTES]), ck.HEADER)[0]
    po = int(hd["payload_off"])
    img[112:120] = np.uint64(ck.payload_checksum(bytes(img[po:]))).tobytes()


def _corruptions():
    def flipped_byte(img, c):  # caught by the checksum
        img[c.payload_off + int(c.offsets[np.flatnonzero(c.lengths)[0]])] ^= 0x10
        return img

    def pad_byte(img, c):  # a non-zero pad byte behind a row that is no multiple of 16 bytes, the checksum recomputed
        r = int(np.flatnonzero(c.lengths % 16 != 0)[0])
        img[c.payload_off + int(c.offsets[r]) + int(c.lengths[r])] = 1
        _fix_checksum(img)
        return img

    def list_entry_w(img, c):  # a list entry set to w, the checksum recomputed: the device validation
        r = int(np.flatnonzero(c.forms == ck.ROW_FORMS.index("list"))[-1])
        at = c.payload_off + int(c.offsets[r]) + int(c.lengths[r]) - 2  # its last entry
        img[at:at + 2] = np.uint16(c.width).tobytes()
        _fix_checksum(img)
        return img

    return [flipped_byte, pad_byte, list_entry_w]


@pytest.mark.parametrize("corrupt", _corruptions(), ids=lambda f: f.__name__)
@pytest.mark.parametrize("device_image", [False, True], ids=["file", "device"])
def test_a_bad_image_is_refused_and_the_table_is_untouched(oracle, a_file, tmp_path, corrupt, device_image):
    """The live table holds A's stream (B merged with A), so the good image
    subtracts; the corrupt one is refused before anything indexes by it."""
    ref = _reference(oracle, RN, RD, RW)
    c = ck.read_checkpoint(a_file)
    img = corrupt(bytearray(open(a_file, "rb").read()), c)
    with _table(RN, RD, RW, ref["pb"]) as t:
        t.merge(a_file)
        snap = _snapshot(t)
        if device_image:
            code, _ = _code(t.subtract_device, _device(t, img))
        else:
            bad = tmp_path / "bad.ckpt"
            bad.write_bytes(img)
            code, _ = _code(t.subtract, str(bad))
        assert code == _lib.CMS_E_PARAM
        assert _unchanged(t, snap)
        t.subtract(a_file)  # the good image then subtracts
        _check_counters(t, ref["B"])


def _one_row_image(c, r, counters, mass):
    """An image of c's shape and hash parameters whose only non-zero row is r."""
    cu = np.zeros((c.num_owners, c.depth, c.width), np.uint64)
    cu[r] = counters
    masses = np.zeros(c.num_owners, np.uint64)
    masses[r] = mass
    return cu, masses


def test_an_underflow_is_refused_and_the_table_is_untouched(oracle, tmp_path):
    """A mass underflow, and a COUNTER underflow that the masses do not show:
    the same owner with equal mass over other buckets (the live row rolled by
    one bucket), once for each live state -- a list (against a list and against
    a dense image row), a dense narrow row, a hot row."""
    ref = _reference(oracle, RN, RD, RW)
    forms, compact = _layout(RW)
    with _table(RN, RD, RW, ref["pb"]) as t:
        c = _saved(t, tmp_path, "b.ckpt")
        state = _live_states(t, c)
        snap = _snapshot(t)
        live = ref["B"].astype(np.uint64)
        cases = []
        for want in ("list", "list-dense", "narrow", "u32"):
            ok = np.isin(state, NARROW) if want == "narrow" else state == want.split("-")[0]
            ok &= (c.masses > 0) & (live.max(axis=(1, 2)) != live.min(axis=(1, 2)))
            if not ok.any():  # (only a layout without list rows lacks a state)
                assert want.startswith("list") and not (forms and compact), want
                continue
            cases.append((want, int(np.flatnonzero(ok)[0])))
        for want, r in cases:
            rolled = np.roll(live[r], 1, axis=1)  # equal row sums, other buckets
            assert np.any(rolled > live[r])
            cu, masses = _one_row_image(c, r, rolled, int(c.masses[r]))
            kw = {}
            if want == "list":
                kw["lists"] = {r: np.stack([np.repeat(np.arange(RW), rolled[i].astype(np.int64)) for i in range(RD)])}
            data = ck.build_checkpoint(cu, c.a, c.b, seed=42, masses=masses, **kw)
            with pytest.raises(ValueError):
                ck.diff_counters(c, ck.Checkpoint(data))
            code, msg = _code(t.subtract_device, _device(t, data))
            assert code == _lib.CMS_E_OVERFLOW and "owner row %d:" % r in msg, (want, r, msg)
            assert _unchanged(t, snap), want
        # a mass one above the live row's (the counters are the live row's own)
        r = int(np.flatnonzero(c.masses > 0)[0])
        cu, masses = _one_row_image(c, r, live[r], int(c.masses[r]) + 1)
        p = tmp_path / "m.ckpt"
        p.write_bytes(ck.build_checkpoint(cu, c.a, c.b, seed=42, masses=masses))
        code, msg = _code(t.subtract, str(p))
        assert code == _lib.CMS_E_OVERFLOW and "below zero" in msg
        assert _unchanged(t, snap)
        # the row itself, whole, then subtracts
        cu, masses = _one_row_image(c, r, live[r], int(c.masses[r]))
        t.subtract_device(_device(t, ck.build_checkpoint(cu, c.a, c.b, seed=42, masses=masses)))
        exp = ref["B"].copy()
        exp[r] = 0
        _check_counters(t, exp)


def test_other_hash_parameters_are_refused(oracle, a_file):
    ha, hb = oracle.hash_params(42, RD)
    hb2 = hb.copy()
    hb2[RD - 1] += 1
    with SketchTable(RN, depth=RD, width=RW, seed=42) as t:
        t.set_hash_params(ha, hb2)
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]))
        t.finalize()
        snap = _snapshot(t)
        code, _ = _code(t.subtract, a_file)
        assert code == _lib.CMS_E_PARAM
        assert _unchanged(t, snap)


def test_owner_id_sections_must_agree(oracle, tmp_path):
    n, d, w = 300, 3, 100
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    other = ids.copy()
    other[n // 2] += 1  # one ID differs (still ascending)
    rng = np.random.Generator(np.random.PCG64(8))
    rows, keys = rng.integers(0, n, 5000), rng.integers(0, 3000, 5000)
    ha, hb = oracle.hash_params(42, d)
    with_ids, without = str(tmp_path / "ids.ckpt"), str(tmp_path / "plain.ckpt")
    with SketchTable(n, depth=d, width=w, seed=42, owner_ids=ids) as a:
        a.ingest(ids[rows[:100]], keys[:100])
        a.save(with_ids)
    with SketchTable(n, depth=d, width=w, seed=42) as a:
        a.ingest(rows[:100], keys[:100])
        a.save(without)
    rest = oracle.build_table(n, d, w, ha, hb, rows[100:], keys[100:], np.ones(rows.size - 100, np.float32))
    for live_ids, path, ok in ((None, with_ids, False), (ids, without, False), (other, with_ids, False),
                               (ids, with_ids, True), (None, without, True)):
        with SketchTable(n, depth=d, width=w, seed=42, owner_ids=live_ids) as t:
            t.ingest(rows if live_ids is None else live_ids[rows], keys)
            t.finalize()
            snap = _snapshot(t)
            if ok:
                t.subtract(path)
                _check_counters(t, rest)
            else:
                code, _ = _code(t.subtract, path)
                assert code == _lib.CMS_E_PARAM
                assert _unchanged(t, snap)


def test_an_fp64_handle_refuses_the_subtraction(tmp_path):
    n, d, w = 200, 3, 101
    with SketchTable(n, depth=d, width=w, seed=42, counters="f64") as t:
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]), np.array([1, 2, 1, 1], np.float32))
        t.finalize()
        before = t.read_counters()
        image = t.save_device()
        path = str(tmp_path / "f.ckpt")
        t.save(path)
        for fn, arg in ((t.subtract_device, image), (t.subtract, path)):
            code, msg = _code(fn, arg)
            assert code == _lib.CMS_E_STATE and "fp64" in msg, msg
        assert np.array_equal(t.read_counters().view(np.uint64), before.view(np.uint64))
        assert t.stats()["pairs_ingested"] == 4


def test_a_per_owner_handle_refuses_the_subtraction(a_file):
    with SketchTable.per_owner_shapes(40) as t:
        assert _code(t.subtract, a_file)[0] == _lib.CMS_E_STATE
        assert _code(t.subtract_device, _device(t, open(a_file, "rb").read()))[0] == _lib.CMS_E_STATE


def test_a_handle_with_a_communicator_refuses_the_subtraction(a_file):
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
        code, msg = _code(t.subtract, a_file)
        assert code == _lib.CMS_E_STATE and "communicator" in msg
        assert np.array_equal(t.read_counters(), before)


def test_an_empty_handle_accepts_only_an_image_of_no_mass(a_file):
    c = ck.read_checkpoint(a_file)
    zeros = ck.build_checkpoint(np.zeros((RN, RD, RW), np.uint64), c.a, c.b, seed=42)
    with SketchTable(RN, depth=RD, width=RW, seed=42) as t:
        code, msg = _code(t.subtract, a_file)
        assert code == _lib.CMS_E_OVERFLOW and "below zero" in msg
        assert t.stats()["pairs_ingested"] == 0 and not t.read_counters().any()
        t.subtract_device(_device(t, zeros))
        assert t.stats()["pairs_ingested"] == 0 and not t.read_counters().any()
        t.merge(a_file)  # the handle is as it was: empty, and takes the image
        assert np.array_equal(t.read_counters(), c.counters())


# ---- the wrapper's argument errors ----

def test_subtract_device_argument_errors():
    import torch
    with SketchTable(64, depth=3, width=128, seed=42) as t:
        t.ingest(np.array([0, 1]), np.array([5, 6]))
        image = t.save_device()
        before = t.read_counters()
        with pytest.raises(ValueError):
            t.subtract_device(image.cpu())  # a CPU tensor
        with pytest.raises(ValueError):
            t.subtract_device(image[:image.numel() // 4 * 4].view(torch.int32))  # not uint8
        with pytest.raises(ValueError):
            t.subtract_device(image[::2])  # not contiguous
        if torch.cuda.device_count() > 1:
            other = (t.device + 1) % torch.cuda.device_count()
            with pytest.raises(ValueError):
                t.subtract_device(image.to(torch.device("cuda", other)))  # another GPU
        assert np.array_equal(t.read_counters(), before)
        t.subtract_device(image)
        assert not t.read_counters().any()
