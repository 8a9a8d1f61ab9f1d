"""GPU: a live sketch table folded to a width that divides its own
(cms_fold_table: k_fold_scan, the host's ckpt::compact_form, k_fold_pack;
DESIGN.md 4.12).  Two references throughout: the oracle's table of the same
stream at the narrow width, counter for counter, and the no-GPU specification
checkpoint.fold_checkpoint of the source's own image, byte for byte.

Source tables are either ingested (whatever forms the builders store) or
installed with load_device(build_checkpoint(...)) where a test needs a row in a
given form.  Every counter table is a stream's, so the oracle can rebuild it at
any width.  No test provokes a fault: every image is the writer's own.
"""
import ctypes
import os

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib, checkpoint as ck

pytestmark = pytest.mark.gpu

LIST_KEYS = int(os.environ.get("CMS_LIST_KEYS", "256"))
N_KEYS = 20000
F = {name: i for i, name in enumerate(ck.ROW_FORMS)}
REQUIRED = [("list", ("list",)), ("list", ("u4", "u8", "u16")), ("u1", ("u2", "u4", "u8", "u16")), ("u4", ("u8",)),
            ("u8", ("u16",)), ("u16", ("u16",)), ("u32", ("u32",)), ("zero", ("zero",))]


def _flag(name):
    return os.environ.get(name, "") not in ("", "0")


def _forms_on():
    return not _flag("CMS_NO_FORMS")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _device(t, data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", t.device))


def _bytes(x):
    return bytes(x.cpu().numpy().tobytes())


def _image(t):
    return _bytes(t.save_device())


def _code(fn, *args):
    with pytest.raises(_lib.CmsError) as ei:
        fn(*args)
    return ei.value.code, str(ei.value)


def _spec(image, wf, forms=None):
    return ck.fold_checkpoint(image, wf, list_keys=LIST_KEYS, forms=_forms_on() if forms is None else forms)


def _names(c):
    return [ck.ROW_FORMS[f] for f in c.forms]


def _check_fold(t, wf, narrow, forms=None):
    """fold_device(wf) against the oracle's narrow table and the specification; returns the decoded image."""
    before = _image(t)
    got = _bytes(t.fold_device(wf))
    c = ck.Checkpoint(got)
    assert c.width == wf
    bad = np.flatnonzero((c.counters() != narrow).any(axis=(1, 2)))
    assert bad.size == 0, ("owners whose folded counters differ from the oracle's", wf, bad[:20])
    spec = _spec(before, wf, forms)
    s = ck.Checkpoint(spec)
    assert _names(c) == _names(s), [(r, x, y) for r, (x, y) in enumerate(zip(_names(c), _names(s))) if x != y][:10]
    assert got == spec, wf  # byte for byte: directory, sorted list entries, pad bytes, checksum
    assert t.fold_size(wf) == len(got)
    assert _image(t) == before
    return c


# ---- 1: every form, every route ----

def _free_keys(oracle, a, b, w, count, start):
    """`count` keys from `start` on that share no bucket in any sketch row at width w."""
    cand = np.arange(start, start + 40 * count, dtype=np.int64)
    h = np.asarray(oracle.hash_keys(a, b, w, cand)).T  # [d][keys]
    used = [set() for _ in a]
    out = []
    for i, k in enumerate(cand.tolist()):
        if all(int(h[r, i]) not in used[r] for r in range(len(a))):
            for r in range(len(a)):
                used[r].add(int(h[r, i]))
            out.append(k)
            if len(out) == count:
                return np.array(out, np.int64)
    raise AssertionError("not enough collision-free keys")


def _designed_stream(oracle, n, d, w):
    """(rows, keys, vals, widened): owner r belongs to class r % 9 --
      0 no keys; 1 a few unit keys (a list); 2 three keys, one repeated (a list with a repeated bucket);
      3 70 keys that share no bucket at w (the list would be longer than the 1-bit row); 4 300+ unit keys (2-bit);
      5 600+ unit keys (4-bit); 6 one key 100 times and 300 unit keys (u8); 7 one key 1000 times (u16);
      8 a few unit keys again, which `widened` stores wider than they need, as merges and subtractions leave rows.
    Owner 9 * 3 + 7 has a weight of 70000: mass >= 2^16, a u32 row."""
    a, b = oracle.hash_params(42, d)
    rows, keys, vals = [], [], []

    def add(r, k, v=None):
        k = np.asarray(k, np.int64) % N_KEYS
        rows.append(np.full(k.size, r, np.int64))
        keys.append(k)
        vals.append(np.ones(k.size, np.float32) if v is None else np.asarray(v, np.float32))

    free = {}
    widened = {}
    rng = np.random.Generator(np.random.PCG64(n))

    def some(m):  # m distinct keys (arithmetic progressions would spread evenly over the buckets)
        return rng.choice(N_KEYS, size=m, replace=False)

    for r in range(n):
        c, i = r % 9, r // 9
        if c == 1:
            add(r, r * 31 + 5 + 977 * np.arange(1 + i % 12))
        elif c == 2:
            add(r, np.repeat(r * 17 + 3 + 131 * np.arange(3), [2 + i % 4, 1, 1]))
        elif c == 3:
            if i % 8 not in free:
                free[i % 8] = _free_keys(oracle, a, b, w, 70, 1000 * (i % 8))
            add(r, free[i % 8])
        elif c == 4:
            add(r, some(300 + 5 * (i % 20)))
        elif c == 5:
            add(r, some(600 + 10 * (i % 30)))
        elif c == 6:
            add(r, np.concatenate([np.full(100, r * 5 + 1), some(300)]))
        elif c == 7:
            if i == 3:
                add(r, [r * 3 + 1, r * 3 + 2], [70000, 2])
            else:
                add(r, np.concatenate([np.full(1000, r * 3 + 1), r * 19 + 7 * np.arange(i % 5)]))
        elif c == 8:
            add(r, r * 23 + 1 + 457 * np.arange(1 + i % 6))
            widened[r] = ("u4", "u8", "u16", "u32", "u2", "u1")[i % 6]
    return np.concatenate(rows), np.concatenate(keys), np.concatenate(vals), widened


def _designed_image(oracle, n, d, w):
    """The stream's table at w as an image: every row in its compact form, the `widened` rows as named."""
    a, b = oracle.hash_params(42, d)
    rows, keys, vals, widened = _designed_stream(oracle, n, d, w)
    table = oracle.build_table(n, d, w, a, b, rows, keys, vals).astype(np.uint64)
    natural = ck.Checkpoint(ck.compact_checkpoint(ck.build_checkpoint(table, a, b, seed=42, pairs_ingested=rows.size)))
    forms, lists = _names(natural), {}
    for r, f in widened.items():
        forms[r] = f if int(table[r].max()) < 1 << ck._BITS[f] else "u16"
    for r, f in enumerate(forms):
        if f == "list":
            lists[r] = natural.list_entries(r)
    data = ck.build_checkpoint(table, a, b, seed=42, forms=forms, lists=lists, pairs_ingested=rows.size)
    return data, (rows, keys, vals)


def test_every_form_every_route(oracle):
    n, d, w = 517, 4, 1024
    default = _forms_on() and not _flag("CMS_NO_COMPACT") and LIST_KEYS == 256
    a, b = oracle.hash_params(42, d)
    data, (rows, keys, vals) = _designed_image(oracle, n, d, w)
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.load_device(_device(t, data))
        src = ck.Checkpoint(_image(t))
        form, _ = t.owner_forms()
        held = np.array([SketchTable.FORMS[f] for f in form], dtype=object)
        held[src.forms == F["zero"]] = "zero"
        pairs = set()
        for wf in (512, 256, 32, 1):
            narrow = oracle.build_table(n, d, wf, a, b, rows, keys, vals)
            c = _check_fold(t, wf, narrow)
            assert np.array_equal(c.masses, src.masses) and c.pairs_ingested == src.pairs_ingested == rows.size
            assert np.array_equal(c.a, src.a) and np.array_equal(c.b, src.b) and c.seed == 42
            pairs |= set(zip(held.tolist(), _names(c)))
        print("(source, image) pairs", sorted(pairs))
        if default:
            for s, targets in REQUIRED:
                assert any((s, x) in pairs for x in targets), ((s, targets), sorted(pairs))
            for s in ("u4", "u8", "u16", "u32"):  # a dense row that folds into a list: what merges widened
                assert (s, "list") in pairs, (s, sorted(pairs))


# ---- 2: the folded table is the narrow table ----

def _stream(n, seed, pairs=30000):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = np.minimum(rng.zipf(1.2, pairs) - 1, n - 9).astype(np.int64)  # (the last eight owners have no keys)
    keys = rng.integers(0, N_KEYS, pairs).astype(np.int64)
    vals = np.ones(pairs, np.float32)
    vals[:3] = 30000  # owner rows[0..2]: masses that pass 2^16
    return rows, keys, vals


def test_the_folded_table_is_the_narrow_table():
    n, d, w, wf = 300, 4, 1024, 256
    rows, keys, vals = _stream(n, 11)
    all_rows = np.arange(n)
    with SketchTable(n, depth=d, width=w, seed=42) as t, SketchTable(n, depth=d, width=wf, seed=42) as ref:
        t.ingest(rows, keys, vals)
        t.finalize()
        ref.ingest(rows, keys, vals)
        ref.finalize()
        with t.folded(wf) as s:
            assert (s.width, s.depth, s.num_owners) == (wf, d, n)
            code, _ = _code(s.similarities, 0, all_rows)
            assert code == _lib.CMS_E_STATE  # not finalized, as after from_checkpoint
            s.finalize()
            assert np.array_equal(s.read_counters(), ref.read_counters())
            for q in (0, 1, 7, n // 2, n - 1):
                assert _same(s.similarities(q, all_rows), ref.similarities(q, all_rows)), q
                for x, y in zip(s.most_similar(q, 10), ref.most_similar(q, 10)):
                    assert _same(x, y), q
            for x, y in zip(s.top_k_all(10), ref.top_k_all(10)):
                assert _same(x, y)
            pq = [(r, k) for r in (0, 1, 7, n - 1) for k in (1, 5, 17, 4242, 19999)]
            assert [s.point_query(r, k) for r, k in pq] == [ref.point_query(r, k) for r, k in pq]
            assert s.stats()["pairs_ingested"] == ref.stats()["pairs_ingested"] == rows.size
            s.compact()
            ref.compact()
            assert _image(s) == _image(ref)


# ---- 3: the source is untouched ----

def test_the_source_is_untouched():
    n, d, w, k = 300, 4, 128, 10  # (kept lists need w % 128 == 0)
    rows, keys, vals = _stream(n, 12, 20000)
    rng = np.random.Generator(np.random.PCG64(5))
    touched = rng.choice(n - 9, size=n // 20, replace=False)
    drow, dkey = touched[rng.integers(0, touched.size, 400)], rng.integers(0, N_KEYS, 400)
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(rows, keys, vals)
        code, _ = _code(t.similarities, 0, np.arange(n))
        assert code == _lib.CMS_E_STATE
        t.fold_device(64)
        code, _ = _code(t.similarities, 0, np.arange(n))
        assert code == _lib.CMS_E_STATE  # a source that is not finalized stays so
        t.finalize()
        t.top_k_refresh(k)  # the whole job: the kept lists
        t.ingest(drow, dkey)
        t.finalize()
        t.similarities(3, np.arange(n))
        before = (_image(t), t.stats(), t.similarities(3, np.arange(n)), t.owner_forms())
        for wf in (64, 32, 1, 128):
            t.fold_device(wf)
        after = (_image(t), t.stats(), t.similarities(3, np.arange(n)), t.owner_forms())
        assert after[0] == before[0] and after[1] == before[1] and _same(after[2], before[2])
        assert all(np.array_equal(x, y) for x, y in zip(after[3], before[3]))
        got = t.top_k_refresh(k)
        n_touched, _, full = t.refresh_stats()
        assert full == 1, "the fold dropped the kept lists: the refresh was a whole job"
        assert n_touched == np.unique(drow).size < n
        for x, y in zip(got, t.top_k_all(k)):
            assert _same(x, y)


# ---- 4: across widths ----

def test_merge_and_subtract_across_widths(oracle):
    n, d, w, wf = 200, 4, 1024, 256
    a, b = oracle.hash_params(42, d)
    wide_s, narrow_s = _stream(n, 21, 20000), _stream(n, 22, 20000)
    first = oracle.build_table(n, d, wf, a, b, *narrow_s)
    both = first + oracle.build_table(n, d, wf, a, b, *wide_s)
    with SketchTable(n, depth=d, width=w, seed=42) as wide, SketchTable(n, depth=d, width=wf, seed=42) as narrow:
        wide.ingest(*wide_s)
        narrow.ingest(*narrow_s)
        narrow.finalize()
        image = wide.fold_device(narrow.width)
        narrow.merge_device(image)
        narrow.finalize()
        assert np.array_equal(narrow.read_counters(), both)
        assert narrow.stats()["pairs_ingested"] == wide_s[0].size + narrow_s[0].size
        assert _same(narrow.similarities(0, np.arange(n)), np.where(np.arange(n) == 0, oracle.cosine_cm(both[0], both[0]),
                                                                    oracle.similarities_row(both, 0)))
        narrow.subtract_device(image)
        narrow.finalize()
        assert np.array_equal(narrow.read_counters(), first)
        assert narrow.stats()["pairs_ingested"] == narrow_s[0].size


# ---- 5: edges of the group walk ----

EDGES = [(4, 64, (32,)), (4, 32, (16,)), (3, 96, (48, 24, 3)), (3, 100, (50, 25, 1)), (1, 1024, (512, 16, 1)),
         (5, 128, (64, 32, 1))]


@pytest.mark.parametrize("d,w,divisors", EDGES, ids=lambda v: str(v).replace(" ", ""))
def test_edges_of_the_group_walk(oracle, d, w, divisors):
    n = 8
    a, b = oracle.hash_params(42, d)
    rows = np.concatenate([np.repeat(np.arange(6), [1, 3, 40, 300, 700, 2]), [5]])  # owners 6 and 7 have no keys
    keys = (rows * 31 + 7 * np.arange(rows.size)) % N_KEYS
    vals = np.ones(rows.size, np.float32)
    vals[-1] = 70000  # owner 5 is hot
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(rows, keys, vals)
        t.finalize()
        src = ck.Checkpoint(_image(t))
        assert ck.ROW_FORMS[src.forms[5]] == "u32"
        for wf in divisors:
            c = _check_fold(t, wf, oracle.build_table(n, d, wf, a, b, rows, keys, vals))
            if wf == 1:  # every counter is the mass
                assert np.array_equal(c.counters()[:, :, 0], np.repeat(src.masses[:, None], d, axis=1).astype(np.float64))
            if wf % 32:
                assert set(_names(c)) <= {"zero", "u16", "u32"}


# ---- 6: the widest shape ----

def test_the_widest_shape(oracle):
    n, d, w = 6, 1, 32768
    a, b = oracle.hash_params(42, d)
    rows = np.concatenate([np.repeat(np.arange(5), [2, 200, 3000, 9000, 1]), [4]])  # owner 5 has no keys
    keys = (rows * 131 + 17 * np.arange(rows.size)) % 1_000_000
    vals = np.ones(rows.size, np.float32)
    vals[-1] = 70000
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(rows, keys, vals)
        t.finalize()
        print("source forms", _names(ck.Checkpoint(_image(t))))
        for wf in (16384, 32768):
            _check_fold(t, wf, oracle.build_table(n, d, wf, a, b, rows, keys, vals))


# ---- 7: modes ----

def test_frac_bits_gives_no_list(oracle):
    n, d, w, wf = 40, 4, 128, 32
    a, b = oracle.hash_params(42, d)
    rows = np.repeat(np.arange(n - 4), 3)
    keys = (rows * 31 + 977 * np.arange(rows.size)) % N_KEYS
    vals = np.full(rows.size, 1.5, np.float32)
    with SketchTable(n, depth=d, width=w, seed=42, frac_bits=1) as t:
        t.ingest(rows, keys, vals)
        t.finalize()
        c = _check_fold(t, wf, oracle.build_table(n, d, wf, a, b, rows, keys, vals))
        assert c.frac_bits == 1 and "list" not in _names(c)
        with t.folded(wf) as s:
            assert s.frac_bits == 1
            assert np.array_equal(s.read_counters(), c.counters())


@pytest.mark.parametrize("var", ["CMS_NO_FORMS", "CMS_NO_COMPACT"])
def test_layout_modes_of_the_source(oracle, monkeypatch, var):
    """The rule takes the handle's forms setting: a CMS_NO_FORMS source gives
    zero / u16 / u32 rows, fold_checkpoint(..., forms=False); CMS_NO_COMPACT
    changes where rows live, not which forms the handle stores."""
    for v in ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_NO_VMM"):
        monkeypatch.setenv(v, "1" if v == var else "0")
    n, d, w = 60, 4, 1024
    a, b = oracle.hash_params(42, d)
    rows, keys, vals = _stream(n, 31, 6000)
    forms = var != "CMS_NO_FORMS"
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(rows, keys, vals)
        t.finalize()
        for wf in (256, 32):
            c = _check_fold(t, wf, oracle.build_table(n, d, wf, a, b, rows, keys, vals), forms=forms)
            if not forms:
                assert set(_names(c)) == {"zero", "u16", "u32"}
            else:
                assert "list" in _names(c)


# ---- 8: refusals and empty cases ----

def test_refusals():
    import torch
    n, d, w = 16, 4, 128
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(np.arange(8), np.arange(8) * 7)
        t.finalize()
        before = _image(t)
        for bad in (3, 0, -1, -64, 256, 96):
            code, msg = _code(t.fold_device, bad)
            assert code == _lib.CMS_E_PARAM, (bad, msg)
            code, _ = _code(t.fold_size, bad)
            assert code == _lib.CMS_E_PARAM
        # a capacity one byte short: CMS_E_PARAM, *bytes set, the buffer untouched
        size = t.fold_size(64)
        buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda:%d" % t.device)
        torch.cuda.synchronize()
        got = ctypes.c_int64(-1)
        rc = t._lib.cms_fold_table_device(t._h, 64, ctypes.c_void_p(buf.data_ptr()), size - 1, ctypes.byref(got))
        assert rc == _lib.CMS_E_PARAM and got.value == size
        assert bool((buf == 0xA5).all())
        assert _image(t) == before
    with SketchTable(20, depth=3, width=128, seed=42, counters="f64") as t:
        t.ingest(np.array([0, 1, 2, 2]), np.array([5, 6, 7, 7]), np.array([1, 2, 1, 1], np.float32))
        t.finalize()
        code, msg = _code(t.fold_device, 64)
        assert code == _lib.CMS_E_STATE and "fp64" in msg, msg
    with SketchTable.per_owner_shapes(40) as t:
        code, msg = _code(t.fold_device, 1)
        assert code == _lib.CMS_E_STATE and "per-owner" in msg, msg


def test_an_empty_handle_folds_to_zero_rows():
    n, d, w, wf = 24, 4, 128, 32
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        image = t.fold_device(wf)
        c = ck.Checkpoint(_bytes(image))
        assert c.width == wf and set(_names(c)) == {"zero"} and c.payload_bytes == 0 and c.pairs_ingested == 0
        assert _bytes(image) == _spec(_image(t), wf)
        with SketchTable(n, depth=d, width=wf, seed=42) as s:
            s.load_device(image)
            assert not s.read_counters().any() and s.stats()["pairs_ingested"] == 0
        t.ingest(np.array([0, 1]), np.array([5, 6]))
        t.reset()
        assert _bytes(t.fold_device(wf)) == _bytes(image)


def test_a_folded_counter_of_2_32_overflows(oracle):
    """tests/test_fold_host.py's image: the loader accepts it (a u32 row's
    counters are not held to its mass), the fold refuses it."""
    a, b = oracle.hash_params(42, 2)
    c = np.zeros((3, 2, 64), np.uint64)
    c[1, 1, 3] = c[1, 1, 3 + 32] = 1 << 31  # two counters of 2^31 in one residue class of 32, 16 and 1
    c[2, 0, 5] = 7
    data = ck.build_checkpoint(c, a, b, seed=42, masses=np.array([0, (1 << 32) - 1, 7], np.uint64))
    with SketchTable(3, depth=2, width=64, seed=42) as t:
        t.load_device(_device(t, data))
        before = _image(t)
        for wf in (32, 16, 1):  # in registers, and through the LDS image
            code, msg = _code(t.fold_device, wf)
            assert code == _lib.CMS_E_OVERFLOW and "owner row 1" in msg, msg
        assert _image(t) == before
        assert _bytes(t.fold_device(64)) == _spec(before, 64)  # nothing folds: nothing overflows


# ---- 9: the file path ----

def test_the_file_path(tmp_path):
    n, d, w, wf = 120, 4, 1024, 256
    rows, keys, vals = _stream(n, 41, 8000)
    path = tmp_path / "folded.ckpt"
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        t.ingest(rows, keys, vals)
        t.finalize()
        t.save_folded(str(path), wf)
        assert path.read_bytes() == _bytes(t.fold_device(wf))
        assert sorted(p.name for p in tmp_path.iterdir()) == ["folded.ckpt"]  # no .tmp left behind
        with SketchTable.from_checkpoint(str(path)) as s, t.folded(wf) as s2:
            assert s.width == wf
            assert np.array_equal(s.read_counters(), s2.read_counters())
