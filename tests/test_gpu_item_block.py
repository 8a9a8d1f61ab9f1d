"""GPU: the staged block cosine (cms_item.hip: cms_similarity_block,
cms_item_estimates_batch) on DESIGNED tables -- counters and storage forms
chosen one by one, written by the checkpoint format's numpy writer
(mahout_amd.checkpoint.build_checkpoint(forms=..., lists=...)) and installed
with SketchTable.load_device -- against similarities() (k_pair_cosine), the
oracle's cosine on the numpy counters, and taste.item_estimate.  Bit for bit,
NaN matching NaN; no tolerance anywhere.

Shapes (d, w), about 24 owners each, at least two owners of every form the
shape has, an all-zero owner, a "zero"-form owner, two hot u32 owners whose
row norms reach 2^53 (the sequential route; asserted from the numpy table):

  (3, 128)    every form, u1 included
  (4, 96)     u4, u8, list, u16, u32
  (2, 20)     no narrow forms; w % 4 == 0
  (2, 7)      the w & 3 path
  (2, 1056)   the lists the small shapes cannot hold: a stored list is at most
              as long as the dense u16 row (2 + 2 d m <= 2 d w, so m <= 127 at
              (3, 128) and m <= 95 at (4, 96)); 255 entries in one bucket need
              w >= 256 and LIST_MAX_KEYS = 1024 keys need w >= 1056.  The
              small shapes carry the longest list they can hold, all of it in
              one bucket of a sketch row
  (2, 8224)   wider than the staged image (item_max_staged_width = 8192): the
              route through k_pair_cosine
"""
import ctypes
import os
import re

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib, checkpoint as ck, taste

pytestmark = pytest.mark.gpu

SHAPES = [(3, 128), (4, 96), (2, 20), (2, 7), (2, 1056), (2, 8224)]
CAP = {"u1": 1, "u2": 3, "u4": 15, "u8": 255, "u16": 65535}
HERE = os.path.dirname(os.path.abspath(__file__))


def _kernel_constant(name):
    src = open(os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_item.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE = _kernel_constant("kItemTile")
MAX_STAGED = _kernel_constant("kItemMaxWidth")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _list_counts(ent, w):
    return np.stack([np.bincount(e, minlength=w) for e in ent]).astype(np.uint64)


def design(d, w):
    """(counters [n][d][w] uint64, forms [n], lists {row: entries [d][m]}, names [n])."""
    rng = np.random.Generator(np.random.PCG64(100 * d + w))
    rows, forms, lists, names = [], [], {}, []

    def add(name, c, form, ent=None):
        if ent is not None:
            lists[len(rows)] = ent
        rows.append(np.asarray(c, np.uint64).reshape(d, w))
        forms.append(form)
        names.append(name)

    dense = ["u1", "u2", "u4", "u8", "u16"]
    for f in dense:
        if not ck.shape_has_form(f, d, w):
            continue
        cap = CAP[f]
        for k in range(2):
            hi = min(cap, 40)
            c = rng.integers(0, hi + 1, (d, w)) * (rng.random((d, w)) < (0.5 if k else 0.9))
            if f == "u16":  # one counter near the form's top, the row mass still below 2^16
                c = rng.integers(0, 4, (d, w)) * (rng.random((d, w)) < 0.5)
                c[np.arange(d), rng.integers(0, w, d)] = 40000 - 7 * k
            else:
                c[np.arange(d), rng.integers(0, w, d)] = cap
            add(f + "_%d" % k, c, f)
    for k in range(2):  # hot rows: counters past 2^16
        c = rng.integers(0, 1 << 20, (d, w)) * (rng.random((d, w)) < 0.6)
        c[0, k % w] = (1 << 22) + k
        add("u32_%d" % k, c, "u32")
    big = []
    for k in range(2):  # row norms of 2^53 (k = 0) and 3 * 2^52 (k = 1): the sequential fp64 route
        c = rng.integers(0, 1 << 12, (d, w)) * (rng.random((d, w)) < 0.7)
        c[k % d] = 0
        c[k % d, rng.permutation(w)[:2 + k]] = 1 << 26
        big.append(len(rows))
        add("big_%d" % k, c, "u32")
    add("zeros", np.zeros((d, w)), None)  # a dense row of zeros
    add("zero_form", np.zeros((d, w)), "zero")
    if ck.shape_has_form("list", d, w):
        mmax = min(ck.LIST_MAX_KEYS, ck.LIST_MAX_ENTRIES // d, (2 * d * w - 2) // (2 * d))
        for k, m in enumerate((3, min(40, mmax))):
            ent = rng.integers(0, w, (d, m))
            add("list_%d" % k, _list_counts(ent, w), "list", ent)
        m = mmax if w < 256 else 300
        ent = rng.integers(0, w, (d, m))
        ent[0, :min(m, 255)] = w - 3  # 255 entries in one bucket (the longest list, where that is shorter)
        add("list_bucket", _list_counts(ent, w), "list", ent)
        if mmax == ck.LIST_MAX_KEYS:
            ent = rng.integers(0, w, (d, mmax))
            add("list_max", _list_counts(ent, w), "list", ent)
    while len(rows) < 20:  # default forms, mixed magnitudes
        top = int(rng.choice([1, 3, 15, 255, 3000]))
        add("mix_%d" % len(rows), rng.integers(0, top + 1, (d, w)) * (rng.random((d, w)) < 0.5), None)
    c = np.stack(rows)
    nrm = (c.astype(object) ** 2).sum(axis=2)  # exact
    assert nrm[big[0]].max() == 2 ** 53 and nrm[big[1]].max() == 3 * 2 ** 52
    assert sum(int(x.max()) >= 2 ** 53 for x in nrm) == 2
    if "list_bucket" in names and w >= 256:
        assert int(c[names.index("list_bucket"), 0].max()) >= 255
    return c, forms, lists, names


class Designed:
    pass


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "d%d-w%d" % s)
def table(request, oracle):
    """One designed table per shape: the handle, its numpy counters and the
    oracle's whole similarity matrix (computed once, shared, never changed)."""
    import torch
    d, w = request.param
    c, forms, lists, names = design(d, w)
    n = c.shape[0]
    ids = 1000 + 7 * np.arange(n, dtype=np.int64)
    a, b = oracle.hash_params(42, d)
    image = ck.build_checkpoint(c, a, b, seed=42, owner_ids=ids, forms=forms, lists=lists)
    t = SketchTable(n, depth=d, width=w, seed=42, owner_ids=ids)
    dev = torch.device("cuda", t.device)
    t.load_device(torch.frombuffer(bytearray(image), dtype=torch.uint8).to(dev))
    t.finalize()
    assert np.array_equal(t.read_counters(), c)
    if not any(os.environ.get(v, "") not in ("", "0") for v in ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_LIST_KEYS")):
        fc, st = ck.Checkpoint(image).form_counts(), t.stats()  # the handle holds the designed forms
        assert st["hot_rows"] == fc.get("u32", 0) >= 4 and st["list_rows"] == fc.get("list", 0)
        assert (st["u8_rows"], st["nibble_rows"], st["crumb_rows"], st["bit_rows"]) == tuple(
            fc.get(f, 0) for f in ("u8", "u4", "u2", "u1"))
    ot = np.ascontiguousarray(c, np.float64)
    S = np.stack([oracle.similarities_row(ot, q) for q in range(n)])
    for q in range(n):
        S[q, q] = oracle.cosine_cm(ot[q], ot[q])
    S.setflags(write=False)
    x = Designed()
    x.t, x.c, x.ids, x.S, x.names, x.d, x.w, x.n = t, c, ids, S, names, d, w, n
    yield x
    t.close()


def test_design_covers_the_forms():
    for d, w in SHAPES:
        c, forms, lists, names = design(d, w)
        assert 20 <= c.shape[0] <= 28
        for f in ("u1", "u2", "u4", "u8", "u16", "u32", "list"):
            if ck.shape_has_form(f, d, w):
                assert forms.count(f) >= 2, (d, w, f)
        assert "zero" in forms and "zeros" in names
        assert ("list_max" in names) == (w >= 1056)
    assert [ck.shape_has_form("u1", d, w) for d, w in SHAPES[:4]] == [True, False, False, False]
    assert not ck.shape_has_form("u8", 2, 20) and 7 & 3 and not 20 & 3
    assert MAX_STAGED < 8224 and all(w <= MAX_STAGED for _, w in SHAPES[:5])


def test_block_equals_rows_oracle_and_transpose(table):
    x = table
    B = x.t.similarity_block(x.ids, x.ids)
    assert B.shape == (x.n, x.n) and B.dtype == np.float64
    for i in range(x.n):
        assert _same(B[i], x.t.similarities(x.ids[i], x.ids)), (x.names[i], "against similarities()")
    bad = np.argwhere(~((B == x.S) | (np.isnan(B) & np.isnan(x.S))))
    assert bad.size == 0, [(x.names[i], x.names[j], B[i, j], x.S[i, j]) for i, j in bad[:8]]
    assert _same(B, B.T)
    zero = [x.names.index("zeros"), x.names.index("zero_form")]
    assert np.isnan(B[zero]).all() and np.isnan(B[:, zero]).all()  # NaN everywhere
    live = x.c.reshape(x.n, -1).max(axis=1) > 0  # every owner with a counter is at least similar to itself
    assert np.isfinite(B[live, live]).all() and np.isfinite(B).sum() > x.n * x.n // 2


def test_block_shapes_and_repeats(table):
    x = table
    ids = x.ids
    assert _same(x.t.similarity_block(ids[3:4], ids), x.S[3:4])           # n1 = 1
    assert _same(x.t.similarity_block(ids, ids[5:6]), x.S[:, 5:6])         # n2 = 1
    assert x.t.similarity_block(ids[:0], ids).shape == (0, x.n)            # n1 = 0
    assert x.t.similarity_block(ids, ids[:0]).shape == (x.n, 0)            # n2 = 0
    rep1 = np.array([2, 2, 0, x.n - 1, 2, 0])
    assert _same(x.t.similarity_block(ids[rep1], ids[rep1]), x.S[np.ix_(rep1, rep1)])
    # more right owners than the kernel's tile holds (repeats): several tiles, the last one partial
    rng = np.random.Generator(np.random.PCG64(x.w))
    cols = np.concatenate([np.arange(x.n), rng.integers(0, x.n, 2 * TILE + 37 - x.n)])
    assert cols.size > 2 * TILE and cols.size % TILE != 0
    rows = np.array([0, x.names.index("big_0"), x.names.index("zeros"), x.n - 1, 1])
    assert _same(x.t.similarity_block(ids[rows], ids[cols]), x.S[np.ix_(rows, cols)])


def test_block_errors(table):
    x = table
    lib = _lib.load()
    vp = ctypes.c_void_p
    ids1 = x.ids[:3].copy()
    ids2 = np.array([x.ids[0], 999, x.ids[1]], np.int64)  # 999: no such owner
    out = np.full((3, 3), -7.25)
    rc = lib.cms_similarity_block(x.t._h, ids1.ctypes.data_as(vp), 3, ids2.ctypes.data_as(vp), 3, out.ctypes.data_as(vp))
    assert rc == _lib.CMS_E_NO_SUCH_ID and np.all(out == -7.25)  # out untouched
    rc = lib.cms_similarity_block(x.t._h, ids2.ctypes.data_as(vp), 3, ids1.ctypes.data_as(vp), 3, out.ctypes.data_as(vp))
    assert rc == _lib.CMS_E_NO_SUCH_ID and np.all(out == -7.25)
    with pytest.raises(_lib.CmsError) as e:
        x.t.item_estimates_batch([0, 1], [999], [1.0], [0, 1], x.ids[:1])
    assert e.value.code == _lib.CMS_E_NO_SUCH_ID
    with pytest.raises(_lib.CmsError) as e:
        x.t.item_estimates_batch([0, 1], x.ids[:1], [1.0], [0, 1], [999])
    assert e.value.code == _lib.CMS_E_NO_SUCH_ID


def test_state_errors():
    with SketchTable(4, depth=2, width=64) as t:  # before finalize(): the error similarities() gives
        t.ingest([0, 1], [5, 6])
        with pytest.raises(_lib.CmsError) as want:
            t.similarities(0, [1])
        for call in (lambda: t.similarity_block([0], [1]),
                     lambda: t.item_estimates_batch([0, 1], [0], [1.0], [0, 1], [1]),
                     lambda: t.item_recommend_batch([0], [0], [0, 1], [0], [1.0], 3)):
            with pytest.raises(_lib.CmsError) as got:
                call()
            assert got.value.code == want.value.code == _lib.CMS_E_STATE and str(got.value) == str(want.value)
    with SketchTable(2, depth=2, width=64, counters="f64") as t:  # refused whatever the handle's state
        _refusals(t)
        t.ingest_csr(np.array([0, 2, 4], np.int64), np.array([1, 2, 2, 3], np.int64), np.ones(4, np.float32))
        t.finalize()
        _refusals(t)
    with SketchTable(2, per_owner=True) as t:
        _refusals(t)


def _refusals(t):
    for call in (lambda: t.similarity_block([0], [1]),
                 lambda: t.item_estimates_batch([0, 1], [0], [1.0], [0, 1], [1]),
                 lambda: t.item_recommend_batch([0], [0], [0, 1], [0], [1.0], 3)):
        with pytest.raises(_lib.CmsError) as e:
            call()
        assert e.value.code == _lib.CMS_E_STATE and "not available" in str(e.value)


# ---- estimates on the same tables ----

def users_of(x):
    """Designed users: (preferred rows, values).  Every form mix; one and two
    preferences; only zero owners (every similarity NaN); more than a tile."""
    rng = np.random.Generator(np.random.PCG64(7 * x.w + x.d))
    zero = [x.names.index("zeros"), x.names.index("zero_form")]
    users = [np.arange(x.n),                          # every owner, so every form
             rng.permutation(x.n)[:x.n // 2],
             np.array([4]),                           # 1 preference: NaN
             np.array([1, x.names.index("big_1")]),   # 2 preferences
             np.array(zero + zero),                   # all NaN
             np.concatenate([rng.integers(0, x.n, TILE + 9), zero, rng.integers(0, x.n, TILE)]),  # 2 tiles and a bit
             np.zeros(0, np.int64)]                   # none
    return [(u, (rng.integers(1, 11, u.size) / 2).astype(np.float32)) for u in users]


def _batch(x, users, cands):
    po = np.concatenate([[0], np.cumsum([u.size for u, _ in users])])
    co = np.concatenate([[0], np.cumsum([c.size for c in cands])])
    pi = x.ids[np.concatenate([u for u, _ in users])] if po[-1] else np.zeros(0, np.int64)
    pv = np.concatenate([v for _, v in users]) if po[-1] else np.zeros(0, np.float32)
    ci = x.ids[np.concatenate(cands)] if co[-1] else np.zeros(0, np.int64)
    return po, pi, pv, co, ci


@pytest.mark.parametrize("capper", [None, (1.5, 4.0)], ids=["uncapped", "capped"])
def test_item_estimates_batch(table, capper):
    x = table
    users = users_of(x)
    assert users[5][0].size > 2 * TILE
    cands = [np.arange(x.n) for _ in users]
    cands[1] = np.array([0, 0, 3, x.n - 1])  # a short, repeating candidate list
    cands[3] = np.zeros(0, np.int64)          # no candidates
    po, pi, pv, co, ci = _batch(x, users, cands)
    got = x.t.item_estimates_batch(po, pi, pv, co, ci, capper)
    assert got.dtype == np.float32 and got.size == co[-1]
    want = np.array([taste.item_estimate(x.S[c, u], v, capper) for (u, v), cs in zip(users, cands) for c in cs.tolist()],
                    np.float32)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    per_user = [got[co[i]:co[i + 1]] for i in range(len(users))]
    assert np.isnan(per_user[2]).all() and np.isnan(per_user[4]).all() and np.isnan(per_user[6]).all()
    assert np.isfinite(per_user[0]).sum() > x.n // 2 and np.isfinite(per_user[5]).sum() > x.n // 2
    if capper:
        fin = got[np.isfinite(got)]
        assert fin.min() >= 1.5 and fin.max() <= 4.0
    # the batch equals one call per user
    for i, ((u, v), cs) in enumerate(zip(users, cands)):
        one = x.t.item_estimates_batch([0, u.size], x.ids[u], v, [0, cs.size], x.ids[cs], capper)
        assert _same(one, per_user[i]), i
