"""GPU: the exact CosineSimilarity over an attached DataModel (cms_exact.hip:
cms_exact_attach_csr, cms_exact_similarities, cms_exact_pairs,
cms_exact_top_k_rows) against the plain-Python restatement of
CosineSimilarity.userSimilarity (tests/exact_ref.py).  Bit for bit, NaN
matching NaN; no tolerance anywhere.  Every model is compared over all its
pairs and all its query rows unless its test says otherwise.

  tile edges    CMS_EXACT_TILE=64, 200 owners (three full tiles and one of 8), 40
                items, half-star values: an item every owner holds, an item of one
                owner, a posting list that begins on a tile's first row and one that
                ends on a tile's last row, owners of 0 and 1 preferences, an owner
                whose values are all 0.0; unweighted and weighted; k = 5 and k = 250
  ties          eight identical owners and a query whose k-th score 12 candidates
                share; scattered and negative owner IDs
  default tile  n = T + 37 owners (T read from cms_exact.h), 32 query rows with
                T - 1, T and n - 1 among them; posting lists longer than a wave
  routes        values 0.1 .. 0.8 (s = 27: owners past 2^53 and below it in one
                model), a 1e8 value (s = 0, one owner past 2^53), thirds and negative
                values (s = 25: negative units through the tile), and the same with a
                768th (no s: wholly sequential); pairs, rows and the top-k slab agree
                with each other and with the restatement
  state         CMS_E_STATE before attach and after detach, CMS_E_NO_SUCH_ID, a
                refused CSR keeps the model, a second attach replaces it, every
                handle kind, the sketch table's image byte-identical throughout
  known answers the reference's own numbers for the exact cosine
"""
import json
import os
import re

import numpy as np
import pytest

import exact_ref as R
from mahout_amd import SketchTable, _lib
from mahout_amd.sketch import frac_bits_for

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden_cms.json")))


def _kernel_constant(name):
    src = open(os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_exact.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE = _kernel_constant("kExactTile")


def _open(M, weighted=False, tile=None):
    """A minimal handle (its sketch table is never ingested) with M attached.
    CMS_EXACT_TILE is read when the handle is created."""
    old = os.environ.get("CMS_EXACT_TILE")
    try:
        if tile is not None:
            os.environ["CMS_EXACT_TILE"] = str(tile)
        t = SketchTable(M.n, depth=1, width=32, weighted=weighted, device=0, owner_ids=M.owner_ids)
    finally:
        if tile is not None:
            if old is None:
                del os.environ["CMS_EXACT_TILE"]
            else:
                os.environ["CMS_EXACT_TILE"] = old
    t.attach_exact(M.offsets, M.keys, M.vals)
    return t


def _check_lists(M, t, rows, ref_rows, k):
    """exact_top_k_rows of `rows` against TopItems.getTopUsers over the restatement's rows."""
    ids, sc, cnt = t.exact_top_k_rows(rows, k)
    for i, r in enumerate(rows):
        eids, esc = M.top_k(int(r), k, ref_rows[i])
        c = int(cnt[i])
        assert c == eids.size, (r, c, eids.size)
        assert ids[i, :c].tolist() == eids.tolist(), r
        assert R.same_bits(sc[i, :c], esc).all(), r
        assert (ids[i, c:] == -1).all() and np.isnan(sc[i, c:]).all()


def _check_model(M, t, weighted, ks):
    """Every pair through exact_pairs and exact_similarities, every row's top-k."""
    ref = M.all_pairs(weighted)
    n = M.n
    i1, i2 = np.divmod(np.arange(n * n), n)
    got = t.exact_pairs(M.owner_ids[i1], M.owner_ids[i2]).reshape(n, n)
    bad = np.argwhere(~R.same_bits(got, ref))
    assert bad.size == 0, (bad[:5].tolist(), [(got[a, b], ref[a, b]) for a, b in bad[:5]])
    for r in range(n):
        assert R.same_bits(t.exact_similarities(int(M.owner_ids[r]), M.owner_ids), ref[r]).all(), r
    for k in ks:
        _check_lists(M, t, np.arange(n), ref, k)
    return ref


# ---- tile edges ----

def _tile_edge_model():
    rng = np.random.Generator(np.random.PCG64(64))
    n, half = 200, [0.5 * v for v in range(1, 11)]
    prefs = []
    for r in range(n):
        p = {0: float(rng.choice(half))}                       # item 0: every owner that has preferences
        for it in rng.choice(np.arange(4, 40), int(rng.integers(3, 8)), replace=False):
            p[int(it)] = float(rng.choice(half))
        if 64 <= r <= 90:
            p[2] = float(rng.choice(half))                     # item 2: begins on tile 1's first row
        if 100 <= r <= 127:
            p[3] = float(rng.choice(half))                     # item 3: ends on tile 1's last row
        prefs.append(p)
    prefs[17][1] = 4.5                                         # item 1: a single owner
    prefs[5] = {}                                              # no preference
    prefs[6] = {0: 3.5}                                        # one preference
    prefs[70] = {k: 0.0 for k in prefs[70]}                    # every value 0.0
    prefs[191] = {k: 0.0 for k in list(prefs[191])[:2]}        # ... in the short last tile too
    M = R.Model.from_lists([list(p.items()) for p in prefs], owner_ids=np.arange(n) * 3 - 100)
    # the design holds what it claims
    owners_of = lambda it: [r for r in range(n) if it in prefs[r]]  # noqa: E731
    assert owners_of(0) == [r for r in range(n) if r != 5] and owners_of(1) == [17]
    assert owners_of(2)[0] == 64 and owners_of(3)[-1] == 127 and 64 % 64 == 0 and 128 % 64 == 0
    assert frac_bits_for(M.vals) == 1
    return M


@pytest.fixture(scope="module")
def tile_edge_model():
    return _tile_edge_model()


@pytest.mark.parametrize("weighted", [False, True])
def test_tile_edges(tile_edge_model, weighted):
    M = tile_edge_model
    with _open(M, weighted, tile=64) as t:
        ref = _check_model(M, t, weighted, ks=(5, 250))
        assert np.isnan(ref[5]).all() and np.isnan(ref[70]).all() and not np.isnan(ref[6, 7])
        # a single owner by ID, as mostSimilarUserIDs asks
        ids, sc = t.exact_most_similar(int(M.owner_ids[64]), 5)
        eids, esc = M.top_k(64, 5, ref[64])
        assert ids.tolist() == eids.tolist() and R.same_bits(sc, esc).all()
        # repeated and unordered query rows
        rows = np.array([199, 0, 64, 64, 5, 127, 128, 63])
        _check_lists(M, t, rows, ref[rows], 7)


# ---- ties ----

def test_ties_scattered_negative_ids():
    rng = np.random.Generator(np.random.PCG64(12))
    prefs = [[(0, 1.0), (1, 2.0)] for _ in range(8)]            # eight identical owners
    prefs += [[(2, 3.0)] for _ in range(12)]                    # twelve that tie below them
    prefs += [[(0, 1.0), (1, 2.0), (2, 1.0)]]                   # the query
    for _ in range(9):                                          # the rest share no item with the query: 0.0
        its = rng.choice([3, 4, 5], int(rng.integers(1, 4)), replace=False)
        prefs.append([(int(i), float(rng.integers(1, 6))) for i in its])
    n = len(prefs)
    order = rng.permutation(n)                                  # the groups scattered over the rows
    prefs = [prefs[i] for i in order]
    ids = np.sort(rng.choice(np.arange(-10 ** 12, 10 ** 12, 10 ** 7), n, replace=False))
    assert (ids < 0).any() and (ids > 0).any()
    M = R.Model.from_lists(prefs, owner_ids=ids)
    q = int(np.argwhere(order == 20)[0, 0])
    with _open(M, tile=64) as t:
        ref = _check_model(M, t, False, ks=(3, 10, 40))
    s = ref[q].copy()
    s[q] = np.nan
    top = np.sort(s[~np.isnan(s)])[::-1]
    assert (s == top[9]).sum() == 12 and (s > top[9]).sum() == 8  # the 10th score is shared by 12 candidates


# ---- the default tile, two tiles ----

def test_default_tile_two_tiles():
    rng = np.random.Generator(np.random.PCG64(8192))
    n = TILE + 37
    half = np.arange(1, 11) * 0.5
    cnt = rng.integers(4, 9, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    keys = np.concatenate([np.sort(rng.choice(300, c, replace=False)) for c in cnt]).astype(np.int64) * 11 - 500
    vals = rng.choice(half, keys.size).astype(np.float32)
    M = R.Model(np.arange(n) * 2 + 1, off, keys, vals)
    assert np.bincount((keys + 500) // 11).max() > 64  # posting lists longer than a wave's 64 lanes
    special = [0, TILE - 1, TILE, n - 1]
    rows = np.sort(np.concatenate([special, rng.choice(np.setdiff1d(np.arange(n), special), 28, replace=False)]))
    assert rows.size == 32 and np.unique(rows).size == 32
    ref = np.stack([M.similarities_row(int(r)) for r in rows])
    with _open(M) as t:
        for i, r in enumerate(rows):
            assert R.same_bits(t.exact_similarities(int(M.owner_ids[r]), M.owner_ids), ref[i]).all(), r
        _check_lists(M, t, rows, ref, 100)
        _check_lists(M, t, rows, ref, 512)


# ---- routes ----

def _route_model(kind):
    rng = np.random.Generator(np.random.PCG64(27))
    n, items = 60, 12
    if kind == "tenths":        # 0.1 .. 0.8: s = 27
        pool = [np.float32(0.1 * v) for v in range(1, 9)]
    elif kind == "big":         # one 1e8 among small integers: s = 0
        pool = [np.float32(v) for v in range(1, 6)]
    elif kind == "thirds":      # negative and non-dyadic before rounding: float32 thirds have s = 25
        pool = [np.float32(v) for v in (1 / 3, -1 / 3, 2 / 3, -2 / 3, 1.0, -0.5)]
    else:                       # "no_shift": a 768th beside them needs 33 fractional bits
        pool = [np.float32(v) for v in (1 / 3, -1 / 3, 2 / 3, -1 / 768, 1.0, -0.5)]
    prefs = []
    for r in range(n):
        its = rng.choice(items, int(rng.integers(1, 6)), replace=False)
        prefs.append([(int(i), pool[int(rng.integers(len(pool)))]) for i in its])
    if kind == "tenths":
        for r in range(0, 12):  # owners of 0.1 alone
            prefs[r] = [(k, np.float32(0.1)) for k, _ in prefs[r]]
        prefs[12] = [(k, np.float32(0.8)) for k, _ in prefs[12]]
    if kind == "big":
        prefs[33] = [(1, np.float32(1e8)), (4, np.float32(2.0))]
    prefs[59] = []
    return R.Model.from_lists(prefs, owner_ids=np.arange(n) * 5 - 77)


def _flags(M):
    """(s or None, per-owner U >= 2^53) from numpy and Python integers alone."""
    try:
        s = frac_bits_for(M.vals, 30)
    except ValueError:
        return None, np.ones(M.n, bool)
    units = [int(u) for u in np.ldexp(M.vals.astype(np.float64), s)]
    if any(abs(u) >= 2 ** 31 for u in units):
        return None, np.ones(M.n, bool)
    U = [sum(u * u for u in units[int(M.offsets[r]):int(M.offsets[r + 1])]) for r in range(M.n)]
    return s, np.array([u >= 2 ** 53 for u in U])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["tenths", "big", "thirds", "no_shift"])
def test_routes(kind, weighted):
    M = _route_model(kind)
    s, seq = _flags(M)
    if kind == "tenths":
        assert s == 27 and seq[12] and not seq[:12].any() and 5 < seq.sum() < M.n - 5
    elif kind == "big":
        assert s == 0 and seq.tolist() == [r == 33 for r in range(M.n)]
    elif kind == "thirds":
        assert s == 25 and not seq.any() and (M.vals < 0).any()
    else:
        assert s is None and seq.all()
    with _open(M, weighted, tile=64) as t:
        ref = _check_model(M, t, weighted, ks=(4, M.n + 5))
    if kind in ("thirds", "no_shift"):
        assert (ref[~np.isnan(ref)] < 0).any()  # negative similarities are among them


# ---- state ----

def _small_model(seed, n=20):
    rng = np.random.Generator(np.random.PCG64(seed))
    prefs = [[(int(i), float(rng.integers(1, 6))) for i in rng.choice(15, int(rng.integers(1, 6)), replace=False)]
             for _ in range(n)]
    return R.Model.from_lists(prefs, owner_ids=np.arange(n) * 7 + 3)


def _state_error(fn, code):
    with pytest.raises(_lib.CmsError) as ei:
        fn()
    assert ei.value.code == code


def test_state_and_the_sketch_table_is_left_alone():
    import torch
    A, B = _small_model(1), _small_model(2)
    ids = A.owner_ids
    with SketchTable(A.n, depth=3, width=64, device=0, owner_ids=ids) as t:
        t.ingest_csr(A.offsets, A.keys, A.vals)
        t.finalize()
        before = t.save_device().clone()
        sims_before = t.similarities(int(ids[0]), ids)
        calls = [lambda: t.exact_similarities(int(ids[0]), ids), lambda: t.exact_pairs(ids[:3], ids[3:6]),
                 lambda: t.exact_top_k_rows([0, 1], 3), lambda: t.exact_most_similar(int(ids[0]), 3)]
        for c in calls:
            _state_error(c, _lib.CMS_E_STATE)
        t.attach_exact(A.offsets, A.keys, A.vals)
        _check_model(A, t, False, ks=(3,))
        _state_error(lambda: t.exact_similarities(int(ids[0]) + 1, ids), _lib.CMS_E_NO_SUCH_ID)
        _state_error(lambda: t.exact_similarities(int(ids[0]), [int(ids[1]), 10 ** 9]), _lib.CMS_E_NO_SUCH_ID)
        _state_error(lambda: t.exact_pairs([int(ids[0])], [-5]), _lib.CMS_E_NO_SUCH_ID)
        _state_error(lambda: t.exact_most_similar(-5, 3), _lib.CMS_E_NO_SUCH_ID)
        _state_error(lambda: t.exact_top_k_rows([A.n], 3), _lib.CMS_E_PARAM)
        # refused models: unsorted keys, a key twice -- the attached model stays
        row = next(r for r in range(B.n) if B.offsets[r + 1] - B.offsets[r] >= 2)
        lo = int(B.offsets[row])
        swapped, twice = B.keys.copy(), B.keys.copy()
        swapped[[lo, lo + 1]] = swapped[[lo + 1, lo]]
        twice[lo + 1] = twice[lo]
        for keys in (swapped, twice):
            _state_error(lambda: t.attach_exact(B.offsets, keys, B.vals), _lib.CMS_E_PARAM)
        _check_model(A, t, False, ks=(3,))
        # a second attach replaces the first
        t.attach_exact(B.offsets, B.keys, B.vals)
        _check_model(B, t, False, ks=(3,))
        t.detach_exact()
        for c in calls:
            _state_error(c, _lib.CMS_E_STATE)
        t.detach_exact()  # nothing attached: nothing to do
        assert torch.equal(t.save_device(), before)
        assert R.same_bits(t.similarities(int(ids[0]), ids), sims_before).all()


@pytest.mark.parametrize("kind", ["u32_before_finalize", "f64", "per_owner"])
def test_every_handle_kind(kind):
    A = _small_model(3)
    if kind == "per_owner":
        t = SketchTable.per_owner_shapes(A.n, device=0, owner_ids=A.owner_ids, weighted=True)
    else:
        t = SketchTable(A.n, depth=2, width=40, device=0, owner_ids=A.owner_ids, weighted=True,
                        counters="f64" if kind == "f64" else "u32")
    with t:
        t.attach_exact(A.offsets, A.keys, A.vals)
        _check_model(A, t, True, ks=(4,))


# ---- the reference's own known answers ----

def test_known_answers_of_the_reference():
    kat = GOLDEN["reference_kats"]["VectorSimilarityMeasuresTest.testCosineSimilarity"]
    a, b = kat["a"], kat["b"]
    M = R.Model.from_lists([list(enumerate(a)), list(enumerate(b))])
    with _open(M) as t:
        got = t.exact_similarities(0, [1])[0]
    assert abs(got - kat["cosine"]) < kat["epsilon"]
    assert R.same_bits(got, M.similarity(0, 1)).all()

    kat = GOLDEN["reference_kats"]["ItemSimilarityJobTest.testCompleteJob"]
    users, items, prefs = zip(*[map(int, ln.split(",")) for ln in kat["lines"]])
    item_ids = sorted(set(items))
    by_item = [[(u, float(p)) for u, i, p in zip(users, items, prefs) if i == it] for it in item_ids]
    M = R.Model.from_lists(by_item, owner_ids=np.array(item_ids))
    with _open(M) as t:
        for i1, i2, exp in kat["pairs"]:
            got = t.exact_similarities(i1, [i2])[0]
            assert abs(got - exp) < kat["epsilon"]
            assert R.same_bits(got, M.similarity(item_ids.index(i1), item_ids.index(i2))).all()
