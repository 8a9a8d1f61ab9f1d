"""GPU: the co-rated similarities (cms_common_*) against tests/common_ref.py, bit
for bit, NaN matching NaN, on both sides and both weightings.  Every query is
checked twice: its whole slab row through common_top_k with k past the row
(k_common_tile, or k_common_pairs for a non-eligible query) and through
common_similarities (k_common_pairs alone); the route by the scopes' launches."""
import numpy as np
import pytest

import common_ref as R
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.datamodel import GenericDataModel

pytestmark = pytest.mark.gpu
CASES = [(m, s, w) for m in R.MEASURES for s in ("owner", "key") for w in (False, True)]


def _open(M, weighted=False):
    """A minimal handle, timing on, with M attached (CMS_COMMON_TILE is read when the handle is created)."""
    t = SketchTable(len(M.owner_ids), depth=1, width=32, weighted=weighted, device=0, owner_ids=M.owner_ids)
    t.attach_exact(M.offsets, M.keys, M.vals)
    t.set_timing(True, 2)
    return t


def _check(M, t, measure, side, queries, weighted, launches):
    """The slab rows of `queries` (list indices of the side) by both kernels, and
    the (common_tile, common_pairs) launches that took; returns the restatement's rows."""
    ids = M.ids[side]
    k = min(512, ids.size + 3)
    ref = [M.row(measure, side, q, weighted) for q in queries]
    t.reset_timing()
    got_ids, got_sc, cnt = t.common_top_k(ids[queries], k, measure, side)
    assert (t.timing("common_tile")[1], t.timing("common_pairs")[1]) == launches
    for i, q in enumerate(queries):
        eids, esc = M.top_k(side, q, k, ref[i])
        c = int(cnt[i])
        assert c == eids.size and got_ids[i, :c].tolist() == eids.tolist(), (measure, side, q)
        assert R.same_bits(got_sc[i, :c], esc).all(), (measure, side, q)
        assert (got_ids[i, c:] == -1).all() and np.isnan(got_sc[i, c:]).all()
        assert R.same_bits(t.common_similarities(int(ids[q]), ids, measure, side), ref[i]).all(), (measure, side, q)
    return ref


HALF = [0.5 * v for v in range(-4, 11) if v != 0]
EMPTY, LONG, CONSTANT, SINGLE, ALONE = 5, 6, 7, 8, 9


def _tile_edge_model(n):
    rng = np.random.Generator(np.random.PCG64(n))
    prefs = []
    for r in range(n):
        p = {0: float(rng.choice(HALF))}  # item 0: every owner
        for it in rng.choice(np.arange(3, 69), int(rng.integers(2, 7)), replace=False):
            p[int(it)] = float(rng.choice(HALF))
        prefs.append(p)
    for r in {0, n - 1}:
        prefs[r][1] = 2.5  # item 1: the first and the last owner
    for r in {62, 63, 64} & set(range(n)):
        prefs[r][2] = -1.5  # item 2: around a tile's last cell and the next one's first
    prefs[EMPTY] = {}
    prefs[LONG] = {it: float(rng.choice(HALF)) for it in range(0, 60, 3)}
    prefs[CONSTANT] = {it: 3.0 for it in [0, *range(3, 69)]}  # and every item has an owner
    prefs[SINGLE] = {0: 4.5}
    prefs[ALONE] = {69: 1.0}
    M = R.Model([list(p.items()) for p in prefs], owner_ids=np.arange(n) * 3 - 100)
    assert M.item_keys.tolist() == list(range(70)) and min(M.vals) < 0 and len(prefs[LONG]) == 20
    return M


@pytest.mark.parametrize("measure,side,weighted", CASES)
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_tile_edges(monkeypatch, n, measure, side, weighted):
    """CMS_COMMON_TILE=64 around one and two owner tiles, two item tiles (70 items); see _tile_edge_model."""
    monkeypatch.setenv("CMS_COMMON_TILE", "64")
    M = _tile_edge_model(n)
    owners = sorted({0, n - 1, 62, min(n - 1, 63), min(n - 1, 64), EMPTY, LONG, CONSTANT, SINGLE, ALONE})
    queries = owners if side == "owner" else [0, 1, 2, 63, 64, 69]
    with _open(M, weighted) as t:
        ref = dict(zip(queries, _check(M, t, measure, side, queries, weighted, (1, 0))))  # every list is eligible
    if side == "owner":  # the degenerate pairs are what they claim, by the restatement alone
        assert np.isnan(ref[EMPTY]).all() and np.isnan(np.delete(ref[ALONE], ALONE)).all()
        assert np.isnan(ref[SINGLE][0]) == np.isnan(ref[CONSTANT]).all() == (measure == "pearson")
    else:
        assert np.isnan(ref[69][:69]).all() and not np.isnan(ref[0][1:69]).all()


@pytest.mark.parametrize("measure", R.MEASURES)
def test_default_tile_two_pearson_tiles(monkeypatch, measure):
    monkeypatch.delenv("CMS_COMMON_TILE", raising=False)
    rng = np.random.Generator(np.random.PCG64(1500))
    M = R.Model([[(int(i), float(rng.integers(1, 6))) for i in rng.choice(30, 3, replace=False)] for _ in range(1500)])
    with _open(M) as t:
        _check(M, t, measure, "owner", [0, 1471, 1472, 1499], False, (1, 0))


@pytest.mark.parametrize("measure,side,weighted", CASES)
def test_routes(monkeypatch, measure, side, weighted):
    monkeypatch.setenv("CMS_COMMON_TILE", "64")
    rng = np.random.Generator(np.random.PCG64(51))
    pool = [np.float32(v) for v in (1 / 3, -1 / 3, 2 / 3, -1 / 768, 1.0, -0.5)]  # no shift: 33 fractional bits
    no_shift = R.Model([[(int(i), pool[int(rng.integers(6))]) for i in rng.choice(12, int(rng.integers(1, 6)), replace=False)]
                        for _ in range(40)])
    big = [[(int(i), float(rng.integers(1, 6))) for i in rng.choice(12, int(rng.integers(2, 6)), replace=False)]
           for _ in range(40)]
    big[33] = [(1, 2.0 ** 26), (4, 2.0), (7, 3.0)]  # U = 2^52 + 13 >= 2^51, and item 1's posting list holds it too
    big = R.Model(big)
    assert no_shift.item_keys.tolist() == big.item_keys.tolist() == list(range(12))
    with _open(no_shift, weighted) as t:
        _check(no_shift, t, measure, side, [0, 7, 11], weighted, (0, 1))  # whole rows by the pair kernel
    with _open(big, weighted) as t:
        _check(big, t, measure, side, [2, 5], weighted, (1, 1))  # eligible queries: the tile, then the hot column
        _check(big, t, measure, side, [33 if side == "owner" else 1], weighted, (0, 1))  # the hot query, scored whole


@pytest.mark.parametrize("weighted", [False, True])
def test_pairs_and_the_taste_classes(weighted):
    M = _tile_edge_model(65)
    model = GenericDataModel({int(u): dict(zip(*M.lists["owner"][r])) for r, u in enumerate(M.owner_ids)})
    w = taste.Weighting.WEIGHTED if weighted else taste.Weighting.UNWEIGHTED
    rng = np.random.Generator(np.random.PCG64(3))
    classes = (taste.UncenteredCosineSimilarity, taste.PearsonCorrelationSimilarity, taste.EuclideanDistanceSimilarity)
    for measure, cls in zip(R.MEASURES, classes):
        sim = cls(model, w, device=0)
        try:
            for side, fn in (("owner", sim.userSimilarity), ("key", sim.itemSimilarity)):
                L, ids = M.lists[side], M.ids[side]
                a, b = rng.integers(0, ids.size, 40), rng.integers(0, ids.size, 40)
                exp = [R.similarity(measure, L[i], L[j], M.num[side], weighted) for i, j in zip(a, b)]
                assert R.same_bits(sim.table.common_pairs(ids[a], ids[b], measure, side), exp).all()
                assert all(R.same_bits(fn(int(ids[i]), int(ids[j])), e).all() for i, j, e in zip(a[:8], b[:8], exp))
            row = M.row(measure, "owner", 0, weighted)
            assert sim.mostSimilarUserIDs(int(M.owner_ids[0]), 5).tolist() == M.top_k("owner", 0, 5, row)[0].tolist()
            assert sim.allSimilarItemIDs(3).tolist() == M.item_keys[~np.isnan(M.row(measure, "key", 3, weighted))].tolist()
            with pytest.raises(taste.NoSuchItemException):
                sim.itemSimilarity(3, 10 ** 6)
        finally:
            sim.close()


def test_state_and_parameters():
    M = _tile_edge_model(63)
    ids = M.owner_ids

    def refused(fn, code):
        with pytest.raises(_lib.CmsError) as ei:
            fn()
        assert ei.value.code == code

    with SketchTable(ids.size, depth=1, width=32, device=0, owner_ids=ids) as t:
        calls = [lambda **kw: t.common_similarities(int(ids[0]), ids, **kw),
                 lambda **kw: t.common_pairs(ids[:3], ids[3:6], **kw), lambda **kw: t.common_top_k(ids[:2], 3, **kw)]
        for c in calls:
            refused(c, _lib.CMS_E_STATE)
        t.attach_exact(M.offsets, M.keys, M.vals)
        for c in calls:
            refused(lambda: c(measure=3), _lib.CMS_E_PARAM)
            refused(lambda: c(side=2), _lib.CMS_E_PARAM)
        refused(lambda: t.common_similarities(int(ids[0]) + 1, ids), _lib.CMS_E_NO_SUCH_ID)
        refused(lambda: t.common_pairs([int(ids[0])], [-5]), _lib.CMS_E_NO_SUCH_ID)
        refused(lambda: t.common_top_k([int(ids[0])], 3, side="key"), _lib.CMS_E_NO_SUCH_ID)  # an owner ID is no key
        refused(lambda: t.common_similarities(0, [0, 70], side="key"), _lib.CMS_E_NO_SUCH_ID)
        t.detach_exact()
        for c in calls:
            refused(c, _lib.CMS_E_STATE)
