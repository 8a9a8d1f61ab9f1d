"""GPU: the set similarities (cms_set_*) against tests/set_ref.py on both sides (R.agrees: the same bits, or
log-likelihood's bound).  A query's slab row comes back through set_top_k with k the number of lists (k_set_tile)
and is held against set_similarities and set_pairs (k_set_pairs) bit for bit, in the order numpy gives on that row."""
import functools

import numpy as np
import pytest

import set_ref as R
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.datamodel import GenericDataModel

pytestmark = pytest.mark.gpu
bits = lambda a: np.asarray(a, np.float64).view(np.int64)  # noqa: E731


@functools.lru_cache(maxsize=None)
def _model(n, side, other=40):
    """A seeded boolean model with n lists on `side` and `other` on the other face, owners 3 and 5 empty, every
    key held; (owner IDs, key IDs, offsets, keys) and per side (IDs, the lists as sets, num)."""
    rows, cols = (n, other) if side == "owner" else (other, n)
    rng = np.random.Generator(np.random.PCG64(n))
    A = rng.random((rows, cols)) < 0.12
    A[[3, 5]] = False
    for c in np.nonzero(~A.any(axis=0))[0]:
        A[7 + int(c) % (rows - 7), c] = True
    oid, kid = np.arange(rows) * 3 - 100, np.arange(cols) * 7 + 5
    off = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64)
    faces = {"owner": (oid, [frozenset(np.nonzero(r)[0]) for r in A], cols),
             "key": (kid, [frozenset(np.nonzero(c)[0]) for c in A.T], rows)}
    return oid, kid, off, kid[np.nonzero(A)[1]], faces


def _expected(measure, face, side, qs, cs):
    _, L, num = face
    return [[R.similarity(measure, L[q], L[c], num, side) for c in cs] for q in qs]


def _check_rows(t, measure, face, side, queries, k):
    """set_top_k of `queries` against the device's own set_similarities rows, and those against the restatement."""
    ids, L, _ = face
    got_ids, got_sc, cnt = t.set_top_k(ids[queries], k, measure, side)
    for i, q in enumerate(queries):
        row = t.set_similarities(int(ids[q]), ids, measure, side)
        exp = _expected(measure, face, side, [q], range(len(L)))[0]
        assert all(R.agrees(measure, g, e, S) for g, (e, S) in zip(row, exp)), (measure, side, q)
        keep = np.nonzero(~np.isnan(row) & (np.arange(ids.size) != q))[0]
        order = keep[np.lexsort((ids[keep], -row[keep]))][:k]  # score descending, then ID ascending
        c = int(cnt[i])
        assert c == order.size and got_ids[i, :c].tolist() == ids[order].tolist(), (measure, side, q)
        assert (bits(got_sc[i, :c]) == bits(row[order])).all(), (measure, side, q)
        assert (got_ids[i, c:] == -1).all() and np.isnan(got_sc[i, c:]).all()
    return got_ids, cnt


@pytest.mark.parametrize("side", ["owner", "key"])
@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_tile_edges(monkeypatch, n, measure, side):
    """CMS_SET_TILE=64: one tile short of full, full, two and three tiles; 40 lists on the other face."""
    monkeypatch.setenv("CMS_SET_TILE", "64")
    oid, _, off, keys, faces = _model(n, side)
    ids = faces[side][0]
    with SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid) as t:
        t.attach_sets(off, keys)
        t.set_timing(True, 2)
        _, cnt = _check_rows(t, measure, faces[side], side, list(range(n)), n)
        assert t.timing("set_tile")[1] == 1 and t.timing("set_pairs")[1] == n  # the slab once; a row per query
        assert measure != "city_block" or (cnt == n - 1).all()  # never NaN: every other list is ranked
        pairs = t.set_pairs(np.repeat(ids, n), np.tile(ids, n), measure, side).reshape(n, n)
        for q in (0, 3, 62, n - 1):  # elementwise and one-against-many: the same kernel, the same bits
            assert (bits(pairs[q]) == bits(t.set_similarities(int(ids[q]), ids, measure, side))).all()


@pytest.mark.parametrize("measure", ["cooccurrence", "tanimoto"])
def test_default_tile_two_tiles(monkeypatch, measure):
    """16384 + 65 owners of two or three items: owner 0 and every second owner of the second tile hold {0, 1, 2}."""
    monkeypatch.delenv("CMS_SET_TILE", raising=False)
    n, rng = 16384 + 65, np.random.Generator(np.random.PCG64(16384))
    lists = [np.sort(rng.choice(50, int(rng.integers(2, 4)), replace=False)) for _ in range(n)]
    for r in [0, *range(16384, n, 2)]:
        lists[r] = np.arange(3)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    oid = np.arange(n, dtype=np.int64)
    face = (oid, [frozenset(x.tolist()) for x in lists], 50)
    with SketchTable(n, depth=1, width=32, device=0, owner_ids=oid) as t:
        t.attach_sets(off, np.concatenate(lists))
        got_ids, _ = _check_rows(t, measure, face, "owner", [0, 16383, 16384, 16385, n - 1], 512)
        assert (got_ids[0] >= 16384).sum() >= 32 and (got_ids[2] < 16384).any()  # both tiles reach the lists


@pytest.mark.parametrize("measure", R.MEASURES)
def test_degenerate_pairs(measure):
    """The host test's designed pairs as owners of one model (keys 0..59), through set_pairs and set_similarities."""
    names = sorted(R.DESIGNED)
    lists = [sorted(R.DESIGNED[nm][i]) for nm in names for i in (0, 1)] + [list(range(60))]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    oid = np.arange(len(lists), dtype=np.int64) + 10
    with SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid) as t:
        t.attach_sets(off, np.concatenate([np.asarray(x, np.int64) for x in lists]))
        a, b = oid[0:-1:2], oid[1:-1:2]
        for x, y in ((a, b), (b, a)):
            got = t.set_pairs(x, y, measure, "owner")
            exp = [R.similarity(measure, lists[i - 10], lists[j - 10], 60) for i, j in zip(x, y)]
            assert all(R.agrees(measure, g, e, S) for g, (e, S) in zip(got, exp)), (got, exp)
        both = names.index("both_empty") * 2 + 10
        assert np.isnan(t.set_similarities(both, [both + 1], measure)[0]) == (measure != "city_block")


def test_the_taste_classes_on_a_boolean_and_a_valued_model():
    oid, kid, off, keys, faces = _model(65, "owner")
    boolean = GenericDataModel.from_csr(oid, off, keys, None)
    valued = GenericDataModel.from_csr(oid, off, keys, np.full(keys.size, 2.5, np.float32))
    classes = {"tanimoto": taste.TanimotoCoefficientSimilarity, "loglikelihood": taste.LogLikelihoodSimilarity,
               "city_block": taste.CityBlockSimilarity}
    for (measure, cls), model in zip(classes.items(), (boolean, valued, boolean)):
        sim = cls(model, device=0)
        try:
            for side, one, many in (("owner", sim.userSimilarity, sim.userSimilarities),
                                    ("key", sim.itemSimilarity, sim.itemSimilarities)):
                ids = faces[side][0]
                row = many(int(ids[9]), ids)
                exp = _expected(measure, faces[side], side, [9], range(ids.size))[0]
                assert all(R.agrees(measure, g, e, S) for g, (e, S) in zip(row, exp))
                assert bits(one(int(ids[9]), int(ids[11]))) == bits(row[11])
            row = sim.userSimilarities(int(oid[9]), oid)
            keep = np.nonzero(~np.isnan(row) & (oid != oid[9]))[0]
            top5 = oid[keep[np.lexsort((oid[keep], -row[keep]))][:5]].tolist()
            hood = taste.NearestNUserNeighborhood(5, sim, model)
            assert sim.mostSimilarUserIDs(int(oid[9]), 5).tolist() == hood.getUserNeighborhood(int(oid[9])).tolist() == top5
            o, nb = hood.getUserNeighborhoods(oid[[9, 3]])  # owner 3 is empty: NaN by log-likelihood alone
            assert nb[:o[1]].tolist() == top5 and o[2] - o[1] == (0 if measure == "loglikelihood" else 5)
            similar = sim.allSimilarItemIDs(int(kid[2]))
            assert similar.tolist() == kid[~np.isnan(sim.itemSimilarities(int(kid[2]), kid))].tolist() and similar.size
            sim.refresh()
            assert bits(sim.userSimilarity(int(oid[9]), int(oid[11]))) == bits(row[11])
            for refused, call in ((NotImplementedError, lambda: sim.setPreferenceInferrer(object())),
                                  (NotImplementedError, lambda: sim.estimatePreferences(int(oid[9]), top5, kid[:3])),
                                  (taste.NoSuchItemException, lambda: sim.itemSimilarity(int(kid[2]), 10 ** 6))):
                pytest.raises(refused, call)
        finally:
            sim.close()


def test_state_and_parameters():
    oid, kid, off, keys, _ = _model(63, "owner")

    def refused(fn, code):
        with pytest.raises(_lib.CmsError) as ei:
            fn()
        assert ei.value.code == code

    with SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid) as t:
        calls = [lambda **kw: t.set_similarities(int(oid[0]), oid, **kw),
                 lambda **kw: t.set_pairs(oid[:3], oid[3:6], **kw), lambda **kw: t.set_top_k(oid[:2], 3, **kw)]
        for c in calls:
            refused(c, _lib.CMS_E_STATE)
        t.attach_sets(off, keys)
        for c in calls:
            for bad in ({"measure": 4}, {"measure": -1}, {"side": 2}):
                refused(lambda: c(**bad), _lib.CMS_E_PARAM)
        refused(lambda: t.set_similarities(int(oid[0]) + 1, oid), _lib.CMS_E_NO_SUCH_ID)
        refused(lambda: t.set_pairs([int(oid[0])], [-5]), _lib.CMS_E_NO_SUCH_ID)
        refused(lambda: t.set_top_k([int(oid[0])], 3, side="key"), _lib.CMS_E_NO_SUCH_ID)  # an owner ID is no key
        refused(lambda: t.set_similarities(int(kid[0]), [int(kid[1]), 4], side="key"), _lib.CMS_E_NO_SUCH_ID)
        t.detach_exact()
        for c in calls:
            refused(c, _lib.CMS_E_STATE)
