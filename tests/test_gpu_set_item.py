"""GPU: the item-based estimates over the set similarities (cms_set_item_*, k_set_item_estimate) against
tests/set_item_ref.py, float32 bit for bit with NaN matching NaN.  Co-occurrence, Tanimoto and city block are held to
the restated similarities.  Log-likelihood's similarity is only specified to a bound (cms_set.h), so for it the
restatement's loop is fed the values the device's own set_similarities returns for the same pairs: that relies on
cms_set.h's statement that equal (k, n1, n2, num) give equal bits within one build, whichever kernel forms them.
The boolean order model's fp64 sums differ between the orders only in the last bit, which the float32 estimate
does not show; the weighted order model (signed values, a cancelling preference sum) is the one a wrong order fails."""
import functools

import numpy as np
import pytest

import set_item_ref as I
import set_ref as R
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.datamodel import GenericDataModel

pytestmark = pytest.mark.gpu
KINDS = ("weighted", "boolean")
CAP = (1.0, 4.0)


def same(got, exp):
    g, e = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    return bool(((g.view(np.int32) == e.view(np.int32)) | (np.isnan(g) & np.isnan(e))).all())


@functools.lru_cache(maxsize=None)
def _model(n, users=40, rate=0.12):
    """A seeded model of `users` users over n items, every item held, user 3 without and user 5 with one preference:
    (owner IDs, item IDs, offsets, the users' item indices, values in halves from 0.5 to 5.0)."""
    rng = np.random.Generator(np.random.PCG64(n))
    A = rng.random((users, n)) < rate
    A[3] = False
    A[5] = np.arange(n) == n // 2
    for c in np.nonzero(~A.any(axis=0))[0]:
        A[7 + int(c) % (users - 7), c] = True
    lists = [np.nonzero(r)[0] for r in A]
    off = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64)
    return np.arange(users) * 3 - 100, np.arange(n) * 7 + 5, off, lists, rng.integers(1, 11, int(off[-1])) / np.float32(2)


def _attached(oid, kid, off, lists, vals=None):
    t = SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid)
    t.attach_sets(off, kid[np.concatenate(lists)], vals)
    return t


def _expected(t, measure, kind, kid, lists, u, vals, cands, capper=None):
    """The restatement for user u's candidates (item indices); log-likelihood over the device's own similarities."""
    row = (lambda c, ps: t.set_similarities(int(kid[c]), kid[ps], measure, "key").tolist()) \
        if measure == "loglikelihood" else None
    return I.estimates(measure, kind, [x.tolist() for x in lists], lists[u].tolist(), vals, cands, capper, row)


def _batch(t, measure, kind, kid, off, lists, vals, users, cands, capper=None):
    """set_item_estimates_batch for users with the per-user candidate index arrays cands, split per user."""
    po = np.concatenate([[0], np.cumsum([lists[u].size for u in users])])
    co = np.concatenate([[0], np.cumsum([len(c) for c in cands])])
    pv = None if vals is None else np.concatenate([vals[off[u]:off[u + 1]] for u in users])
    got = t.set_item_estimates_batch(po, kid[np.concatenate([lists[u] for u in users])], pv, co,
                                     kid[np.concatenate(cands).astype(np.int64)], measure, kind, capper)
    return np.split(got, co[1:-1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_tile_edges(monkeypatch, n, measure, kind):
    """CMS_SET_EST_TILE=64: one tile short of full, full, two and three tiles; every user a query and every item a
    candidate, the user's own items among them (includeKnownItems), in one launch."""
    monkeypatch.setenv("CMS_SET_EST_TILE", "64")
    oid, kid, off, lists, vals = _model(n)
    capper = CAP if kind == "weighted" else None
    with _attached(oid, kid, off, lists) as t:
        t.set_timing(True, 2)
        got = _batch(t, measure, kind, kid, off, lists, vals, range(oid.size), [np.arange(n)] * oid.size, capper)
        assert t.timing("set_item_estimate")[1] == 1
        for u in range(oid.size):
            uv = vals[off[u]:off[u + 1]]
            assert same(got[u], _expected(t, measure, kind, kid, lists, u, uv, range(n), capper)), (u, got[u])
            if measure == "city_block":  # never NaN: every preferred item is a data point of every candidate
                assert np.isnan(got[u]).all() == (lists[u].size < (2 if kind == "weighted" else 1))
        assert np.isnan(got[3]).all() and (kind == "boolean" or np.isnan(got[5]).all())  # no preference; the count rule


@pytest.mark.parametrize("kind", KINDS)
def test_order_models(kind):
    lists, vals, sizes = I.order_model(kind)
    m, lists = len(sizes), [np.array(x, np.int64) for x in lists]
    oid, kid = np.arange(len(lists), dtype=np.int64), np.arange(m + 1, dtype=np.int64) + 10
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
    av = np.ones(off[-1], np.float32)
    av[:m] = 1.0 if vals is None else vals
    with _attached(oid, kid, off, lists, av) as t:
        got = _batch(t, "tanimoto", kind, kid, off, lists, av, [0], [np.array([m])])[0]
        assert same(got, [I.estimate(kind, [1.0 / s for s in sizes], vals)])
        cnt, items, v = t.set_item_recommend_batch([0], 3, "tanimoto", kind)  # the attached values, the same order
        assert cnt[0] == 1 and items[0, 0] == kid[m] and same(v[0, :1], got)


@pytest.mark.parametrize("kind", KINDS)
def test_default_tile_two_tiles(monkeypatch, kind):
    """The kind's default tile and 65 items more: candidates on both tiles' first and last index, a user whose
    candidates all lie in the second tile (the first holds none and is not launched) and one without candidates."""
    monkeypatch.delenv("CMS_SET_EST_TILE", raising=False)
    T = 2688 if kind == "weighted" else 4096
    n, rng = T + 65, np.random.Generator(np.random.PCG64(T))
    edge = np.array([0, T - 1, T, n - 1])
    lists = [np.union1d(rng.choice(n, 30, replace=False), edge[u % 2::2]) for u in range(6)]
    lists.append(np.setdiff1d(np.arange(n), np.concatenate(lists)))  # every item is held
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
    oid, kid = np.arange(7, dtype=np.int64), np.arange(n, dtype=np.int64) * 3
    vals = rng.integers(1, 11, int(off[-1])) / np.float32(2)
    cands = [np.concatenate([edge, rng.choice(n, 40)]) for _ in range(4)] + [T + np.arange(65), np.zeros(0, int)]
    with _attached(oid, kid, off, lists) as t:
        got = _batch(t, "tanimoto", kind, kid, off, lists, vals, range(6), cands)
        for u in range(6):
            exp = _expected(t, "tanimoto", kind, kid, lists, u, vals[off[u]:off[u + 1]], cands[u].tolist())
            assert same(got[u], exp) and (u == 5 or not np.isnan(got[u]).all()), u


STRATEGIES = {"preferred": taste.PreferredItemsNeighborhoodCandidateItemsStrategy,
              "all_unknown": taste.AllUnknownItemsCandidateItemsStrategy}


@pytest.mark.parametrize("kind,measure", [("weighted", "tanimoto"), ("boolean", "loglikelihood")])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_recommend_batch(strategy, kind, measure):
    """60 users x 150 items, list for list against the restatement around taste's FastIDSet candidates and top items."""
    oid, kid, off, lists, vals = _model(150, 60, 0.05)
    model = GenericDataModel.from_csr(oid, off, kid[np.concatenate(lists)], vals)
    capper = CAP if kind == "weighted" else None
    with _attached(oid, kid, off, lists, vals) as t:
        cnt, items, v = t.set_item_recommend_batch(oid, 10, measure, kind, strategy, False, capper)
        for u in range(oid.size):
            exp = []
            if lists[u].size:
                cands = STRATEGIES[strategy]().doGetCandidateItems(kid[lists[u]], model, False).toList()
                est = _expected(t, measure, kind, kid, lists, u, vals[off[u]:off[u + 1]], [(c - 5) // 7 for c in cands], capper)
                exp = taste.get_top_items(10, cands, est)
            assert [i for i, _ in exp] == items[u, :cnt[u]].tolist() and same(v[u, :cnt[u]], [e for _, e in exp]), u


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("cls", [taste.GenericItemBasedRecommender, taste.GenericBooleanPrefItemBasedRecommender])
def test_the_taste_route(cls, valued):
    """Both recommenders over Tanimoto on a boolean and on a valued model: the device route (one set_item_estimate
    launch per recommend_all) equals the host route the same recommender takes with a bare ItemSimilarity."""
    oid, kid, off, lists, vals = _model(150, 60, 0.05)
    model = GenericDataModel.from_csr(oid, off, kid[np.concatenate(lists)], vals if valued else None)
    sim = taste.TanimotoCoefficientSimilarity(model, 0)
    try:
        class Plain:  # no device capability
            itemSimilarities = sim.itemSimilarities

        sim.table.set_timing(True, 2)
        for known, strat in enumerate(STRATEGIES.values()):
            device = cls(model, sim, strat()).recommend_all(oid, 10, bool(known))
            host = cls(model, Plain(), strat()).recommend_all(oid[::4], 10, bool(known))
            for a, b in zip(device[::4], host):
                assert [i for i, _ in a] == [i for i, _ in b] and same([x for _, x in a], [x for _, x in b])
        assert device[3] == [] and any(device) and sim.table.timing("set_item_estimate")[1] == 2
        one = cls(model, sim).doEstimatePreferences(int(oid[9]), kid[:20])
        assert same(one, cls(model, Plain()).doEstimatePreferences(int(oid[9]), kid[:20])) and not np.isnan(one).all()
    finally:
        sim.close()


def test_unknown_ids_state_and_parameters():
    oid, kid, off, lists, vals = _model(63)

    def refused(fn, code):
        with pytest.raises(_lib.CmsError) as ei:
            fn()
        assert ei.value.code == code

    with SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid) as t:
        est = lambda pi=kid[:2], ci=[4, int(kid[7]), 4], **kw: t.set_item_estimates_batch(  # noqa: E731
            [0, len(pi)], pi, np.ones(len(pi), np.float32), [0, len(ci)], ci, **kw)
        rec = lambda **kw: t.set_item_recommend_batch(oid[:2], 5, **kw)  # noqa: E731
        for c in (est, rec):
            refused(c, _lib.CMS_E_STATE)
        t.attach_sets(off, kid[np.concatenate(lists)])
        for c in (est, rec):
            for bad in ({"measure": 4}, {"measure": -1}, {"kind": 2}):
                refused(lambda: c(**bad), _lib.CMS_E_PARAM)
        refused(lambda: rec(strategy=2), _lib.CMS_E_PARAM)
        refused(lambda: t.set_item_recommend_batch([int(oid[0]) + 1], 5), _lib.CMS_E_NO_SUCH_ID)
        refused(lambda: est(pi=np.array([kid[0], 4])), _lib.CMS_E_NO_SUCH_ID)  # an unknown preferred item
        got = est(measure="city_block", kind="weighted")  # an unknown candidate, twice: NaN; the known one is served
        assert np.isnan(got[[0, 2]]).all() and not np.isnan(got[1])
        assert np.isnan(t.set_item_estimates_batch([0, 0], np.zeros(0, np.int64), None, [0, 1], kid[:1])).all()
