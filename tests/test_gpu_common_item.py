"""GPU: the item-based estimates over the co-rated similarities (cms_common_item_*, k_common_item_estimate) against
tests/common_item_ref.py, float32 bit for bit with NaN matching NaN: the kernel performs the reference's operations
on identical operands in the same order, so there is no tolerance anywhere."""
import ctypes
import functools

import numpy as np
import pytest

import common_item_ref as CI
import common_ref as C
import set_item_ref as I
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.datamodel import GenericDataModel

pytestmark = pytest.mark.gpu
CAP = (1.0, 4.0)
UNKNOWN = 4  # no item key (7 i + 5)
STRATEGIES = {"preferred": taste.PreferredItemsNeighborhoodCandidateItemsStrategy,
              "all_unknown": taste.AllUnknownItemsCandidateItemsStrategy}
_model = functools.lru_cache(maxsize=None)(CI.model)


@functools.lru_cache(maxsize=None)
def _sims(measure, weighted, *model_args):
    return CI.Sims(measure, _model(*model_args)[0], weighted)


def same(got, exp):
    g, e = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    return bool(((g.view(np.int32) == e.view(np.int32)) | (np.isnan(g) & np.isnan(e))).all())


def _table(m, weighted=False):
    t = SketchTable(m.owner_ids.size, depth=1, width=32, weighted=weighted, device=0, owner_ids=m.owner_ids)
    t.attach_exact(m.offsets, m.keys, m.vals)
    return t


def _batch(t, m, prefs, vals, cand_keys, measure, kind, capper=None):
    """One call for users with the item indices prefs[u] (in order), values vals[u] and candidate keys cand_keys[u]."""
    po = np.concatenate([[0], np.cumsum([len(x) for x in prefs])])
    co = np.concatenate([[0], np.cumsum([len(c) for c in cand_keys])])
    got = t.common_item_estimates_batch(po, m.item_keys[np.concatenate(prefs).astype(np.int64)], np.concatenate(vals), co,
                                        np.concatenate(cand_keys).astype(np.int64), measure, kind, capper)
    return np.split(got, co[1:-1])


def _every_user_every_item(monkeypatch, model_args, measure, kind, capper=None, weighted=False):
    """CMS_COMMON_EST_TILE=64; every user a query and every item a candidate -- the user's own items too -- plus an
    unknown key and, for user 0, a repeated candidate, in one launch; something must come out that is no NaN."""
    monkeypatch.setenv("CMS_COMMON_EST_TILE", "64")
    m, lists, vals = _model(*model_args)
    n, sims = m.item_keys.size, _sims(measure, weighted, *model_args)
    cands = [list(range(n)) + [None] + [3] * (u == 0) for u in range(len(lists))]
    keys = [np.array([UNKNOWN if c is None else m.item_keys[c] for c in cs]) for cs in cands]
    with _table(m, weighted) as t:
        t.set_timing(True, 2)
        got = _batch(t, m, lists, vals, keys, measure, kind, capper)
        assert t.timing("common_item_estimate")[1] == 1
    for u, cs in enumerate(cands):
        assert same(got[u], CI.estimates(sims, kind, lists[u].tolist(), vals[u], cs, capper)), (u, got[u])
    assert np.isnan(got[3]).all() and not np.isnan(np.concatenate(got)).all()  # user 3 has no preference
    return got


@pytest.mark.parametrize("kind", ["weighted", "boolean"])
@pytest.mark.parametrize("measure", C.MEASURES)
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_tile_edges(monkeypatch, n, measure, kind):
    """One tile short of full, full, two and three tiles; the weighted kind under a capper."""
    _every_user_every_item(monkeypatch, (n,), measure, kind, CAP if kind == "weighted" else None)


@pytest.mark.parametrize("measure", ["pearson", "euclidean"])
@pytest.mark.parametrize("variant", [None, "big", "noshift"])
def test_weighting_and_fallbacks(monkeypatch, variant, measure):
    """None: Weighting.WEIGHTED attached.  big: item 21 (U = 2^51) is not eligible, as user 8's and 9's preferred item
    and as everyone's candidate; under Euclidean its similarities are data points, under Pearson its constant ratings
    make them NaN.  noshift: no item is eligible, the whole batch takes the merge join.
    (tests/test_common_item_host.py confirms both models on the CPU.)"""
    got = _every_user_every_item(monkeypatch, (65, 40, 0.12, variant), measure, "weighted", weighted=variant is None)
    assert (variant, measure) != ("big", "euclidean") or not np.isnan([g[21] for g in got]).all()


def test_order():
    """set_item_ref's weighted order model under Euclidean: user 1 alone holds the candidate (at 0.0) and rates
    preferred item i at sizes[i] - 1, so the similarity with item i is 1 / sizes[i] from one common user; user 0's
    values +1, +1, -1, -1 cancel.  The restatement's float32 estimate differs between the two orders; the device
    gives each order its own."""
    _, pv, sizes = I.order_model("weighted")
    k = len(sizes)
    m = C.Model([[(i, pv[i]) for i in range(k)], [(i, sizes[i] - 1.0) for i in range(k)] + [(k, 0.0)]])
    sims, pv, order = CI.Sims("euclidean", m), np.array(pv, np.float32), np.arange(k)
    assert [sims(k, i) for i in range(k)] == [1.0 / s for s in sizes]
    asc, rev = (CI.estimates(sims, "weighted", o.tolist(), pv[o], [k]) for o in (order, order[::-1]))
    assert asc.view(np.int32) != rev.view(np.int32)
    with _table(m) as t:
        for o, exp in ((order, asc), (order[::-1], rev)):
            assert same(_batch(t, m, [o], [pv[o]], [[k]], "euclidean", "weighted")[0], exp)


def test_default_tile_two_tiles(monkeypatch):
    """Pearson weighted at its default tile of 1024 over 1100 items: candidates on both tiles' edges and inside, a
    user whose candidates all lie in the second tile, and one without candidates."""
    monkeypatch.delenv("CMS_COMMON_EST_TILE", raising=False)
    args = (1100, 8, 0.25)
    (m, lists, vals), sims, rng = _model(*args), _sims("pearson", False, *args), np.random.Generator(np.random.PCG64(1))
    cands = [np.concatenate([[0, 1023, 1024, 1099], rng.choice(1100, 20)]), 1024 + np.arange(76), np.zeros(0, int)]
    with _table(m) as t:
        got = _batch(t, m, lists[:3], vals[:3], [m.item_keys[c] for c in cands], "pearson", "weighted")
    for u, c in enumerate(cands):
        assert same(got[u], CI.estimates(sims, "weighted", lists[u].tolist(), vals[u], c.tolist())), u
    assert not np.isnan(got[0]).all() and not np.isnan(got[1]).all()


@functools.lru_cache(maxsize=None)
def _taste():
    """60 users x 150 items as a DataModel, Pearson over it (the device route), and the host route's lists for
    every third user under both strategies: the same recommender over a similarity whose model is an equal but
    distinct object, so servesItemModel is false and every candidate goes through itemSimilarities."""
    m, _, _ = _model(150, 60, 0.15)
    model, twin = (GenericDataModel.from_csr(m.owner_ids, m.offsets, m.keys, m.vals) for _ in range(2))
    sim, other = taste.PearsonCorrelationSimilarity(model, device=0), taste.PearsonCorrelationSimilarity(twin, device=0)
    host = {s: taste.GenericItemBasedRecommender(model, other, STRATEGIES[s]()).recommend_all(m.owner_ids[::3], 10)
            for s in STRATEGIES}
    other.close()
    return m, model, sim, host


def _same_lists(device, host):
    return len(device) == len(host) and all(
        [i for i, _ in a] == [i for i, _ in b] and same([x for _, x in a], [x for _, x in b]) for a, b in zip(device, host))


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_recommend_batch(strategy):
    m, model, sim, host = _taste()
    cnt, items, v = sim.table.common_item_recommend_batch(m.owner_ids, 10, "pearson", "weighted", strategy, False,
                                                          taste.build_capper(model))
    device = [list(zip(items[u, :cnt[u]].tolist(), v[u, :cnt[u]])) for u in range(cnt.size)]
    assert _same_lists(device[::3], host[strategy]) and device[3] == [] and any(device)


def test_the_taste_route():
    m, model, sim, host = _taste()
    sim.table.set_timing(True, 2)
    sim.table.reset_timing()
    device = taste.GenericItemBasedRecommender(model, sim).recommend_all(m.owner_ids, 10)
    assert sim.table.timing("common_item_estimate")[1] == 1
    assert _same_lists(device[::3], host["preferred"]) and any(device)


def test_unknown_ids_state_and_parameters():
    m, lists, vals = _model(63)
    kid, mine = m.item_keys, m.item_keys[lists[0][:3]]  # user 0 holds all three: their Euclidean similarities are no NaN

    def refused(fn, code):
        with pytest.raises(_lib.CmsError) as ei:
            fn()
        assert ei.value.code == code

    with SketchTable(m.owner_ids.size, depth=1, width=32, device=0, owner_ids=m.owner_ids) as t:
        est = lambda pi=mine[:2], ci=(UNKNOWN, int(mine[2]), UNKNOWN), **kw: t.common_item_estimates_batch(  # noqa: E731
            [0, len(pi)], pi, np.ones(len(pi), np.float32), [0, len(ci)], ci, **kw)
        rec = lambda **kw: t.common_item_recommend_batch(m.owner_ids[:2], 5, **kw)  # noqa: E731
        for c in (est, rec):
            refused(c, _lib.CMS_E_STATE)
        t.attach_exact(m.offsets, m.keys, m.vals)
        for c in (est, rec):
            for bad in ({"measure": 3}, {"measure": -1}, {"kind": 2}):
                refused(lambda: c(**bad), _lib.CMS_E_PARAM)
        refused(lambda: rec(strategy=2), _lib.CMS_E_PARAM)
        refused(lambda: t.common_item_recommend_batch([int(m.owner_ids[0]) + 1], 5), _lib.CMS_E_NO_SUCH_ID)
        refused(lambda: est(pi=np.array([kid[0], UNKNOWN])), _lib.CMS_E_NO_SUCH_ID)
        # an unknown preferred item, through the C interface: nothing is written
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        off, pi, pv, out = np.array([0, 2]), np.array([kid[0], UNKNOWN]), np.ones(2, np.float32), np.full(2, 7.0, np.float32)
        assert t._lib.cms_common_item_estimates_batch(t._h, 1, 0, 1, p(off), p(pi), p(pv), p(off), p(kid[:2].copy()), 0,
                                                      0.0, 0.0, p(out)) == _lib.CMS_E_NO_SUCH_ID and (out == 7.0).all()
        got = est(measure="euclidean", kind="boolean")  # an unknown candidate, twice: NaN; the known one is served
        assert np.isnan(got[[0, 2]]).all() and not np.isnan(got[1])
