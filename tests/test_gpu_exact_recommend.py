"""GPU: GenericUserBasedRecommender over the exact CosineSimilarity
(cms_exact.hip k_exact_estimate: cms_exact_estimate_preferences_batch,
cms_exact_recommend_batch; taste.GenericUserBasedRecommender over a
taste.CosineSimilarity; accuracy.recommendation_accuracy) against the
plain-Python restatement of the sim == null branch (tests/exact_rec_ref.py).
Bit for bit, NaN matching NaN; no tolerance anywhere.

  tile edges     CMS_EXACT_EST_TILE=64, 40 users over 200 items, values 0.1 .. 0.8:
                 63, 64, 65 and 136 candidates in shuffled order, candidates on a
                 tile's first and last slot held by a neighbour, neighbour lists that
                 begin before the candidates and end after them, neighbourhoods of 1,
                 2 and 17 in non-ascending order; unweighted and weighted; the batch
                 of all cases equals the single calls
  semantics      the user in its own neighbourhood, an empty neighbour and an all-0.0
                 neighbour (NaN similarity), one and two data points, the 0.0 data
                 point, totalSimilarity 0.0 (+-inf) with and without the capper, an
                 order that changes the bits, unknown / repeated / own candidate keys,
                 an empty neighbourhood, models with non-eligible rows
  default tile   2,200 items, a user with more than 2048 candidates: batch == single
  recommend      120 users x 200 items, n = 10: exact_recommend_batch list for list,
                 with and without the known items; the Taste route's recommend_all ==
                 recommend per user == the table call
  state          CMS_E_STATE without a model, NoSuchUserException with nothing
                 written, the sketch table's image and a CosineCM recommender's
                 outputs unchanged
  two paths meet the collision-free construction of test_gpu_sketch_accuracy.py: the
                 sketch branch and the exact branch agree bit for bit
  report fields  at (2, 32) every field of recommendation_accuracy from a numpy
                 recomputation; at least one list or estimate differs
"""
import os

import numpy as np
import pytest

import exact_rec_ref as X
import exact_ref as R
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.accuracy import recommendation_accuracy
from mahout_amd.datamodel import GenericDataModel, NoSuchUserException
from mahout_amd.sketch import frac_bits_for

pytestmark = pytest.mark.gpu

SEED = 42


def _open(M, weighted=False, tile=None, **kw):
    """A minimal handle (its sketch table is never ingested) with M attached.
    CMS_EXACT_EST_TILE is read when the handle is created."""
    old = os.environ.get("CMS_EXACT_EST_TILE")
    try:
        if tile is not None:
            os.environ["CMS_EXACT_EST_TILE"] = str(tile)
        t = SketchTable(M.n, depth=1, width=32, weighted=weighted, device=0, owner_ids=M.owner_ids, **kw)
    finally:
        if tile is not None:
            if old is None:
                del os.environ["CMS_EXACT_EST_TILE"]
            else:
                os.environ["CMS_EXACT_EST_TILE"] = old
    t.attach_exact(M.offsets, M.keys, M.vals)
    return t


def _check(M, t, user, nb, items, weighted=False, capper=None):
    """The single call for owner ROW user, neighbour ROWS nb and item KEYS
    items against the restatement; returns the estimates."""
    got = t.exact_estimate_preferences(int(M.owner_ids[user]), M.owner_ids[np.asarray(nb, np.int64)], items, capper)
    ref = X.estimates(M, user, nb, items, weighted, capper)
    bad = np.nonzero(~X.same_bits32(got, ref))[0]
    assert bad.size == 0, (user, list(nb), [(int(items[i]), got[i], ref[i]) for i in bad[:5]])
    return got


def _batch(M, t, cases, capper=None):
    """One batch call of cases = [(user row, neighbour rows, item keys)]: the list of per-case estimates."""
    nbo = np.zeros(len(cases) + 1, np.int64)
    ito = np.zeros(len(cases) + 1, np.int64)
    np.cumsum([len(c[1]) for c in cases], out=nbo[1:])
    np.cumsum([len(c[2]) for c in cases], out=ito[1:])
    nb = np.concatenate([M.owner_ids[np.asarray(c[1], np.int64)] for c in cases] + [np.zeros(0, np.int64)])
    it = np.concatenate([np.asarray(c[2], np.int64) for c in cases] + [np.zeros(0, np.int64)])
    out = t.exact_estimate_preferences_batch(M.owner_ids[[c[0] for c in cases]], nbo, nb, ito, it, capper)
    return [out[ito[i]:ito[i + 1]] for i in range(len(cases))]


# ---- tile edges ----

KEY = lambda item: int(item) * 7 - 300  # noqa: E731  (item keys are not the dense indices)


def _tile_edge_model():
    rng = np.random.Generator(np.random.PCG64(2048))
    n, items = 40, 200
    pool = [np.float32(0.1 * v) for v in range(1, 9)]
    prefs = []
    for r in range(n):
        held = np.arange(items) if r in (3, 4) else rng.choice(items, int(rng.integers(50, 90)), replace=False)
        prefs.append([(KEY(i), pool[int(rng.integers(8))]) for i in held])  # rows 3 and 4 hold every item
    M = R.Model.from_lists(prefs, owner_ids=np.arange(n) * 3 - 50)
    assert frac_bits_for(M.vals) == 27
    return M


def _tile_edge_cases(M):
    rng = np.random.Generator(np.random.PCG64(65))
    cases = []
    for c in (63, 64, 65, 136):
        cand = np.sort(rng.choice(np.arange(20, 180), c, replace=False))  # dense indices == item numbers here
        shuffled = np.array([KEY(i) for i in rng.permutation(cand)], np.int64)
        for user, nb in ((0, [3]), (1, [4, 3]), (2, [39, 4, 30, 3, 25, 21, 38, 17, 16, 11, 12, 9, 7, 8, 5, 2, 6])):
            assert len(nb) in (1, 2, 17) and nb != sorted(nb) or len(nb) == 1
            for r in nb:  # every list begins before the candidates and ends after them
                keys = M.row(r)[0]
                assert keys[0] < KEY(cand[0]) and keys[-1] > KEY(cand[-1])
            cases.append((user, nb, shuffled))
    return cases


@pytest.fixture(scope="module")
def tile_edge_model():
    M = _tile_edge_model()
    assert np.unique(M.keys).size == 200  # dense index == item number
    return M, _tile_edge_cases(M)


@pytest.mark.parametrize("weighted", [False, True])
def test_tile_edges(tile_edge_model, weighted):
    M, cases = tile_edge_model
    with _open(M, weighted, tile=64) as t:
        singles = [_check(M, t, u, nb, items, weighted) for u, nb, items in cases]
        for (u, nb, items), est in zip(cases, singles):
            if len(nb) == 1:
                assert np.isnan(est).all()  # one neighbour: never two data points
            else:  # rows 3 and 4 hold every item: the first and last slot of every tile carry a value
                by_item = est[np.argsort(items)]
                edges = [e for e in (0, 63, 64, 127, 128, items.size - 1) if e < items.size]
                assert not np.isnan(by_item[edges]).any()
        for got, est in zip(_batch(M, t, cases), singles):
            assert X.same_bits32(got, est).all()
        capped = _check(M, t, 2, cases[2][1], cases[2][2], weighted, capper=(0.4, 0.5))
        assert capped.min() == np.float32(0.4) and capped.max() == np.float32(0.5)


# ---- semantics ----

def _semantics_model():
    a = [(0, 1.0), (1, 1.0), (7, 2.0), (8, -1.0)]
    return R.Model.from_lists([
        [(0, 1.0), (1, 2.0), (2, 0.5)],               # 0: the user
        [(0, 1.0), (1, 1.0), (5, 4.0), (6, 1.0)],     # 1
        [(0, 2.0), (1, 1.0), (5, 0.0), (6, 2.0)],     # 2: holds item 5 with 0.0
        [(0, 2.0), (1, 3.0), (6, 3.0)],               # 3: lacks item 5
        [],                                           # 4: no preference: NaN similarity
        [(0, 0.0), (1, 0.0), (5, 0.0)],               # 5: every value 0.0: NaN similarity
        a, [(k, -v) for k, v in a],                   # 6, 7: similarities s and -s: totalSimilarity 0.0
    ], owner_ids=[10, 20, 30, 40, 50, 60, 70, 80])


@pytest.mark.parametrize("weighted", [False, True])
def test_semantics(weighted):
    M = _semantics_model()
    sims = M.similarities_row(0, weighted)
    assert np.isnan(sims[4]) and np.isnan(sims[5]) and sims[6] == -sims[7] and sims[6] > 0
    with _open(M, weighted, tile=64) as t:
        five = np.array([5], np.int64)
        own = _check(M, t, 0, [0, 1, 2, 0], five, weighted)             # the user in its own neighbourhood
        assert X.same_bits32(own, _check(M, t, 0, [1, 2], five, weighted)).all() and not np.isnan(own[0])
        assert np.isnan(_check(M, t, 0, [1, 3], five, weighted)[0])     # exactly one data point
        assert np.isnan(_check(M, t, 0, [1, 4], five, weighted)[0])     # ... beside an empty neighbour
        assert np.isnan(_check(M, t, 0, [1, 5], five, weighted)[0])     # ... beside an all-0.0 neighbour
        two = _check(M, t, 0, [4, 1, 5, 2], five, weighted)[0]          # two: the second is the 0.0 of row 2
        assert two == np.float32(sims[1] * 4.0 / (sims[1] + sims[2]))
        assert _check(M, t, 0, [1, 1], five, weighted)[0] == np.float32(4.0)  # a neighbour named twice counts twice
        inf = _check(M, t, 0, [6, 7], [7, 8], weighted)                 # totalSimilarity 0.0
        assert np.isposinf(inf[0]) and np.isneginf(inf[1])
        assert _check(M, t, 0, [6, 7], [7, 8], weighted, capper=(0.5, 5.0)).tolist() == [5.0, 0.5]
        # unknown, repeated and own candidate keys, in the caller's order
        keys = np.array([6, 999, 5, 6, 0, -4, 5, 2, 6], np.int64)
        got = _check(M, t, 0, [3, 2, 1], keys, weighted, capper=(0.0, 5.0))
        assert np.isnan(got[[1, 5, 7]]).all() and not np.isnan(got[[0, 2, 4]]).any()
        assert got[0] == got[3] == got[8] and got[2] == got[6]
        # an empty neighbourhood, and no candidate at all
        assert np.isnan(t.exact_estimate_preferences(10, [], keys)).all()
        assert t.exact_estimate_preferences(10, [20, 30], []).size == 0
        assert t.exact_estimate_preferences_batch([], [0], [], [0], []).size == 0


def test_order_of_the_neighbourhood_decides_the_bits():
    M = X.order_model()  # asserted on the host: the orders below differ in the restatement
    with _open(M, tile=64) as t:
        e = [_check(M, t, 0, nb, [9])[0] for nb in ([1, 2, 3, 4], [1, 3, 4, 2], [2, 3, 4, 1])]
    assert np.isposinf(e[0]) and e[1] > 1e15 and e[2] < -1e15


def _route_model(kind):
    rng = np.random.Generator(np.random.PCG64(30))
    n, items = 30, 12
    if kind == "big":   # s = 0; the owner of a 1e8 value is past 2^53
        pool = [np.float32(v) for v in range(1, 6)]
    else:               # a 768th needs 33 fractional bits: no s, every row is non-eligible
        pool = [np.float32(v) for v in (1 / 3, -1 / 3, 2 / 3, -1 / 768, 1.0, -0.5)]
    prefs = [[(int(i), pool[int(rng.integers(len(pool)))]) for i in rng.choice(items, int(rng.integers(3, 9)), replace=False)]
             for _ in range(n)]
    if kind == "big":
        prefs[7] = [(1, np.float32(1e8)), (4, np.float32(2.0)), (6, np.float32(3.0))]
    return R.Model.from_lists(prefs, owner_ids=np.arange(n) * 5 - 77)


@pytest.mark.parametrize("kind", ["no_shift", "big"])
def test_models_with_non_eligible_rows(kind):
    M = _route_model(kind)
    try:
        s = frac_bits_for(M.vals, 30)
    except ValueError:
        s = None
    assert (s is None) == (kind == "no_shift")
    if kind == "big":
        units = np.ldexp(M.vals.astype(np.float64), s)[int(M.offsets[7]):int(M.offsets[8])]
        assert float((units * units).sum()) >= 2.0 ** 53
    keys = np.arange(12)
    with _open(M, tile=64) as t:
        cases = []
        for u in range(M.n):
            nb = X.neighborhood(M, u, 6)
            if kind == "big" and u != 7 and 7 not in nb:
                nb = np.concatenate([nb[:3], [7], nb[3:]])  # the non-eligible row among the neighbours
            cases.append((u, nb, keys))
        singles = [_check(M, t, u, nb, items) for u, nb, items in cases]
        assert sum(int((~np.isnan(e)).sum()) for e in singles) > M.n
        for got, est in zip(_batch(M, t, cases), singles):
            assert X.same_bits32(got, est).all()


# ---- the default tile: a user with more than 2048 candidates ----

def test_default_tile_batch_equals_single():
    rng = np.random.Generator(np.random.PCG64(2200))
    items, n = 2200, 6
    pool = [np.float32(0.5 * v) for v in range(1, 11)]
    prefs = []
    for r in range(n):
        held = rng.choice(items, 40 if r == 0 else 1500, replace=False)
        prefs.append([(int(i) * 3 + 1, pool[int(rng.integers(10))]) for i in held])
    M = R.Model.from_lists(prefs, owner_ids=np.arange(n) + 100)
    cases = []
    for u in range(n):  # user 0: every candidate of recommend(); the others: a sample, some keys unknown
        nb = [r for r in (5, 3, 4, 1, 2, 0) if r != u]
        cand = X.all_other_items(M, u, nb) if u == 0 else rng.choice(items * 3 + 9, 100, replace=False)
        cases.append((u, nb, np.array(cand, np.int64)))
    assert cases[0][2].size > 2048  # two tiles for user 0
    with _open(M) as t:
        singles = [_check(M, t, u, nb, it) for u, nb, it in cases]
        assert (~np.isnan(singles[0])).sum() > 2048
        for got, est in zip(_batch(M, t, cases), singles):
            assert X.same_bits32(got, est).all()


# ---- recommend ----

N_NB, HOW_MANY = 10, 10


@pytest.fixture(scope="module")
def rec_model():
    rng = np.random.Generator(np.random.PCG64(120))
    n, items = 120, 200
    pool = [np.float32(0.5 * v) for v in range(1, 11)]  # half stars: many tied estimates
    prefs = [[(int(i) * 11 - 500, pool[int(rng.integers(10))])
              for i in rng.choice(items, int(rng.integers(8, 30)), replace=False)] for _ in range(n)]
    prefs[17] = []  # no preference: an empty neighbourhood, nothing recommended
    M = R.Model.from_lists(prefs, owner_ids=np.arange(n) * 13 - 400)
    capper = (float(M.vals.min()), float(M.vals.max()))
    nbs = [X.neighborhood(M, u, N_NB) for u in range(n)]
    lists = {known: [X.recommend(M, u, nbs[u], HOW_MANY, include_known=known, capper=capper) for u in range(n)]
             for known in (False, True)}
    return M, capper, nbs, lists


def _as_lists(cnt, items, vals):
    return [[(int(items[u, j]), vals[u, j]) for j in range(int(cnt[u]))] for u in range(cnt.size)]


def _same_lists(a, b):
    return len(a) == len(b) and all(
        [i for i, _ in x] == [i for i, _ in y] and X.same_bits32([v for _, v in x], [v for _, v in y]).all()
        for x, y in zip(a, b))


def _flat(M, nbs):
    off = np.zeros(len(nbs) + 1, np.int64)
    np.cumsum([len(x) for x in nbs], out=off[1:])
    return off, M.owner_ids[np.concatenate(nbs).astype(np.int64)]


@pytest.mark.parametrize("known", [False, True])
def test_recommend_batch_is_the_reference_list_for_list(rec_model, known):
    M, capper, nbs, lists = rec_model
    off, nb = _flat(M, nbs)
    with _open(M) as t:
        got = _as_lists(*t.exact_recommend_batch(M.owner_ids, off, nb, HOW_MANY, known, capper))
    for u in range(M.n):
        assert _same_lists([got[u]], [lists[known][u]]), (u, got[u], lists[known][u])
    assert got[17] == [] and sum(len(x) == HOW_MANY for x in got) > M.n // 2
    values = np.concatenate([[v for _, v in x] for x in got if x])
    assert np.unique(values).size < values.size  # tied values are among them


def test_taste_route(rec_model):
    M, capper, nbs, lists = rec_model
    dm = GenericDataModel.from_csr(M.owner_ids, M.offsets, M.keys, M.vals)
    sim = taste.CosineSimilarity(dm, device=0)
    try:
        nbh = taste.NearestNUserNeighborhood(N_NB, sim, dm)
        rec = taste.GenericUserBasedRecommender(dm, nbh, sim)
        off, nb = nbh.getUserNeighborhoods(M.owner_ids)
        assert (off.tolist(), nb.tolist()) == tuple(x.tolist() for x in _flat(M, nbs))
        for known in (False, True):
            every = rec.recommend_all(M.owner_ids, HOW_MANY, known)
            assert _same_lists(every, lists[known])
            assert _same_lists(every, _as_lists(*sim.table.exact_recommend_batch(M.owner_ids, off, nb, HOW_MANY, known,
                                                                                  capper)))
            for u in range(0, M.n, 3 if known else 1):
                assert _same_lists([rec.recommend(int(M.owner_ids[u]), HOW_MANY, known)], [every[u]]), u
        # estimatePreference: the user's own value, else the estimate
        u = 5
        own_key, own_val = M.row(u)[0][0], M.row(u)[1][0]
        assert rec.estimatePreference(int(M.owner_ids[u]), int(own_key)) == own_val
        other = next(i for i, _ in lists[False][u])
        assert X.same_bits32(rec.estimatePreference(int(M.owner_ids[u]), other),
                             X.estimates(M, u, nbs[u], [other], capper=capper)).all()
        with pytest.raises(NoSuchUserException):
            rec.recommend_all([int(M.owner_ids[0]), 12345], HOW_MANY)
        with pytest.raises(NoSuchUserException):
            rec.doEstimatePreferences(int(M.owner_ids[0]), [12345], [other])
    finally:
        sim.close()


# ---- state ----

def _code(fn):
    with pytest.raises(_lib.CmsError) as ei:
        fn()
    return ei.value.code


def test_state_and_nothing_else_is_touched(rec_model):
    import ctypes
    import torch
    M, capper, nbs, lists = rec_model
    ids = M.owner_ids
    off, nb = _flat(M, nbs)
    dm = GenericDataModel.from_csr(ids, M.offsets, M.keys, M.vals)
    cm = taste.CosineCM(dm, taste.FixedShapeConfig(3, 64), taste.HashFunctionBuilder(SEED), device=0)
    try:
        t = cm.table
        cm_rec = taste.GenericUserBasedRecommender(dm, taste.NearestNUserNeighborhood(N_NB, cm, dm), cm)
        before = t.save_device().clone()
        lists_before = cm_rec.recommend_all(ids, HOW_MANY)
        est_before = cm_rec.doEstimatePreferences(int(ids[0]), ids[nbs[0]], M.keys[:50])
        calls = [lambda: t.exact_estimate_preferences(int(ids[0]), ids[1:4], M.keys[:5]),
                 lambda: t.exact_estimate_preferences_batch(ids[:2], [0, 1, 2], ids[2:4], [0, 1, 2], M.keys[:2]),
                 lambda: t.exact_recommend_batch(ids, off, nb, HOW_MANY)]
        for c in calls:
            assert _code(c) == _lib.CMS_E_STATE
        t.attach_exact(M.offsets, M.keys, M.vals)
        got = _as_lists(*t.exact_recommend_batch(ids, off, nb, HOW_MANY, False, capper))
        assert _same_lists(got, lists[False])
        _check(M, t, 0, nbs[0], M.keys[:50])
        # an unknown user, an unknown neighbour: CMS_E_NO_SUCH_ID and nothing written
        for users, nbo, nbi in (([int(ids[0]), 12345], [0, 1, 2], ids[1:3]), (ids[:2], [0, 1, 2], [int(ids[1]), 12345])):
            us, nbo, nbi = (np.ascontiguousarray(x, np.int64) for x in (users, nbo, nbi))
            assert _code(lambda: t.exact_recommend_batch(us, nbo, nbi, 3)) == _lib.CMS_E_NO_SUCH_ID
            ito, keys = np.array([0, 2, 4], np.int64), np.ascontiguousarray(M.keys[:4])
            assert _code(lambda: t.exact_estimate_preferences_batch(us, nbo, nbi, ito, keys)) == _lib.CMS_E_NO_SUCH_ID
            cnt, it, va = np.full(2, -9, np.int32), np.full((2, 3), -9, np.int64), np.full((2, 3), -9.0, np.float32)
            est = np.full(4, -9.0, np.float32)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            assert t._lib.cms_exact_recommend_batch(t._h, 2, p(us), p(nbo), p(nbi), 3, 0, 0, 0.0, 0.0, p(cnt), p(it),
                                                    p(va)) == _lib.CMS_E_NO_SUCH_ID
            assert t._lib.cms_exact_estimate_preferences_batch(t._h, 2, p(us), p(nbo), p(nbi), p(ito), p(keys), 0, 0.0,
                                                               0.0, p(est)) == _lib.CMS_E_NO_SUCH_ID
            assert (cnt == -9).all() and (it == -9).all() and (va == -9.0).all() and (est == -9.0).all()
        t.detach_exact()
        for c in calls:
            assert _code(c) == _lib.CMS_E_STATE
        # the sketch table and what the CosineCM recommender gives are what they were
        assert torch.equal(t.save_device(), before)
        assert _same_lists(cm_rec.recommend_all(ids, HOW_MANY), lists_before)
        assert X.same_bits32(cm_rec.doEstimatePreferences(int(ids[0]), ids[nbs[0]], M.keys[:50]), est_before).all()
    finally:
        cm.close()


@pytest.mark.parametrize("kind", ["u32_before_finalize", "f64", "per_owner"])
def test_every_handle_kind(kind):
    M = _semantics_model()
    if kind == "per_owner":
        t = SketchTable.per_owner_shapes(M.n, device=0, owner_ids=M.owner_ids, weighted=True)
    else:
        t = SketchTable(M.n, depth=2, width=40, device=0, owner_ids=M.owner_ids, weighted=True,
                        counters="f64" if kind == "f64" else "u32")
    with t:
        t.attach_exact(M.offsets, M.keys, M.vals)
        _check(M, t, 0, [3, 2, 1], [5, 6, 0, 999], True)
        cnt, items, vals = t.exact_recommend_batch([10], [0, 3], [40, 30, 20], 5)
        assert _same_lists(_as_lists(cnt, items, vals), [X.recommend(M, 0, [3, 2, 1], 5, True)])


# ---- two independent paths meet ----

def _distinct_keys(oracle, depth, width, count):
    """The first `count` keys of 1000, 1001, ... whose buckets differ from every
    chosen key's in every sketch row (greedy)."""
    a, b = oracle.hash_params(SEED, depth)
    cand = np.arange(1000, 1000 + 40 * count, dtype=np.int64)
    h = oracle.hash_keys(a, b, width, cand)
    used = [set() for _ in range(depth)]
    keys = []
    for k, hk in zip(cand.tolist(), h.tolist()):
        if all(hk[r] not in used[r] for r in range(depth)):
            for r in range(depth):
                used[r].add(hk[r])
            keys.append(k)
            if len(keys) == count:
                break
    keys = np.array(keys, np.int64)
    assert keys.size == count
    hk = oracle.hash_keys(a, b, width, keys)
    assert all(np.unique(hk[:, r]).size == count for r in range(depth))
    return keys


@pytest.fixture(scope="module")
def owners(oracle):
    keys = _distinct_keys(oracle, 3, 4096, 64)
    rng = np.random.Generator(np.random.PCG64(96))
    prefs = []
    for r in range(96):
        its = rng.choice(keys, int(rng.integers(3, 13)), replace=False)
        prefs.append([(int(i), float(rng.integers(1, 6))) for i in its])
    prefs[40] = []                       # an owner without preferences: an empty neighbourhood
    prefs[41] = list(prefs[7])           # a twin
    return R.Model.from_lists(prefs, owner_ids=np.arange(96) * 11 - 300)


def _recommenders(M, depth, width):
    dm = GenericDataModel.from_csr(M.owner_ids, M.offsets, M.keys, M.vals)
    cm = taste.CosineCM(dm, taste.FixedShapeConfig(depth, width), taste.HashFunctionBuilder(SEED), device=0)
    assert (cm.depth, cm.width) == (depth, width)
    ex = taste.CosineSimilarity(dm, device=0)
    recs = tuple(taste.GenericUserBasedRecommender(dm, taste.NearestNUserNeighborhood(N_NB, s, dm), s) for s in (cm, ex))
    return cm, ex, recs


def test_collision_free_sketch_branch_is_the_exact_branch(owners):
    M = owners
    ids = M.owner_ids
    cm, ex, (s_rec, e_rec) = _recommenders(M, 3, 4096)
    try:
        t = cm.table
        t.attach_exact(M.offsets, M.keys, M.vals)
        nbr, _, cnt = t.exact_top_k_rows(np.arange(M.n), N_NB)
        off = np.zeros(M.n + 1, np.int64)
        np.cumsum(cnt, out=off[1:])
        nb = nbr[np.arange(N_NB)[None, :] < cnt[:, None]]
        for capper in (None, (1.0, 5.0)):
            sk = _as_lists(*t.recommend_batch(ids, off, nb, ids, M.offsets, M.keys, HOW_MANY, False, capper))
            xa = _as_lists(*t.exact_recommend_batch(ids, off, nb, HOW_MANY, False, capper))
            assert _same_lists(sk, xa)
        assert xa[40] == [] and sum(len(x) > 0 for x in xa) > 80
        rep = recommendation_accuracy(s_rec, e_rec, ids, HOW_MANY)
    finally:
        cm.close()
        ex.close()
    assert _same_lists(rep["sketch_lists"], rep["exact_lists"]) and _same_lists(rep["exact_lists"], xa)
    assert (rep["precision_at_n"] == 1.0).all()
    pairs = sum(len(x) for x in xa)
    for part in ("sketch_list", "exact_list"):
        f = rep[part]
        assert f["pairs"] == pairs and f["nan_pairs"] == 0
        assert f["abs_err_mean"] == 0.0 and f["abs_err_max"] == 0.0 and f["signed_err_mean"] == 0.0


# ---- the report is what it says ----

def _figures(sketch, exact):
    nan = np.isnan(sketch) | np.isnan(exact)
    e = (sketch - exact)[~nan]
    return {"pairs": int(e.size), "nan_pairs": int(nan.sum()), "abs_err_mean": float(np.abs(e).mean()),
            "abs_err_max": float(np.abs(e).max()), "signed_err_mean": float(e.mean())}


def test_report_fields_are_their_formulas(owners):
    M = owners
    users = M.owner_ids[np.concatenate([np.arange(0, M.n, 2), [41, 7]])]  # not every user, not in order throughout
    cm, ex, (s_rec, e_rec) = _recommenders(M, 2, 32)
    try:
        rep = recommendation_accuracy(s_rec, e_rec, users, HOW_MANY)
        S, E = rep["sketch_lists"], rep["exact_lists"]
        assert _same_lists(S, [s_rec.recommend(int(u), HOW_MANY) for u in users])
        assert _same_lists(E, [e_rec.recommend(int(u), HOW_MANY) for u in users])
        precision = np.ones(users.size)
        s_at_e, x_at_e, s_at_s, x_at_s = [], [], [], []
        for i, u in enumerate(users.tolist()):
            si, ei = [k for k, _ in S[i]], [k for k, _ in E[i]]
            if ei:
                precision[i] = len(set(si) & set(ei)) / len(ei)
                s_at_e += s_rec.doEstimatePreferences(u, s_rec._nb.getUserNeighborhood(u), ei).tolist()
                x_at_e += [v for _, v in E[i]]
            if si:
                s_at_s += [v for _, v in S[i]]
                x_at_s += e_rec.doEstimatePreferences(u, e_rec._nb.getUserNeighborhood(u), si).tolist()
    finally:
        cm.close()
        ex.close()
    assert np.array_equal(rep["precision_at_n"], precision)
    assert precision[list(users).index(M.owner_ids[40])] == 1.0 and E[list(users).index(M.owner_ids[40])] == []
    for part, (s, x) in (("exact_list", (s_at_e, x_at_e)), ("sketch_list", (s_at_s, x_at_s))):
        exp = _figures(np.array(s, np.float64), np.array(x, np.float64))
        assert rep[part] == exp, (part, rep[part], exp)
        assert exp["pairs"] > 0
    # the two recommenders do differ here: the test cannot pass on identical inputs
    assert not _same_lists(S, E)
    assert rep["exact_list"]["abs_err_max"] > 0.0 and (precision < 1.0).any()
