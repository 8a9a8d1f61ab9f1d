"""GPU: the user-based recommenders over the co-rated and the set similarities (cms_neighbor.hip k_nb_estimate<KIND>:
cms_neighbor_estimate_preferences_batch, cms_neighbor_recommend_batch; taste.GenericUserBasedRecommender and
taste.GenericBooleanPrefUserBasedRecommender) against the plain-Python restatement tests/user_est_ref.py, bit for
bit, NaN matching NaN.  The restatement's similarities come from tests/common_ref.py and tests/set_ref.py, for
log-likelihood from the handle's own set_pairs (held to its bound in tests/test_gpu_set_similarity.py), so the
estimate comparison stays exact."""
import os

import numpy as np
import pytest

import common_ref as C
import set_ref as S
import user_est_ref as U
from exact_rec_ref import same_bits32
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.datamodel import GenericDataModel

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("measure", ["pearson", "tanimoto"])
KIND = pytest.mark.parametrize("kind", ["generic", "boolean"])
KEY = lambda item: int(item) * 7 - 300  # noqa: E731  (item keys are not the dense indices)


def _open(M, tile=None):
    """A minimal handle with M attached; CMS_NB_EST_TILE is read when the handle is created."""
    os.environ["CMS_NB_EST_TILE"] = str(tile or 0)
    try:
        t = SketchTable(len(M.owner_ids), depth=1, width=32, device=0, owner_ids=M.owner_ids)
    finally:
        del os.environ["CMS_NB_EST_TILE"]
    t.attach_exact(M.offsets, M.keys, M.vals)
    return t


def _sims(M, t, measure, user):
    """userSimilarity(row user, every row) under measure, as the reference computes it."""
    if measure in SketchTable.COMMON_MEASURES:
        return M.row(measure, "owner", user)
    if measure == "loglikelihood":
        return t.set_pairs(np.full(len(M.owner_ids), M.owner_ids[user]), M.owner_ids, measure)
    L = M.lists["owner"]
    return np.array([S.similarity(measure, L[user][0], y[0], M.num["owner"])[0] for y in L], np.float64)


def _rows(M):
    return [dict(zip(k, v)) for k, v in M.lists["owner"]]


def _check(M, t, measure, kind, user, nb, items, capper=None, sims=None):
    """The single call for owner ROW user, neighbour ROWS nb and item KEYS items against the restatement."""
    got = t.neighbor_estimate_preferences(int(M.owner_ids[user]), M.owner_ids[np.asarray(nb, np.int64)], items, measure,
                                          kind, capper)
    sims = _sims(M, t, measure, user) if sims is None else sims
    ref = U.estimates(kind, _rows(M), sims, user, nb, items, None if kind == "boolean" else capper)
    bad = np.nonzero(~same_bits32(got, ref))[0]
    assert bad.size == 0, (measure, kind, user, list(nb), [(int(items[i]), got[i], ref[i]) for i in bad[:5]])
    return got


def _batch_equals(M, t, measure, kind, cases, singles, capper=None):
    """One batch call of cases = [(user row, neighbour rows, item keys)] gives the single calls' estimates."""
    nbo = np.cumsum([0] + [len(c[1]) for c in cases])
    ito = np.cumsum([0] + [len(c[2]) for c in cases])
    nb = M.owner_ids[np.concatenate([np.asarray(c[1], np.int64) for c in cases])]
    out = t.neighbor_estimate_preferences_batch(M.owner_ids[[c[0] for c in cases]], nbo, nb, ito,
                                                np.concatenate([c[2] for c in cases]), measure, kind, capper)
    assert same_bits32(out, np.concatenate(singles)).all()


@pytest.fixture(scope="module")
def edge_model():
    """40 users over 200 items, values 0.5 .. 5.0; rows 3 and 4 hold every item, so the first and last slot of
    every tile carry a value and their lists begin before and end after every tile."""
    rng = np.random.Generator(np.random.PCG64(2048))
    held = [np.arange(200) if r in (3, 4) else rng.choice(200, int(rng.integers(50, 90)), replace=False) for r in range(40)]
    return C.Model([[(KEY(i), np.float32(0.5 * rng.integers(1, 11))) for i in h] for h in held], np.arange(40) * 3 - 50)


@KIND
@BOTH
def test_tile_edges(edge_model, measure, kind):
    M, rng = edge_model, np.random.Generator(np.random.PCG64(65))
    nb = [39, 4, 30, 3, 25, 21, 38, 17, 16, 11, 12, 9, 7, 8, 5, 2, 6]
    cases = [(2, nb, np.array([KEY(i) for i in rng.permutation(rng.choice(np.arange(20, 180), c, replace=False))]))
             for c in (63, 64, 65, 130)]
    with _open(M, tile=64) as t:
        singles = [_check(M, t, measure, kind, u, n, it, (1.0, 4.5)) for u, n, it in cases]
        for (_, _, it), est in zip(cases, singles):  # a tile's first and last slot
            assert not np.isnan(est[np.argsort(it)][[e for e in (0, 63, 64, 127, 128, it.size - 1) if e < it.size]]).any()
        _batch_equals(M, t, measure, kind, cases, singles, (1.0, 4.5))


@KIND
@BOTH
def test_chunk_edges(edge_model, measure, kind):
    """Neighbourhoods of 1 .. 65 in non-ascending order: the user inside (place 5) and as the only member of the
    second chunk of either G (places 16 and 32), rows named again in later chunks."""
    M, user = edge_model, 1
    seq = [int(r) for r in np.random.Generator(np.random.PCG64(7)).permutation(np.arange(2, 40))]
    seq = (seq + seq[3:])[:65]
    seq[5] = seq[16] = seq[32] = user
    assert seq != sorted(seq) and len(set(seq[:16]) & set(seq[32:])) > 1
    items = np.array([KEY(i) for i in range(0, 200, 3)])
    with _open(M, tile=64) as t:
        sims = _sims(M, t, measure, user)
        for size in (1, 2, 15, 16, 17, 31, 32, 33, 65):
            _check(M, t, measure, kind, user, seq[:size], items, sims=sims)


SEMANTICS = [[(0, 1.0), (1, 2.0), (2, 4.0), (3, 3.0)],             # 0: the user
             [(0, 1.0), (1, 1.0), (2, 3.0), (5, 4.0), (6, 1.0)],   # 1
             [(0, 2.0), (1, 1.0), (3, 4.0), (5, 0.0), (6, 2.0)],   # 2: holds item 5 with 0.0
             [(0, 2.0), (1, 3.0), (2, 1.0), (6, 3.0)],             # 3: lacks item 5
             [(5, 2.0), (6, 1.0), (8, 1.0)],                       # 4: nothing in common with the user: NaN similarity
             [],                                                   # 5: no preference
             [(1, 4.0), (2, 1.0), (3, 2.0), (5, 1.5)]]             # 6


@KIND
@pytest.mark.parametrize("measure", ["pearson", "tanimoto", "uncentered_cosine", "euclidean", "city_block", "loglikelihood"])
def test_semantics(measure, kind):
    M = C.Model(SEMANTICS, owner_ids=[10, 20, 30, 40, 50, 60, 70])
    keys = np.array([6, 999, 5, 6, 0, -4, 5, 2, 6], np.int64)  # unknown, repeated and own keys, in the caller's order
    five = np.array([5], np.int64)
    with _open(M, tile=64) as t:
        sims = _sims(M, t, measure, 0)
        assert np.isnan(sims[4]) == (measure != "city_block")
        est = lambda nb, items=five, capper=None: _check(M, t, measure, kind, 0, nb, items, capper, sims)  # noqa: E731
        assert np.isnan(est([1, 3])[0]) == (kind == "generic")     # one data point
        assert not np.isnan(est([5, 1, 2])[0])                     # two: the second is row 2's 0.0
        assert np.isnan(est([1, 4, 6])[0]) == (kind == "boolean" and measure != "city_block")  # NaN: skipped, or NaN
        assert same_bits32(est([0, 6, 1, 0]), est([6, 1])).all()   # the user in its own neighbourhood
        est([1, 1])                                                # a neighbour named twice counts twice
        got = est([3, 2, 1, 6], keys, (0.5, 3.0))
        assert np.isnan(got[[1, 5]]).all() and got[0] == got[3] == got[8] and got[2] == got[6]
        assert np.isnan(t.neighbor_estimate_preferences(10, [], keys, measure, kind)).all()   # an empty neighbourhood
        assert t.neighbor_estimate_preferences(10, [20, 30], [], measure, kind).size == 0


@KIND
def test_order_of_the_neighbourhood_decides_the_bits(kind):
    M = C.Model(U.GENERIC_ORDER_PREFS)  # asserted on the host: the two orders differ in the restatement
    with _open(M, tile=64) as t:
        e = [_check(M, t, "pearson", kind, 0, nb, [9])[0] for nb in U.GENERIC_ORDERS]
        assert not same_bits32(e[0], e[1])
        if kind == "generic":  # totalSimilarity == 0.0 without and with the capper
            assert np.isinf(e[0]) and _check(M, t, "pearson", kind, 0, U.GENERIC_ORDERS[0], [9], (0.5, 5.0))[0] in (0.5, 5.0)


@KIND
@BOTH
def test_model_with_non_eligible_rows(measure, kind):
    rng = np.random.Generator(np.random.PCG64(30))
    pool = [np.float32(v) for v in (1 / 3, -1 / 3, 2 / 3, -1 / 768, 1.0, -0.5)]  # a 768th: no shift, every row merge-joins
    M = C.Model([[(int(i), pool[int(rng.integers(6))]) for i in rng.choice(12, int(rng.integers(3, 9)), replace=False)]
                 for _ in range(30)], owner_ids=np.arange(30) * 5 - 77)
    with _open(M, tile=64) as t:
        singles = [_check(M, t, measure, kind, u, [int(r) for r in rng.permutation(30)[:6]], np.arange(12))
                   for u in range(30)]
    assert sum(int((~np.isnan(e)).sum()) for e in singles) > 30


def test_default_tile_batch_equals_single():
    rng = np.random.Generator(np.random.PCG64(1100))
    M = C.Model([[(int(i) * 3 + 1, np.float32(0.5 * rng.integers(1, 11)))
                  for i in rng.choice(1100, 40 if r == 0 else 800, replace=False)] for r in range(6)], np.arange(6) + 100)
    cases = [(u, [r for r in (5, 3, 4, 1, 2, 0) if r != u], M.item_keys if u == 0 else rng.choice(3400, 100, replace=False))
             for u in range(6)]
    with _open(M) as t:
        singles = [_check(M, t, "pearson", "generic", u, nb, it) for u, nb, it in cases]
        assert (~np.isnan(singles[0])).sum() > 896  # more than the generic tile: two workgroups for user 0
        _batch_equals(M, t, "pearson", "generic", cases, singles)


def _same_lists(a, b):
    return len(a) == len(b) and all([i for i, _ in x] == [i for i, _ in y] and
                                    same_bits32([v for _, v in x], [v for _, v in y]).all() for x, y in zip(a, b))


def _as_lists(cnt, items, vals):
    return [[(int(items[u, j]), vals[u, j]) for j in range(int(cnt[u]))] for u in range(cnt.size)]


@pytest.mark.parametrize("cls,sim_cls,values", [
    (taste.GenericUserBasedRecommender, taste.PearsonCorrelationSimilarity, True),
    (taste.GenericBooleanPrefUserBasedRecommender, taste.LogLikelihoodSimilarity, False)])
def test_recommend(cls, sim_cls, values):
    rng = np.random.Generator(np.random.PCG64(120))
    prefs = [[(int(i) * 11 - 500, np.float32(0.5 * rng.integers(1, 11)) if values else np.float32(1.0))
              for i in rng.choice(200, int(rng.integers(8, 30)), replace=False)] for _ in range(120)]
    prefs[17] = []  # no preference: an empty neighbourhood, nothing recommended
    M = C.Model(prefs, owner_ids=np.arange(120) * 13 - 400)
    ids, rows = M.owner_ids, _rows(M)
    dm = GenericDataModel.from_csr(ids, M.offsets, M.keys, M.vals if values else None)
    sim = sim_cls(dm, device=0)
    try:
        nbh = taste.NearestNUserNeighborhood(10, sim, dm)
        rec = cls(dm, nbh, sim)
        off, nb = nbh.getUserNeighborhoods(ids)
        every = rec.recommend_all(ids, 10)
        assert _same_lists(every, _as_lists(*sim.table.neighbor_recommend_batch(ids, off, nb, 10, sim.MEASURE, cls.KIND,
                                                                                False, rec._capper)))
        assert every[17] == [] and sum(len(x) == 10 for x in every) > 60
        for u in range(120):
            nbr = np.searchsorted(ids, nb[off[u]:off[u + 1]])
            assert _same_lists([rec.recommend(int(ids[u]), 10)], [every[u]]), u
            if nbr.size:  # the restatement: FastIDSet candidates, the loop, TopItems
                cand = rec.getAllOtherItems(ids[nbr], int(ids[u])).toList()
                est = U.estimates(cls.KIND, rows, _sims(M, sim.table, sim.MEASURE, u), u, nbr, cand, rec._capper)
                assert _same_lists([taste.get_top_items(10, cand, est)], [every[u]]), u
    finally:
        sim.close()


def test_state_and_the_cosine_route_is_unchanged():
    M = C.Model(SEMANTICS, owner_ids=[10, 20, 30, 40, 50, 60, 70])
    ids = M.owner_ids

    def code(call):
        with pytest.raises(_lib.CmsError) as e:
            call()
        return e.value.code

    with SketchTable(7, depth=1, width=32, device=0, owner_ids=ids) as t:
        assert code(lambda: t.neighbor_estimate_preferences(10, [20], [5])) == _lib.CMS_E_STATE
        t.attach_exact(M.offsets, M.keys, M.vals)
        for measure, kind in (((2, 1), 0), ((0, 3), 0), ((1, 4), 1), ((0, 1), 2)):  # (family, measure), kind
            assert code(lambda: t.neighbor_estimate_preferences(10, [20], [5], measure, kind)) == _lib.CMS_E_PARAM
            assert code(lambda: t.neighbor_recommend_batch([10], [0, 1], [20], 3, measure, kind)) == _lib.CMS_E_PARAM
        assert code(lambda: t.neighbor_estimate_preferences(10, [12345], [5])) == _lib.CMS_E_NO_SUCH_ID
    dm = GenericDataModel.from_csr(ids, M.offsets, M.keys, M.vals)
    sim = taste.CosineSimilarity(dm, device=0)
    try:
        nbh = taste.NearestNUserNeighborhood(3, sim, dm)
        rec = taste.GenericUserBasedRecommender(dm, nbh, sim)
        off, nb = nbh.getUserNeighborhoods(ids)
        assert _same_lists(rec.recommend_all(ids, 4),
                           _as_lists(*sim.table.exact_recommend_batch(ids, off, nb, 4, False, rec._capper)))
        assert same_bits32(rec.doEstimatePreferences(10, [20, 30, 70], [5, 6]),
                           sim.table.exact_estimate_preferences(10, [20, 30, 70], [5, 6], rec._capper)).all()
        with pytest.raises(NotImplementedError):
            taste.GenericBooleanPrefUserBasedRecommender(dm, nbh, sim)
    finally:
        sim.close()
