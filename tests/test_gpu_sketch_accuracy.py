"""GPU: the sketch accuracy report (mahout_amd.accuracy.sketch_accuracy) and
taste.CosineSimilarity.

  two independent paths meet   64 item keys whose buckets are distinct in every
      sketch row at (d, w) = (3, 4096), 96 owners over them with integer values:
      every sketch row is the owner's exact vector, so the sketch cosine and the
      exact cosine are one number bit for bit, the lists are identical, recall is
      1 and every error is 0.0
  the report is what it says   the same owners at (2, 32), where 64 keys share 32
      buckets: at least one pair differs, and every field equals a numpy
      recomputation from the returned triples, the oracle's sketch cosine and the
      restatement of CosineSimilarity (tests/exact_ref.py)
  taste.CosineSimilarity       on a TasteTestCase-shaped model against the
      restatement; NearestNUserNeighborhood over it returns the same list

Bit equality everywhere, NaN matching NaN.
"""
import numpy as np
import pytest

import exact_ref as R
from mahout_amd import SketchTable, taste
from mahout_amd.accuracy import sketch_accuracy
from mahout_amd.datamodel import GenericDataModel, NoSuchUserException

pytestmark = pytest.mark.gpu

SEED = 42
K = 10


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
    prefs[40] = []                       # an owner without preferences: NaN on both sides
    prefs[41] = list(prefs[7])           # a twin
    return R.Model.from_lists(prefs, owner_ids=np.arange(96) * 11 - 300)


def _table(M, depth, width):
    t = SketchTable(M.n, depth=depth, width=width, seed=SEED, device=0, owner_ids=M.owner_ids)
    t.ingest_csr(M.offsets, M.keys, M.vals)
    t.finalize()
    t.attach_exact(M.offsets, M.keys, M.vals)
    return t


def _same(a, b):
    return bool(R.same_bits(a, b).all())


def test_collision_free_sketch_is_the_exact_cosine(owners):
    M = owners
    ids = M.owner_ids
    with _table(M, 3, 4096) as t:
        for r in range(M.n):
            s, x = t.similarities(int(ids[r]), ids), t.exact_similarities(int(ids[r]), ids)
            assert _same(s, x), r
            assert _same(x, M.similarities_row(r)), r
        rep = sketch_accuracy(t, ids, K)
    assert (rep["recall_at_k"] == 1.0).all()
    assert np.array_equal(rep["sketch_counts"], rep["exact_counts"])
    assert np.array_equal(rep["sketch_ids"], rep["exact_ids"]) and _same(rep["sketch_scores"], rep["exact_scores"])
    assert rep["exact_counts"][40] == 0 and (rep["exact_counts"][np.arange(M.n) != 40] == K).all()
    for part in ("sketch_list", "exact_list"):
        f = rep[part]
        assert f["pairs"] == (M.n - 1) * K and f["nan_pairs"] == 0
        assert f["abs_err_mean"] == 0.0 and f["abs_err_max"] == 0.0 and f["signed_err_mean"] == 0.0


def _figures(sketch, exact):
    nan = np.isnan(sketch) | np.isnan(exact)
    e = (sketch - exact)[~nan]
    return {"pairs": int(e.size), "nan_pairs": int(nan.sum()), "abs_err_mean": float(np.abs(e).mean()),
            "abs_err_max": float(np.abs(e).max()), "signed_err_mean": float(e.mean())}


def test_report_fields_are_their_formulas(owners, oracle):
    M = owners
    ids = M.owner_ids
    d, w = 2, 32
    a, b = oracle.hash_params(SEED, d)
    rows_of = np.repeat(np.arange(M.n), np.diff(M.offsets))
    tab = oracle.build_table(M.n, d, w, a, b, rows_of, M.keys, M.vals)
    sk = np.stack([[oracle.cosine_cm(tab[i], tab[j]) for j in range(M.n)] for i in range(M.n)])
    ex = M.all_pairs()
    assert (~R.same_bits(sk, ex)).any()  # collisions: the two cosines differ somewhere
    queries = np.concatenate([np.arange(0, M.n, 3), [40, 41]])  # not every owner, not in row order throughout
    with _table(M, d, w) as t:
        rep = sketch_accuracy(t, ids[queries], K)
    nq = queries.size
    # the triples are the two top-k lists
    for i, q in enumerate(queries):
        others = np.arange(M.n) != q
        for name, mat in (("sketch", sk), ("exact", ex)):
            eids, esc = oracle.top_users(ids[others], mat[q][others], K)
            c = int(rep[name + "_counts"][i])
            assert c == eids.size and rep[name + "_ids"][i, :c].tolist() == eids.tolist(), (name, q)
            assert _same(rep[name + "_scores"][i, :c], esc)
            assert (rep[name + "_ids"][i, c:] == -1).all() and np.isnan(rep[name + "_scores"][i, c:]).all()
    # every field from the triples
    row = {int(v): r for r, v in enumerate(ids)}
    recall = np.ones(nq)
    s_pairs, e_pairs = [], []
    for i, q in enumerate(queries):
        cs, ce = int(rep["sketch_counts"][i]), int(rep["exact_counts"][i])
        si, ei = rep["sketch_ids"][i, :cs], rep["exact_ids"][i, :ce]
        if ce:
            recall[i] = len(set(ei.tolist()) & set(si.tolist())) / ce
        s_pairs += [(rep["sketch_scores"][i, t], ex[q, row[int(si[t])]]) for t in range(cs)]
        e_pairs += [(sk[q, row[int(ei[t])]], rep["exact_scores"][i, t]) for t in range(ce)]
    assert np.array_equal(rep["recall_at_k"], recall)
    assert recall[list(queries).index(40)] == 1.0 and rep["exact_counts"][list(queries).index(40)] == 0
    for part, pairs in (("sketch_list", s_pairs), ("exact_list", e_pairs)):
        arr = np.array(pairs, np.float64).reshape(-1, 2)
        exp = _figures(arr[:, 0], arr[:, 1])
        assert rep[part] == exp, (part, rep[part], exp)
        assert exp["pairs"] > 0


def _taste_model():
    # the shape of TasteTestCase.getDataModel(): a few users over three items, values 0.1 .. 0.8
    return GenericDataModel({1: {0: 0.1, 1: 0.3}, 2: {0: 0.2, 1: 0.3, 2: 0.3}, 3: {0: 0.4, 1: 0.3, 2: 0.5},
                             4: {0: 0.7, 1: 0.3, 2: 0.8}, 5: {1: 0.6, 2: 0.2}, 6: {2: 0.5}})


@pytest.mark.parametrize("weighting", [taste.Weighting.UNWEIGHTED, taste.Weighting.WEIGHTED])
def test_taste_cosine_similarity(weighting):
    dm = _taste_model()
    weighted = weighting == taste.Weighting.WEIGHTED
    M = R.Model(dm.user_ids, dm.offsets, dm.keys, dm.values)
    ref = M.all_pairs(weighted)
    sim = taste.CosineSimilarity(dm, weighting, device=0)
    try:
        users = dm.getUserIDs()
        for i, u in enumerate(users):
            for j, v in enumerate(users):
                assert _same(sim.userSimilarity(int(u), int(v)), ref[i, j]), (u, v)
            assert _same(sim.itemSimilarities(int(u), users), ref[i])
            assert sim.allSimilarItemIDs(int(u)).tolist() == users[~np.isnan(ref[i])].tolist()
            for k in (1, 3, 10):
                eids, _ = M.top_k(i, k, ref[i])
                assert sim.mostSimilarUserIDs(int(u), k).tolist() == eids.tolist()
            nb = taste.NearestNUserNeighborhood(3, sim, dm)
            assert nb.getUserNeighborhood(int(u)).tolist() == M.top_k(i, 3, ref[i])[0].tolist()
        with pytest.raises(NoSuchUserException):
            sim.userSimilarity(1, 99)
        with pytest.raises(ValueError):
            sim.mostSimilarUserIDs(1, 0)
    finally:
        sim.close()


def test_taste_cosine_similarity_over_a_transposed_model_and_without_values():
    dm = _taste_model()
    tm = dm.transposed()  # owners are the items, keyed by user
    M = R.Model(tm.user_ids, tm.offsets, tm.keys, tm.values)
    sim = taste.CosineSimilarity(tm, device=0)
    try:
        items = tm.getUserIDs()
        for i, a in enumerate(items):
            for j, b in enumerate(items):
                assert _same(sim.itemSimilarity(int(a), int(b)), M.similarity(i, j))
        with pytest.raises(taste.NoSuchItemException):
            sim.itemSimilarity(0, 99)
    finally:
        sim.close()
    with pytest.raises(ValueError):  # CosineSimilarity.java:41
        taste.CosineSimilarity(GenericDataModel.from_csr(dm.user_ids, dm.offsets, dm.keys, None), device=0)
