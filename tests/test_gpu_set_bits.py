"""GPU: cms_set_top_k_all and cms_set_block (k_set_bits_mfma) against the posting-list walk bit for bit and against
tests/set_ref.py.  Every model holds a list with every cross index (1), two identical lists (0, 2) and, on the owner
side, an empty one (3); lengths from {2, 9, 40} keep log-likelihood's decimal restatement to few distinct inputs."""
import ctypes
import functools

import numpy as np
import pytest

import set_ref as R
from mahout_amd import SketchTable, _lib, taste
from mahout_amd.datamodel import GenericDataModel

pytestmark = pytest.mark.gpu
bits = lambda a: np.asarray(a, np.float64).view(np.int64)  # noqa: E731
# lists on the side under test (fragment and tile edges, in rows and in columns) with cross indices around one
# MFMA step (64), one stage (256) and two stages
SHAPES = [(31, 63), (32, 64), (33, 65), (127, 255), (128, 256), (129, 257), (130, 513)]


@functools.lru_cache(maxsize=None)
def _model(n, num, side, seed=0):
    """(owner IDs, offsets, keys, the side's IDs ascending, the lists as a boolean [n][num])."""
    rng = np.random.Generator(np.random.PCG64(1000 * n + num + seed))
    L = np.zeros((n, num), bool)
    for a in range(n):
        L[a, rng.choice(num, min(num, int(rng.choice((2, 9, 40)))), replace=False)] = True
    L[1], L[2] = True, L[0]
    if side == "owner":
        L[3] = False
    A = L if side == "owner" else L.T
    oid, kid = np.arange(A.shape[0]) * 3 - 100, np.arange(A.shape[1]) * 7 + 5
    off = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64)
    return oid, off, kid[np.nonzero(A)[1]], (oid if side == "owner" else kid), L


@functools.lru_cache(maxsize=None)
def _expected(n, num, side, measure, seed=0):
    L = _model(n, num, side, seed)[4].astype(np.int64)
    K, ln = L @ L.T, L.sum(axis=1)
    return [[R.from_counts(measure, int(K[i, j]), int(ln[i]), int(ln[j]), num, side) for j in range(n)] for i in range(n)]


def _table(n, num, side, seed=0):
    oid, off, keys, _, _ = _model(n, num, side, seed)
    t = SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid)
    t.attach_sets(off, keys)
    t.set_timing(True, 2)
    return t


def _check(t, n, num, side, measure, seed=0):
    """The three properties of one case; returns (top_k_all's triple, the block)."""
    ids, exp = _model(n, num, side, seed)[3], _expected(n, num, side, measure, seed)
    top = t.set_top_k_all(n, measure, side)
    for got, ref in zip(top, t.set_top_k(ids, n, measure, side)):
        assert got.tobytes() == ref.tobytes(), (measure, side)
    blk = t.set_similarity_block(ids, ids, measure, side)
    for i in range(n):
        assert (bits(blk[i]) == bits(t.set_similarities(int(ids[i]), ids, measure, side))).all(), (measure, side, i)
        assert all(R.agrees(measure, g, e, S) for g, (e, S) in zip(blk[i], exp[i])), (measure, side, i)
        c = int(top[2][i])
        assert (bits(top[1][i, :c]) == bits(blk[i, np.searchsorted(ids, top[0][i, :c])])).all()
    return top, blk


@pytest.mark.parametrize("side", ["owner", "key"])
@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("n,num", SHAPES)
def test_shapes(monkeypatch, n, num, measure, side):
    monkeypatch.delenv("CMS_SET_BITS_MB", raising=False)
    monkeypatch.delenv("CMS_SET_BITS_KSEG", raising=False)
    with _table(n, num, side) as t:
        _check(t, n, num, side, measure)
        # one launch for the job and one for the block, over one matrix; the walk only in set_top_k's own call
        assert t.timing("set_bits_mfma")[1] == 2 and t.timing("set_bits_pack")[1] == 1 and t.timing("set_tile")[1] == 1


@pytest.mark.parametrize("measure", ["cooccurrence", "loglikelihood"])
def test_three_segments(monkeypatch, measure):
    """CMS_SET_BITS_KSEG at one stage, 513 cross indices: the counts are carried over two segment ends."""
    monkeypatch.setenv("CMS_SET_BITS_KSEG", "256")
    with _table(130, 513, "owner") as t:
        _, blk = _check(t, 130, 513, "owner", measure)
        assert measure != "cooccurrence" or blk[1, 1] == 513.0


@pytest.mark.parametrize("side", ["owner", "key"])
def test_route_and_budget(monkeypatch, side):
    """CMS_SET_BITS_MB=0: the same two calls through k_set_tile and k_set_pairs, the same bits."""
    n, num = 129, 257
    ids = _model(n, num, side)[3]
    got = {}
    for mb in ("16384", "0"):
        monkeypatch.setenv("CMS_SET_BITS_MB", mb)
        with _table(n, num, side) as t:
            got[mb] = (*t.set_top_k_all(n, "loglikelihood", side), t.set_similarity_block(ids, ids[:5], "tanimoto", side))
            dense, walk = t.timing("set_bits_mfma")[1], t.timing("set_tile")[1] + t.timing("set_pairs")[1]
            assert (dense, walk) == ((2, 0) if mb != "0" else (0, 2))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["16384"], got["0"]))


def test_block_ids_and_errors():
    n, num = 33, 65
    oid, off, keys, ids, _ = _model(n, num, "key")
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with SketchTable(oid.size, depth=1, width=32, device=0, owner_ids=oid) as t:
        for call in (lambda: t.set_top_k_all(3), lambda: t.set_similarity_block(oid[:2], oid[:2])):
            with pytest.raises(_lib.CmsError) as ei:
                call()
            assert ei.value.code == _lib.CMS_E_STATE
        t.attach_sets(off, keys)
        i1, i2 = ids[[7, 2, 2, 32, 0, 7]], ids[[5, 5, 31, 1, 0]]  # repeated and unsorted, on both arguments
        blk = t.set_similarity_block(i1, i2, "tanimoto", "key")
        for i, a in enumerate(i1):
            assert (bits(blk[i]) == bits(t.set_similarities(int(a), i2, "tanimoto", "key"))).all()
        out, bad = np.full(6, 7.0), np.array([ids[0], ids[1] + 1, ids[2]], np.int64)
        for a, b in ((bad, ids[:2]), (ids[:2], bad)):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert t._lib.cms_set_block(t._h, 1, 1, ptr(a), a.size, ptr(b), b.size, ptr(out)) == _lib.CMS_E_NO_SUCH_ID
        assert (out == 7.0).all()


def test_a_second_attach_drops_the_matrix():
    n, num = 33, 65
    oid, off_a, keys_a, _, _ = _model(n, num, "owner")
    _, off_b, keys_b, _, _ = _model(n, num, "owner", seed=1)
    with SketchTable(n, depth=1, width=32, device=0, owner_ids=oid) as t:
        t.attach_sets(off_a, keys_a)
        a = t.set_similarity_block(oid, oid, "cooccurrence")
        t.attach_sets(off_b, keys_b)
        b = t.set_similarity_block(oid, oid, "cooccurrence")
        assert a.tobytes() != b.tobytes()
        for i in range(n):
            assert (bits(b[i]) == bits(t.set_similarities(int(oid[i]), oid, "cooccurrence"))).all()
        assert t.set_top_k_all(5, "cooccurrence")[0].tobytes() == t.set_top_k(oid, 5, "cooccurrence")[0].tobytes()


@pytest.mark.parametrize("valued", [False, True])
def test_the_taste_methods(valued):
    n, num = 33, 65
    oid, off, keys, _, _ = _model(n, num, "owner")
    model = GenericDataModel.from_csr(oid, off, keys, np.full(keys.size, 2.5, np.float32) if valued else None)
    sim = (taste.LogLikelihoodSimilarity if valued else taste.TanimotoCoefficientSimilarity)(model, device=0)
    try:
        items, ids, sc, cnt = sim.allMostSimilarItemIDs(4)
        assert items.tolist() == list(model.getItemIDs()) and ids.shape == (num, 4)
        blk = sim.itemSimilarityBlock(items[::-1], items[:7])
        for i in (0, 1, 40, num - 1):
            row = sim.itemSimilarities(int(items[i]), items)
            keep = np.nonzero(~np.isnan(row) & (items != items[i]))[0]
            order = keep[np.lexsort((items[keep], -row[keep]))][:4]
            assert ids[i, :cnt[i]].tolist() == items[order].tolist() and (bits(sc[i, :cnt[i]]) == bits(row[order])).all()
            assert (bits(blk[num - 1 - i]) == bits(row[:7])).all()
        users, uids, _, ucnt = sim.allMostSimilarUserIDs(3)
        assert users.tolist() == oid.tolist()
        for u in (0, 3, n - 1):  # owner 3 is empty
            assert uids[u, :ucnt[u]].tolist() == sim.mostSimilarUserIDs(int(oid[u]), 3).tolist()
        pytest.raises(taste.NoSuchItemException, lambda: sim.itemSimilarityBlock([int(items[0])], [10 ** 6]))
    finally:
        sim.close()
