"""GPU: threshold neighbourhoods (cms_threshold_neighbors: k_thr_mark,
k_thr_rowmask, k_thr_scan, k_thr_fill over the four slab producers) against the
oracle -- `T/impl/neighborhood/ThresholdUserNeighborhood.java:77-97` restated
in numpy over oracle.similarities_row / oracle.per_owner_similarity: drop NaN
and self, keep `>= threshold`, ascending owner ID; FastIDSet order through
taste.FastIDSet.  Bit for bit; no tolerance, no skipped case.  Expected lists
never come from the library.

The tables of sections 1-3 are DESIGNED (mahout_amd.checkpoint.build_checkpoint
+ SketchTable.load_device), and each test asserts on the CPU, before the GPU is
used, that the cases it is about occur in its design.

  1  permutation and tails: the MFMA path at d = 2, n = 333 (and 1, 64, 65,
     130): multi-limb owners at the highest rows (position != row), int8 and
     counters-<=-4 owners, empty owners, identical owners, six thresholds.
     w = 128 is the narrowest MFMA width; the fp4 operand class exists only
     where w % 256 == 0 (cosine_prepare), so the same design also runs at
     w = 256, where fp4_owners > 0 is asserted
  2  chunks: CMS_THRESHOLD_SLAB_ROWS=128, all owners and out-of-order,
     repeated queries over non-adjacent tiles (n = 333: 3 tiles; n = 700: 6)
  3  the other producers: the pair kernel (w = 30), fp64 counters, per-owner shapes
  4  the capacity protocol and the refusals
  5  the call changes nothing of the handle
  6  taste.ThresholdUserNeighborhood: neighbourhoods, recommend, recommend_all,
     the temporary user
"""
import ctypes
import os

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib, checkpoint as ck, taste
from mahout_amd.datamodel import GenericDataModel
from mahout_amd.synth import movielens_like, to_csr, zipf_stream

pytestmark = pytest.mark.gpu

SEED = 42
INF = float("inf")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def load_design(c, a, b, owner_ids=None, weighted=False, env=None):
    """A finalized handle holding the designed table c [n][d][w] (u32
    counters for an integer table, fp64 counters for a float one)."""
    import torch

    n, d, w = c.shape
    f64 = c.dtype.kind == "f"
    image = ck.build_checkpoint(c, a, b, seed=SEED, owner_ids=owner_ids)
    saved = {k: os.environ.pop(k, None) for k in ("CMS_THRESHOLD_SLAB_ROWS",)}
    os.environ.update(env or {})
    try:  # (the tunables are read once, at creation)
        t = SketchTable(n, depth=d, width=w, seed=SEED, weighted=weighted, counters="f64" if f64 else "u32")
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    try:
        dev = torch.device("cuda", t.device)
        t.load_device(torch.frombuffer(bytearray(image), dtype=torch.uint8).to(dev))
        t.finalize()
        assert np.array_equal(_bits(t.read_counters()), _bits(c.astype(np.float64)))
    except BaseException:
        t.close()
        raise
    return t


def sim_matrix(oracle, table, weighted=False):
    return np.stack([oracle.similarities_row(table, q, weighted) for q in range(table.shape[0])])


def expected(S, ids, qrows, thr):
    """(offsets, neighbour IDs, scores) of the reference loop for the owner
    rows qrows: NaN and self dropped, s >= thr kept, ascending owner row."""
    qrows = np.asarray(qrows, np.int64)
    rows = S[qrows]
    with np.errstate(invalid="ignore"):
        keep = ~np.isnan(rows) & (rows >= thr)
    keep[np.arange(qrows.size), qrows] = False
    off = np.zeros(qrows.size + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    cols = np.nonzero(keep)[1]
    return off, np.asarray(ids, np.int64)[cols], rows[keep]


def assert_lists(got, exp, what=""):
    off, ids, sc = got
    eoff, eids, esc = exp
    assert np.array_equal(off, eoff), (what, "offsets")
    assert np.array_equal(ids, eids), (what, "ids")
    if sc is not None:
        assert not np.isnan(sc).any()
        assert np.array_equal(_bits(sc), _bits(esc)), (what, "scores")


def fastidset_order(exp):
    """The expected CSR with every list passed through taste.FastIDSet."""
    off, ids, sc = exp
    oi, os_ = ids.copy(), sc.copy()
    for q in range(off.size - 1):
        lo, hi = int(off[q]), int(off[q + 1])
        s = taste.FastIDSet()
        for i in ids[lo:hi].tolist():
            s.add(i)
        order = s.toList()
        score_of = dict(zip(ids[lo:hi].tolist(), sc[lo:hi].tolist()))
        oi[lo:hi] = order
        os_[lo:hi] = [score_of[i] for i in order]
    return off, oi, os_


# ------------------------------------------- 1. permutation and tails ----

def mfma_design(n, d, w, seed):
    """(counters, owner IDs, kinds).  From n = 16 on: two empty owners, two
    identical owners whose every row norm is a perfect square (similarity
    exactly 1.0), owners whose counters are all <= 4, int8 owners, and the
    multi-limb owners (a counter >= 128, 2 to 4 limbs) at the HIGHEST rows:
    the MFMA layout puts multi-limb owners first, so no owner keeps its row."""
    rng = _rng(seed)
    c = np.zeros((n, d, w), np.uint64)
    kinds = np.array(["int8"] * n, dtype=object)
    if n >= 16:
        n_multi = min(10, n // 8)
        kinds[n - n_multi:] = "multi"
        kinds[[3, n // 2]] = "empty"
        kinds[[1, n - n_multi - 2]] = "twin"
        free = np.flatnonzero(kinds == "int8")
        kinds[free[::3]] = "fp4"
    for r in range(n):
        k = kinds[r]
        if k == "empty":
            continue
        if k == "twin":
            c[r, :, 7], c[r, :, 100] = 3, 4  # row norms 25: sqrt exact, cosine exactly 1.0
            continue
        hi = 5 if k == "fp4" else 100
        c[r] = rng.integers(0, hi, (d, w)) * (rng.random((d, w)) < 0.5)
        c[r, 0, int(rng.integers(0, w))] = hi - 1
        if k == "multi":  # 2 limbs below 2^14, up to 4 below 2^28
            top = [200, 16000, 70000, 3000000][r % 4]
            c[r, rng.integers(0, d, 3), rng.integers(0, w, 3)] = rng.integers(128, top, 3)
            c[r, 1, 5] = top
    ids = (np.cumsum(rng.integers(1, 50, n)) - 1000).astype(np.int64)
    return c, ids, kinds


_CASES = {}


def mfma_case(oracle, n, w):
    key = (n, w)
    if key not in _CASES:
        c, ids, kinds = mfma_design(n, 2, w, 7000 + n)
        S = sim_matrix(oracle, c.astype(np.float64))
        S.setflags(write=False)
        _CASES[key] = (c, ids, kinds, S)
    return _CASES[key]


def star(S, kinds):
    """(q0, r0, v*): a pair of int8 owners whose similarity is the median of q0's row."""
    n = S.shape[0]
    if n < 16:
        return None
    q0 = int(np.flatnonzero(kinds == "int8")[2])
    cand = [r for r in range(n) if r != q0 and not np.isnan(S[q0, r])]
    r0 = sorted(cand, key=lambda r: S[q0, r])[len(cand) // 2]
    return q0, r0, float(S[q0, r0])


def check_design(c, ids, kinds, S):
    n = c.shape[0]
    assert not np.array_equal(ids, np.arange(n))  # owner IDs are not the row indices
    if n < 16:
        return
    cmax = c.reshape(n, -1).max(axis=1)
    multi = np.flatnonzero(kinds == "multi")
    assert multi.size > 0 and (cmax[multi] >= 128).all() and (cmax[kinds != "multi"] < 128).all()
    assert multi.min() > np.flatnonzero(kinds != "multi").max()  # highest rows: position != row for everyone
    assert (cmax[multi] >= 1 << 14).any() and (cmax[multi] < 1 << 14).any()  # 2-limb and deeper owners
    fp4 = np.flatnonzero(kinds == "fp4")
    assert fp4.size > 0 and (cmax[fp4] <= 4).all() and (cmax[fp4] > 0).all()
    assert ((cmax[kinds == "int8"] > 4) & (cmax[kinds == "int8"] < 128)).all()
    empty = np.flatnonzero(kinds == "empty")
    assert empty.size == 2 and np.isnan(S[empty]).all() and np.isnan(S[:, empty]).all()
    t1, t2 = np.flatnonzero(kinds == "twin")
    assert np.array_equal(c[t1], c[t2]) and S[t1, t2] == 1.0 and S[t2, t1] == 1.0
    off_diag = S[~np.eye(n, dtype=bool)]
    assert np.sum(off_diag == 1.0) == 2  # only the twins reach 1.0


def thresholds_for(S, kinds, ids, full):
    st = star(S, kinds)
    if st is None:  # a single owner has no pair to take v* from
        return [-INF, 0.5]
    q0, r0, v = st
    up = float(np.nextafter(v, INF))
    # v* lists the pair, the next double does not
    assert ids[r0] in expected(S, ids, [q0], v)[1] and ids[r0] not in expected(S, ids, [q0], up)[1]
    assert 0.0 < v < 1.0
    return [-INF, INF, 1.0, 0.0, v, up] if full else [-INF, v]


@pytest.mark.parametrize("n,w", [(333, 128), (333, 256), (1, 128), (64, 128), (65, 128), (130, 128)])
def test_mfma_permutation_and_tails(oracle, n, w):
    c, ids, kinds, S = mfma_case(oracle, n, w)
    check_design(c, ids, kinds, S)
    ths = thresholds_for(S, kinds, ids, full=n == 333)
    a, b = oracle.hash_params(SEED, 2)
    allq = np.arange(n)
    sizes = set()
    with load_design(c, a, b, owner_ids=ids) as t:
        for thr in ths:
            exp = expected(S, ids, allq, thr)
            sizes.add(int(exp[0][-1]))
            assert_lists(t.threshold_neighbors(ids, thr), exp, (n, w, thr))
        st = t.stats()
        if n >= 16:
            assert st["multi_limb_owners"] == int(np.sum(kinds == "multi")) > 0
            # the fp4 operand class needs whole 128-byte stages of 4-bit counters: w % 256 == 0
            if w % 256 == 0 and os.environ.get("CMS_NO_FP4", "") in ("", "0"):
                assert st["fp4_owners"] >= int(np.sum(kinds == "fp4")) > 0
            else:
                assert st["fp4_owners"] == 0
    if n == 333:
        # +inf lists nobody, 1.0 the twins alone; -inf and 0.0 list the same (no similarity is negative here)
        assert 0 in sizes and 2 in sizes and len(sizes) == 5


# ------------------------------------------------------------ 2. chunks ----

@pytest.mark.parametrize("n", [333, 700])
def test_chunked_equals_unchunked(oracle, n):
    c, ids, kinds, S = mfma_case(oracle, n, 128)
    check_design(c, ids, kinds, S)
    q0, r0, v = star(S, kinds)
    a, b = oracle.hash_params(SEED, 2)
    n_multi = int(np.sum(kinds == "multi"))
    # the layout: multi-limb owners first, then (no fp4 class at w = 128) the
    # single-limb owners in row order -- row r < n - n_multi sits at position
    # n_multi + r, so these rows fall in position tiles 2, 0, 1 (n = 333: every
    # tile) or 4, 0, 2 (n = 700: three non-adjacent tiles), out of order, one twice
    rows = [300, 5, 150, 300, n - 1] if n == 333 else [600, 5, 300, 5]
    tiles = [(r + n_multi) // 128 if r < n - n_multi else 0 for r in rows]
    assert tiles == ([2, 0, 1, 2, 0] if n == 333 else [4, 0, 2, 0])
    gaps = [300, 5, 300]  # n = 333: tiles 2 and 0 only -- two runs with a tile between them
    with load_design(c, a, b, owner_ids=ids, env={"CMS_THRESHOLD_SLAB_ROWS": "100"}) as t, \
            load_design(c, a, b, owner_ids=ids) as whole:  # (100 rounds up to one 128-row tile)
        for thr in (v, -INF):
            exp = expected(S, ids, np.arange(n), thr)
            got = t.threshold_neighbors(ids, thr)
            assert_lists(got, exp, ("all", thr))
            assert_lists(whole.threshold_neighbors(ids, thr), got)
            for qs in (rows, gaps):
                exp = expected(S, ids, qs, thr)
                got = t.threshold_neighbors(ids[qs], thr)
                assert_lists(got, exp, (qs, thr))
                assert_lists(whole.threshold_neighbors(ids[qs], thr), got)
            assert np.array_equal(t.threshold_neighbor_counts(ids[rows], thr), np.diff(expected(S, ids, rows, thr)[0]))


# --------------------------------------------------- 3. other producers ----

@pytest.mark.parametrize("weighted", [False, True])
def test_pair_kernel_width(oracle, weighted):
    n, d, w = 70, 3, 30
    rng = _rng(30)
    c = (rng.integers(0, 300, (n, d, w)) * (rng.random((n, d, w)) < 0.4)).astype(np.uint64)
    c[11] = 0
    c[40] = c[12]
    ids = (np.cumsum(rng.integers(1, 9, n)) - 50).astype(np.int64)
    a, b = oracle.hash_params(SEED, d)
    S = sim_matrix(oracle, c.astype(np.float64), weighted)
    assert w % 128 != 0 and np.isnan(S[11]).all() and c.max() >= 256
    vals = S[5][~np.isnan(S[5])]
    v = float(np.sort(vals)[vals.size // 2])
    with load_design(c, a, b, owner_ids=ids, weighted=weighted) as t, \
            load_design(c, a, b, owner_ids=ids, weighted=weighted, env={"CMS_THRESHOLD_SLAB_ROWS": "1"}) as t128:
        for thr in (-INF, v, float(np.nextafter(v, INF)), 0.0, INF):
            assert_lists(t.threshold_neighbors(ids, thr), expected(S, ids, np.arange(n), thr), (weighted, thr))
        qs = [69, 0, 35, 0]
        assert_lists(t.threshold_neighbors(ids[qs], v), expected(S, ids, qs, v))
        assert t.stats()["multi_limb_owners"] == -1  # no limb images at this width: the pair kernel
        # 200 queries over a 128-row chunk: two chunks of the row-chunked path
        many = np.arange(200) % n
        assert_lists(t128.threshold_neighbors(ids[many], v), expected(S, ids, many, v))


def test_fp64_handle(oracle):
    n, d, w = 40, 3, 64
    rng = _rng(64)
    c = np.where(rng.random((n, d, w)) < 0.6, rng.normal(0.1, 2.0, (n, d, w)), 0.0)
    c[7] = 0.0
    ids = (np.arange(n) * 3 + 2).astype(np.int64)
    assert (c < 0).any() and (c != np.round(c * 1024) / 1024).any()  # negative and non-dyadic
    a, b = oracle.hash_params(SEED, d)
    S = sim_matrix(oracle, c)
    ok = S[~np.isnan(S)]
    assert (ok < 0).any() and (ok > 0).any() and np.isnan(S[7]).all()
    v = float(np.sort(S[3][~np.isnan(S[3])])[n // 2])
    with load_design(c, a, b, owner_ids=ids) as t:
        assert t.counters == "f64"
        for thr in (-INF, v, float(np.nextafter(v, INF)), 0.0, -0.05, INF):
            assert_lists(t.threshold_neighbors(ids, thr), expected(S, ids, np.arange(n), thr), thr)
        qs = [39, 38, 4, 5, 6, 39, 0]  # consecutive rows and a repeat
        assert_lists(t.threshold_neighbors(ids[qs], v), expected(S, ids, qs, v))


def test_per_owner_handle_is_asymmetric(oracle):
    n = 40
    users, items, ratings = movielens_like(n, 300, 2500, seed=5, min_per_user=5)
    uid = np.unique(users)
    assert uid.size == n
    rows = np.searchsorted(uid, users)
    order = np.lexsort((items, rows))
    off, keys, vals = to_csr(rows[order], items[order], n, ratings[order])
    a, b = oracle.hash_params(SEED, 32)
    t = SketchTable.per_owner_shapes(n, seed=SEED, owner_ids=uid)
    try:
        t.ingest_csr(off, keys, vals)
        t.configure_owner_shapes(1.0, 300)
        with pytest.raises(_lib.CmsError) as ei:
            t.threshold_neighbors(uid, 0.5)
        assert ei.value.code == _lib.CMS_E_STATE
        t.finalize()
        shapes = t.owner_shapes()[2:]
        assert len(set(zip(shapes[0].tolist(), shapes[1].tolist()))) > 3  # heterogeneous shapes
        S = np.array([[oracle.per_owner_similarity(off, keys, vals, shapes, a, b, u, v) for v in range(n)]
                      for u in range(n)])
        ok = S[~np.isnan(S) & ~np.eye(n, dtype=bool)]
        thr = float(np.sort(ok)[ok.size // 2])
        with np.errstate(invalid="ignore"):
            M = (S >= thr) & ~np.eye(n, dtype=bool)
        assert (M & ~M.T).any()  # some v is in u's list while u is not in v's
        assert_lists(t.threshold_neighbors(uid, thr), expected(S, uid, np.arange(n), thr))
        assert_lists(t.threshold_neighbors(uid[[9, 3, 9]], -INF), expected(S, uid, [9, 3, 9], -INF))
    finally:
        t.close()


# ----------------------------------------------------------- 4. protocol ----

def raw_call(t, q, thr, order, capacity, with_ids=True, with_scores=True):
    q = np.ascontiguousarray(q, np.int64)
    off = np.full(q.size + 1, -7, np.int64)
    ids = np.full(max(capacity, 1), -7, np.int64) if with_ids else None
    sc = np.full(max(capacity, 1), -7.0) if with_scores else None
    total = ctypes.c_int64(-7)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    rc = t._lib.cms_threshold_neighbors(t._h, p(q), q.size, thr, order, p(off), p(ids), p(sc), capacity,
                                        ctypes.byref(total))
    return rc, off, ids, sc, total.value


def test_capacity_protocol_and_refusals(oracle):
    n, w = 130, 128
    c, ids, kinds, S = mfma_case(oracle, n, w)
    q0, r0, v = star(S, kinds)
    a, b = oracle.hash_params(SEED, 2)
    exp = expected(S, ids, np.arange(n), v)
    tot = int(exp[0][-1])
    assert tot > n
    with load_design(c, a, b, owner_ids=ids, env={"CMS_THRESHOLD_SLAB_ROWS": "128"}) as t:  # two chunks
        # count only == np.diff(offsets) of the full call
        rc, off, _, _, total = raw_call(t, ids, v, 0, 0, with_ids=False, with_scores=False)
        assert rc == 0 and total == tot and np.array_equal(off, exp[0])
        assert np.array_equal(t.threshold_neighbor_counts(ids, v), np.diff(exp[0]))
        # capacity == total
        rc, off, gi, gs, total = raw_call(t, ids, v, 0, tot)
        assert rc == 0 and total == tot
        assert_lists((off, gi[:tot], gs[:tot]), exp)
        # capacity == total - 1: refused, offsets and total complete
        rc, off, _, _, total = raw_call(t, ids, v, 0, tot - 1)
        assert rc == _lib.CMS_E_PARAM and total == tot and np.array_equal(off, exp[0])
        # ... also when the first chunk alone is already too much
        rc, off, _, _, total = raw_call(t, ids, v, 0, 1)
        assert rc == _lib.CMS_E_PARAM and total == tot and np.array_equal(off, exp[0])
        # no scores
        rc, off, gi, _, total = raw_call(t, ids, v, 0, tot + 5, with_scores=False)
        assert rc == 0 and np.array_equal(gi[:tot], exp[1]) and (gi[tot:] == -7).all()
        got = t.threshold_neighbors(ids, v, scores=False)
        assert got[2] is None
        assert_lists(got, exp)
        # nq == 0
        rc, off, _, _, total = raw_call(t, np.zeros(0, np.int64), v, 0, 4)
        assert rc == 0 and total == 0 and off.tolist() == [0]
        off0, ids0, sc0 = t.threshold_neighbors([], v)
        assert off0.tolist() == [0] and ids0.size == 0 and sc0.size == 0
        # refusals
        rc, off, _, _, total = raw_call(t, [int(ids[0]), int(ids[0]) - 1], v, 0, 100)
        assert rc == _lib.CMS_E_NO_SUCH_ID and total == -7 and (off == -7).all()
        assert raw_call(t, ids, float("nan"), 0, tot)[0] == _lib.CMS_E_PARAM
        assert raw_call(t, ids, v, 2, tot)[0] == _lib.CMS_E_PARAM
        assert t._lib.cms_threshold_neighbors(t._h, None, 1, v, 0, None, None, None, 0, None) == _lib.CMS_E_PARAM
        with pytest.raises(_lib.CmsError) as ei:
            t.threshold_neighbors(ids, float("nan"))
        assert ei.value.code == _lib.CMS_E_PARAM
        with pytest.raises(_lib.CmsError) as ei:
            t.threshold_neighbors([int(ids[-1]) + 1], v)
        assert ei.value.code == _lib.CMS_E_NO_SUCH_ID
        # FastIDSet order == the FastIDSet reordering of ID order, scores with their IDs
        fexp = fastidset_order(exp)
        assert not np.array_equal(fexp[1], exp[1])
        assert_lists(t.threshold_neighbors(ids, v, order="fastidset"), fexp)
        assert_lists(t.threshold_neighbors(ids[:3], -INF), expected(S, ids, [0, 1, 2], -INF))
    with SketchTable(8, depth=2, width=128, seed=SEED) as t:
        t.ingest([0, 1, 2], [5, 5, 6])
        with pytest.raises(_lib.CmsError) as ei:
            t.threshold_neighbors([0], 0.5)
        assert ei.value.code == _lib.CMS_E_STATE


class CallLog:
    """The library, with the capacity of every cms_threshold_neighbors call noted."""

    def __init__(self, lib):
        self._lib = lib
        self.capacities = []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def cms_threshold_neighbors(self, h, q, nq, thr, order, off, oi, os_, cap, total):
        self.capacities.append(cap)
        return self._lib.cms_threshold_neighbors(h, q, nq, thr, order, off, oi, os_, cap, total)


def test_binding_retries_once_with_the_total(oracle):
    """A first guess below the total: exactly one more call, with the total."""
    n, w = 65, 128
    c, ids, kinds, S = mfma_case(oracle, n, w)
    a, b = oracle.hash_params(SEED, 2)
    exp = expected(S, ids, np.arange(n), -INF)
    assert exp[0][-1] > 10
    with load_design(c, a, b, owner_ids=ids) as t:
        lib = t._lib
        t._lib = log = CallLog(lib)
        try:
            got = t.threshold_neighbors(ids, -INF, capacity=10)
            assert log.capacities == [10, int(exp[0][-1])]
            fits = t.threshold_neighbors(ids, -INF)
            assert log.capacities[2:] == [n * (n - 1)]  # the default guess holds every list here: one call
        finally:
            t._lib = lib
        assert_lists(got, exp)
        assert_lists(fits, exp)


# ---------------------------------------------------- 5. nothing changes ----

PREPARED = ("multi_limb_owners", "deep_limb_owners", "fp4_owners")  # what the first all-pairs preparation fills


def test_call_changes_nothing(oracle):
    d, w, n = 4, 128, 200
    owners, keys = zipf_stream(500, n, 5000, seed=8)
    ids = np.arange(n, dtype=np.int64)

    def prepare(t):
        t.ingest(owners[:4000], keys[:4000])
        t.finalize()
        first = t.top_k_refresh(5)
        t.ingest(owners[4000:], keys[4000:])  # touched marks for the next refresh
        t.finalize()
        return first

    with SketchTable(n, depth=d, width=w, seed=SEED) as t, SketchTable(n, depth=d, width=w, seed=SEED) as u:
        first = prepare(t)
        before = (t.read_counters(), t.stats(), t.refresh_stats(), t.similarities(3, ids))
        t.threshold_neighbors(ids, 0.3)
        t.threshold_neighbors(ids[[7, 150, 7]], -INF, order="fastidset", scores=False)
        t.threshold_neighbor_counts(ids, 0.9)
        after = (t.read_counters(), t.stats(), t.refresh_stats(), t.similarities(3, ids))
        assert np.array_equal(before[0], after[0])
        assert {k: x for k, x in before[1].items() if k not in PREPARED} == \
               {k: x for k, x in after[1].items() if k not in PREPARED}
        assert before[2] == after[2]
        assert np.array_equal(_bits(before[3]), _bits(after[3]))
        # a following refresh is what it is on a handle that never saw the calls
        got = t.top_k_refresh(5)
        first_u = prepare(u)
        want = u.top_k_refresh(5)
        assert t.refresh_stats() == u.refresh_stats()
        for x, y in zip(first + got, first_u + want):
            assert np.array_equal(x, y, equal_nan=True)


# -------------------------------------------------------------- 6. Taste ----

D6, W6, HOW6 = 4, 1024, 5


def taste_model(seed=5, drop=None):
    users, items, ratings = movielens_like(n_users=60, n_items=300, n_ratings=3000, seed=seed)
    if drop is not None:
        keep = users != drop
        users, items, ratings = users[keep], items[keep], ratings[keep]
    uid = np.unique(users)
    rows = np.searchsorted(uid, users)
    order = np.lexsort((items, rows))
    rows, items, ratings = rows[order], items[order], ratings[order]
    off = np.zeros(uid.size + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=uid.size), out=off[1:])
    return uid, rows, items, ratings, GenericDataModel.from_csr(uid, off, items, ratings)


def test_threshold_user_neighborhood(oracle):
    uid, rows, items, ratings, model = taste_model()
    a, b = oracle.hash_params(SEED, D6)
    table = oracle.build_table(uid.size, D6, W6, a, b, rows, items, ratings)
    S = sim_matrix(oracle, table)
    ok = S[~np.isnan(S) & ~np.eye(uid.size, dtype=bool)]
    thr = float(np.quantile(ok, 0.6))
    sim = taste.CosineCM(model, taste.FixedShapeConfig(D6, W6), taste.HashFunctionBuilder(SEED))
    try:
        nbh = taste.ThresholdUserNeighborhood(thr, sim, model)
        rec = taste.GenericUserBasedRecommender(model, nbh, sim)
        hoods = {}
        for u in uid.tolist():  # the reference loop, over the pair path
            s = taste.FastIDSet()
            for other in model.getUserIDs().tolist():
                if other != u:
                    x = sim.userSimilarity(u, other)
                    if not np.isnan(x) and x >= thr:
                        s.add(other)
            hoods[u] = s.toList()
            assert nbh.getUserNeighborhood(u).tolist() == hoods[u], u
        sizes = [len(x) for x in hoods.values()]
        assert min(sizes) < max(sizes) and sum(sizes) > 10 * uid.size
        off, flat = nbh.getUserNeighborhoods(uid)
        assert flat.tolist() == [i for u in uid.tolist() for i in hoods[u]]
        assert np.diff(off).tolist() == sizes
        # recommend: the estimates of the oracle over that neighbourhood
        some = [int(uid[i]) for i in (0, 7, 23, 59)]
        for u in some:
            nb = hoods[u]
            cand = rec.getAllOtherItems(nb, u).toList()
            assert len(cand) > HOW6
            est = np.array([oracle.estimate_preference(table, a, b, int(np.searchsorted(uid, u)),
                                                       np.searchsorted(uid, nb), it, capper=rec._capper)
                            for it in cand], np.float32)
            want = taste.get_top_items(HOW6, cand, est)
            got = rec.recommend(u, HOW6)
            assert [i for i, _ in got] == [i for i, _ in want] and len(got) == min(HOW6, int(np.sum(~np.isnan(est)))) > 0
            assert [float(x) for _, x in got] == [float(x) for _, x in want]
        every = rec.recommend_all(uid, HOW6)
        for u, lst in zip(uid.tolist(), every):
            one = rec.recommend(u, HOW6)
            assert [(i, float(x)) for i, x in lst] == [(i, float(x)) for i, x in one], u
        with pytest.raises(taste.NoSuchUserException):
            nbh.getUserNeighborhood(int(uid[-1]) + 1)
    finally:
        sim.close()


def test_threshold_neighborhood_of_the_temporary_user(oracle):
    uid_all = np.unique(movielens_like(n_users=60, n_items=300, n_ratings=3000, seed=5)[0])
    gone = int(uid_all[7])
    users, items, ratings = movielens_like(n_users=60, n_items=300, n_ratings=3000, seed=5)
    tk, tv = items[users == gone], ratings[users == gone].astype(np.float32)
    uid, rows, i2, r2, base = taste_model(drop=gone)
    T = taste.PlusAnonymousUserDataModel.TEMP_USER_ID
    a, b = oracle.hash_params(SEED, D6)
    # the oracle's table with the profile's sketch in front: row -1 of ext[1:]
    ext = np.concatenate([oracle.build_table(1, D6, W6, a, b, np.zeros(tk.size, np.int64), tk, tv),
                          oracle.build_table(uid.size, D6, W6, a, b, rows, i2, r2)])
    table = ext[1:]
    sims = np.array([oracle.cosine_cm(ext[0], table[r]) for r in range(uid.size)])
    thr = float(np.quantile(sims[~np.isnan(sims)], 0.5))
    model = taste.PlusAnonymousUserDataModel(base)
    sim = taste.CosineCM(model, taste.FixedShapeConfig(D6, W6), taste.HashFunctionBuilder(SEED))
    try:
        nbh = taste.ThresholdUserNeighborhood(thr, sim, model)
        rec = taste.GenericUserBasedRecommender(model, nbh, sim)
        with pytest.raises(taste.NoSuchUserException):
            rec.recommend(T, HOW6)  # no temporary preferences yet
        model.setTempPrefs(tk, tv)
        s = taste.FastIDSet()
        for o in uid[~np.isnan(sims) & (sims >= thr)].tolist():
            s.add(o)
        nb = s.toList()
        assert 5 < len(nb) < uid.size
        assert nbh.getUserNeighborhood(T).tolist() == nb
        cand = rec.getAllOtherItems(nb, T).toList()
        est = np.array([oracle.estimate_preference(table, a, b, -1, np.searchsorted(uid, nb), it, capper=rec._capper)
                        for it in cand], np.float32)
        want = taste.get_top_items(HOW6, cand, est)
        got = rec.recommend(T, HOW6)
        assert [i for i, _ in got] == [i for i, _ in want] and len(got) == min(HOW6, int(np.sum(~np.isnan(est)))) > 0
        assert [float(x) for _, x in got] == [float(x) for _, x in want]
        # the temporary user is nobody's neighbour
        off, flat = nbh.getUserNeighborhoods(uid)
        assert T not in flat.tolist() and off[-1] == flat.size
    finally:
        sim.close()
