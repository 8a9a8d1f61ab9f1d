"""GPU: the all-pairs sketch cosine (cms_top_k_all: k_cosine_sym, k_cosine_mls,
k_cosine_tile, k_cosine_big, the candidate lists of cms_topk.hip) on DESIGNED
tables -- counters chosen one by one in numpy, written as a checkpoint image
by the format's numpy writer (mahout_amd.checkpoint.build_checkpoint) and
installed with SketchTable.load_device -- against the oracle run on the same
numpy table (`T/impl/similarity/CosineCM.java:83-96`,
`T/impl/common/DoubleCountMinSketch.java:124-147`,
`T/impl/recommender/TopItems.java:91-136`).  Bit for bit, NaN matching NaN; no
tolerance anywhere.  A hashed stream cannot place a row dot next to the
estimate/exact switch, two row quotients within 2^-17 of each other, a counter
on a class edge, or fourteen thousand scores on one threshold; a designed
table can, and every test first asserts on the CPU, from the numpy table, that
its table does.

Every test also asserts read_counters() == the design: the loader against an
independent producer of its format.

  a  estimate/exact switch of k_cosine_sym's one-register running minimum
  b  near ties (row quotients within 2^-17), int8 and fp4
  c  class edges: fp4 | int8 | 2 | 3-4 | 5 limbs, norms at 2^53
  d  thresholds: hundreds of similarities within 1e-5 of a row's k-th score
  e  multi-wave bands and the rectangle enumeration of k_cosine_sym
  f  k_cosine_big's symmetric mode (depth 6), bands and rectangles
  g  candidate-list overflow and the exact recompute (topk_redo > 0), also
     sharded and through cms_top_k_refresh

Widths.  The MFMA kernels exist where w % 128 == 0 (mfma_eligible: 128-byte K
slices); a narrower table -- w = 64 -- takes the exact per-row pair kernel for
everything, top_k_all included.  The fp4 class exists where w % 256 == 0
(cosine_prepare: whole 128-byte stages of packed 4-bit counters).  So the
whole-matrix cases run at w = 64 (the per-row path on the same designed
inputs) AND at w = 128, the narrowest width that reaches k_cosine_sym; the
band, rectangle and overflow cases, whose launch-count proof needs the waves,
run at w = 128; the fp4 cases at w = 256.  At w = 128 owners with counters <= 4
are int8-class, and the class-edge test asserts exactly that as well.

The file passes under CMS_NO_FORMS=1, CMS_NO_COMPACT=1 and CMS_NO_VMM=1: the
loader expands what a handle cannot hold, and nothing here asserts a stored
form.
"""
import math
import os

import numpy as np
import pytest

from mahout_amd import SketchTable, checkpoint as ck

pytestmark = pytest.mark.gpu

SYM_BLK, BIG_BLK = 768, 256  # rows per block of the symmetric waves: k_cosine_sym (kSymBlk), k_cosine_big (kTA)
N1 = 513                     # one 768-row block; top_k_all(512) reports every pair of every owner
K1 = 512


def _flag(name):
    return os.environ.get(name, "") not in ("", "0")


def _has_mfma(w):
    return w % 128 == 0  # mfma_eligible: narrower tables take the per-row pair kernel throughout


def _has_fp4(w):
    return w % 256 == 0 and not _flag("CMS_NO_FP4")


def class_stats(t, w):
    """(multi_limb_owners, fp4_owners) of stats(); both -1 where the width has no limb images."""
    st = t.stats()
    got = (st["multi_limb_owners"], st["fp4_owners"])
    if not _has_mfma(w):
        assert got == (-1, -1), got
    return got


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ab_est_max(d):
    """The largest row dot k_cosine_sym keeps in estimate form at depth d:
    floor(0.5 / (2^-21 + 2^(rbits - 23))), rbits = max(1, ceil(log2 d))."""
    rbits = max(1, (d - 1).bit_length())
    return math.floor(0.5 / (2.0 ** -21 + 2.0 ** (rbits - 23)))


# ---------------------------------------------------------------- CPU side --

def row_dots(c):
    """(dots [d][n][n], norms [n][d]) of a table, exact: every sum here is an
    integer below 2^53 (asserted), so fp64 BLAS sums are exact in any order."""
    f = c.astype(np.float64)
    nrm = (f * f).sum(axis=2)
    assert nrm.max() < 2.0 ** 53
    return np.stack([f[:, r, :] @ f[:, r, :].T for r in range(c.shape[1])]), nrm


def row_quotients(c):
    """(quotients [d][n][n] -- AB / (sqrt(Na) * sqrt(Nb)), the reference's own
    three correctly rounded operations, +inf where a row does not qualify --,
    dots [d][n][n])."""
    ab, nrm = row_dots(c)
    s = np.sqrt(nrm)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = s.T[:, :, None] * s.T[:, None, :]
        q = np.where(den != 0, ab / den, np.inf)
    return q, ab


# ---- a: tables whose row dots straddle ab_est_max ----

def switch_table(d, w, seed):
    """513 int8-class owners.  400 "main" owners: every row is level
    L = sqrt(M / w) plus zero-sum noise of a per-(owner, row) amplitude, so
    every main pair's row dots lie within a few thousand of M while norms and
    quotients vary; 60 higher owners (dots up to 1.7 M) and 53 lower ones."""
    rng = _rng(seed)
    M = ab_est_max(d)
    L = math.sqrt(M / w)
    kind = rng.permutation(N1)  # < 400 main, < 460 high, else low: interleaved in row order
    scale = np.where(kind < 400, 1.0, np.where(kind < 460, rng.uniform(1.05, 1.3, N1), rng.uniform(0.5, 0.95, N1)))
    level = np.minimum(L * scale, 104.9)[:, None] * np.ones((1, d))
    amax = np.minimum(22, np.floor(level) - 6)
    amp = np.floor(rng.random((N1, d)) * (amax + 1))
    base = np.floor(level)[:, :, None] + (rng.random((N1, d, w)) < (level - np.floor(level))[:, :, None])
    x = np.floor(rng.random((N1, d, w // 2)) * (amp[:, :, None] + 1))
    z = np.concatenate([x, -x], axis=2)
    z = np.take_along_axis(z, rng.random((N1, d, w)).argsort(axis=2), axis=2)
    return (base + z).astype(np.int64).astype(np.uint64)


def switch_counts(c):
    """Pairs (i < j) by where the dot of their minimum row falls, and pairs
    whose running minimum changes form (estimate <-> exact) in row order."""
    d = c.shape[1]
    M = ab_est_max(d)
    q, ab = row_quotients(c)
    iu = np.triu_indices(c.shape[0], 1)
    q, ab = q[:, iu[0], iu[1]], ab[:, iu[0], iu[1]]
    dot_min = np.take_along_axis(ab, q.argmin(axis=0)[None, :], axis=0)[0]
    cur = np.full(q.shape[1], np.inf)
    form = np.full(q.shape[1], -1)
    up = np.zeros(q.shape[1], bool)
    down = np.zeros(q.shape[1], bool)
    for r in range(d):
        take = q[r] < cur
        f = (ab[r] > M).astype(np.int64)
        change = take & (form >= 0) & (f != form)
        up |= change & (f == 1)
        down |= change & (f == 0)
        cur = np.where(take, q[r], cur)
        form = np.where(take, f, form)
    return {"below": int(((dot_min >= M - 64) & (dot_min <= M)).sum()),
            "above": int(((dot_min >= M + 1) & (dot_min <= M + 64)).sum()),
            "far": int(((dot_min >= M + 1) & (dot_min <= 2 * M)).sum()),
            "up": int(up.sum()), "down": int(down.sum()), "both": int((up & down).sum())}


# ---- b: owner pairs whose two row quotients nearly tie ----

MARGIN = 2.0 ** -17


def near_tie_table(fp4, w, seed):
    """513 owners at depth 2 (counters <= 4, or int8-class),
    made of 256 owner pairs (A, B) found by a seeded search: among the
    quotients of every two vectors of a random pool, two neighbours in sorted
    order give rows 0 and 1 of one pair.  168 pairs lie inside the 2^-17
    margin (84 with the smaller quotient in row 0, 84 in row 1) and 88 just
    outside it (1.05 to 2 margins apart)."""
    rng = _rng(seed)
    P = 1500
    if fp4:
        V = rng.integers(1, 5, (P, w)) * (rng.random((P, w)) < 0.6)
    else:
        V = rng.integers(1, 61, (P, w)) * (rng.random((P, w)) < 0.7)
        V[np.arange(P), rng.integers(0, w, P)] = rng.integers(5, 128, P)
    f = V.astype(np.float64)
    s = np.sqrt((f * f).sum(axis=1))
    iu = np.triu_indices(P, 1)
    qv = ((f @ f.T) / (s[:, None] * s[None, :]))[iu]
    order = np.argsort(qv, kind="stable")
    qs = qv[order]
    used = np.zeros(P, bool)
    pairs = []  # (vector of A row 0, of B row 0, of A row 1, of B row 1)

    def pick(lo, hi, count, later_smaller):
        # t and the first u > t with qs[u] >= qs[t] * (1 + lo): accepted when it is also below hi
        u = np.searchsorted(qs, qs * (1 + lo), side="left")
        u = np.maximum(u, np.arange(qs.size) + 1)
        ok = np.flatnonzero((u < qs.size))
        ok = ok[(qs[u[ok]] > qs[ok]) & (qs[u[ok]] - qs[ok] < hi * qs[ok]) & (qs[u[ok]] - qs[ok] > lo * qs[ok])]
        got = 0
        for t in rng.permutation(ok).tolist():
            e0, e1 = order[t], order[u[t]]  # e0: the smaller quotient
            idx = [iu[0][e0], iu[1][e0], iu[0][e1], iu[1][e1]]
            if len(set(idx)) < 4 or used[idx].any():
                continue
            used[idx] = True
            flip = later_smaller(got)
            pairs.append(tuple(idx[2:] + idx[:2]) if flip else tuple(idx))
            got += 1
            if got == count:
                return
        raise AssertionError("the search found too few pairs")

    pick(2.0 ** -40, MARGIN * 0.98, 168, lambda g: g % 2 == 1)
    pick(MARGIN * 1.05, MARGIN * 2, 88, lambda g: g % 2 == 1)
    free = np.flatnonzero(~used)
    place = rng.permutation(N1)
    c = np.zeros((N1, 2, w), np.uint64)
    for p, (a0, b0, a1, b1) in enumerate(pairs):
        c[place[2 * p]] = V[[a0, a1]]
        c[place[2 * p + 1]] = V[[b0, b1]]
    c[place[512]] = V[free[:2]]
    return c


def near_tie_counts(c):
    """Pairs (i < j) of a depth-2 table whose two quotients differ by a
    relative amount in (0, 2^-17): (smaller in row 0, smaller in row 1), and
    the pairs between one and two margins apart."""
    q, _ = row_quotients(c)
    iu = np.triu_indices(c.shape[0], 1)
    q0, q1 = q[0][iu], q[1][iu]
    lo = np.minimum(q0, q1)
    fin = np.isfinite(q0) & np.isfinite(q1) & (lo > 0)
    rel = np.where(fin, np.abs(q0 - q1) / np.where(fin, lo, 1.0), np.inf)
    inside = (rel > 0) & (rel < MARGIN)
    return int((inside & (q0 < q1)).sum()), int((inside & (q1 < q0)).sum()), int(((rel > MARGIN) & (rel < 2 * MARGIN)).sum())


# ---- c: class edges ----

EDGES = [0, 1, 4, 5, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 26]


def four_squares(N):
    """Four non-negative integers whose squares sum to N (Lagrange), largest first."""
    a = math.isqrt(N)
    while True:
        r1 = N - a * a
        b = math.isqrt(r1)
        for bb in range(b, max(b - 50, -1), -1):
            r2 = r1 - bb * bb
            c = math.isqrt(r2)
            for cc in range(c, max(c - 2000, -1), -1):
                r3 = r2 - cc * cc
                e = math.isqrt(r3)
                if e * e == r3:
                    return a, bb, cc, e
        a -= 1


def edge_table(w, extra=None, seed=7):
    """513 owners at depth 3 whose largest counters are EDGES[i % 11], in row
    order (46 or 47 owners of each value, interleaved).  An owner's other
    counters are at most 2^20, so every row norm stays below 2^53.  extra:
    "five" (owner 7 gets a counter of 2^28: five limbs), "below" (a row of
    owner 7 has the largest norm below 2^53: four squares summing to
    2^53 - 1), "at" (that, and a row of owner 18 with norm exactly 2^53)."""
    rng = _rng(seed + w)
    d = 3
    top = np.array(EDGES, np.int64)[np.arange(N1) % len(EDGES)]
    hi = np.minimum(top, 2 ** 20)
    c = np.floor(rng.random((N1, d, w)) * (hi[:, None, None] + 1)).astype(np.int64)
    c *= rng.random((N1, d, w)) < 0.3
    c[np.arange(N1), rng.integers(0, d, N1), rng.integers(0, w, N1)] = top
    if extra == "five":
        c[7, 1, 5] = 2 ** 28
    if extra in ("below", "at"):
        c[7, 0] = 0
        c[7, 0, [3, 40, 41, w - 1]] = four_squares(2 ** 53 - 1)
    if extra == "at":
        c[18, 1] = 0
        c[18, 1, [0, 77]] = 2 ** 26
    return c.astype(np.uint64)


# ---- d: similarities crowded on the thresholds ----

def screen_table(w, seed=11):
    """3000 int8-class owners at (5, w) in 50 clusters of 60, shuffled over
    the four 768-row blocks: a query, four near copies of it, and 55 members
    of a family P -- one vector with, per row, one counter moved from a bucket
    to another.  Family members are within ~1e-5 of one another (and of the
    query's fifth score), which is where the 4e-6 screen and the thresholds
    rounded down to fp16 / fp32 decide."""
    rng = _rng(seed)
    d, n = 5, 3000
    c = np.zeros((n, d, w), np.int64)
    place = rng.permutation(n)
    o = 0

    def moved(v):
        v = v.copy()
        j = rng.integers(0, w, d)
        jj = (j + rng.integers(1, w, d)) % w
        v[np.arange(d), j] += 1
        v[np.arange(d), jj] -= 1
        return v

    for _ in range(50):
        base = rng.integers(80, 121, (d, w))
        q = base + rng.integers(-2, 3, (d, w))
        p = base + rng.integers(-2, 3, (d, w))
        members = [q] + [moved(q) for _ in range(4)] + [moved(p) for _ in range(55)]
        for m in members:
            c[place[o]] = m
            o += 1
    assert o == n and c.min() >= 5 and c.max() <= 127
    return c.astype(np.uint64)


def min_quotient_matrix(c):
    """The similarity matrix [n][n] (NaN on the diagonal and where no row
    qualifies), one sketch row at a time."""
    f = c.astype(np.float64)
    nrm = (f * f).sum(axis=2)
    assert nrm.max() < 2.0 ** 53
    s = np.full((c.shape[0], c.shape[0]), np.inf)
    for r in range(c.shape[1]):
        sq = np.sqrt(nrm[:, r])
        den = sq[:, None] * sq[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.minimum(s, np.where(den != 0, (f[:, r, :] @ f[:, r, :].T) / den, np.inf))
    s = np.where(np.isfinite(s), np.minimum(s, 1.0), np.nan)
    np.fill_diagonal(s, np.nan)
    return s


def screen_counts(c, k):
    """Per query row: how many other owners' similarities lie within 1e-5 of
    the row's k-th score."""
    s = min_quotient_matrix(c)
    kth = -np.sort(-np.nan_to_num(s, nan=-1.0), axis=1)[:, k - 1]
    return (np.abs(s - kth[:, None]) <= 1e-5).sum(axis=1) - 1


# ---- e, f, g: class-designed random tables ----

def random_int8(n, d, w, seed):
    """Sparse random owners with counters in 1..30 and a largest counter in 5..104: int8 class."""
    rng = _rng(seed)
    c = rng.integers(1, 31, (n, d, w)) * (rng.random((n, d, w)) < 0.35)
    c[np.arange(n), 0, np.arange(n) % w] = 5 + np.arange(n) % 100
    return c.astype(np.uint64)


def random_fp4(n, d, w, seed):
    """Sparse random owners with counters <= 4: fp4 class where the width has one."""
    rng = _rng(seed)
    return (rng.integers(1, 5, (n, d, w)) * (rng.random((n, d, w)) < 0.4)).astype(np.uint64)


def shared_sketch_table(n, d, w, seed):
    """Four of every five owners (rows i with i % 5 < 4) hold ONE sketch --
    items each rated once by the same users -- so every pair among them has
    the same similarity and every offer between them is admitted (score >=
    thr); the rest are ordinary.  Why four fifths: a compaction leaves a list
    k entries, so in the worst case (compacted just before the band) a band
    of L waves must bring more than cap - k admitted offers: a wave offers a
    row two blocks, 2 blk f of them sharing its sketch, and L 2 blk f > cap - k
    needs f > 0.66 both for k_cosine_sym (L = 2, blk = 768, cap = 2048) and
    for k_cosine_big (L = 3, blk = 256, cap = 1024)."""
    c = random_int8(n, d, w, seed)
    c[np.arange(n) % 5 < 4] = random_int8(1, d, w, seed + 1)[0]
    return c


# ---------------------------------------------------------------- GPU side --

@pytest.fixture(scope="module")
def hp(oracle):
    cache = {}

    def get(d):
        if d not in cache:
            cache[d] = oracle.hash_params(42, d)
        return cache[d]
    return get


def load_designed(c, hp):
    """A finalized handle holding the designed table, installed through the
    loader from the numpy writer's image; read_counters() must return it."""
    import torch
    n, d, w = c.shape
    a, b = hp(d)
    image = ck.build_checkpoint(c, a, b, seed=42)
    t = SketchTable(n, depth=d, width=w, seed=42)
    try:
        dev = torch.device("cuda", t.device)
        t.load_device(torch.frombuffer(bytearray(image), dtype=torch.uint8).to(dev))
        t.finalize()
        got = t.read_counters()
        bad = np.flatnonzero((got != c).any(axis=(1, 2)))
        assert bad.size == 0, ("owners whose counters differ from the design", bad[:20], bad.size)
    except BaseException:
        t.close()
        raise
    return t


def assert_lists_equal(got, want, what):
    """Two (ids, scores, counts) list sets: the same counts and, within them, the same IDs and score bits."""
    ids, sc, cnt = got
    wids, wsc, wcnt = want
    assert np.array_equal(cnt, wcnt), (what, np.flatnonzero(cnt != wcnt)[:10])
    live = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    bad = np.flatnonzero((live & (ids != wids)).any(axis=1))
    assert bad.size == 0, (what, "ids", bad[:10], bad.size)
    eq = (sc == wsc) | (np.isnan(sc) & np.isnan(wsc))
    bad = np.flatnonzero((live & ~eq).any(axis=1))
    assert bad.size == 0, (what, "scores", bad[:10], bad.size)


def assert_rows_match_oracle(oracle, ot, lists, rows, k):
    ids, sc, cnt = lists
    n = ot.shape[0]
    owners = np.arange(n)
    for q in rows:
        eids, esc = oracle.top_users(owners, oracle.similarities_row(ot, int(q)), k)
        assert ids[q, :cnt[q]].tolist() == eids.tolist(), q
        assert _same(sc[q, :cnt[q]], esc), q


def sample_rows(n, count=30):
    return sorted(set(range(0, n, max(1, n // (count - 1)))) | {n - 1})


def check_whole_matrix(oracle, t, c):
    """n = 513, k = 512: every pair of every owner from the all-pairs kernels
    against the oracle, the per-row path, and similarities()."""
    n = c.shape[0]
    ot = np.ascontiguousarray(c, np.float64)
    allp = t.top_k_all(K1)
    assert t.stats()["topk_redo"] == 0  # (read before the per-row path, which counts its own re-selections here)
    assert_rows_match_oracle(oracle, ot, allp, range(n), K1)
    assert_lists_equal(allp, t.top_k_rows(0, n, K1), "top_k_all against top_k_rows")
    for q in (0, 7, 18, 255, n - 1):
        others = np.delete(np.arange(n), q)  # (userSimilarity(q, q) is a value; the row restatement marks self NaN)
        assert _same(t.similarities(q, others), oracle.similarities_row(ot, q)[others]), q
    return allp


# ---- a ----

@pytest.mark.parametrize("d,w", [(2, 64), (4, 64), (5, 64), (5, 128), (2, 128), (4, 128)])
def test_estimate_exact_switch(oracle, hp, d, w):
    """Row dots on both sides of ab_est_max (699,050 at d <= 2, 524,288 at
    d = 3..4, 349,525 at d = 5), where the running minimum of k_cosine_sym
    changes between its estimate form and its exact form and the dot is
    recovered as rint(est * sa * sb) with the whole 2^-21 budget in use."""
    assert [ab_est_max(x) for x in (1, 2, 3, 4, 5)] == [699050, 699050, 524288, 524288, 349525]
    c = switch_table(d, w, seed=100 + 10 * d + w)
    top = c.reshape(N1, -1).max(axis=1)
    assert top.min() >= 5 and top.max() <= 127  # every owner int8-class
    cnt = switch_counts(c)
    assert cnt["below"] >= 200 and cnt["above"] >= 200, cnt  # min-row dots in [M - 64, M] and [M + 1, M + 64]
    assert cnt["far"] >= 2000, cnt                             # ... in [M + 1, 2 M]
    assert cnt["up"] >= 200 and cnt["down"] >= 200, cnt        # the state changes form in row order, either way
    if d >= 3:
        assert cnt["both"] >= 50, cnt                          # ... both ways within one output
    nrm = (c.astype(np.float64) ** 2).sum(axis=2)
    assert np.unique(nrm).size > N1  # varied norms, not one repeated vector
    with load_designed(c, hp) as t:
        check_whole_matrix(oracle, t, c)
        assert class_stats(t, w) == ((0, 0) if _has_mfma(w) else (-1, -1))


# ---- b ----

@pytest.mark.parametrize("fp4,w", [(False, 64), (False, 128), (True, 256)], ids=["int8-64", "int8-128", "fp4-256"])
def test_near_ties(oracle, hp, fp4, w):
    """Pairs whose two row quotients differ by less than 2^-17 relative without
    being equal: the fp32 comparison of k_cosine_sym falls back to the exact
    one (exact_less), in either row order; pairs just outside the margin take
    the fp32 decision."""
    c = near_tie_table(fp4, w, seed=77 + w)
    top = c.reshape(N1, -1).max(axis=1)
    assert (top.max() <= 4 and top.min() >= 1) if fp4 else (top.min() >= 5 and top.max() <= 127)
    early, late, outside = near_tie_counts(c)
    assert early + late >= 100 and early >= 40 and late >= 40, (early, late)
    assert outside >= 50, outside
    with load_designed(c, hp) as t:
        check_whole_matrix(oracle, t, c)
        assert class_stats(t, w) == ((0, N1 if fp4 and _has_fp4(w) else 0) if _has_mfma(w) else (-1, -1))


# ---- c ----

@pytest.mark.parametrize("w", [128, 256])
def test_class_edges(oracle, hp, w):
    """Largest counters on every class edge: 4 | 5 (fp4 | int8, where the
    width has an fp4 class), 127 | 128 (one | two limbs), 16383 | 16384 (two |
    three), 2^21 - 1 | 2^21 (three | four), 2^26, and empty owners, which
    appear in no list."""
    c = edge_table(w)
    top = c.reshape(N1, -1).max(axis=1).astype(np.int64)
    assert sorted(set(top.tolist())) == EDGES and np.bincount(np.searchsorted(EDGES, top)).min() >= 46
    assert np.array_equal(top[:11], EDGES)  # interleaved in row order
    with load_designed(c, hp) as t:
        ids, sc, cnt = check_whole_matrix(oracle, t, c)
        assert class_stats(t, w) == (int((top >= 128).sum()), int((top <= 4).sum()) if _has_fp4(w) else 0)
        assert t.stats()["exact_norms"] == 1
        empty = top == 0
        assert np.all(cnt[empty] == 0) and np.all(cnt[~empty] == int((~empty).sum()) - 1)
        live = np.arange(K1)[None, :] < cnt[:, None]
        assert not np.isin(ids[live], np.flatnonzero(empty)).any()


@pytest.mark.parametrize("extra,exact", [("five", 0), ("below", 1), ("at", 0)])
def test_class_edges_fallbacks(oracle, hp, extra, exact):
    """A five-limb owner (a counter of 2^28: the multi-limb tiles stop at four
    limbs) and an owner whose row norm reaches 2^53 send the whole job to the
    per-row path; the largest norm below 2^53 does not."""
    c = edge_table(128, extra)
    n7 = sum(int(x) ** 2 for x in c[7, 0].tolist())
    if extra == "five":
        assert int(c.max()) == 2 ** 28
    else:
        assert n7 == 2 ** 53 - 1  # the largest row norm below 2^53
        if extra == "at":
            assert sum(int(x) ** 2 for x in c[18, 1].tolist()) == 2 ** 53
    with load_designed(c, hp) as t:
        assert t.stats()["exact_norms"] == exact
        n = c.shape[0]
        ot = np.ascontiguousarray(c, np.float64)
        allp = t.top_k_all(K1)
        assert_rows_match_oracle(oracle, ot, allp, range(n), K1)
        assert_lists_equal(allp, t.top_k_rows(0, n, K1), "top_k_all against top_k_rows")
        for q in (7, 18, n - 1):
            others = np.delete(np.arange(n), q)
            assert _same(t.similarities(q, others), oracle.similarities_row(ot, q)[others]), q


# ---- d ----

@pytest.mark.parametrize("w", [64, 128])
def test_threshold_screening(oracle, hp, w):
    """Four blocks, k = 5: most rows have dozens of candidates within 1e-5 of
    their k-th score while their thresholds rise from wave to wave (w = 128;
    at w = 64 the per-row path selects among the same crowded scores)."""
    k = 5
    c = screen_table(w)
    near = screen_counts(c, k)
    assert int((near >= 20).sum()) >= 2000, int((near >= 20).sum())
    n = c.shape[0]
    with load_designed(c, hp) as t:
        allp = t.top_k_all(k)
        assert t.stats()["topk_redo"] == 0
        assert_lists_equal(allp, t.top_k_rows(0, n, k), "top_k_all against top_k_rows")
        assert_rows_match_oracle(oracle, np.ascontiguousarray(c, np.float64), allp, sample_rows(n), k)


# ---- e, f: bands and rectangles ----

def band_launches(nbk, k):
    """Launches of one pass over nbk blocks (band_list of top_k_all)."""
    wv = count = 0
    while wv <= nbk // 2:
        L = 1 if wv < 8 else max(1, min(32, wv * 25 // max(1, k)))
        wv += min(L, nbk // 2 - wv + 1)
        count += 1
    return count


def check_bands(oracle, hp, c, k, blk, expect_f4, expect_i8, no_redo=True):
    """The whole job on a table of designed classes: equal to the per-row path
    on every row and to the oracle on ~30, no redo, and -- the proof that
    multi-wave bands ran -- fewer launches per pass than the pass has waves."""
    n = c.shape[0]
    with load_designed(c, hp) as t:
        t.set_timing(True, 2)
        t.reset_timing()
        allp = t.top_k_all(k)
        launches = {"f4": t.timing("topk_all_waves_f4")[1], "i8": t.timing("topk_all_waves_i8")[1]}
        t.set_timing(False)
        st = t.stats()
        print("topk_redo", st["topk_redo"], "launches", launches)
        assert st["topk_redo"] == 0 or not no_redo
        nm, nf = st["multi_limb_owners"], st["fp4_owners"]
        assert nm == 0
        n8 = n - nm - nf
        f0 = min(n, nm + (n8 + blk - 1) // blk * blk)  # the fp4 region starts on a block boundary
        nbk_f4 = (n - f0 + blk - 1) // blk
        nbk_i8 = (n - nm + blk - 1) // blk if n8 > 0 else 0
        assert (nbk_f4 >= 19) == expect_f4 and (nbk_i8 >= 19) == expect_i8, (nbk_f4, nbk_i8)
        assert n % blk != 0  # a partial last block
        for name, nbk, expect in (("f4", nbk_f4, expect_f4), ("i8", nbk_i8, expect_i8)):
            if expect:
                assert 0 < launches[name] < nbk // 2 + 1, (name, launches, nbk)
                assert launches[name] == band_launches(nbk, k), (name, launches, nbk)
            else:
                assert launches[name] == 0, (name, launches)
        assert_lists_equal(allp, t.top_k_rows(0, n, k), "top_k_all against top_k_rows")
        assert_rows_match_oracle(oracle, np.ascontiguousarray(c, np.float64), allp, sample_rows(n), k)
    return nbk_f4, nbk_i8


def test_sym_bands_int8_rect(oracle, hp):
    """31 int8 blocks of 768: the band from wave 8 on is 8 waves wide (g.rect = 1)."""
    _, nbk = check_bands(oracle, hp, random_int8(23100, 2, 128, 201), 10, SYM_BLK, False, True)
    assert nbk >= 30


def test_sym_bands_fp4_rect(oracle, hp):
    """31 fp4 blocks of 768 (w = 256: the narrowest width with an fp4 class)."""
    f4 = _has_fp4(256)  # (CMS_NO_FP4: the same owners are int8-class)
    nbk = check_bands(oracle, hp, random_fp4(23100, 2, 256, 202), 10, SYM_BLK, f4, not f4)
    assert max(nbk) >= 30


@pytest.mark.parametrize("alike", [True, False], ids=["alike", "unlike"])
def test_sym_bands_mixed_fsel(oracle, hp, alike):
    """10 int8 blocks beside 20 fp4 blocks: the fp4 pass runs a 3-wave band,
    the int8 pass 8-wave bands restricted to pairs with an int8 block (fsel:
    no rectangles).

    alike: the int8-class owners are fp4-like sketches times 3, so both
    classes' similarities have one distribution and no list overflows.
    unlike: the int8-class owners are random_int8 sketches, for which fp4
    owners are better candidates than int8 ones: the thresholds their first
    eight waves leave (mostly int8 partners) admit a large share of the 8-wave
    band's fp4 partners, and on the MI355X about a hundred lists overflow and
    are recomputed (topk_redo was 102) -- so here the redo count is printed,
    not asserted, and the lists must be exact all the same."""
    n, n8 = 22500, 7400
    c = random_fp4(n, 2, 256, 203)
    rows8 = np.sort(_rng(204).permutation(n)[:n8])
    c[rows8] = 3 * random_fp4(n8, 2, 256, 206) if alike else random_int8(n8, 2, 256, 205)
    if alike:
        c[rows8, 0, rows8 % 256] = 6  # (every one of them int8-class: a counter above 4)
    nbk_f4, nbk_i8 = check_bands(oracle, hp, c, 10, SYM_BLK, _has_fp4(256), True, no_redo=alike)
    assert (nbk_f4, nbk_i8) == ((20, 30) if _has_fp4(256) else (0, 30))


@pytest.mark.parametrize("n,k", [(7700, 10), (4900, 100)])
def test_big_symmetric_mode(oracle, hp, n, k):
    """Depth 6: sym_lds_bytes(6) exceeds 160 KiB, so the waves run on
    k_cosine_big's symmetric mode with 256-row blocks -- 31 blocks and an
    8-wave rectangle band at k = 10, 20 blocks and a 2-wave band at k = 100."""
    _, nbk = check_bands(oracle, hp, random_int8(n, 6, 128, 300 + k), k, BIG_BLK, False, True)
    assert nbk >= (30 if k == 10 else 19)
    assert band_launches(nbk, k) == (9 if k == 10 else 10)


# ---- g: overflow and the exact recompute ----

@pytest.mark.parametrize("n,d,w", [(14000, 2, 128), (5200, 6, 128)], ids=["sym", "big"])
def test_overflow_redo(oracle, hp, n, d, w):
    """80 % of the owners share one sketch: a band of L >= 2 waves offers each
    of them more 1.0 scores than its candidate list has room for, the lists
    overflow, and the rows are recomputed exactly (slab_top_k_positions) --
    the ID tie-break over thousands of equal scores included.  The sharded job
    and the incremental refresh go through the same path."""
    k = 10
    c = shared_sketch_table(n, d, w, 400 + d)
    shared = np.arange(n) % 5 < 4
    assert (c[shared] == c[0]).all() and c[0].max() >= 5 and c.max() <= 127
    blk = SYM_BLK if d <= 5 else BIG_BLK
    nbk = (n + blk - 1) // blk
    assert nbk >= 19 and band_launches(nbk, k) < nbk // 2 + 1  # a band of L >= 2 waves
    ot = np.ascontiguousarray(c, np.float64)
    rows = sample_rows(n)
    with load_designed(c, hp) as t:
        allp = t.top_k_all(k)
        redo = t.stats()["topk_redo"]
        assert redo > 0
        perrow = t.top_k_rows(0, n, k)
        assert_lists_equal(allp, perrow, "top_k_all against top_k_rows")
        assert_rows_match_oracle(oracle, ot, allp, rows, k)
        first = np.flatnonzero(shared)[:k + 1]  # a shared owner's list: the k lowest shared IDs but its own
        assert allp[0][first[-1]].tolist() == first[:k].tolist()
        # sharded
        parts = [t.top_k_all_partial(k, s, 3) for s in range(3)]
        assert_lists_equal(t.top_k_merge(k, parts), perrow, "3 shards merged against top_k_rows")
        # refresh after a small further batch
        assert_lists_equal(t.top_k_refresh(k), perrow, "first refresh (whole job) against top_k_rows")
        rng = _rng(9)
        brow = np.concatenate([rng.integers(0, n, 40), [0, 3, n - 1]]).astype(np.int64)
        bkey = rng.integers(0, 5000, brow.size).astype(np.int64)
        t.ingest(brow, bkey)
        t.finalize()
        a, b = hp(d)
        ot2 = ot + oracle.build_table(n, d, w, a, b, brow, bkey)
        assert np.array_equal(t.read_counters(), ot2)
        refreshed = t.top_k_refresh(k)
        fresh = t.top_k_all(k)
        assert t.stats()["topk_redo"] > redo
        assert_lists_equal(refreshed, fresh, "refresh against a fresh top_k_all")
        assert_lists_equal(fresh, t.top_k_rows(0, n, k), "fresh top_k_all against top_k_rows")
        assert_rows_match_oracle(oracle, ot2, refreshed, sorted(set(rows) | set(brow.tolist())), k)
