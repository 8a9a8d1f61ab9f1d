"""Per-owner all-pairs (cms_profiles.hip) on the designed DataModels of
tests/po_designs.py: every kernel top_k_all / top_k_rows / similarities is
routed through -- k_po_pairs<64> (LDS row, LDS hash table, global scratch
row), k_po_group_pairs (dense and sparse dots), k_po_bigq,
k_po_wide_bound<1|2> and k_po_pairs<256> (sweep, global row) -- at the
thresholds between them, with exact ties at the prune's k-th score, query
windows that do not start at row 0, and norms past 2^53.

The reference is oracle.per_owner_similarity for every ordered pair (one
matrix per design, computed once and shared) and oracle.top_users on its
rows; every comparison is bit for bit, NaN equal to NaN.
tests/test_per_owner_designed_host.py shows on the CPU that each design has
the property its test here relies on; the counters and launch counts below
show that the path in question ran."""
import contextlib

import numpy as np
import pytest

import po_designs as P
from mahout_amd import SketchTable

pytestmark = pytest.mark.gpu

KNOBS = ("CMS_PO_NO_PRUNE", "CMS_PO_NO_BIGQ", "CMS_PO_BOUND_ROWS", "CMS_PO_BOUND_PART2", "CMS_PO_DENSE_X4")
PRUNE_ON = {"CMS_PO_NO_PRUNE": 0}
BIGQ_ON = {"CMS_PO_NO_BIGQ": 0}


@contextlib.contextmanager
def handle(D, oracle, monkeypatch, env=None, weighted=False):
    """A finalized per-owner handle of design D.  The knobs are read when the
    handle is created: the ones a test is about are set here, before it."""
    for name, v in (env or {}).items():
        assert name in KNOBS
        monkeypatch.setenv(name, str(v))
    with SketchTable.per_owner_shapes(D.n, seed=P.SEED, weighted=weighted, owner_ids=D.uid) as t:
        t.ingest_csr(D.off, D.keys, D.vals)
        t.set_owner_delta_epsilon(*D.delta_epsilon(oracle))
        t.finalize()
        _, _, w, d = t.owner_shapes()
        assert np.array_equal(w, D.w) and np.array_equal(d, D.d)
        t.set_timing(True, 2)
        yield t


def launches(t, scope):
    t.synchronize()
    return t.timing(scope)[1]


def check_lists(D, oracle, lists, k, rows=None, weighted=False):
    """lists[i] is the mostSimilar list of owner row rows[i]: the oracle's
    TopItems loop over the reference row, IDs and scores."""
    ids, sc, cnt = lists
    rows = range(D.n) if rows is None else rows
    assert len(ids) == len(rows)
    for i, q in enumerate(rows):
        eids, esc = D.expected_list(oracle, q, k, weighted)
        c = int(cnt[i])
        assert ids[i, :c].tolist() == eids.tolist(), (D.name, q, k)
        assert P.same(sc[i, :c], esc), (D.name, q, k)


def wide_counters(t):
    st = t.stats()
    return st["po_wide_pairs"], st["po_wide_exact"]


def bounded_in_lists(D, oracle, k, part2=True, weighted=False):
    """(query, bounded candidate) pairs of the expected lists: each of them
    must have survived the bound."""
    b = D.bounded(part2)
    return sum(int(b[D.rows_of(D.expected_list(oracle, q, k, weighted)[0])].sum()) for q in range(D.n))


# ------------------------------------------------------------------ (a) --

@pytest.mark.parametrize("weighted", [False, True])
def test_pairs64_every_row_kind(oracle, monkeypatch, weighted):
    """k_po_pairs<64> through `similarities`: cached and streamed queries
    against the LDS row, the LDS hash table and the global scratch row; empty
    owners, an all-zero sketch and zero-valued preferences."""
    D = P.get(oracle, "pairs64")
    R = D.ref(oracle, weighted)
    with handle(D, oracle, monkeypatch, weighted=weighted) as t:
        n0 = launches(t, "po_pair_cosine")
        for q in range(D.n):
            assert P.same(t.similarities(int(D.uid[q]), D.uid), R[q]), q
        assert launches(t, "po_pair_cosine") == n0 + D.n  # one k_po_pairs launch per row
        for q, c in [(8, 5), (5, 8), (0, 3), (3, 0), (12, 12)]:
            assert P.same(t.similarity(int(D.uid[q]), int(D.uid[c])), R[q, c])
        for k in (3, D.n - 1):
            check_lists(D, oracle, t.top_k_all(k), k, weighted=weighted)


# ------------------------------------------------------------------ (b) --

GROUP_ENVS = {
    "default": {},
    "part2_in_groups": {"CMS_PO_BOUND_PART2": 0},
    "all_sparse": {"CMS_PO_BOUND_PART2": 0, "CMS_PO_DENSE_X4": 0},
    "all_dense": {"CMS_PO_BOUND_PART2": 0, "CMS_PO_DENSE_X4": 1 << 20},
}


@pytest.mark.parametrize("variant", list(GROUP_ENVS))
def test_group_kernel_class_edges(oracle, monkeypatch, variant):
    """k_po_group_pairs on classes at every width edge with 1 .. 129 members:
    top_k_all lists, and with k = n - 1 every computed row, equal the oracle;
    the same under all-sparse and all-dense dots."""
    D = P.get(oracle, "group")
    with handle(D, oracle, monkeypatch, GROUP_ENVS[variant]) as t:
        for k in (7, D.n - 1):  # k = n - 1: the list is the whole row, sorted
            g0 = launches(t, "po_group_pairs")
            check_lists(D, oracle, t.top_k_all(k), k)
            assert launches(t, "po_group_pairs") > g0
        if variant == "default":  # the per-pair kernel on a few whole rows as well
            R = D.ref(oracle)
            for q in (0, 100, D.n - 1):
                assert P.same(t.similarities(int(D.uid[q]), D.uid), R[q])


# ---------------------------------------------------------- (c) (d) (f) --

def test_big_queries_and_survivor_lists(oracle, monkeypatch):
    """k_po_bigq (classes of 1 .. 257 members; w d = 38,912 taken, 40,960
    passed by -- in this default routing to the bound kernel and
    k_po_pairs<256>), the bound kernel and its three survivor lists: the
    pruned top_k_all(10) and the unpruned whole rows (k = n - 1: big queries
    against every bounded owner through k_po_pairs<256>) equal the oracle."""
    D = P.get(oracle, "mixed")
    k = P.PRUNE_K
    with handle(D, oracle, monkeypatch, {**PRUNE_ON, **BIGQ_ON}) as t:
        lists = t.top_k_all(k)
        check_lists(D, oracle, lists, k)
        pairs, exact = wide_counters(t)
        assert pairs == D.n * int(D.bounded().sum())
        assert bounded_in_lists(D, oracle, k) <= exact < pairs  # pruned, and every listed pair survived
        assert launches(t, "po_bigq") == 1 and launches(t, "po_wide_bound") == 1
        assert launches(t, "po_group_pairs") == 1 and launches(t, "po_pair_cosine") >= 1
        check_lists(D, oracle, t.top_k_all(D.n - 1), D.n - 1)
        pairs2, exact2 = wide_counters(t)
        # tcnt < k: nothing pruned (the big queries' part-2 candidates are k_po_bigq's, not the bound kernel's)
        assert D.bigq_pairs() > 0
        assert (pairs2 - pairs, exact2 - exact) == (pairs, pairs - D.bigq_pairs())


MIXED_ENVS = {
    "no_bigq": {"CMS_PO_NO_BIGQ": 1, **PRUNE_ON},
    "no_prune": {"CMS_PO_NO_PRUNE": 1, **BIGQ_ON},
    "part2_in_groups": {"CMS_PO_BOUND_PART2": 0, **PRUNE_ON, **BIGQ_ON},
    "bound_rows2": {"CMS_PO_BOUND_ROWS": 2, **PRUNE_ON, **BIGQ_ON},
}


@pytest.mark.parametrize("variant", list(MIXED_ENVS))
def test_big_queries_under_every_routing(oracle, monkeypatch, variant):
    """The mixed design's lists and whole rows (k = n - 1) under the other
    routings.  With the prune off, or part 2 left to the group kernel, the
    2048 x 20 class's pairs with the big queries are k_po_group_pairs' and
    the 2048 x 19 class's are k_po_bigq's (the w d <= 38,912 split; the host
    test restates the routing): those pairs rank near the end of their rows,
    so only the whole rows pin them."""
    D = P.get(oracle, "mixed")
    env = MIXED_ENVS[variant]
    with handle(D, oracle, monkeypatch, env) as t:
        for k in (P.PRUNE_K, D.n - 1):
            b0, w0, g0 = launches(t, "po_bigq"), launches(t, "po_wide_bound"), launches(t, "po_group_pairs")
            check_lists(D, oracle, t.top_k_all(k), k)
            assert launches(t, "po_bigq") - b0 == (0 if env.get("CMS_PO_NO_BIGQ") else 1)
            assert launches(t, "po_wide_bound") - w0 == (0 if env.get("CMS_PO_NO_PRUNE") else 1)
            assert launches(t, "po_group_pairs") - g0 == 1
        if env.get("CMS_PO_NO_PRUNE"):
            assert wide_counters(t) == (0, 0)
        if "CMS_PO_BOUND_PART2" in env:  # only the wide owners are bounded
            assert wide_counters(t)[0] == 2 * D.n * int(D.wide().sum())


WINDOWS = [(1, 64), (37, 63), (37, 64), (37, 65), (1, 7), (37, 7), (-1, 1), (-7, 7)]


def test_top_k_rows_from_a_later_row(oracle, monkeypatch):
    """top_k_rows with row_begin != 0 (q0 in k_po_bigq, the bound kernel, the
    listed pairs' store and the redo scatter): windows of 1, 7, 63, 64 and 65
    rows from rows 1, 37 and n - 1 equal the same rows of top_k_all and the
    oracle's lists."""
    D = P.get(oracle, "mixed")
    k = P.PRUNE_K
    with handle(D, oracle, monkeypatch, {**PRUNE_ON, **BIGQ_ON}) as t:
        ids, sc, cnt = t.top_k_all(k)
        for rb, rc in WINDOWS:
            rb = rb % D.n
            rows = range(rb, rb + rc)
            b0, w0 = launches(t, "po_bigq"), launches(t, "po_wide_bound")
            got = t.top_k_rows(rb, rc, k)
            check_lists(D, oracle, got, k, rows)
            assert np.array_equal(got[2], cnt[rb:rb + rc])
            for i, q in enumerate(rows):
                assert got[0][i, :cnt[q]].tolist() == ids[q, :cnt[q]].tolist() and P.same(got[1][i, :cnt[q]], sc[q, :cnt[q]])
            has_big = bool((D.nnz[rb:rb + rc] > P.PO_BIG_QUERY).any())
            assert launches(t, "po_bigq") - b0 == int(has_big)
            assert launches(t, "po_wide_bound") - w0 == 1
        assert sum(bool((D.nnz[rb % D.n:rb % D.n + rc] > P.PO_BIG_QUERY).any()) for rb, rc in WINDOWS) >= 3


# ------------------------------------------------------------------ (e) --

PRUNE_ENVS = {
    "rows1": {"CMS_PO_BOUND_ROWS": 1},
    "rows2": {"CMS_PO_BOUND_ROWS": 2},
    "part2_off": {"CMS_PO_BOUND_PART2": 0},
    "part2_on_rows2": {"CMS_PO_BOUND_PART2": 1, "CMS_PO_BOUND_ROWS": 2},
}


def _prune_case(oracle, monkeypatch, nb, env, weighted=False):
    D = P.get(oracle, "prune", nb)
    k = P.PRUNE_K
    part2 = bool(int(env.get("CMS_PO_BOUND_PART2", 1)))
    nbound = int(D.bounded(part2).sum())
    with handle(D, oracle, monkeypatch, {**PRUNE_ON, **env}, weighted) as t:
        check_lists(D, oracle, t.top_k_all(k), k, weighted=weighted)
        pairs, exact = wide_counters(t)
        assert pairs == D.n * nbound
        # something was pruned; every bounded pair of the expected lists (the ties among them) was not
        listed = bounded_in_lists(D, oracle, k, part2, weighted)
        if weighted:  # normalizeWeightResult takes every score >= 0 to 1.0: no bound is below a k-th score
            assert 0 < listed <= exact == pairs
        else:
            assert 0 < listed <= exact < pairs
        assert launches(t, "po_wide_bound") == 1
        # a list longer than the narrow candidates can fill: nothing may be pruned
        k2 = P.prune_long_k(D)
        check_lists(D, oracle, t.top_k_all(k2), k2, weighted=weighted)
        pairs2, exact2 = wide_counters(t)
        assert pairs2 - pairs == pairs and exact2 - exact == pairs


@pytest.mark.parametrize("nb", [1, 63, 64, 65])
def test_prune_keeps_ties_at_the_kth_score(oracle, monkeypatch, nb):
    """Bounded owners whose score ties the narrow candidates' k-th score
    (exactly 1.0) and who sort ahead of them: the expected lists hold them, so
    the bound's strict `<` must have kept them -- while other pairs are pruned."""
    _prune_case(oracle, monkeypatch, nb, {})


@pytest.mark.parametrize("variant", list(PRUNE_ENVS))
def test_prune_ties_under_bound_knobs(oracle, monkeypatch, variant):
    _prune_case(oracle, monkeypatch, 65, PRUNE_ENVS[variant])


def test_prune_ties_weighted(oracle, monkeypatch):
    _prune_case(oracle, monkeypatch, 65, {}, weighted=True)


def test_prune_ties_without_prune(oracle, monkeypatch):
    D = P.get(oracle, "prune", 65)
    with handle(D, oracle, monkeypatch, {"CMS_PO_NO_PRUNE": 1}) as t:
        check_lists(D, oracle, t.top_k_all(P.PRUNE_K), P.PRUNE_K)
        assert wide_counters(t) == (0, 0) and launches(t, "po_wide_bound") == 0


# ------------------------------------------------------------------ (g) --

@pytest.mark.parametrize("env", [{}, {"CMS_PO_BOUND_ROWS": 2}, {"CMS_PO_BOUND_PART2": 0}],
                         ids=["default", "bound_rows2", "part2_in_groups"])
def test_inexact_regime_on_every_path(oracle, monkeypatch, env):
    """Norms past 2^53 replayed in the reference's sequential order: through
    the group kernel's redo list, k_po_bigq's redo list, a wide owner's own
    norm, and queries of sum v >= 2^26 (never pruned, global-row list).  Every
    redo pair is one more `po_pair_cosine` launch beside the slab's own one,
    and the design gives their number exactly; a window holding only the big
    query has k_po_bigq's redo pairs alone, the rows after it the group
    kernel's alone.  (A heavy query kept off the global-row list would end in
    the library's `needed a global bucket row` error: its pairs with the
    owners past 4096 counters have valueA past 2^53 -- the host test.)"""
    D = P.get(oracle, "inexact")
    R = D.ref(oracle)
    part2 = bool(int(env.get("CMS_PO_BOUND_PART2", 1)))
    big = D.tags["big"]
    with handle(D, oracle, monkeypatch, {**PRUNE_ON, **BIGQ_ON, **env}) as t:
        p0 = launches(t, "po_pair_cosine")
        check_lists(D, oracle, t.top_k_all(5), 5)
        pairs, exact = wide_counters(t)
        assert pairs == D.n * int(D.bounded(part2).sum())
        assert launches(t, "po_bigq") == 1 and launches(t, "po_wide_bound") == 1
        group_redo, bigq_redo = D.redo_pairs(oracle, part2=part2)
        assert group_redo > 0 and bigq_redo > 0
        assert launches(t, "po_pair_cosine") - p0 == 1 + group_redo + bigq_redo
        # the heavy queries' pairs with every bounded owner were computed, not pruned
        heavy = [D.tags[x] for x in ("n_heavy", "w_heavy", "w_heavy_lds", "p2_heavy")]
        assert exact >= len(heavy) * int(D.bounded(part2).sum())
        check_lists(D, oracle, t.top_k_all(D.n - 1), D.n - 1)  # whole rows
        for rb, rc in [(big, 1), (big + 1, D.n - big - 1), (1, 7)]:
            rows = range(rb, rb + rc)
            p0 = launches(t, "po_pair_cosine")
            check_lists(D, oracle, t.top_k_rows(rb, rc, 5), 5, rows)
            g, b = D.redo_pairs(oracle, rows, part2=part2)
            assert (g == 0) == (rb == big) and (b == 0) == (big not in rows)
            assert launches(t, "po_pair_cosine") - p0 == 1 + g + b
        for q in range(D.n):
            assert P.same(t.similarities(int(D.uid[q]), D.uid), R[q]), q
