"""CPU companion of tests/test_gpu_per_owner_designed.py: shows from the
oracle alone that every designed DataModel of tests/po_designs.py has the
property its GPU test relies on -- the intended shapes, the path edges, exact
ties at the k-th score, each survivor kind in the expected lists, norms past
2^53 where claimed -- and that the cached reference matrix is
oracle.per_owner_similarity pair for pair."""
import numpy as np
import pytest

import po_designs as P


def _own_norms(oracle, D, r):
    """Exact sum of squares of every row of owner r's own sketch."""
    a, b = oracle.hash_params(P.SEED, 32)
    sk = oracle.export_profile(D.off, D.keys, D.vals, r, int(D.w[r]), int(D.d[r]), a, b)
    return [sum(int(x) ** 2 for x in row) for row in sk]


def _norms_at(oracle, D, q, c):
    """Exact valueA of every row of q's sketch built at c's shape."""
    a, b = oracle.hash_params(P.SEED, 32)
    sk = oracle.export_profile(D.off, D.keys, D.vals, q, int(D.w[c]), int(D.d[c]), a, b)
    return [sum(int(x) ** 2 for x in row) for row in sk]


DESIGNS = [("pairs64",), ("group",), ("mixed",), ("prune", 1), ("prune", 63), ("prune", 64), ("prune", 65),
           ("inexact",)]


@pytest.mark.parametrize("key", DESIGNS, ids=lambda k: "-".join(map(str, k)))
def test_shapes_and_reference_composition(oracle, key):
    D = P.get(oracle, *key)
    de, ep = D.delta_epsilon(oracle)  # asserts oracle.owner_shapes(de, ep) == the intended (w, d)
    assert (de > 0).all() and (ep > 0).all()
    a, b = oracle.hash_params(P.SEED, 32)
    rng = np.random.default_rng(1)
    if D.n <= 40:
        pairs = [(u1, u2) for u1 in range(D.n) for u2 in range(D.n)]
    else:
        pairs = [(int(x), int(y)) for x, y in rng.integers(0, D.n, (300, 2))]
        pairs += [(r, c) for r in D.tags.values() if isinstance(r, int) for c in D.tags.values() if isinstance(c, int)]
    for weighted in (False, True):
        R = D.ref(oracle, weighted)
        for u1, u2 in pairs:
            e = oracle.per_owner_similarity(D.off, D.keys, D.vals, D.shapes, a, b, u1, u2, weighted)
            assert P.same(R[u1, u2], e), (u1, u2, weighted)


def test_group_design_sparse_oracle_agrees(oracle):
    """Unit preferences: oracle.per_owner_rows_csr is a second opinion on the
    whole matrix."""
    D = P.get(oracle, "group")
    assert D.unit
    a, b = oracle.hash_params(P.SEED, 32)
    R = D.ref(oracle)
    for q0 in range(0, D.n, 64):
        qs = np.arange(q0, min(D.n, q0 + 64))
        assert P.same(oracle.per_owner_rows_csr(D.off, D.keys, D.shapes, a, b, qs, threads=4), R[qs])


def test_pairs64_design_edges(oracle):
    D = P.get(oracle, "pairs64")
    assert {0, 1, 63, 64, 65, 255, 256, 257, 600} <= set(D.nnz.tolist())
    assert {1, 2, 4095, 4096, 4097, 9000, 16384, 16385} <= set(D.w.tolist())
    assert {1, 2, 5, 32} <= set(D.d.tolist())
    # cached (<= 256) and streamed queries meet the LDS row, the table's range and the global row
    assert ((D.nnz <= P.PO_CACHED) & (D.nnz > 0)).sum() >= 4 and (D.nnz > P.PO_CACHED).sum() >= 4
    assert (D.w > P.PO_HIST).sum() >= 4 and (D.w <= P.PO_HIST).sum() >= 4
    R = D.ref(oracle)
    dead = D.tags["empty"] + [D.tags["zero_sketch"]]
    for c in dead:  # an all-zero candidate sketch: den == 0 in every row
        assert np.isnan(R[:, c]).all()
    for q in dead:  # and an all-zero query
        assert np.isnan(R[q]).all()
    live = [r for r in range(D.n) if r not in dead]
    assert not np.isnan(R[np.ix_(live, live)]).any()
    for r in D.tags["zero_vals"]:  # zero-valued preferences among non-zero ones
        v = D.vals[D.off[r]:D.off[r + 1]]
        assert (v == 0).any() and (v > 0).any()
    assert not P.same(D.ref(oracle, True), R)  # the weighted matrix is another one


def test_group_design_edges(oracle):
    D = P.get(oracle, "group")
    cl = D.classes()
    assert sorted({w for w, _ in cl}) == P.GROUP_WIDTHS
    assert {1, 63, 64, 65, 129} <= {len(v) for v in cl.values()}
    nn = set(D.nnz.tolist())
    for w in P.GROUP_SWITCH:  # nnz = w - 1 (sparse), w and w + 1 (dense) against a class of width w
        assert {w - 1, w, w + 1} <= nn and any(cw == w for cw, _ in cl)
    assert any(x % 8 and x > 8 for x in nn) and any(x % 64 and x > 64 for x in nn)
    assert set((D.nnz % 8).tolist()) == set(range(8))
    # dense and sparse both occur for every class under the default switch (w <= nnz)
    for w, _ in cl:
        assert (D.nnz >= w).any() and ((D.nnz < w) & (D.nnz > 0)).any() or w == 1
    R = D.ref(oracle)
    assert len(np.unique(R[~np.isnan(R)])) > 1000  # scores spread: lists are not all ties


def test_mixed_design_edges(oracle):
    D = P.get(oracle, "mixed")
    cl = D.classes()
    narrow = {s: v for s, v in cl.items() if s[0] <= P.PO_GROUP_W}
    assert {1, 2, 3, 5, 64, 65, 257} <= {len(v) for v in narrow.values()}
    dws = {w * d for w, d in narrow}
    assert P.PO_BIG_MAX_DW in dws and 2048 * 20 in dws
    assert {4096, 4097, 5000, 6000} <= set(D.nnz.tolist())
    assert {16384, 16385} <= set(D.w.tolist()) and D.part2().sum() >= 2 and D.wide().sum() >= 6
    big = np.flatnonzero(D.nnz > P.PO_BIG_QUERY)
    assert big.size >= 4 and (big >= 37).all() and (big < 37 + 63).all()  # inside every window from row 37
    # each survivor kind of the bound kernel has a pair in the expected top-k
    kinds = set()
    sweep = grow = False
    for q in range(D.n):
        ids, _ = D.expected_list(oracle, q, P.PRUNE_K)
        for c in D.rows_of(ids):
            if D.wide()[c]:
                kinds.add(D.survivor_kind(q, c))
                if D.nnz[q] > P.PO_BIG_QUERY:
                    sweep |= D.w[c] <= P.PO_BIGROW
                    grow |= D.w[c] > P.PO_BIGROW
    assert kinds == {0, 1, 2} and sweep and grow
    # the w d <= 38,912 split: a big query's pair with the 2048 x 19 class is k_po_bigq's; with the 2048 x 20
    # class it is the group kernel's when part 2 is not bounded (no prune, or CMS_PO_BOUND_PART2=0) and
    # the bound kernel's (then k_po_pairs<256>'s) by default
    c19, c20 = D.tags["c19"], D.tags["c20"]
    assert D.w[c19] * D.d[c19] == P.PO_BIG_MAX_DW and D.w[c20] * D.d[c20] == 2048 * 20
    for q in big:
        for kw in ({}, {"prune": False}, {"part2": False}):
            assert D.narrow_route(q, c19, **kw) == "bigq"
        assert D.narrow_route(q, c20) == "bound"
        assert D.narrow_route(q, c20, prune=False) == "group" and D.narrow_route(q, c20, part2=False) == "group"
        assert D.narrow_route(q, c19, bigq=False, prune=False) == "group"
    small = int(np.flatnonzero(D.nnz <= P.PO_BIG_QUERY)[0])
    assert D.narrow_route(small, c19, prune=False) == "group" and D.narrow_route(small, c20, prune=False) == "group"
    # and the narrow candidates alone fill a list of PRUNE_K for every query (tcnt >= k: the prune is armed)
    R = D.ref(oracle)
    nar = ~D.bounded()
    assert all((~np.isnan(R[q, nar])).sum() - (1 if nar[q] else 0) >= P.PRUNE_K for q in range(D.n))


@pytest.mark.parametrize("nb", [1, 63, 64, 65])
def test_prune_design_ties(oracle, nb):
    D = P.get(oracle, "prune", nb)
    k = P.PRUNE_K
    assert int(D.bounded().sum()) == nb and D.bounded()[:nb].all()
    if nb > 1:
        assert D.part2().sum() > 0 and D.wide().sum() > 0
        assert (D.d[D.bounded()] == 1).any() and (D.d[D.bounded()] > 1).any()  # CMS_PO_BOUND_ROWS=2 meets d = 1
    assert not D.bounded(part2=False)[D.part2()].any()
    R = D.ref(oracle)
    n1 = D.tags["narrow1"]
    assert len(n1) >= k + 1
    live = D.nnz > 0
    assert (R[np.ix_(np.flatnonzero(live), n1)] == 1.0).all()  # shape (1, 1): exactly 1.0
    assert set((D.nnz % 8).tolist()) == set(range(8))
    ties = D.tags["ties"]
    assert len(ties) == min(nb, 6)
    for q, c in ties:
        assert D.bounded()[c] and D.uid[c] < D.uid[n1].min() and c < min(n1)
        assert R[q, c] == 1.0
        ids, sc = D.expected_list(oracle, q, k)
        assert D.uid[c] in ids.tolist() and sc[-1] == 1.0  # the tie sits at the k-th score
        row = R[q].copy()
        row[q] = np.nan
        assert (row == 1.0).sum() > k  # more candidates at that score than places
        assert sum(int(D.uid[r]) in ids.tolist() for r in n1) == k - 1
        # collision-free at the twin's shape: valueA_0 = sum v^2, so the row-0 bound is exactly 1.0 too
        assert _norms_at(oracle, D, q, c)[0] == int(D.nnz[q])
    # a list longer than any query's narrow candidates can fill: nothing may be pruned
    k2 = P.prune_long_k(D)
    for part2 in (True, False):
        nar = ~D.bounded(part2)
        assert all((~np.isnan(R[q, nar])).sum() - (1 if nar[q] and live[q] else 0) < k2 for q in range(D.n))


def test_inexact_design_norms(oracle):
    D = P.get(oracle, "inexact")
    T = D.tags
    lim = 1 << 53
    nh, big = T["n_heavy"], T["big"]
    # a narrow class member past 2^53 whose class k_po_bigq takes: the group redo, and met by `big` the k_po_bigq redo
    assert D.w[nh] <= P.PO_PART2_W and int(D.w[nh]) * int(D.d[nh]) <= P.PO_BIG_MAX_DW
    assert max(_own_norms(oracle, D, nh)) >= lim
    assert D.nnz[big] > P.PO_BIG_QUERY and D.narrow_route(big, nh) == "bigq" and D.narrow_route(big, T["p2_heavy"]) == "bigq"
    assert D.narrow_route(T["w9000"], nh) == "group" and D.narrow_route(nh, 8) == "group"
    assert D.w[T["w_heavy"]] > P.PO_HIST and max(_own_norms(oracle, D, T["w_heavy"])) >= lim      # a wide owner's norm
    assert D.part2()[T["p2_heavy"]] and max(_own_norms(oracle, D, T["p2_heavy"])) >= lim
    for q in ("n_heavy", "w_heavy", "w_heavy_lds", "p2_heavy"):  # sum v >= 2^26: never pruned
        r = T[q]
        assert D.nnz[r] <= P.PO_CACHED and D.vals[D.off[r]:D.off[r + 1]].astype(np.float64).sum() >= 2 ** 26
        for c in ("w9000", "w16385", "w_heavy"):  # valueA past 2^53 at a width past the LDS row: the global-row list
            assert D.w[T[c]] > P.PO_HIST and max(_norms_at(oracle, D, r, T[c])) >= lim
    R = D.ref(oracle)
    assert not np.isnan(R).any()
    # the sequential sums are visible: pairs of each redo list whose reference score is not what exact
    # integers rounded once would give (a kernel that missed the redo returns the latter)
    differs = {"group": 0, "bigq": 0, "bound": 0}
    for q in range(D.n):
        for c in range(D.n):
            if R[q, c] != D.exact_integer_value(oracle, q, c):
                differs[D.narrow_route(q, c)] += 1
    assert differs["group"] >= 5 and differs["bigq"] >= 2 and differs["bound"] >= 5, differs
    assert R[big, nh] != D.exact_integer_value(oracle, big, nh)
    group_redo, bigq_redo = D.redo_pairs(oracle)
    assert group_redo >= 30 and bigq_redo >= 2
    # with part 2 in the group kernel p2_heavy's column is the group kernel's too (big's pair stays k_po_bigq's)
    g2, b2 = D.redo_pairs(oracle, part2=False)
    assert g2 > group_redo and b2 == bigq_redo
    assert group_redo + bigq_redo < 65536 // 16  # far below the library's redo capacity
    nar = ~D.bounded()
    assert all((~np.isnan(R[q, nar])).sum() - (1 if nar[q] else 0) >= 5 for q in range(D.n))
