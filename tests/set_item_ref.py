"""Plain-Python restatement of the item-based recommenders' estimates over the set similarities
(tests/set_ref.py): GenericItemBasedRecommender.doEstimatePreference (:231-259, "weighted") and
GenericBooleanPrefItemBasedRecommender.doEstimatePreference (:52-64, "boolean") as float loops in preference
order, and the designed models whose estimates tell that order from another."""
import itertools
import math

import numpy as np

import set_ref as R


def estimate(kind, sims, prefs=None, capper=None):
    """sims[i] = itemSimilarity(candidate, the user's i-th preferred item), prefs[i] that preference's float."""
    preference = total = 0.0
    count = 0
    for i, s in enumerate(sims):
        if s != s:
            continue
        if kind == "weighted":
            preference += s * float(np.float32(prefs[i]))
        total += s
        count += 1
    if kind == "boolean":
        return np.float32(total) if count else np.float32(math.nan)
    if count <= 1:
        return np.float32(math.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.float32(np.float64(preference) / np.float64(total))
    if capper is not None:
        lo, hi = np.float32(capper[0]), np.float32(capper[1])
        e = hi if e > hi else lo if e < lo else e
    return e


def item_users(lists):
    """item -> the frozenset of the users (positions in lists) that hold it."""
    out = {}
    for u, items in enumerate(lists):
        for i in items:
            out.setdefault(int(i), set()).add(u)
    return {i: frozenset(s) for i, s in out.items()}


def estimates(measure, kind, lists, prefs, vals, cands, capper=None, sim_row=None):
    """One estimate per candidate for a user with the preferred items prefs (in order) and their values.  sim_row(c,
    prefs) replaces the restated similarities (log-likelihood: the device's own values); an unknown candidate is NaN."""
    iu = item_users(lists)
    row = sim_row or (lambda c, ps: [R.similarity(measure, iu[c], iu[p], len(lists), "key")[0] for p in ps])
    return np.array([estimate(kind, row(c, list(prefs)), vals, capper) if c in iu else math.nan for c in cands],
                    np.float32)


def order_model(kind):
    """(lists, values or None, sizes): user 0 holds the preferred items 0 .. m-1, user 1 holds them and the candidate,
    item m, alone; item i has sizes[i] holders, so its Tanimoto similarity with the candidate is 1 / sizes[i].
    boolean: the first three odd sizes whose similarities sum to other fp64 bits in ascending than in reversed order
    (the float32 estimate hides that last bit).  weighted: sizes (a, b, a, b) under the values (+1, +1, -1, -1), the
    first whose cancelling preference sum gives another float32 estimate in reversed order: there the order shows."""
    odd, weighted = range(3, 41, 2), kind == "weighted"
    vals = [1.0, 1.0, -1.0, -1.0] if weighted else None
    pairs = ((a, b, a, b) for a, b in itertools.permutations(odd, 2))
    for sizes in pairs if weighted else itertools.permutations(odd, 3):
        sims = [1.0 / s for s in sizes]
        if weighted:
            asc, rev = estimate(kind, sims, vals), estimate(kind, sims[::-1], vals[::-1])
        else:
            asc, rev = np.float64(sum(sims)), np.float64(sum(sims[::-1]))
        if asc.tobytes() != rev.tobytes():
            m = len(sizes)
            fill = [[i for i in range(m) if sizes[i] - 2 > f] for f in range(max(sizes) - 2)]
            return [list(range(m)), list(range(m + 1))] + fill, vals, sizes
    raise AssertionError("no such sizes")
