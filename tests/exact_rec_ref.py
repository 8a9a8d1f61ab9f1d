"""Plain-Python restatement of GenericUserBasedRecommender over a similarity
that is no CosineCM (T/impl/recommender/GenericUserBasedRecommender.java:84-105,
134-198, the sim == null branch), the reference of every exact-recommender
test: Python float loops in the reference's order.  Similarities and
neighbourhoods come from exact_ref.Model (similarity, top_k), candidates from
taste.FastIDSet and the ranking from taste.get_top_items, both host-tested.
"""
import math

import numpy as np

from exact_ref import Model
from mahout_amd import taste


def estimate(M, sims, user, neighborhood, item, capper=None):
    """doEstimatePreference(user, neighborhood, item) (:134-184) over model M
    (exact_ref.Model) for owner ROWS user / neighborhood and the item KEY;
    sims[r] = userSimilarity(user, row r).  np.float32."""
    if len(neighborhood) == 0:  # :135-137
        return np.float32(np.nan)
    preference = 0.0
    total = 0.0
    count = 0
    for r in neighborhood:  # :148
        r = int(r)
        if r == user:  # :149
            continue
        _, vals, at = M._rows[r]
        j = at.get(int(item))  # dataModel.getPreferenceValue(userID, itemID) (:154): null when absent
        if j is None:
            continue
        s = float(sims[r])  # :162
        if math.isnan(s):
            continue
        preference += s * vals[j]  # :164-166 (vals: the float32 values as doubles)
        total += s
        count += 1
    if count <= 1:  # :176-178
        return np.float32(np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.float32(np.float64(preference) / np.float64(total))  # :179, Java's double division then (float)
    if capper is not None:  # EstimatedPreferenceCapper.capEstimate
        lo, hi = np.float32(capper[0]), np.float32(capper[1])
        if e > hi:
            e = hi
        elif e < lo:
            e = lo
    return e


def estimates(M, user, neighborhood, items, weighted=False, capper=None):
    """estimate for every item key of items: float32 [len(items)]."""
    sims = M.similarities_row(int(user), weighted)
    return np.array([estimate(M, sims, int(user), neighborhood, it, capper) for it in items], np.float32).reshape(-1)


def item_set(M, r):
    """GenericDataModel.getItemIDsFromUser of owner row r."""
    keys = M._rows[r][0]
    s = taste.FastIDSet(len(keys))
    for k in keys:
        s.add(k)
    return s


def all_other_items(M, user, neighborhood, include_known=False):
    """getAllOtherItems (:187-198) in FastIDSet iteration order."""
    possible = taste.FastIDSet()
    for r in neighborhood:
        possible.addAll(item_set(M, int(r)))
    if not include_known:
        possible.removeAll(item_set(M, int(user)))
    return possible.toList()


def neighborhood(M, user, n, weighted=False):
    """NearestNUserNeighborhood(n): owner rows, in TopItems.getTopUsers order."""
    ids, _ = M.top_k(int(user), n, M.similarities_row(int(user), weighted))
    return np.searchsorted(M.owner_ids, ids)


def recommend(M, user, nb, how_many, weighted=False, include_known=False, capper=None):
    """recommend(user, how_many) (:84-105) with the neighbourhood nb (owner rows): [(item, float32)]."""
    if len(nb) == 0:
        return []
    items = all_other_items(M, user, nb, include_known)
    return taste.get_top_items(how_many, items, estimates(M, user, nb, items, weighted, capper))


def order_model():
    """User 0 and two pairs of neighbours (1, 2) and (3, 4), the second of each
    pair holding the first's values negated: its similarity with user 0 is the
    first's negated, exactly.  In the order 1, 2, 3, 4 totalSimilarity is
    (s1 - s1) + s3 - s3 = 0.0; in the order 1, 3, 4, 2 it is ((s1 + s3) - s3) - s1,
    which the rounding of s1 + s3 leaves off zero."""
    a = [(0, 0.2), (1, 0.3), (9, 0.7)]
    c = [(0, 0.4), (2, 0.5), (9, 0.3)]
    neg = lambda p: [(k, -v) for k, v in p]  # noqa: E731
    return Model.from_lists([[(0, 0.1), (1, 0.3), (2, 0.5)], a, neg(a), c, neg(c)])


def same_bits32(a, b):
    """Element-wise over float32: the same bits, or both NaN."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))
