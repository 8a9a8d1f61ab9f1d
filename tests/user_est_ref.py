"""Plain-Python restatement of the two user-based estimates over a similarity
array handed in: GenericUserBasedRecommender.doEstimatePreference with
sim == null (T/impl/recommender/GenericUserBasedRecommender.java:134-184) and
GenericBooleanPrefUserBasedRecommender.doEstimatePreference (:45-61).
rows[r]: owner row r's preferences as {item key: float value}; sims[r]:
userSimilarity(user, row r) under whichever measure; nb: owner rows in the
caller's order."""
import math

import numpy as np

NAN32 = np.float32(np.nan)


def estimate(kind, rows, sims, user, nb, item, capper=None):
    if len(nb) == 0:  # :135-137, :46-48
        return NAN32
    if kind == "boolean":
        total, found = np.float32(0.0), False
        for r in nb:
            if r != user and item in rows[r]:  # :55
                found = True
                with np.errstate(over="ignore"):
                    total = np.float32(total + np.float32(sims[r]))  # :57, float += (float) double; NaN not skipped
        return total if found else NAN32
    preference = total = 0.0
    count = 0
    for r in nb:
        if r == user or item not in rows[r]:  # :149, :154
            continue
        s = float(sims[r])
        if math.isnan(s):  # :162-163
            continue
        preference += s * float(np.float32(rows[r][item]))
        total += s
        count += 1
    if count <= 1:  # :176-178
        return NAN32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.float32(np.float64(preference) / np.float64(total))
    if capper is not None:
        lo, hi = np.float32(capper[0]), np.float32(capper[1])
        e = hi if e > hi else lo if e < lo else e
    return e


def estimates(kind, rows, sims, user, nb, items, capper=None):
    nb = [int(r) for r in nb]
    return np.array([estimate(kind, rows, sims, user, nb, int(it), capper) for it in items], np.float32).reshape(-1)


# Order models: a neighbourhood whose two orders give different bits.
# generic: Pearson similarities +1, -1, +s, -s with user 0 (exact_rec_ref.order_model's idea): four common items
# with small integer values keep every sum exact, and y -> c - y negates the centred sums exactly.  All hold item 9.
# In the order 1, 2, 3, 4 totalSimilarity is 0.0; in 1, 3, 4, 2 the rounding of 1 + s leaves it off zero.
_ROW = lambda vals, nine: [(i, float(v)) for i, v in enumerate(vals)] + ([(9, nine)] if nine else [])  # noqa: E731
GENERIC_ORDER_PREFS = [_ROW((1, 2, 3, 5), None), _ROW((1, 2, 3, 5), 0.7), _ROW((5, 4, 3, 1), 0.3),
                       _ROW((1, 2, 4, 3), 0.2), _ROW((6, 5, 3, 4), 0.9)]
GENERIC_ORDERS = ([1, 2, 3, 4], [1, 3, 4, 2])
# boolean: float32 similarities whose sum depends on the order: (1 + 2^-24) + 2^-24 rounds twice to even
BOOLEAN_ORDER_SIMS = [np.nan, 1.0, 2.0 ** -24, 2.0 ** -24, -1.0]  # by owner row; row 0 is the user
BOOLEAN_ORDERS = ([1, 2, 3, 4], [2, 3, 1, 4])
