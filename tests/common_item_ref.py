"""Plain-Python restatement of the item-based recommenders' estimates over the co-rated similarities:
tests/set_item_ref.py's estimate loops over tests/common_ref.py's similarities on the key side, the candidate as X
(itemSimilarities(candidate, preferredIDs)); and the seeded models the CPU and the GPU test share."""
import math

import numpy as np

import common_ref as C
import set_item_ref as I


class Sims:
    """itemSimilarity(item c, item p) by dense item index over a common_ref.Model, each pair computed once."""

    def __init__(self, measure, model, weighted=False):
        self.args, self.lists, self.num, self.memo = (measure, weighted), model.lists["key"], model.num["key"], {}

    def __call__(self, c, p):
        if (c, p) not in self.memo:
            self.memo[c, p] = C.similarity(self.args[0], self.lists[c], self.lists[p], self.num, self.args[1])
        return self.memo[c, p]


def estimates(sims, kind, prefs, vals, cands, capper=None):
    """One float32 per candidate index (None: a key the model lacks, NaN) for a user whose preferred item indices
    are prefs, in order, with the values vals."""
    return np.array([math.nan if c is None else I.estimate(kind, [sims(c, p) for p in prefs], vals, capper)
                     for c in cands], np.float32)


def model(n, users=40, rate=0.12, variant=None):
    """A seeded model of `users` users over n items, every item held, user 3 without and user 5 with one preference:
    (common_ref.Model with owner IDs 3r - 100 and item keys 7i + 5, per-user item indices, per-user float32 values).
    Values are halves from 0.5 to 5.0 (a shift exists, every item is eligible), or by variant
      "big"      integers 1..5, and item n // 3 held by users 8 and 9 alone at 2^25 each: its U = 2^51 is not eligible;
      "noshift"  the halves, but user 7's first value is 2^-31: no s <= 30 makes it an integer (exact_shift_for)."""
    rng = np.random.Generator(np.random.PCG64(n))
    A = rng.random((users, n)) < rate
    A[3] = False
    A[5] = np.arange(n) == n // 2
    for c in np.nonzero(~A.any(axis=0))[0]:
        A[7 + int(c) % (users - 7), c] = True
    V = (rng.integers(1, 11, A.shape) / np.float32(2)).astype(np.float32)
    if variant == "big":
        V = np.ceil(V)
        A[:, n // 3] = False
        A[8:10, n // 3], V[8:10, n // 3] = True, 2.0 ** 25
    elif variant == "noshift":
        V[7, np.nonzero(A[7])[0][0]] = 2.0 ** -31
    lists = [np.nonzero(r)[0] for r in A]
    vals = [V[u, lists[u]] for u in range(users)]
    m = C.Model([[(int(i) * 7 + 5, float(v)) for i, v in zip(lists[u], vals[u])] for u in range(users)],
                np.arange(users) * 3 - 100)
    return m, lists, vals
