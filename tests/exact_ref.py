"""Plain-Python restatement of CosineSimilarity.userSimilarity
(T/impl/similarity/CosineSimilarity.java:44-103), the reference of every
exact-cosine test: Python float loops in the reference's order, math.sqrt,
oracle.normalize_weight_result(r, count, count, weighted) and
oracle.top_users.  No numpy reductions: every sum is the sequential fp64 sum
the JVM forms.
"""
import math

import numpy as np

from oracle import oracle as O


def _similarity(xk, xv, yv, y_at, weighted):
    """xk / xv / yv: Python lists (keys ascending, values as doubles of the
    float32 preferences); y_at: y's item -> index."""
    x_len, y_len = len(xk), len(yv)
    if x_len == 0 or y_len == 0:  # :52-54
        return math.nan
    sum_x2 = sum_y2 = sum_xy = 0.0
    for i in range(x_len):  # :60-75
        x = xv[i]
        sum_x2 += x * x
        j = y_at.get(xk[i])  # hasPrefWithItemID, then the scan for the item (:65-74)
        if j is not None:
            sum_xy += x * yv[j]
    for y in yv:  # :76-80
        sum_y2 += y * y
    count = x_len + y_len  # :82
    den = math.sqrt(sum_x2) * math.sqrt(sum_y2)  # computeResult :92-103
    if den == 0.0:
        return math.nan
    result = sum_xy / den
    if math.isnan(result):  # :85
        return result
    return O.normalize_weight_result(result, count, count, weighted)  # :86


def _lists(keys, vals):
    k = [int(x) for x in keys]
    v = [float(x) for x in np.asarray(vals, np.float32)]
    return k, v, {key: j for j, key in enumerate(k)}


def user_similarity(xk, xv, yk, yv, weighted=False):
    """userSimilarity of two preference lists (item keys ascending, values
    float32 as PreferenceArray.getValue returns them)."""
    xk, xv, _ = _lists(xk, xv)
    _, yv, y_at = _lists(yk, yv)
    return _similarity(xk, xv, yv, y_at, weighted)


class Model:
    """A DataModel as a CSR over owner rows (owner IDs ascending)."""

    def __init__(self, owner_ids, offsets, keys, vals):
        self.owner_ids = np.ascontiguousarray(owner_ids, np.int64)
        assert np.all(np.diff(self.owner_ids) > 0)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.keys = np.ascontiguousarray(keys, np.int64)
        self.vals = np.ascontiguousarray(vals, np.float32)
        self.n = self.owner_ids.size
        self._rows = [_lists(*self.row(r)) for r in range(self.n)]

    @classmethod
    def from_lists(cls, prefs, owner_ids=None):
        """prefs: per owner row a list of (key, value); the keys are sorted here."""
        off, keys, vals = [0], [], []
        for p in prefs:
            p = sorted(p)
            keys += [k for k, _ in p]
            vals += [v for _, v in p]
            off.append(len(keys))
        ids = np.arange(len(prefs)) if owner_ids is None else owner_ids
        return cls(ids, off, keys, vals)

    def row(self, r):
        lo, hi = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.keys[lo:hi], self.vals[lo:hi]

    def similarity(self, r1, r2, weighted=False):
        xk, xv, _ = self._rows[r1]
        _, yv, y_at = self._rows[r2]
        return _similarity(xk, xv, yv, y_at, weighted)

    def similarities_row(self, r, weighted=False):
        """userSimilarity(row r, every row): the slab row of query r."""
        return np.array([self.similarity(r, c, weighted) for c in range(self.n)], np.float64)

    def all_pairs(self, weighted=False):
        return np.stack([self.similarities_row(r, weighted) for r in range(self.n)])

    def top_k(self, r, k, sims):
        """TopItems.getTopUsers over every other owner from r's similarity row: (ids, scores)."""
        others = np.arange(self.n) != r
        return O.top_users(self.owner_ids[others], sims[others], k)


def same_bits(a, b):
    """Element-wise: the same bits (0.0 == -0.0 is not enough), or both NaN."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
