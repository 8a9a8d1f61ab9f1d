"""Plain-Python restatement of AbstractSimilarity.userSimilarity / itemSimilarity
(AbstractSimilarity.java:110-222, :224-301) with the endings of
UncenteredCosineSimilarity, PearsonCorrelationSimilarity and
EuclideanDistanceSimilarity: float loops in the reference's order, math.sqrt."""
import math

import numpy as np

MEASURES = ("uncentered_cosine", "pearson", "euclidean")


def sums(xk, xv, yk, yv):
    """The merge walk: (sumXY, sumX, sumY, sumX2, sumY2, sumXYdiff2, count) over the common keys, ascending."""
    sxy = sx = sy = sx2 = sy2 = sd2 = 0.0
    n = i = j = 0
    while i < len(xk) and j < len(yk):
        if xk[i] == yk[j]:
            x, y = xv[i], yv[j]
            sxy += x * y
            sx += x
            sx2 += x * x
            sy += y
            sy2 += y * y
            diff = x - y
            sd2 += diff * diff
            n += 1
        step_x, step_y = xk[i] <= yk[j], xk[i] >= yk[j]
        i, j = i + step_x, j + step_y
    return sxy, sx, sy, sx2, sy2, sd2, n


def finish(measure, s, xlen, ylen, num, weighted):
    sxy, sx, sy, sx2, sy2, sd2, n = s
    if xlen == 0 or ylen == 0 or n == 0:  # (n == 0 is NaN in Java by every ending; Python would raise)
        return math.nan
    if measure == "euclidean":
        r = 1.0 / (1.0 + math.sqrt(sd2) / math.sqrt(n))
    else:
        if measure == "pearson":
            mean_x, mean_y = sx / n, sy / n
            sxy, sx2, sy2 = sxy - mean_y * sx, sx2 - mean_x * sx, sy2 - mean_y * sy
        if sx2 < 0.0 or sy2 < 0.0:
            return math.nan  # Math.sqrt of a negative is NaN, and so is everything after it
        den = math.sqrt(sx2) * math.sqrt(sy2)
        if den == 0.0:
            return math.nan
        r = sxy / den
    if math.isnan(r):
        return r
    if weighted:  # normalizeWeightResult (:313-330)
        scale = 1.0 - float(n) / float(num + 1)
        r = -1.0 + scale * (1.0 + r) if r < 0.0 else 1.0 - scale * (1.0 - r)
    return -1.0 if r < -1.0 else 1.0 if r > 1.0 else r


def similarity(measure, x, y, num, weighted=False):
    """x, y: (keys ascending, float32 values) of the two lists."""
    xv, yv = ([float(v) for v in np.asarray(a[1], np.float32)] for a in (x, y))
    return finish(measure, sums(list(x[0]), xv, list(y[0]), yv), len(xv), len(yv), num, weighted)


class Model:
    """A DataModel from per-owner lists of (item key, value), both faces: side
    "owner" is the owners' lists over item keys, side "key" the items' lists
    over owner rows, the items in ascending key order."""

    def __init__(self, prefs, owner_ids=None):
        rows = [sorted(p) for p in prefs]
        self.owner_ids = np.arange(len(rows), dtype=np.int64) if owner_ids is None else np.asarray(owner_ids, np.int64)
        self.offsets = np.cumsum([0] + [len(p) for p in rows]).astype(np.int64)
        self.keys = np.array([k for p in rows for k, _ in p], np.int64)
        self.vals = np.array([v for p in rows for _, v in p], np.float32)
        posting = {}
        for r, p in enumerate(rows):
            for k, v in p:
                posting.setdefault(k, []).append((r, v))
        self.item_keys = np.array(sorted(posting), np.int64)
        split = lambda p: ([k for k, _ in p], [v for _, v in p])  # noqa: E731
        self.lists = {"owner": [split(p) for p in rows], "key": [split(posting[int(k)]) for k in self.item_keys]}
        self.ids = {"owner": self.owner_ids, "key": self.item_keys}
        self.num = {"owner": len(self.item_keys), "key": len(rows)}  # getNumItems(), getNumUsers()

    def row(self, measure, side, i, weighted=False):
        """similarity(list i, every list of the side): the slab row of query i."""
        L = self.lists[side]
        return np.array([similarity(measure, L[i], y, self.num[side], weighted) for y in L], np.float64)

    def top_k(self, side, i, k, sims):
        """NaN skipped, the query excluded, similarity descending then index ascending: (ids, scores)."""
        order = sorted((j for j in range(len(sims)) if j != i and not math.isnan(sims[j])), key=lambda j: (-sims[j], j))[:k]
        return self.ids[side][order], sims[order]


def same_bits(a, b):
    """Element-wise: the same bits (0.0 == -0.0 is not enough), or both NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
