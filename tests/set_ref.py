"""Plain-Python restatement of the reference's set similarities over Python sets
and ints: the co-occurrence count, TanimotoCoefficientSimilarity (:62-113),
CityBlockSimilarity (:54-96) and LogLikelihoodSimilarity (:52-108) with
LogLikelihood.logLikelihoodRatio (:62-111).  Log-likelihood runs the reference's
sequence of operations in decimal at 50 digits and also gives S, the sum of the
absolute values of the eleven xLogX terms that sequence evaluates."""
import functools
import math
from decimal import Decimal, localcontext

import numpy as np

MEASURES = ("cooccurrence", "tanimoto", "city_block", "loglikelihood")

# designed pairs (x, y, num): num at least the size of the union
DESIGNED = {
    "disjoint": ([1, 3, 5], [2, 4, 6], 9),
    "identical": ([1, 2, 3, 4], [1, 2, 3, 4], 10),
    "identical_all": ([0, 1, 2, 3], [0, 1, 2, 3], 4),  # k12 = k21 = k22 = 0: the ratio is 0.0
    "one_empty": ([], [2, 4], 6),
    "both_empty": ([], [], 6),
    "k22_zero": ([0, 1, 2], [2, 3, 4], 5),
    "subset": ([1, 2, 3, 4, 5, 6], [2, 4], 8),  # k12 = 0
    "ends_meet": ([1, 9], [0, 9], 10),
    "interleaved": (list(range(0, 60, 2)), list(range(0, 60, 3)), 60),
}


@functools.lru_cache(maxsize=None)
def _log_likelihood(k, n1, n2, num):
    """(1 - 1 / (1 + llr), S) for logLikelihoodRatio(k, n2 - k, n1 - k, num - n1 - n2 + k)."""
    with localcontext() as ctx:
        ctx.prec = 50
        terms = []

        def xlogx(x):
            terms.append(Decimal(0) if x == 0 else Decimal(x) * Decimal(x).ln())
            return terms[-1]

        def entropy(*e):
            r = xlogx(sum(e))
            for v in e:
                r = r - xlogx(v)
            return r

        k11, k12, k21, k22 = k, n2 - k, n1 - k, num - n1 - n2 + k
        assert min(k11, k12, k21, k22) >= 0
        row, col, mat = entropy(k11 + k12, k21 + k22), entropy(k11 + k21, k12 + k22), entropy(k11, k12, k21, k22)
        llr = Decimal(0) if row + col < mat else 2 * (row + col - mat)
        assert len(terms) == 11
        return float(1 - 1 / (1 + llr)), float(sum(abs(t) for t in terms))


def from_counts(measure, k, n1, n2, num, side="owner"):
    """(the similarity, S) of two lists of lengths n1 and n2 sharing k entries; S is 0.0 but for log-likelihood."""
    if measure == "city_block":
        return 1.0 / (1.0 + (n1 + n2 - 2 * k)), 0.0
    if measure == "tanimoto" and side == "owner" and (n1 == 0 or n2 == 0):
        return (math.nan if n1 == n2 else 0.0), 0.0
    if k == 0:
        return math.nan, 0.0
    if measure == "cooccurrence":
        return float(k), 0.0
    if measure == "tanimoto":
        return k / (n1 + n2 - k), 0.0
    return _log_likelihood(k, n1, n2, num)


def similarity(measure, x, y, num, side="owner"):
    return from_counts(measure, len(set(x) & set(y)), len(x), len(y), num, side)


def agrees(measure, got, exp, S):
    """NaN matches NaN; the same bits for the three exact measures; for
    log-likelihood |got - exp| <= 2^-48 S + 2^-52 (derived in tests/test_set_host.py)."""
    if math.isnan(got) or math.isnan(exp):
        return math.isnan(got) and math.isnan(exp)
    if measure == "loglikelihood":
        return abs(got - exp) <= 2.0 ** -48 * S + 2.0 ** -52
    return np.float64(got).view(np.int64) == np.float64(exp).view(np.int64)
