"""CPU: what the set similarity kernels share with the host (cms_set.h, built as
tests/cpp/set_host_shim.hip) against tests/set_ref.py: set_intersection_size and
set_finish on designed pairs, in both orders and by both sides' rules, and the
reference's own known answers.  Co-occurrence, Tanimoto and city block must have the restatement's bits.  For
log-likelihood the bound is |got - reference| <= 2^-48 S + 2^-52 with S the sum
of the absolute values of the eleven xLogX terms: each xLogX carries at most
about 3 * 2^-53 relative error (a 1-ulp log, one product, one conversion), so
the terms together err by at most 3 * 2^-53 S; they meet about ten additions
and subtractions whose results are at most S in magnitude, each rounding by at
most 2^-53 S; so the entropy combination errs by at most 13 * 2^-53 S, the
factor 2.0 doubles that to 26 * 2^-53 S < 2^-48 S, the map llr -> 1 - 1/(1+llr)
has slope at most 1 for llr >= 0, and the 2^-52 covers the roundings of the last
two operations, whose results lie in [0, 1]."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import set_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "set_host_shim.hip")
DEPS = [SRC] + [os.path.join(HERE, "..", "mahout_amd", "csrc", f) for f in ("cms_set.h", "cms_exact.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libset_host_shim.so")


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.sh_finish.restype = ctypes.c_double
    lib.sh_finish.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.c_int]
    lib.sh_intersection_size.restype = ctypes.c_int64
    return lib


@pytest.mark.parametrize("side", ["owner", "key"])
@pytest.mark.parametrize("measure", range(4))
@pytest.mark.parametrize("name", sorted(R.DESIGNED))
def test_designed_pairs_both_orders(shim, name, measure, side):
    x, y, num = R.DESIGNED[name]
    for a, b in ((x, y), (y, x)):
        ak, bk = np.array(a, np.int64), np.array(b, np.int64)
        p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        k = shim.sh_intersection_size(p(ak), ctypes.c_int64(ak.size), p(bk), ctypes.c_int64(bk.size))
        assert k == len(set(a) & set(b))
        exp, S = R.similarity(R.MEASURES[measure], a, b, num, side)
        got = shim.sh_finish(measure, k, len(a), len(b), num, int(side == "owner"))
        assert R.agrees(R.MEASURES[measure], got, exp, S), (name, got, exp, S)
    if name == "one_empty" and measure == 1:  # only Tanimoto's userSimilarity tells one empty list from two
        assert got == 0.0 if side == "owner" else math.isnan(got)


# (k, n1, n2, num) -> the value asserted by LogLikelihoodSimilarityTest (testCorrelation, testNoSimilarity) and
# TanimotoCoefficientSimilarityTest (testFullCorrelation1/2, testCorrelation1/2, testNoCorrelation, testItemsSimilarities)
KNOWN = [("loglikelihood", (2, 3, 3, 5), 0.12160727029227925), ("loglikelihood", (2, 3, 4, 5), 0.5423213660693732),
         ("loglikelihood", (3, 4, 3, 5), 0.6905400104897509), ("loglikelihood", (3, 3, 3, 5), 0.8706358464330881),
         ("loglikelihood", (0, 2, 2, 4), math.nan), ("loglikelihood", (4, 4, 4, 4), 0.0),
         ("tanimoto", (1, 1, 1, 1), 1.0), ("tanimoto", (1, 3, 1, 3), 0.3333333333333333),
         ("tanimoto", (1, 2, 2, 3), 0.3333333333333333), ("tanimoto", (2, 3, 3, 4), 0.5),
         ("tanimoto", (0, 2, 1, 3), math.nan), ("tanimoto", (1, 2, 1, 2), 0.5), ("tanimoto", (2, 2, 2, 2), 1.0),
         # counts near 2^31: exact conversions, and S about 2^37
         ("loglikelihood", (10 ** 6, 3 * 10 ** 6, 2 * 10 ** 9, 2 ** 31 - 1), None),
         ("tanimoto", (2 ** 30 - 1, 2 ** 31 - 2, 2 ** 30, 2 ** 31 - 1), None),
         ("city_block", (2 ** 29 + 1, 2 ** 30, 2 ** 30 + 3, 2 ** 31 - 1), None)]


@pytest.mark.parametrize("measure,counts,known", KNOWN)
def test_known_answers(shim, measure, counts, known):
    exp, S = R.from_counts(measure, *counts, side="key")
    if known is not None:  # the restatement against the reference's number, by the rule the shim is held to
        assert R.agrees(measure, known, exp, S), (known, exp, S)
    got = shim.sh_finish(R.MEASURES.index(measure), *counts, 0)
    assert R.agrees(measure, got, exp, S), (got, exp, S)


def test_tile_rounding(shim):
    assert [shim.sh_tile_for(a) for a in (0, 1, 65, 16383, 2 ** 31 - 1)] == [16384, 64, 128, 16384, 16384]
