// cms_set.h -- what the host and the device share of the set similarities
// (cms_set.hip): the measures, the key-only merge join of two ascending lists
// and the measures' endings.  None of them reads a preference value: with x and
// y two lists of one side of the attached model, n1 and n2 their lengths, k the
// size of their intersection and num the other face's count (getNumItems() on
// the user side, getNumUsers() on the item side),
//
//   co-occurrence: (double)k, NaN when k == 0 -- the count the item similarity
//     job's measures start from;
//   Tanimoto (T/impl/similarity/TanimotoCoefficientSimilarity.java:62-113):
//     userSimilarity (:62-86) is NaN when both lists are empty and 0.0 when one
//     is (:70-75); both faces are NaN when k == 0 (:79-81, :108-110), else
//     (double)k / (double)(n1 + n2 - k) (:83-85, :112);
//   city block (T/impl/similarity/CityBlockSimilarity.java:54-96):
//     1.0 / (1.0 + (n1 + n2 - 2k)) on both faces (:93-96), never NaN: a pair with
//     nothing in common scores 1 / (1 + n1 + n2);
//   log-likelihood (T/impl/similarity/LogLikelihoodSimilarity.java:52-108): NaN
//     when k == 0 (:62-64, :98-100), else with llr = LogLikelihood
//     .logLikelihoodRatio(k, n2 - k, n1 - k, num - n1 - n2 + k) (:66-70,
//     :102-106) the value 1.0 - 1.0 / (1.0 + llr) (:71, :107), where
//     (math/.../stats/LogLikelihood.java:62-111) xLogX(x) is 0.0 for x == 0 and
//     x * Math.log(x) otherwise (:62-64), the two- and four-argument entropy are
//     xLogX(sum) minus the elements' xLogX one after the other (:70-80), and the
//     ratio is 0.0 when rowEntropy + columnEntropy < matrixEntropy, else
//     2.0 * (rowEntropy + columnEntropy - matrixEntropy) (:100-111).
//
// These classes are no AbstractSimilarity: no Weighting and no
// normalizeWeightResult apply.
//
// Exactness.  k, n1, n2 and num are exact integers below 2^31, so the
// co-occurrence, Tanimoto and city-block values -- at most one addition and one
// division of exactly converted integers, each correctly rounded -- are the
// reference's bit for bit.  Log-likelihood is NOT claimed bit for bit, and
// cannot be: Math.log is specified only to within 1 ulp, so the reference's own
// value depends on the JVM, and the device's log and the host's log are two
// further 1-ulp implementations.  What holds: the four integers are exact, the
// operations are the reference's in the reference's order, each of them but
// log correctly rounded, so the result lies within 2^-48 S + 2^-52 of the
// real-arithmetic value of that sequence (S the sum of the absolute values of
// the eleven xLogX terms; tests/test_set_host.py derives the bound), and equal
// (k, n1, n2, num) give equal bits within one build.
//
// Everything here is a pure __host__ __device__ function in cms_common.h's
// style; tests/test_set_host.py runs it on the CPU
// (tests/cpp/set_host_shim.hip) against tests/set_ref.py.
#pragma once
#include <math.h>
#include <stdint.h>

#include "cms_exact.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#define __dadd_rn(x, y) ((x) + (y))
#define __dsub_rn(x, y) ((x) - (y))
#define __dmul_rn(x, y) ((x) * (y))
#define __ddiv_rn(x, y) ((x) / (y))
#endif

namespace cms {

// the values of CMS_SET_* (mahout_cms.h)
enum SetMeasure : int32_t { kSetCooccurrence = 0, kSetTanimoto = 1, kSetCityBlock = 2, kSetLogLikelihood = 3 };
constexpr int kSetMeasures = 4;

// LogLikelihood.xLogX and the two entropies, subtracting in the reference's order
CMS_HD double set_xlogx(int64_t x) { return x == 0 ? 0.0 : __dmul_rn((double)x, log((double)x)); }
CMS_HD double set_entropy(int64_t a, int64_t b) {
  return __dsub_rn(__dsub_rn(set_xlogx(a + b), set_xlogx(a)), set_xlogx(b));
}
CMS_HD double set_entropy(int64_t a, int64_t b, int64_t c, int64_t d) {
  return __dsub_rn(__dsub_rn(__dsub_rn(__dsub_rn(set_xlogx(a + b + c + d), set_xlogx(a)), set_xlogx(b)), set_xlogx(c)),
                   set_xlogx(d));
}
CMS_HD double set_log_likelihood_ratio(int64_t k11, int64_t k12, int64_t k21, int64_t k22) {
  const double rowEntropy = set_entropy(k11 + k12, k21 + k22);
  const double columnEntropy = set_entropy(k11 + k21, k12 + k22);
  const double matrixEntropy = set_entropy(k11, k12, k21, k22);
  const double sum = __dadd_rn(rowEntropy, columnEntropy);
  if (sum < matrixEntropy) return 0.0;  // "round off error"
  return __dmul_rn(2.0, __dsub_rn(sum, matrixEntropy));
}

// The measure of one pair from its integers.  owner_side: the rules of
// userSimilarity (Tanimoto's empty lists); the item side's lists of an attached
// model are never empty, and its rule for them (k == 0: NaN) is stated all the
// same.  The lists of one face hold distinct keys of the other, so
// n1 + n2 - k <= num and the fourth cell of the ratio is never negative.
template <int MEASURE>
CMS_HD double set_finish(int64_t k, int64_t n1, int64_t n2, int64_t num, int owner_side) {
  if (MEASURE == kSetCityBlock) return __ddiv_rn(1.0, __dadd_rn(1.0, (double)(n1 + n2 - 2 * k)));
  if (MEASURE == kSetTanimoto && owner_side) {
    if (n1 == 0 && n2 == 0) return __builtin_nan("");
    if (n1 == 0 || n2 == 0) return 0.0;
  }
  if (k == 0) return __builtin_nan("");
  if (MEASURE == kSetCooccurrence) return (double)k;
  if (MEASURE == kSetTanimoto) return __ddiv_rn((double)k, (double)(n1 + n2 - k));
  const double llr = set_log_likelihood_ratio(k, n2 - k, n1 - k, num - n1 - n2 + k);
  return __dsub_rn(1.0, __ddiv_rn(1.0, __dadd_rn(1.0, llr)));
}

// FastIDSet.intersectionSize over two lists whose keys ascend strictly
template <class KEY>
CMS_HD int64_t set_intersection_size(const KEY* xk, int64_t nx, const KEY* yk, int64_t ny) {
  int64_t k = 0;
  for (int64_t i = 0, j = 0; i < nx && j < ny;) {
    const KEY a = xk[i], b = yk[j];
    k += a == b;
    i += a <= b;
    j += b <= a;
  }
  return k;
}

// ---- the tile kernel's shape ----
// Candidates per workgroup: one u32 count each, 64 KiB at the default, so two
// workgroups share a CU's 160 KiB.  CMS_SET_TILE overrides it with any multiple
// of 64 up to the default.
constexpr int kSetTileDefault = 16384;
CMS_HD int set_tile_for(int asked) {
  if (asked <= 0 || asked >= kSetTileDefault) return kSetTileDefault;
  return (asked + 63) / 64 * 64;
}

}  // namespace cms

#if !defined(__HIP_DEVICE_COMPILE__)
#undef __dadd_rn
#undef __dsub_rn
#undef __dmul_rn
#undef __ddiv_rn
#endif
