// cms_common.h -- what the host and the device share of the co-rated
// similarities (cms_common.hip): the measures, the six-sum merge join of two
// preference lists and the measures' endings.
//
// AbstractSimilarity.userSimilarity / itemSimilarity
// (T/impl/similarity/AbstractSimilarity.java:110-222, :224-301) walk two
// preference lists sorted by ascending key and, at each COMMON key in ascending
// order, with x and y the two floats widened to double:
//   sumXY += x*y; sumX += x; sumX2 += x*x; sumY += y; sumY2 += y*y;
//   diff = x - y; sumXYdiff2 += diff*diff; count++
// NaN when either list is empty (:117-119, :232-234).  Then
//   Pearson (centerData, :204-213): meanX = sumX / count, meanY = sumY / count,
//     cXY = sumXY - meanY*sumX, cX2 = sumX2 - meanX*sumX, cY2 = sumY2 - meanY*sumY
//     and the uncentered ending on the centred sums
//     (PearsonCorrelationSimilarity.java:78-91);
//   uncentered cosine (UncenteredCosineSimilarity.java:56-66, and the same text
//     CosineCM.java:70-81): NaN when n == 0 or Math.sqrt(sumX2) *
//     Math.sqrt(sumY2) == 0.0, else sumXY / denominator;
//   Euclidean (EuclideanDistanceSimilarity.java:63-65): 1.0 / (1.0 +
//     Math.sqrt(sumXYdiff2) / Math.sqrt(n)), NaN on its own when n == 0;
// and a non-NaN result goes through normalizeWeightResult(result, count, num)
// (:313-330) with count the number of common entries and num = getNumItems()
// on the user side, getNumUsers() on the item side.
//
// The integer route (k_common_tile).  With the attach's shift s and i32 units
// (cms_exact.h), call a list common-eligible when U = sum of unit^2 < 2^51.
// For two such lists every partial sum the reference forms is an exact
// integer multiple of 2^-s (sumX, sumY) or 2^-2s (the others) below 2^53 in
// magnitude: |sum x_u| <= sum x_u^2 <= U because units are integers,
// |sum x_u y_u| <= sqrt(U_x U_y), and (x_u - y_u)^2 <= 2 (x_u^2 + y_u^2), so
// every partial sum of squared differences is below 2 (U_x + U_y) < 2^53 --
// which is why the bound is 2^51 and not the full-norm cosine's 2^53.  No
// addition of the reference rounds, so integer accumulation in any order and
// ldexp by -s or -2s IS the reference's sum.  sumXYdiff2 comes from its own
// integer cell, the sum of (x_u - y_u)^2 (not from S_xx - 2 S_xy + S_yy).
// Everything after the sums is a correctly rounded fp64 operation on identical
// operands.  Anything else -- no shift, a NaN or infinite value, a list at or
// above 2^51 -- takes common_merge_join, the reference's own loop, on one lane.
//
// Everything here is a pure __host__ __device__ function in cms_exact.h's
// style; tests/test_common_host.py runs it on the CPU
// (tests/cpp/common_host_shim.hip) against tests/common_ref.py.
#pragma once
#include <math.h>
#include <stdint.h>

#include "cms_exact.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#define __dadd_rn(x, y) ((x) + (y))
#define __dsub_rn(x, y) ((x) - (y))
#define __dmul_rn(x, y) ((x) * (y))
#define __ddiv_rn(x, y) ((x) / (y))
#define __dsqrt_rn(x) sqrt(x)  // IEEE: correctly rounded, as Math.sqrt
#endif

namespace cms {

// the values of CMS_SIM_* (mahout_cms.h)
enum CommonMeasure : int32_t { kCommonUncentered = 0, kCommonPearson = 1, kCommonEuclidean = 2 };
constexpr int kCommonMeasures = 3;

// a list (an owner over its items, an item over its posting list) whose sum of
// squared units is below this is common-eligible
constexpr uint64_t kCommonEligible = 1ULL << 51;

// the sums of one pair, as the reference holds them when its loop ends
struct CommonSums {
  double sumXY = 0.0, sumX = 0.0, sumY = 0.0, sumX2 = 0.0, sumY2 = 0.0, sumD2 = 0.0;
  int64_t count = 0;
};

// normalizeWeightResult(result, count, num) (AbstractSimilarity.java:313-330);
// exact_normalize is this with num = count
CMS_HD double common_normalize(double r, int64_t count, int64_t num, int weighted) {
  if (weighted) {
    const double scale = __dsub_rn(1.0, __ddiv_rn((double)count, (double)(num + 1)));
    if (r < 0.0) r = __dadd_rn(-1.0, __dmul_rn(scale, __dadd_rn(1.0, r)));
    else r = __dsub_rn(1.0, __dmul_rn(scale, __dsub_rn(1.0, r)));
  }
  if (r < -1.0) r = -1.0;
  else if (r > 1.0) r = 1.0;
  return r;
}

// The end of userSimilarity / itemSimilarity (:202-221, :280-300) from the
// loop's sums.  A measure reads only its own sums: the others may hold anything.
template <int MEASURE>
CMS_HD double common_finish(double sumXY, double sumX, double sumY, double sumX2, double sumY2, double sumD2,
                            int64_t count, int64_t xlen, int64_t ylen, int64_t num, int weighted) {
  if (xlen == 0 || ylen == 0) return __builtin_nan("");
  double r;
  if (MEASURE == kCommonEuclidean) {
    r = __ddiv_rn(1.0, __dadd_rn(1.0, __ddiv_rn(__dsqrt_rn(sumD2), __dsqrt_rn((double)count))));
  } else {
    if (MEASURE == kCommonPearson) {
      const double n = (double)count;
      const double meanX = __ddiv_rn(sumX, n);
      const double meanY = __ddiv_rn(sumY, n);
      sumXY = __dsub_rn(sumXY, __dmul_rn(meanY, sumX));
      sumX2 = __dsub_rn(sumX2, __dmul_rn(meanX, sumX));
      sumY2 = __dsub_rn(sumY2, __dmul_rn(meanY, sumY));
    }
    if (count == 0) return __builtin_nan("");
    const double den = __dmul_rn(__dsqrt_rn(sumX2), __dsqrt_rn(sumY2));
    if (den == 0.0) return __builtin_nan("");
    r = __ddiv_rn(sumXY, den);
  }
  if (r != r) return r;
  return common_normalize(r, count, num, weighted);
}

template <int MEASURE>
CMS_HD double common_finish(const CommonSums& s, int64_t xlen, int64_t ylen, int64_t num, int weighted) {
  return common_finish<MEASURE>(s.sumXY, s.sumX, s.sumY, s.sumX2, s.sumY2, s.sumD2, s.count, xlen, ylen, num, weighted);
}

// The reference's loop (:136-200, :251-278) over two lists whose keys ascend:
// the six sums and the count, at the common keys in ascending order.
template <class KEY>
CMS_HD CommonSums common_merge_join(const KEY* xk, const float* xv, int64_t nx, const KEY* yk, const float* yv,
                                    int64_t ny) {
  CommonSums s;
  int64_t j = 0;
  for (int64_t i = 0; i < nx && j < ny; ++i) {
    while (j < ny && yk[j] < xk[i]) ++j;
    if (j < ny && yk[j] == xk[i]) {
      const double x = (double)xv[i], y = (double)yv[j];
      s.sumXY = __dadd_rn(s.sumXY, __dmul_rn(x, y));
      s.sumX = __dadd_rn(s.sumX, x);
      s.sumX2 = __dadd_rn(s.sumX2, __dmul_rn(x, x));
      s.sumY = __dadd_rn(s.sumY, y);
      s.sumY2 = __dadd_rn(s.sumY2, __dmul_rn(y, y));
      const double diff = __dsub_rn(x, y);
      s.sumD2 = __dadd_rn(s.sumD2, __dmul_rn(diff, diff));
      ++s.count;
    }
  }
  return s;
}

// ---- the integer route ----
// One common entry's terms from the two units, as the tile kernel's lanes add
// them to a candidate's cells (two's complement: the signed sums wrap as u64).
CMS_HD uint64_t common_term_xy(int32_t xu, int32_t yu) { return (uint64_t)((int64_t)xu * (int64_t)yu); }
CMS_HD uint64_t common_term_sq(int32_t u) { return (uint64_t)((int64_t)u * (int64_t)u); }
CMS_HD uint64_t common_term_lin(int32_t u) { return (uint64_t)(int64_t)u; }
CMS_HD uint64_t common_term_d2(int32_t xu, int32_t yu) {
  const int64_t d = (int64_t)xu - (int64_t)yu;  // |d| < 2^32
  const uint64_t a = (uint64_t)(d < 0 ? -d : d);
  return a * a;  // < 2^64
}

// The cells of one eligible pair as the reference's sums: exact integers below
// 2^53 in magnitude, scaled by a power of two without rounding.
CMS_HD CommonSums common_cells_to_sums(uint64_t sxy, uint64_t sx, uint64_t sy, uint64_t sxx, uint64_t syy, uint64_t d2,
                                       uint32_t count, int s) {
  CommonSums r;
  r.sumXY = ldexp((double)(int64_t)sxy, -2 * s);
  r.sumX = ldexp((double)(int64_t)sx, -s);
  r.sumY = ldexp((double)(int64_t)sy, -s);
  r.sumX2 = ldexp((double)sxx, -2 * s);
  r.sumY2 = ldexp((double)syy, -2 * s);
  r.sumD2 = ldexp((double)d2, -2 * s);
  r.count = (int64_t)count;
  return r;
}

// ---- the tile kernel's shape ----
// LDS bytes of one candidate's cells, by measure: Euclidean holds the u64 sum of
// squared differences and the u32 count; uncentered S_xy (i64), S_xx, S_yy
// (u64) and the count; Pearson adds S_x and S_y (i64).
CMS_HD int common_cell_bytes(int measure) {
  return measure == kCommonEuclidean ? 12 : measure == kCommonUncentered ? 28 : 44;
}
// Candidates per workgroup: the largest multiple of 64 whose cells fit 64 KiB,
// so two workgroups share a CU's 160 KiB (Euclidean 5440, uncentered 2304,
// Pearson 1472).  CMS_COMMON_TILE overrides it with any multiple of 64 up to
// the default.
CMS_HD int common_tile_default(int measure) { return 65536 / common_cell_bytes(measure) / 64 * 64; }
CMS_HD int common_tile_for(int measure, int asked) {
  const int dflt = common_tile_default(measure);
  if (asked <= 0) return dflt;
  const int t = (asked + 63) / 64 * 64;
  return t > dflt ? dflt : t;
}

}  // namespace cms

#if !defined(__HIP_DEVICE_COMPILE__)
#undef __dadd_rn
#undef __dsub_rn
#undef __dmul_rn
#undef __ddiv_rn
#undef __dsqrt_rn
#endif
