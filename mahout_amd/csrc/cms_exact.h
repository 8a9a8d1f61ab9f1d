// cms_exact.h -- what the host and the device share of the exact cosine
// (cms_exact.hip): the attach rules of a DataModel, the merge join of two
// preference lists and the end of CosineSimilarity.userSimilarity.
//
// CosineSimilarity (T/impl/similarity/CosineSimilarity.java:44-103) is the
// full-norm cosine over the raw preferences, the quantity the sketch cosine
// approximates:
//   sumX2, sumXY, sumY2: sequential fp64 sums of (double) x * (double) x and so
//   on (:56-80) -- sumX2 and sumXY in x's preference order (ascending item,
//   GenericUserPreferenceArray is sorted by item), sumXY over the common items
//   only (:65-74), sumY2 in y's order (:76-80);
//   NaN when either list is empty (:52-54) or Math.sqrt(sumX2) *
//   Math.sqrt(sumY2) == 0.0 (:96-101); else sumXY / denominator (:102) and
//   normalizeWeightResult(result, count, count), count = xLength + yLength
//   (:82-87, AbstractSimilarity.java:313-330).
// Everything here is a pure __host__ __device__ function, written as
// cms_ref.h is: the kernels call these and hold no second copy, and
// tests/test_exact_host.py runs them on the CPU against the plain-Python
// restatement (tests/cpp/exact_host_shim.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#include "cms_hash.h"

// One text for both sides: in the host pass the intrinsics below read as the
// plain operators, to the end of this header (as cms_ref.h does it).
#if !defined(__HIP_DEVICE_COMPILE__)
#define __dadd_rn(x, y) ((x) + (y))
#define __dsub_rn(x, y) ((x) - (y))
#define __dmul_rn(x, y) ((x) * (y))
#define __ddiv_rn(x, y) ((x) / (y))
#endif

namespace cms {

// An owner whose sum of squared units is below this is integer-eligible: every
// partial sum the reference forms for two such owners is an exact multiple of
// 2^-2s below 2^53 in magnitude (|partial sumXY| <= sum |x||y| <= sqrt(U_x U_y)).
constexpr uint64_t kExactEligible = 1ULL << 53;
constexpr int kExactMaxShift = 30;
constexpr int kExactNoShift = -1;  // no such s: every owner takes the sequential loop

// frac_bits_for's rule with negative values allowed: the smallest s in
// [0, 30] for which every value times 2^s is an integer of magnitude below
// 2^31; kExactNoShift when there is none (a NaN or infinite value included).
// A larger s only grows the magnitudes, so the smallest s that makes every
// value an integer decides.
CMS_HD int exact_shift_for(const float* vals, int64_t n) {
  int s = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double v = (double)vals[i];
    if (!(fabs(v) <= 1.7976931348623157e308)) return kExactNoShift;  // NaN, +-Infinity
    while (s <= kExactMaxShift && ldexp(v, s) != floor(ldexp(v, s))) ++s;
    if (s > kExactMaxShift) return kExactNoShift;
  }
  for (int64_t i = 0; i < n; ++i)
    if (!(fabs(ldexp((double)vals[i], s)) < 2147483648.0)) return kExactNoShift;
  return s;
}

// the value in units of 2^-s (exact_shift_for's s)
CMS_HD int32_t exact_unit(float v, int s) { return (int32_t)ldexp((double)v, s); }

// One owner's preferences [lo, hi): U = the sum of its squared units,
// saturating (all ones when there is no s), the reference's own sequential
// sumX2 (:63) and Math.sqrt of it (:96).
CMS_HD void exact_owner_sums(const float* vals, int64_t lo, int64_t hi, int s, uint64_t& U, double& sum2,
                             double& root) {
  uint64_t u = s == kExactNoShift ? ~0ULL : 0ULL;
  double a = 0.0;
  for (int64_t t = lo; t < hi; ++t) {
    const double x = (double)vals[t];
    a = __dadd_rn(a, __dmul_rn(x, x));
    if (s != kExactNoShift) {
      const int64_t w = exact_unit(vals[t], s);
      const uint64_t sq = (uint64_t)(w * w);  // < 2^62
      u = u + sq < u ? ~0ULL : u + sq;
    }
  }
  U = u;
  sum2 = a;
#if defined(__HIP_DEVICE_COMPILE__)
  root = __dsqrt_rn(a);
#else
  root = sqrt(a);  // IEEE: correctly rounded, as Math.sqrt
#endif
}

// A DataModel as a CSR: offsets start at 0 and never decrease, and the keys
// of a row are strictly ascending, as GenericDataModel gives them
// (GenericUserPreferenceArray.sortByItem, no item twice).
CMS_HD bool exact_valid_csr(int64_t n, const int64_t* off, const int64_t* keys) {
  if (off[0] != 0) return false;
  for (int64_t r = 0; r < n; ++r)
    if (off[r + 1] < off[r]) return false;
  for (int64_t r = 0; r < n; ++r)  // (the offsets are sound: every t below is within the keys)
    for (int64_t t = off[r] + 1; t < off[r + 1]; ++t)
      if (keys[t] <= keys[t - 1]) return false;
  return true;
}

// sumXY (:58-75) of two lists whose items ascend: x's order, the common items
// only.  ITEM is the key type (the model's dense item index on the device).
template <class ITEM>
CMS_HD double exact_merge_join(const ITEM* xi, const float* xv, int64_t nx, const ITEM* yi, const float* yv,
                               int64_t ny) {
  double sumXY = 0.0;
  int64_t j = 0;
  for (int64_t i = 0; i < nx && j < ny; ++i) {
    while (j < ny && yi[j] < xi[i]) ++j;
    if (j < ny && yi[j] == xi[i]) sumXY = __dadd_rn(sumXY, __dmul_rn((double)xv[i], (double)yv[j]));
  }
  return sumXY;
}

// normalizeWeightResult(result, count, num = count) (AbstractSimilarity.java:313-330)
CMS_HD double exact_normalize(double r, int64_t count, int weighted) {
  if (weighted) {
    const double scale = __dsub_rn(1.0, __ddiv_rn((double)count, (double)(count + 1)));
    if (r < 0.0) r = __dadd_rn(-1.0, __dmul_rn(scale, __dadd_rn(1.0, r)));
    else r = __dsub_rn(1.0, __dmul_rn(scale, __dsub_rn(1.0, r)));
  }
  if (r < -1.0) r = -1.0;
  else if (r > 1.0) r = 1.0;
  return r;
}

// The end of userSimilarity from sumXY, the two stored Math.sqrt(sumX2) and
// the list lengths (:52-54, :82-102).  A pair with no common item has
// sumXY = 0.0 and gives 0.0 / denominator, not NaN.
CMS_HD double exact_finish(double sumXY, double rootX, double rootY, int64_t xlen, int64_t ylen, int weighted) {
  if (xlen == 0 || ylen == 0) return __builtin_nan("");
  const double den = __dmul_rn(rootX, rootY);
  if (den == 0.0) return __builtin_nan("");
  const double r = __ddiv_rn(sumXY, den);
  if (r != r) return r;  // (:85) NaN stays as it is
  return exact_normalize(r, xlen + ylen, weighted);
}

// The integer route's sumXY: the dot of the units is an exact integer below
// 2^53 in magnitude, and 2^-2s scales it without rounding.
CMS_HD double exact_dot_to_sum(int64_t dot, int s) { return ldexp((double)dot, -2 * s); }

// ---- the tile kernel's shape ----
// i64 cells of one candidate tile in LDS: 8192 cells are 64 KiB, so two
// workgroups share a CU's 160 KiB.  CMS_EXACT_TILE overrides it with any
// multiple of 64 up to the default.
constexpr int kExactTile = 8192;
CMS_HD int exact_tile_for(int asked) {
  if (asked <= 0) return kExactTile;
  int t = (asked + 63) / 64 * 64;
  return t > kExactTile ? kExactTile : t;
}

// ---- the estimate kernel's shape ----
// Candidate slots of one (user, tile) in LDS: per slot the dense item index
// (i32), preference and totalSimilarity (f64) and count (i32), 24 bytes; 2048
// slots are 48 KiB, so three workgroups share a CU's 160 KiB.
// CMS_EXACT_EST_TILE overrides it with any multiple of 64 up to the default.
constexpr int kExactEstTile = 2048;
constexpr int kExactEstSlotBytes = 24;
CMS_HD int exact_est_tile_for(int asked) {
  if (asked <= 0) return kExactEstTile;
  int t = (asked + 63) / 64 * 64;
  return t > kExactEstTile ? kExactEstTile : t;
}

}  // namespace cms

#if !defined(__HIP_DEVICE_COMPILE__)
#undef __dadd_rn
#undef __dsub_rn
#undef __dmul_rn
#undef __ddiv_rn
#endif
