// cms_ref.h -- the reference's scalar query semantics, stated once for the
// four table modes (fixed shape or per-owner shapes, u32 or fp64 counters)
// and for the host (tests/test_ref_host.py runs these functions on the CPU
// against the oracle):
//   java_min, normalize_weight, cosine_finish   Math.min, normalizeWeightResult
//   sketch_get      DoubleCountMinSketch.get(key)                     (:94-103)
//   estimate_one    GenericUserBasedRecommender.doEstimatePreference (:134-184)
//   item_estimate_one  GenericItemBasedRecommender.doEstimatePreference (:231-259)
// A mode enters only through its counter accessor: the owner's depth, a
// per-item prepared key, the raw counter at (row, sketch row, key) and the
// scaling of a point query.  Every fp64 step is one IEEE round-to-nearest
// operation, as the JVM computes it: the *_rn intrinsics on the device, the
// plain operators on the host (no contraction: -ffp-contract=off).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "cms_hash.h"
#include "cms_internal.h"

// One text for both sides: in the host pass the intrinsics below read as the
// plain operators, to the end of this header.
#if !defined(__HIP_DEVICE_COMPILE__)
#define __dadd_rn(x, y) ((x) + (y))
#define __dsub_rn(x, y) ((x) - (y))
#define __dmul_rn(x, y) ((x) * (y))
#define __ddiv_rn(x, y) ((x) / (y))
#endif

namespace cms {

// Math.min(a, b) for doubles (NaN wins; -0.0 < +0.0).
CMS_HD double java_min(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && signbit(b)) return b;
  return (a <= b) ? a : b;
}

// normalizeWeightResult(result, count=1, num=0) (AbstractSimilarity.java:313-330):
// WEIGHTED scales by 1 - count/(num+1) = 0, i.e. +-1; then the clamp to [-1, 1].
CMS_HD double normalize_weight(double r, int weighted) {
  if (weighted) {
    const double scale = __dsub_rn(1.0, 1.0 / 1.0);  // 1 - count/(num+1) = 0
    if (r < 0.0) r = __dadd_rn(-1.0, __dmul_rn(scale, __dadd_rn(1.0, r)));
    else r = __dsub_rn(1.0, __dmul_rn(scale, __dsub_rn(1.0, r)));
  }
  if (r < -1.0) r = -1.0;
  else if (r > 1.0) r = 1.0;
  return r;
}

// The end of CosineCM.userSimilarity: minc is the running Math.min over the
// sketch rows whose denominator was not 0, started at Double.MAX_VALUE
// (DoubleCountMinSketch.cosine :143-148: NaN when no row qualified), then
// normalizeWeightResult.
CMS_HD double cosine_finish(double minc, int weighted) {
  double r = minc == DBL_MAX ? __builtin_nan("") : minc;
  if (r == r) r = normalize_weight(r, weighted);
  return r;
}

// ---- counter accessors ----
// depth(row): the owner's sketch rows.  prepare(kp, key): what the neighbour
// loop keeps of one item's reduced key.  counter(row, d, key): the raw counter
// of sketch row d, by a prepared key or (hashing on the spot) by the reduced
// key itself.  scale(est): a point query in preference units.

// Fixed shapes hash an item once for the whole neighbourhood: d * w + bucket
// of every sketch row.  (A plain array, not a struct around one: only that
// stays in registers under the neighbour loop's dynamic index.)
using Buckets = uint32_t[CMS_MAX_DEPTH];
CMS_HD void fixed_buckets(const HashParams& hp, uint64_t kp, Buckets& key) {
  for (int d = 0; d < hp.depth; ++d) key[d] = (uint32_t)d * hp.width + bucket(hp, d, kp);
}

// fixed shape, u32 counters in their storage forms (device only)
struct FixedU32 {
  TableView tv;
  HashParams hp;
  using Key = Buckets;
  __device__ __forceinline__ int depth(int64_t) const { return hp.depth; }
  __device__ __forceinline__ void prepare(uint64_t kp, Key& key) const { fixed_buckets(hp, kp, key); }
  __device__ __forceinline__ double counter(int64_t row, int d, const Key& key) const {
    return (double)tv.get(row, key[d]);
  }
  __device__ __forceinline__ double counter(int64_t row, int d, uint64_t kp) const {
    return (double)tv.get(row, (int64_t)d * hp.width + bucket(hp, d, kp));
  }
  __device__ __forceinline__ double scale(double est) const { return ldexp(est, -hp.frac_bits); }
};

// fixed shape, fp64 counters [n][d][w]
struct FixedF64 {
  const double* tab;
  HashParams hp;
  using Key = Buckets;
  CMS_HD int depth(int64_t) const { return hp.depth; }
  CMS_HD void prepare(uint64_t kp, Key& key) const { fixed_buckets(hp, kp, key); }
  CMS_HD double counter(int64_t row, int d, const Key& key) const {
    return tab[row * ((int64_t)hp.depth * hp.width) + key[d]];
  }
  CMS_HD double counter(int64_t row, int d, uint64_t kp) const {
    return tab[row * ((int64_t)hp.depth * hp.width) + (int64_t)d * hp.width + bucket(hp, d, kp)];
  }
  CMS_HD double scale(double est) const { return est; }
};

// per-owner shapes: every neighbour hashes the item at its own width
struct PoU32 {
  const PoShape* shp;
  const uint32_t* sk;
  HashParams hp;
  using Key = uint64_t;
  CMS_HD int depth(int64_t row) const { return shp[row].d; }
  CMS_HD void prepare(uint64_t kp, Key& key) const { key = kp; }
  CMS_HD double counter(int64_t row, int d, uint64_t kp) const {
    const PoShape s = shp[row];
    return (double)sk[s.soff + (int64_t)d * s.w + bucket_wbq(hp, d, kp, (uint32_t)s.w, s.barrett)];
  }
  CMS_HD double scale(double est) const { return ldexp(est, -hp.frac_bits); }
};

struct PoF64 {
  const PoShape* shp;
  const double* sk;
  HashParams hp;
  using Key = uint64_t;
  CMS_HD int depth(int64_t row) const { return shp[row].d; }
  CMS_HD void prepare(uint64_t kp, Key& key) const { key = kp; }
  CMS_HD double counter(int64_t row, int d, uint64_t kp) const {
    const PoShape s = shp[row];
    return sk[s.soff + (int64_t)d * s.w + bucket_wb(hp, d, kp, (uint32_t)s.w, s.barrett)];
  }
  CMS_HD double scale(double est) const { return est; }
};

// ---- the queries ----

// DoubleCountMinSketch.get(key) (:94-103) of owner `row`: the minimum over its
// sketch rows, from Double.MAX_VALUE.  key: the reduced key or a prepared one.
template <class Acc, class K>
CMS_HD double sketch_get(const Acc& acc, int64_t row, const K& key) {
  const int depth = acc.depth(row);
  double est = DBL_MAX;
  for (int d = 0; d < depth; ++d) {
    const double v = acc.counter(row, d, key);
    if (v < est) est = v;
  }
  return acc.scale(est);
}

// doEstimatePreference with the CosineCM point query
// (GenericUserBasedRecommender.java:134-184) for the item of reduced key kp,
// the neighbourhood walked in the caller's order so the fp64 sums round as in
// Java: pref = (float) get(item) of the neighbour's sketch (0 -> no data
// point), sim = userSimilarity(user, neighbour) (NaN skipped), preference +=
// sim * pref, total += sim; < 2 points -> NaN; (float)(preference / total);
// then the EstimatedPreferenceCapper clamp when enabled.
template <class Acc>
CMS_HD float estimate_one(const Acc& acc, int64_t user_row, const int64_t* nb_rows, const double* sims, int64_t m,
                          uint64_t kp, int use_capper, float lo, float hi) {
  typename Acc::Key key;
  acc.prepare(kp, key);
  double preference = 0.0, total = 0.0;
  int count = 0;
  for (int64_t j = 0; j < m; ++j) {
    const int64_t r = nb_rows[j];
    if (r == user_row) continue;
    const float pref = (float)sketch_get(acc, r, key);
    if (pref == 0.0f) continue;
    const double s = sims[j];
    if (s != s) continue;
    preference = __dadd_rn(preference, __dmul_rn(s, (double)pref));
    total = __dadd_rn(total, s);
    ++count;
  }
  float e = __builtin_nanf("");
  if (count > 1) {
    e = (float)__ddiv_rn(preference, total);
    if (use_capper) {
      if (e > hi) e = hi;
      else if (e < lo) e = lo;
    }
  }
  return e;
}

// GenericItemBasedRecommender.doEstimatePreference (:231-259) for one
// candidate item: sims[i] = itemSimilarity(candidate, the user's i-th
// preferred item), prefs[i] that preference's value, walked in preference
// order so the fp64 sums round as in Java.  NaN similarities are skipped,
// preference += sim * (double) pref and total += sim (one rounded operation
// each); count <= 1 -> NaN; (float)(preference / total); then the
// EstimatedPreferenceCapper clamp when enabled, as in estimate_one.  The
// running state is a struct so a caller may feed the preferences in pieces
// (the kernel's right tiles), in order.
struct ItemEstimate {
  double preference = 0.0, total = 0.0;
  int count = 0;
  CMS_HD void add(const double* sims, const float* prefs, int64_t m) {
    for (int64_t i = 0; i < m; ++i) {
      const double s = sims[i];
      if (s != s) continue;
      preference = __dadd_rn(preference, __dmul_rn(s, (double)prefs[i]));
      total = __dadd_rn(total, s);
      ++count;
    }
  }
  CMS_HD float finish(int use_capper, float lo, float hi) const {
    float e = __builtin_nanf("");
    if (count > 1) {
      e = (float)__ddiv_rn(preference, total);
      if (use_capper) {
        if (e > hi) e = hi;
        else if (e < lo) e = lo;
      }
    }
    return e;
  }
};

CMS_HD float item_estimate_one(const double* sims, const float* prefs, int64_t m, int use_capper, float lo, float hi) {
  ItemEstimate e;
  e.add(sims, prefs, m);
  return e.finish(use_capper, lo, hi);
}

}  // namespace cms

#if !defined(__HIP_DEVICE_COMPILE__)
#undef __dadd_rn
#undef __dsub_rn
#undef __dmul_rn
#undef __ddiv_rn
#endif
