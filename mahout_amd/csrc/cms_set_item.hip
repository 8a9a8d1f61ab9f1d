// cms_set_item.hip -- the item-based recommenders' estimates over the set
// similarities of a handle's DataModel (cms_set.h): for a batch of users, each
// with its preferred items in PreferenceArray order and its candidate items,
//
//   weighted  GenericItemBasedRecommender.doEstimatePreference
//             (T/impl/recommender/GenericItemBasedRecommender.java:231-259):
//             similarities = itemSimilarities(candidate, preferred IDs) (:233),
//             NaN skipped (:239), preference += sim * pref, totalSimilarity +=
//             sim, count++ (:242-244), count <= 1: NaN (:251-253), else
//             (float)(preference / totalSimilarity) and the capper (:254-258):
//             ItemEstimate (cms_ref.h), one data point per add;
//   boolean   GenericBooleanPrefItemBasedRecommender.doEstimatePreference
//             (T/impl/recommender/GenericBooleanPrefItemBasedRecommender.java
//             :52-64): totalSimilarity += sim for every sim that is not NaN,
//             (float) totalSimilarity when there was one, else NaN:
//             BoolItemEstimate (cms_ref.h).
//
// The similarity of candidate c with preferred item p is set_finish<MEASURE>
// (k, n_c, n_p, num, 0) on the key side: k the users that hold both, n_c and
// n_p the posting-list lengths, the candidate first as the reference's call
// has it, num the model's users.  A candidate that is also a preferred item is
// a pair like any other.
//
// k_set_item_estimate<MEASURE, KIND>: one workgroup of 512 threads per (user,
// tile of T consecutive dense item indices [c0, c1)) that holds a candidate of
// the user (cms_set_item_plan.h).  LDS, all on the dynamic base, in the order
// of the types' alignment:
//
//   f64 total[T]; weighted: f64 preference[T]; u32 cnt[T];
//   i32 count[T] (weighted) or found[T] (boolean)
//
// 16 B per item and T = 4096 for boolean (64 KiB), 24 B and T = 2688 for
// weighted (64,512 B): two workgroups share a CU's 160 KiB.  Everything is
// cleared once with 16-byte stores.  The workgroup then takes the user's
// preferred items one after another.  For preferred item p the users of p's
// posting list are dealt to the eight waves; a wave binary-searches that
// user's item list for c0 (not at all in the first tile) and its lanes walk to
// c1, one 4-byte load and one returnless LDS add into cnt per entry -- the walk
// of k_set_tile on the key side; a user's items are distinct, so the 64 adds
// of one wave instruction never meet in a cell.  After a barrier every thread
// takes its items of the tile (i = thread, thread + 512, ...): it reads
// cnt[i], stores 0 back (so no clearing pass runs between two preferred
// items), forms the similarity and, when that is not NaN, adds the data point
// to its own cells.  A second barrier, then the next p.
//
// Order.  A cell of total, preference and count is touched by one thread only,
// the same for every p, and the barriers separate the preferred items: every
// candidate's sums grow in preference order, one correctly rounded operation
// at a time, whatever the scheduling.  There is no f64 atomic anywhere; the
// only atomics are the u32 counts, whose sum does not depend on order.
//
// The epilogue finishes the user's slots that fall into the tile -- a
// contiguous slot range the plan gives the block -- into the batch's slot
// array; the cells of items that are no candidates are never read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "cms_exact_model.h"
#include "cms_ref.h"
#include "cms_set.h"
#include "cms_set_item_plan.h"

namespace cms {

constexpr int kSetItemThreads = 512;  // 8 waves; two workgroups per CU at the default tiles

template <int MEASURE, int KIND>
__global__ __launch_bounds__(kSetItemThreads) void k_set_item_estimate(CommonSide v, SetItemArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char set_item_lds[];
  constexpr bool kWeighted = KIND == kItemEstWeighted;
  const int T = g.T;  // a multiple of 64
  double* total = reinterpret_cast<double*>(set_item_lds);
  double* preference = total + T;  // (weighted only)
  unsigned int* cnt = reinterpret_cast<unsigned int*>(total + (kWeighted ? 2 : 1) * T);
  int32_t* count = reinterpret_cast<int32_t*>(cnt + T);  // boolean: the found flag
  {
    uint4* z = reinterpret_cast<uint4*>(set_item_lds);
    const int n16 = T * set_item_cell_bytes(KIND) / 16;
    for (int i = threadIdx.x; i < n16; i += kSetItemThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  const SetItemTile tile = g.tiles[blockIdx.x];
  const int64_t c0 = (int64_t)tile.tile * T;
  const int64_t c1 = min(v.n, c0 + (int64_t)T);
  const int width = (int)(c1 - c0);
  const int lane = threadIdx.x & 63;
  const int64_t jhi = g.pref_off[tile.user + 1];
  for (int64_t j = g.pref_off[tile.user]; j < jhi; ++j) {
    const int64_t p = g.pref_idx[j];
    const int64_t plo = v.off[p], phi = v.off[p + 1];
    for (int64_t q = plo + (threadIdx.x >> 6); q < phi; q += kSetItemThreads >> 6) {
      const int32_t user = v.key[q];
      int64_t a = v.xoff[user];
      const int64_t hi = v.xoff[user + 1];
      if (c0 > 0) {
        for (int64_t b = hi; a < b;) {  // the user's first item at or past the tile's first
          const int64_t mid = (a + b) >> 1;
          if (v.xlist[mid] < c0) a = mid + 1;
          else b = mid;
        }
      }
      for (int64_t t = a + lane; t < hi; t += 64) {
        const int64_t r = v.xlist[t];
        if (r >= c1) break;
        atomicAdd(&cnt[(int)(r - c0)], 1u);
      }
    }
    __syncthreads();
    const int64_t n_p = phi - plo;
    float pref = 0.0f;
    if (kWeighted) pref = g.pref_val[j];
    for (int i = threadIdx.x; i < width; i += kSetItemThreads) {
      const unsigned int k = cnt[i];
      // all but city block are NaN at k == 0 on the key side (set_finish): no
      // data point, and the candidate's length need not be loaded
      if (MEASURE != kSetCityBlock && k == 0u) continue;
      cnt[i] = 0u;
      const int64_t c = c0 + i;
      const double s = set_finish<MEASURE>((int64_t)k, v.off[c + 1] - v.off[c], n_p, v.num, 0);
      if (kWeighted) {
        ItemEstimate e;
        e.preference = preference[i];
        e.total = total[i];
        e.count = count[i];
        e.add(&s, &pref, 1);
        preference[i] = e.preference;
        total[i] = e.total;
        count[i] = e.count;
      } else {
        BoolItemEstimate e;
        e.total = total[i];
        e.found = count[i];
        e.add(&s, 1);
        total[i] = e.total;
        count[i] = e.found;
      }
    }
    __syncthreads();
  }
  for (int s = threadIdx.x; s < tile.len; s += kSetItemThreads) {
    const int i = (int)(g.slot_item[tile.lo + s] - c0);  // in [0, width) by the plan
    float est;
    if (kWeighted) {
      ItemEstimate e;
      e.preference = preference[i];
      e.total = total[i];
      e.count = count[i];
      est = e.finish(g.use_capper, g.lo, g.hi);
    } else {
      BoolItemEstimate e;
      e.total = total[i];
      e.found = count[i];
      est = e.finish();
    }
    g.est[tile.lo + s] = est;
  }
}

// ---- host side ----

template <int MEASURE, int KIND>
static int launch_set_item_as(cms_handle* h, const CommonSide& v, const SetItemArgs& g, int64_t ntiles) {
  static bool attr_set[64] = {};  // per device: the default tile's cells are (nearly) the whole 64 KiB
  if (!attr_set[h->device & 63]) {
    (void)hipFuncSetAttribute((const void*)k_set_item_estimate<MEASURE, KIND>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              set_item_cell_bytes(KIND) * set_item_tile_default(KIND));
    attr_set[h->device & 63] = true;
  }
  TimedScope ts(h, "set_item_estimate");
  hipLaunchKernelGGL((k_set_item_estimate<MEASURE, KIND>), dim3((unsigned)ntiles), dim3(kSetItemThreads),
                     (size_t)set_item_cell_bytes(KIND) * (size_t)g.T, h->stream, v, g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

template <int KIND>
static int launch_set_item(cms_handle* h, int32_t measure, const CommonSide& v, const SetItemArgs& g, int64_t ntiles) {
  switch (measure) {
    case kSetCooccurrence: return launch_set_item_as<kSetCooccurrence, KIND>(h, v, g, ntiles);
    case kSetTanimoto: return launch_set_item_as<kSetTanimoto, KIND>(h, v, g, ntiles);
    case kSetCityBlock: return launch_set_item_as<kSetCityBlock, KIND>(h, v, g, ntiles);
    default: return launch_set_item_as<kSetLogLikelihood, KIND>(h, v, g, ntiles);
  }
}

static int launch_set_item_kind(cms_handle* h, int32_t measure, int32_t kind, const CommonSide& v, const SetItemArgs& g,
                                int64_t ntiles) {
  return kind == kItemEstWeighted ? launch_set_item<kItemEstWeighted>(h, measure, v, g, ntiles)
                                  : launch_set_item<kItemEstBoolean>(h, measure, v, g, ntiles);
}

int set_item_estimate_batch(cms_handle* h, int32_t measure, int32_t kind, int64_t n, const int64_t* pref_offsets,
                            const int64_t* pref_keys, const float* pref_vals, const int64_t* cand_offsets,
                            const int64_t* cand_keys, int32_t use_capper, float cap_min, float cap_max, float* out) {
  return item_estimate_batch(h, launch_set_item_kind, set_item_tile_for(kind, h->tune.set_est_tile), measure, kind, n,
                             pref_offsets, pref_keys, pref_vals, cand_offsets, cand_keys, use_capper, cap_min, cap_max,
                             out);
}

// The host body of one batch, whichever kernel estimates (k_set_item_estimate here, k_common_item_estimate in
// cms_common_item.hip): the preferred keys' dense indices, the plan at tile T, the uploads, `launch` over the
// plan's tiles, and the slots back in the caller's positions.
int item_estimate_batch(cms_handle* h, ItemEstLaunch launch, int T, int32_t measure, int32_t kind, int64_t n,
                        const int64_t* pref_offsets, const int64_t* pref_keys, const float* pref_vals,
                        const int64_t* cand_offsets, const int64_t* cand_keys, int32_t use_capper, float cap_min,
                        float cap_max, float* out) {
  ExactModel& m = *h->exact;
  const int64_t M = pref_offsets[n], Q = cand_offsets[n];
  // a preferred item the model lacks would throw NoSuchItemException from itemSimilarities: before anything is written
  std::vector<int32_t> pref_idx;
  const int64_t missing = set_item_map_prefs(m.ids, M, pref_keys, pref_idx);
  if (missing >= 0)
    return set_error(CMS_E_NO_SUCH_ID, "no such key %lld in the attached model", (long long)pref_keys[missing]);
  if (Q == 0) return CMS_OK;
  SetItemPlan plan;
  set_item_plan(m.ids, n, cand_offsets, cand_keys, T, plan, [](int64_t users, auto f) {
    parallel_users(users, (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), f);
  });
  const size_t S = plan.slot_item.size();
  if (plan.tiles.size() >= (size_t(1) << 31)) return set_error(CMS_E_PARAM, "too many candidate tiles in one batch");
  std::vector<float> est(S);
  if (S > 0) {
    const int rc = [&]() -> int {
      int rc;
      if ((rc = upload(h, m.i_poff, pref_offsets, (size_t)n + 1)) || (rc = upload(h, m.i_pidx, pref_idx)) ||
          (rc = upload(h, m.e_slot, plan.slot_item)) || (rc = upload(h, m.e_tiles, plan.tiles)))
        return rc;
      if (kind == kItemEstWeighted && (rc = upload(h, m.i_pval, pref_vals, (size_t)M))) return rc;
      CMS_HIP(m.e_est.ensure(sizeof(float) * S));
      const SetItemArgs g{m.i_poff.as<int64_t>(),      m.i_pidx.as<int32_t>(), m.i_pval.as<float>(),
                          m.e_tiles.as<SetItemTile>(), m.e_slot.as<int32_t>(), m.e_est.as<float>(),
                          (int32_t)T,                  use_capper,             cap_min,
                          cap_max};
      if ((rc = launch(h, measure, kind, common_side(h, CMS_SIDE_KEY), g, (int64_t)plan.tiles.size()))) return rc;
      CMS_HIP(hipMemcpyAsync(est.data(), m.e_est.ptr, sizeof(float) * S, hipMemcpyDeviceToHost, h->stream));
      return CMS_OK;
    }();
    const hipError_t synced = hipStreamSynchronize(h->stream);  // whatever was queued is done with the host arrays
    if (rc) return rc;
    CMS_HIP(synced);
  }
  // back to the caller's positions; a key the model lacks has no data point
  for (int64_t i = 0; i < Q; ++i) out[i] = plan.pos_slot[(size_t)i] < 0 ? __builtin_nanf("") : est[(size_t)plan.pos_slot[(size_t)i]];
  return CMS_OK;
}

}  // namespace cms
