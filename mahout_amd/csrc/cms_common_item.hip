// cms_common_item.hip -- the item-based recommenders' estimates over the
// co-rated similarities of a handle's DataModel (cms_common.h): uncentered
// cosine, Pearson and Euclidean.  The semantics are cms_set_item.hip's header's
// with one change: the similarity of candidate c with preferred item p is
// common_finish<MEASURE> over the users that hold both, on the key side -- the
// candidate is X and the preferred item Y, as the reference's itemSimilarities
// (candidate, preferredIDs) has it, xlen and ylen the two posting-list lengths,
// num and weighted the key side's (common_side).  A candidate that is also a
// preferred item is a pair like any other.
//
// k_common_item_estimate<MEASURE, KIND>: one workgroup of 512 threads per (user,
// tile of T consecutive dense item indices [c0, c1)) that holds a candidate of
// the user (cms_set_item_plan.h).  LDS, all on the dynamic base, in the order
// of the types' alignment (cms_common_item.h):
//
//   u64 wide[kWide][T] (k_common_tile's sums); f64 total[T]; weighted: f64
//   preference[T]; u32 cnt[T]; i32 count[T] (weighted) or found[T] (boolean)
//
// cleared once with 16-byte stores.  The workgroup takes the user's preferred
// items one after another; one step, for preferred item p:
//
//   scatter (p common-eligible, iU[p] < 2^51).  p's posting entries (user u,
//   unit y) are dealt to the eight waves, entry e of a round of 512 to wave
//   e % 8, lane e / 8, so a short list still feeds every wave.  A wave stages
//   its up to 64 entries lane-parallel in one go -- user, unit, xoff[u],
//   xoff[u + 1], and each lane its own binary search for c0 in its user's item
//   list (none in the first tile): the dependent loads of 64 entries overlap
//   instead of queueing entry after entry.  The wave then takes the staged
//   entries one after another by readlane, and its lanes walk that user's
//   items up to c1, adding the terms of (x = the candidate's unit, y) to the
//   candidate's cells with LDS atomics and cnt += 1.  A user's items are
//   distinct, so the 64 lanes of one instruction never meet in a cell.
//   barrier
//   finish.  Thread t takes the items t, t + 512, ... of the tile.  cnt == 0:
//   nothing (every measure is NaN with nothing in common).  Else it reads the
//   cells and stores zeros back (no clearing pass between two steps), forms
//   the sums -- common_cells_to_sums when the candidate too is eligible, else
//   common_merge_join over the two posting lists -- and the similarity, and
//   adds the data point to its own ItemEstimate / BoolItemEstimate cells.
//   barrier
//
//   p not eligible (the same test for the whole block; a model without a shift
//   has every iU saturated): no scatter; the threads take the block's slots
//   and run common_merge_join(c, p) per candidate slot into that slot's cells.
//   Cells change hands between two steps; the barriers keep the order.
//
// Order.  preference, total and count of a candidate are touched by one thread
// per step and the barriers separate the steps: the sums grow in preference
// order, one correctly rounded operation at a time, with no f64 atomic.  The
// only atomics are integer ones, whose sums do not depend on order
// (cms_common.h proves the integer route for eligible pairs).
//
// The epilogue finishes the block's slots into the batch's slot array.
#include <hip/hip_runtime.h>

#include "cms_common.h"
#include "cms_common_item.h"
#include "cms_exact_model.h"
#include "cms_ref.h"

namespace cms {

constexpr int kCommonItemThreads = 512;  // 8 waves; two workgroups per CU at the default tiles
constexpr int kCommonItemWaves = kCommonItemThreads / 64;

// lane e's value of a staged 64-bit quantity (e is the same for the whole wave)
__device__ __forceinline__ int64_t wave_get(int64_t x, int e) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(uint32_t)x, e);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), e);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// one data point (NaN: none) into item i's estimate cells
template <int KIND>
__device__ __forceinline__ void common_item_add(double* total, double* preference, int32_t* count, int i, double sim,
                                                float pref) {
  if constexpr (KIND == kItemEstWeighted) {
    ItemEstimate e;
    e.preference = preference[i];
    e.total = total[i];
    e.count = count[i];
    e.add(&sim, &pref, 1);
    preference[i] = e.preference;
    total[i] = e.total;
    count[i] = e.count;
  } else {
    BoolItemEstimate e;
    e.total = total[i];
    e.found = count[i];
    e.add(&sim, 1);
    total[i] = e.total;
    count[i] = e.found;
  }
}

template <int MEASURE, int KIND>
__global__ __launch_bounds__(kCommonItemThreads) void k_common_item_estimate(CommonSide v, SetItemArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char common_item_lds[];
  constexpr bool kWeighted = KIND == kItemEstWeighted;
  constexpr int kWide = common_item_wide(MEASURE);
  static_assert(kWide * 8 + (kWeighted ? 24 : 16) == common_item_cell_bytes(MEASURE, KIND), "common_item_cell_bytes");
  const int T = g.T;  // a multiple of 64
  // Euclidean: [0] the squared differences.  Else [0] S_xy, [1] S_xx, [2] S_yy, Pearson [3] S_x, [4] S_y.
  unsigned long long* wide = reinterpret_cast<unsigned long long*>(common_item_lds);
  double* total = reinterpret_cast<double*>(wide + (size_t)kWide * T);
  double* preference = total + T;  // (weighted only)
  unsigned int* cnt = reinterpret_cast<unsigned int*>(total + (kWeighted ? 2 : 1) * T);
  int32_t* count = reinterpret_cast<int32_t*>(cnt + T);  // boolean: the found flag
  {
    uint4* z = reinterpret_cast<uint4*>(common_item_lds);
    const int n16 = T * common_item_cell_bytes(MEASURE, KIND) / 16;
    for (int i = threadIdx.x; i < n16; i += kCommonItemThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  const SetItemTile tile = g.tiles[blockIdx.x];
  const int64_t c0 = (int64_t)tile.tile * T;
  const int64_t c1 = min(v.n, c0 + (int64_t)T);
  const int width = (int)(c1 - c0);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t jhi = g.pref_off[tile.user + 1];
  for (int64_t j = g.pref_off[tile.user]; j < jhi; ++j) {
    const int64_t p = g.pref_idx[j];
    const int64_t plo = v.off[p], phi = v.off[p + 1];
    const int64_t n_p = phi - plo;
    float pref = 0.0f;
    if (kWeighted) pref = g.pref_val[j];
    if (v.U[p] >= kCommonEligible) {
      // the reference's own loop per candidate slot of the block
      for (int s = threadIdx.x; s < tile.len; s += kCommonItemThreads) {
        const int64_t c = g.slot_item[tile.lo + s];  // in [c0, c1) by the plan
        const int64_t clo = v.off[c], n_c = v.off[c + 1] - clo;
        const CommonSums sums = common_merge_join(v.key + clo, v.val + clo, n_c, v.key + plo, v.val + plo, n_p);
        common_item_add<KIND>(total, preference, count, (int)(c - c0),
                              common_finish<MEASURE>(sums, n_c, n_p, v.num, v.weighted), pref);
      }
      __syncthreads();
      continue;
    }
    for (int64_t base = plo; base < phi; base += kCommonItemThreads) {
      // this wave's entries of the round: base + wave + 8 * lane, lanes [0, m)
      const int64_t left = phi - base - wave;
      const int m = left <= 0 ? 0 : (int)min((int64_t)64, (left + kCommonItemWaves - 1) / kCommonItemWaves);
      int64_t a = 0, hi = 0;
      int32_t yu = 0;
      if (lane < m) {
        const int64_t q = base + wave + (int64_t)kCommonItemWaves * lane;
        const int32_t user = v.key[q];
        yu = v.unit[q];
        a = v.xoff[user];
        hi = v.xoff[user + 1];
        if (c0 > 0) {
          for (int64_t b = hi; a < b;) {  // the user's first item at or past the tile's first
            const int64_t mid = (a + b) >> 1;
            if (v.xlist[mid] < c0) a = mid + 1;
            else b = mid;
          }
        }
      }
      for (int e = 0; e < m; ++e) {
        const int64_t hi_e = wave_get(hi, e);
        const int32_t y = __builtin_amdgcn_readlane(yu, e);
        for (int64_t t = wave_get(a, e) + lane; t < hi_e; t += 64) {
          const int64_t r = v.xlist[t];
          if (r >= c1) break;
          const int32_t x = v.xunit[t];
          const int i = (int)(r - c0);
          if constexpr (MEASURE == kCommonEuclidean) {
            atomicAdd(&wide[i], (unsigned long long)common_term_d2(x, y));
          } else {
            atomicAdd(&wide[i], (unsigned long long)common_term_xy(x, y));
            atomicAdd(&wide[T + i], (unsigned long long)common_term_sq(x));
            atomicAdd(&wide[2 * T + i], (unsigned long long)common_term_sq(y));
            if constexpr (MEASURE == kCommonPearson) {
              atomicAdd(&wide[3 * T + i], (unsigned long long)common_term_lin(x));
              atomicAdd(&wide[4 * T + i], (unsigned long long)common_term_lin(y));
            }
          }
          atomicAdd(&cnt[i], 1u);
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < width; i += kCommonItemThreads) {
      const unsigned int k = cnt[i];
      if (k == 0u) continue;  // nothing in common: NaN by every measure, no data point
      cnt[i] = 0u;
      unsigned long long w[kWide];
#pragma unroll
      for (int a = 0; a < kWide; ++a) {
        w[a] = wide[a * T + i];
        wide[a * T + i] = 0ULL;
      }
      const int64_t c = c0 + i;
      const int64_t clo = v.off[c], n_c = v.off[c + 1] - clo;
      CommonSums sums;
      if (v.U[c] >= kCommonEligible)  // the cells may have wrapped: the reference's own loop
        sums = common_merge_join(v.key + clo, v.val + clo, n_c, v.key + plo, v.val + plo, n_p);
      else if constexpr (MEASURE == kCommonEuclidean)
        sums = common_cells_to_sums(0, 0, 0, 0, 0, w[0], k, v.shift);
      else if constexpr (MEASURE == kCommonUncentered)
        sums = common_cells_to_sums(w[0], 0, 0, w[1], w[2], 0, k, v.shift);
      else
        sums = common_cells_to_sums(w[0], w[3], w[4], w[1], w[2], 0, k, v.shift);
      common_item_add<KIND>(total, preference, count, i, common_finish<MEASURE>(sums, n_c, n_p, v.num, v.weighted),
                            pref);
    }
    __syncthreads();
  }
  for (int s = threadIdx.x; s < tile.len; s += kCommonItemThreads) {
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
static int launch_common_item_as(cms_handle* h, const CommonSide& v, const SetItemArgs& g, int64_t ntiles) {
  static bool attr_set[64] = {};  // per device: the default tile's cells are (nearly) the whole 64 KiB
  if (!attr_set[h->device & 63]) {
    (void)hipFuncSetAttribute((const void*)k_common_item_estimate<MEASURE, KIND>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              common_item_cell_bytes(MEASURE, KIND) * common_item_tile_default(MEASURE, KIND));
    attr_set[h->device & 63] = true;
  }
  TimedScope ts(h, "common_item_estimate");
  hipLaunchKernelGGL((k_common_item_estimate<MEASURE, KIND>), dim3((unsigned)ntiles), dim3(kCommonItemThreads),
                     (size_t)common_item_cell_bytes(MEASURE, KIND) * (size_t)g.T, h->stream, v, g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

template <int KIND>
static int launch_common_item(cms_handle* h, int32_t measure, const CommonSide& v, const SetItemArgs& g,
                              int64_t ntiles) {
  switch (measure) {
    case kCommonUncentered: return launch_common_item_as<kCommonUncentered, KIND>(h, v, g, ntiles);
    case kCommonPearson: return launch_common_item_as<kCommonPearson, KIND>(h, v, g, ntiles);
    default: return launch_common_item_as<kCommonEuclidean, KIND>(h, v, g, ntiles);
  }
}

static int launch_common_item_kind(cms_handle* h, int32_t measure, int32_t kind, const CommonSide& v,
                                   const SetItemArgs& g, int64_t ntiles) {
  return kind == kItemEstWeighted ? launch_common_item<kItemEstWeighted>(h, measure, v, g, ntiles)
                                  : launch_common_item<kItemEstBoolean>(h, measure, v, g, ntiles);
}

int common_item_estimate_batch(cms_handle* h, int32_t measure, int32_t kind, int64_t n, const int64_t* pref_offsets,
                               const int64_t* pref_keys, const float* pref_vals, const int64_t* cand_offsets,
                               const int64_t* cand_keys, int32_t use_capper, float cap_min, float cap_max, float* out) {
  return item_estimate_batch(h, launch_common_item_kind, common_item_tile_for(measure, kind, h->tune.common_est_tile),
                             measure, kind, n, pref_offsets, pref_keys, pref_vals, cand_offsets, cand_keys, use_capper,
                             cap_min, cap_max, out);
}

}  // namespace cms
