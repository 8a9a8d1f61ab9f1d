// cms_neighbor.hip -- the user-based recommenders' estimates over a chosen
// similarity: GenericUserBasedRecommender (generic) and
// GenericBooleanPrefUserBasedRecommender (boolean) with any measure of the
// co-rated family (cms_common.hip) or the set family (cms_set.hip) as
// UserSimilarity, over the attached model's owner side.  cms_neighbor.h states
// the kinds and the LDS layout; the sketch table is neither read nor written.
//
//   - the similarities of a batch: userSimilarity(user, neighbour) of every
//     pair, one elementwise launch of the family's own pair kernel
//     (k_common_pairs<MEASURE> or k_set_pairs<MEASURE>, CMS_SIDE_OWNER) into a
//     device buffer that the estimate kernel reads;
//   - k_nb_estimate<KIND>: one workgroup of 256 threads per (user, tile of T
//     candidate slots), the plan of cms_exact_plan.h.  The neighbourhood is
//     taken in chunks of G neighbours, two barriers a chunk:
//       gather  the chunk's neighbours are dealt to the four waves.  A wave
//               finds where its neighbour's ascending item list reaches the
//               tile's first slot with a wave-wide search (64 lanes probe 64
//               evenly spaced entries, one ballot narrows the range 64-fold a
//               step), walks the list 64 entries a step to the tile's last
//               slot, each lane looks its item up among the slots in LDS and on
//               a hit ORs bit g (the neighbour's place in the chunk) into the
//               slot's mask word and, generic, stores the preference into
//               pref[g][slot].  A neighbour's items are distinct: a (g, slot)
//               cell has one writer, the atomic serves the shared mask word.
//       fold    every thread owns the slots tid, tid + 256, ... and their sums
//               in registers.  It walks the set bits of a slot's mask in
//               ascending g, one data point per bit, and clears the mask; beside
//               that the first G threads load the next chunk's similarities and
//               list ranges into the other half of a double buffer.
//     Ascending g within a chunk and the chunks one after another is the
//     caller's neighbourhood order, so every slot's sums round as the
//     reference's do; which wave gathered which neighbour, and when, decides
//     nothing.  A neighbour that is the user, and for the generic kind one
//     whose similarity is NaN, gets an empty list range: it sets no bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <type_traits>
#include <vector>

#include "cms_exact_model.h"
#include "cms_neighbor.h"
#include "cms_ref.h"

namespace cms {

// the first index p of [a, hi) with item[p] >= first (hi when there is none): the same value on every lane
__device__ __forceinline__ int64_t nb_wave_lower_bound(const int32_t* __restrict__ item, int64_t a, int64_t hi,
                                                       int32_t first, int lane) {
  // every entry before a is below first; the entry at a + n, when a + n < hi, is not
  int64_t n = hi - a;
  while (n > 64) {
    const int64_t step = (n + 63) >> 6;
    const int64_t pos = a + (int64_t)(lane + 1) * step - 1;  // ascending with the lane; past the range: not below
    const int below = pos < a + n && item[pos] < first;
    const int c = __popcll(__ballot(below));  // the probes below first are the lanes [0, c)
    const int64_t end = a + n;
    a += (int64_t)c * step;                   // one past probe c - 1: at most end
    n = (a + step - 1 < end ? a + step - 1 : end) - a;  // probe c, when in range, is not below first
  }
  const int below = lane < n && item[a + lane] < first;
  return a + __popcll(__ballot(below));
}

template <int KIND>
__global__ __launch_bounds__(kNbThreads) void k_nb_estimate(CommonSide v, NbEstArgs g) {
  constexpr int G = nb_chunk(KIND);
  constexpr int kPer = nb_slots_per_thread(KIND);
  using Sum = typename std::conditional<KIND == kNbGeneric, ItemEstimate, BoolUserEstimate>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_lds[];
  double* c_sim = reinterpret_cast<double*>(nb_lds);            // [2][G]
  int64_t* c_lo = reinterpret_cast<int64_t*>(c_sim + 2 * G);    // [2][G]
  int64_t* c_hi = c_lo + 2 * G;                                 // [2][G]
  int32_t* slot = reinterpret_cast<int32_t*>(c_hi + 2 * G);     // [T]
  unsigned int* mask = reinterpret_cast<unsigned int*>(slot + g.T);  // [T]
  float* pref = reinterpret_cast<float*>(mask + g.T);           // [G][T], generic only
  const int T = g.T;
  const ExactEstTile tile = g.tiles[blockIdx.x];
  const int len = tile.len;  // 1 .. T
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t x = g.urow[tile.user];
  const int64_t j0 = g.nb_off[tile.user], jhi = g.nb_off[tile.user + 1];

  // chunk c's neighbours [j0 + c G, ...) into half c & 1: a dead neighbour's range is empty
  auto load_chunk = [&](int64_t c) {
    const int64_t j = j0 + c * G + tid;
    if (tid < G && j < jhi) {
      const int64_t y = g.nb_row[j];
      const double s = g.sims[j];
      const bool dead = y == x || (KIND == kNbGeneric && s != s);
      const int64_t lo = v.off[y];
      const int at = (int)(c & 1) * G + tid;
      c_sim[at] = s;
      c_lo[at] = lo;
      c_hi[at] = dead ? lo : v.off[y + 1];
    }
  };

  for (int i = tid; i < len; i += kNbThreads) {
    slot[i] = g.slot_item[tile.lo + i];
    mask[i] = 0u;
  }
  load_chunk(0);
  __syncthreads();
  const int32_t first = slot[0], last = slot[len - 1];
  Sum sum[kPer];

  const int64_t chunks = (jhi - j0 + G - 1) / G;
  for (int64_t c = 0; c < chunks; ++c) {
    const int half = (int)(c & 1) * G;
    const int64_t left = jhi - (j0 + c * G);
    const int members = left < G ? (int)left : G;
    // ---- gather ----
    for (int m = wave; m < members; m += kNbThreads >> 6) {
      const int64_t hi = c_hi[half + m];
      int64_t a = c_lo[half + m];
      if (a >= hi) continue;  // dead, or no preference at all (the same on every lane)
      a = nb_wave_lower_bound(v.key, a, hi, first, lane);
      for (int64_t t = a + lane; t < hi; t += 64) {
        const int32_t it = v.key[t];
        if (it > last) break;
        int lo = 0;
        for (int up = len; lo < up;) {
          const int mid = (lo + up) >> 1;
          if (slot[mid] < it) lo = mid + 1;
          else up = mid;
        }
        if (lo < len && slot[lo] == it) {
          if constexpr (KIND == kNbGeneric) pref[m * T + lo] = v.val[t];
          atomicOr(&mask[lo], 1u << m);
        }
      }
    }
    __syncthreads();
    // ---- fold, and the next chunk's load beside it ----
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = tid + k * kNbThreads;
      if (i < len) {
        unsigned int bits = mask[i];
        if (bits) {
          mask[i] = 0u;
          do {
            const int m = __ffs(bits) - 1;  // ascending g: the neighbourhood's order
            bits &= bits - 1;
            if constexpr (KIND == kNbGeneric) sum[k].add(&c_sim[half + m], &pref[m * T + i], 1);
            else sum[k].add(&c_sim[half + m], 1);
          } while (bits);
        }
      }
    }
    if (c + 1 < chunks) load_chunk(c + 1);
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = tid + k * kNbThreads;
    if (i < len) {
      if constexpr (KIND == kNbGeneric) g.est[tile.lo + i] = sum[k].finish(g.use_capper, g.lo, g.hi);
      else g.est[tile.lo + i] = sum[k].finish();
    }
  }
}

// ---- host side ----

template <int KIND>
static int launch_nb_estimate(cms_handle* h, const NbEstArgs& g, int64_t ntiles) {
  static bool attr_set[64] = {};  // per device: the generic kind's default tile is nearly the whole 64 KiB
  if (!attr_set[h->device & 63]) {
    (void)hipFuncSetAttribute((const void*)k_nb_estimate<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              nb_lds_bytes(KIND, nb_tile_default(KIND)));
    attr_set[h->device & 63] = true;
  }
  TimedScope ts(h, "nb_estimate");
  hipLaunchKernelGGL(k_nb_estimate<KIND>, dim3((unsigned)ntiles), dim3(kNbThreads), (size_t)nb_lds_bytes(KIND, g.T),
                     h->stream, common_side(h, CMS_SIDE_OWNER), g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int nb_estimate_batch(cms_handle* h, int32_t family, int32_t measure, int32_t kind, int64_t n, const int64_t* user_rows,
                      const int64_t* nb_offsets, const int64_t* nb_rows, const int64_t* item_offsets,
                      const int64_t* item_keys, int32_t use_capper, float cap_min, float cap_max, float* out) {
  ExactModel& m = *h->exact;
  const int64_t M = nb_offsets[n], Q = item_offsets[n];
  if (Q == 0) return CMS_OK;
  const int T = nb_tile_for(kind, h->tune.nb_est_tile);
  ExactEstPlan plan;
  exact_plan_estimates(m.ids, n, item_offsets, item_keys, T, plan, [](int64_t users, auto f) {
    parallel_users(users, (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), f);
  });
  const size_t S = plan.slot_item.size();
  std::vector<float> est(S);
  if (S > 0) {
    // userSimilarity(user, neighbour) of every pair of the batch: one elementwise launch, device to device
    std::vector<int64_t> pair_user((size_t)M);
    for (int64_t u = 0; u < n; ++u)
      std::fill(pair_user.begin() + nb_offsets[u], pair_user.begin() + nb_offsets[u + 1], user_rows[u]);
    const int rc = [&]() -> int {
      int rc;
      if ((rc = upload(h, m.q1, pair_user)) || (rc = upload(h, m.q2, nb_rows, (size_t)M)) ||
          (rc = upload(h, m.e_urow, user_rows, (size_t)n)) || (rc = upload(h, m.e_nboff, nb_offsets, (size_t)n + 1)) ||
          (rc = upload(h, m.e_slot, plan.slot_item)) || (rc = upload(h, m.e_tiles, plan.tiles)))
        return rc;
      CMS_HIP(m.out.ensure(sizeof(double) * (size_t)std::max<int64_t>(M, 1)));
      CMS_HIP(m.e_est.ensure(sizeof(float) * S));
      const CommonPairArgs pg{m.q1.as<int64_t>(), m.q2.as<int64_t>(), nullptr, M, M, 0, 0, m.out.as<double>(), M};
      if ((rc = family == kFamilyCommon ? common_pairs_device(h, measure, CMS_SIDE_OWNER, pg, "nb_pairs")
                                        : set_pairs_device(h, measure, CMS_SIDE_OWNER, pg, "nb_pairs")))
        return rc;
      const NbEstArgs g{m.e_urow.as<int64_t>(),       m.e_nboff.as<int64_t>(), m.q2.as<int64_t>(),  m.out.as<double>(),
                        m.e_tiles.as<ExactEstTile>(), m.e_slot.as<int32_t>(),  m.e_est.as<float>(), (int32_t)T,
                        use_capper,                   cap_min,                 cap_max};
      if ((rc = kind == kNbGeneric ? launch_nb_estimate<kNbGeneric>(h, g, (int64_t)plan.tiles.size())
                                   : launch_nb_estimate<kNbBoolean>(h, g, (int64_t)plan.tiles.size())))
        return rc;
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
