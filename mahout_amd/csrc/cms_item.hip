// cms_item.hip -- blocks of the sketch-cosine matrix and the item-based
// estimate on gfx950 (fixed shapes, u32 counters, rows in any stored form).
//
// GenericItemBasedRecommender.doEstimatePreference (T/impl/recommender/
// GenericItemBasedRecommender.java:231-259) needs, per candidate item, the
// similarities of that item with the user's P preferred items, then a
// weighted sum in preference order.  k_pair_cosine (cms_query.hip) gives one
// workgroup to every pair and reads both rows from memory each time; here one
// workgroup takes one LEFT owner and a list of RIGHT owners and, per sketch
// row,
//   1. expands the left owner's row ONCE into an LDS image of u32 cells (a
//      hot row holds full u32 counters and a list may put 255 entries -- or,
//      from a loader, more -- in one bucket: one cell width serves every
//      stored form),
//   2. lets each wave take right owners in turn and form the integer dot
//      against the image: a list row sums the image at its entries, a dense
//      row streams its stored bytes four counters per lane (conflict-free
//      ds_read_b128 of the image),
//   3. turns the dot into the row's quotient exactly as k_pair_cosine does:
//      (double) u64 dot when both norms are below 2^53, den = nsqrt[a] *
//      nsqrt[b], the quotient into java_min only when den != 0; norms at or
//      above 2^53 take seq_row_sums, the reference's own loop.
// Right owners come in tiles of kItemTile, so any number of them works.
// Epilogues: BLOCK writes out[left][right]; ESTIMATE reduces the tile's
// similarities with the user's preference values in preference order
// (ItemEstimate, cms_ref.h) on one lane and writes one float per left owner.
//
// Widths past kItemMaxWidth (the image would pass the 32 KiB this kernel
// budgets, which keeps four workgroups on a CU) go through k_pair_cosine:
// pairs_route below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "cms_device.h"
#include "cms_internal.h"
#include "cms_pair.h"
#include "cms_ref.h"
#include "cms_rows.h"

namespace cms {

constexpr int kItemThreads = 256;    // four waves: the right owners of a tile are dealt round-robin to them
constexpr int kItemTile = 128;       // right owners per tile (their running minima: 1 KiB of LDS)
constexpr int kItemMaxWidth = 8192;  // widest staged sketch row: 32 KiB of u32 cells
constexpr int64_t kItemRoutePairs = int64_t(1) << 22;  // pairs per k_pair_cosine launch of the wide route

int item_max_staged_width() { return kItemMaxWidth; }
int item_right_tile() { return kItemTile; }

// counters [j, j + 4) (j % 4 == 0, w % 4 == 0) of a dense row, by the form's vector load
__device__ __forceinline__ uint4 dense4(const rows::RowSrc& s, int64_t j) {
  const uint8_t* p = s.p;
  if (s.f >= 0) return *reinterpret_cast<const uint4*>(p + 4 * j);
  if (s.f == kFormU16) {
    const ushort4 v = *reinterpret_cast<const ushort4*>(p + 2 * j);
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  if (s.f == kFormU8) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p + j);
    return make_uint4(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u, v >> 24);
  }
  if (s.f == kFormU4) {
    const uint32_t v = *reinterpret_cast<const uint16_t*>(p + (j >> 1));
    return make_uint4(v & 15u, (v >> 4) & 15u, (v >> 8) & 15u, v >> 12);
  }
  if (s.f == kFormU2) {
    const uint32_t v = p[j >> 2];
    return make_uint4(v & 3u, (v >> 2) & 3u, (v >> 4) & 3u, v >> 6);
  }
  const uint32_t v = (uint32_t)p[j >> 3] >> (j & 4);  // kFormU1
  return make_uint4(v & 1u, (v >> 1) & 1u, (v >> 2) & 1u, (v >> 3) & 1u);
}

// counter j of a dense row (w % 4 != 0: no aligned vector)
__device__ __forceinline__ uint32_t dense1(const rows::RowSrc& s, int64_t j) {
  const uint8_t* p = s.p;
  if (s.f >= 0) return reinterpret_cast<const uint32_t*>(p)[j];
  if (s.f == kFormU16) return reinterpret_cast<const uint16_t*>(p)[j];
  if (s.f == kFormU8) return p[j];
  if (s.f == kFormU4) return (uint32_t)(p[j >> 1] >> ((j & 1) << 2)) & 15u;
  if (s.f == kFormU2) return (uint32_t)(p[j >> 2] >> ((j & 3) << 1)) & 3u;
  return (uint32_t)(p[j >> 3] >> (j & 7)) & 1u;
}

struct ItemArgs {
  const int64_t* left;   // [nl] owner rows
  const int64_t* right;  // BLOCK: [nr] owner rows; ESTIMATE: every user's preferred rows, concatenated
  int64_t nr;            // BLOCK: right owners (ESTIMATE: from pref_off)
  // ESTIMATE: left owner i is a candidate of user left_user[i], whose
  // preferences are right / pref_vals [pref_off[u], pref_off[u + 1])
  const int32_t* left_user;
  const int64_t* pref_off;
  const float* pref_vals;
  int use_capper;
  float lo, hi;
  double* out_sims;  // BLOCK: [nl][nr]
  float* out_est;    // ESTIMATE: [nl]
};

// grid: x = left owners; y = the tiles' stride (BLOCK; 1 for ESTIMATE, whose
// reduction walks every tile in order).  Dynamic LDS: the image, 4 w bytes.
template <bool EST>
__global__ __launch_bounds__(kItemThreads) void k_item_block(TableView tv, const uint64_t* norm, const double* nsqrt,
                                                             HashParams hp, int64_t nrows, int weighted, ItemArgs g) {
  extern __shared__ uint32_t img[];     // [w]: the left owner's sketch row
  __shared__ double s_sim[kItemTile];   // per right owner: the running Math.min, then the similarity
  __shared__ float s_pref[EST ? kItemTile : 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int w = (int)hp.width, depth = hp.depth;
  const int64_t li = blockIdx.x;
  const int64_t a = g.left[li];
  int64_t r0 = 0, nr = g.nr;
  if (EST) {
    const int32_t u = g.left_user[li];
    r0 = g.pref_off[u];
    nr = g.pref_off[u + 1] - r0;
  }
  const int64_t* rr = g.right + r0;
  const bool a_ok = a >= 0 && a < nrows;  // (an owner row outside the table: NaN, as k_pair_cosine answers)
  rows::RowSrc sa{nullptr, 0};
  bool a_list = false;
  uint32_t am = 0;
  if (a_ok) {
    sa = rows::row_src(tv, a);
    a_list = sa.f == kFormList;
    if (a_list) am = tv.list_m(a);
  }
  ItemEstimate est;  // (lane 0 of wave 0)
  const int64_t ntiles = (nr + kItemTile - 1) / kItemTile;
  for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {
    const int64_t j0 = t * kItemTile;
    const int cnt = (int)(nr - j0 < kItemTile ? nr - j0 : kItemTile);
    for (int i = tid; i < cnt; i += kItemThreads) {
      s_sim[i] = DBL_MAX;
      if (EST) s_pref[i] = g.pref_vals[r0 + j0 + i];
    }
    for (int d = 0; a_ok && d < depth; ++d) {
      const int64_t c0 = (int64_t)d * w;
      const uint64_t Na = norm[a * depth + d];
      const double sqa = nsqrt[a * depth + d];
      const bool a_exact = Na < (1ULL << 53);
      __syncthreads();  // the last row's readers are done with the image (and s_sim is initialised)
      if (Na != 0 && a_exact) {  // (uniform) a row of zeros qualifies with no one; an inexact one is read in place
        if (a_list) {
          for (int j = tid; j < w; j += kItemThreads) img[j] = 0u;
          __syncthreads();
          const uint16_t* e = tv.list_row(a, d, am);
          for (uint32_t q = tid; q < am; q += kItemThreads) atomicAdd(&img[e[q]], 1u);
        } else if ((w & 3) == 0) {
          for (int j = tid; j < (w >> 2); j += kItemThreads) reinterpret_cast<uint4*>(img)[j] = dense4(sa, c0 + 4 * j);
        } else {
          for (int j = tid; j < w; j += kItemThreads) img[j] = dense1(sa, c0 + j);
        }
      }
      __syncthreads();
      if (Na == 0) continue;
      for (int i = wv; i < cnt; i += kItemThreads / 64) {
        const int64_t b = rr[j0 + i];
        if (b < 0 || b >= nrows) continue;
        const uint64_t Nb = norm[b * depth + d];
        double valueAB, den;
        if (a_exact && Nb < (1ULL << 53)) {
          den = __dmul_rn(sqa, nsqrt[b * depth + d]);
          if (den == 0.0) continue;  // the quotient enters Math.min only when den != 0
          const rows::RowSrc sb = rows::row_src(tv, b);
          uint64_t dot = 0;
          if (sb.f == kFormList) {
            const uint32_t bm = tv.list_m(b);
            const uint16_t* e = tv.list_row(b, d, bm);
            for (uint32_t q = lane; q < bm; q += 64) dot += img[e[q]];
          } else if (sb.p == nullptr) {
            // (the shared zero row: its norm is 0 and den was 0 above)
          } else if ((w & 3) == 0) {
            for (int j = lane; j < (w >> 2); j += 64) {
              const uint4 x = dense4(sb, c0 + 4 * j), y = reinterpret_cast<const uint4*>(img)[j];
              dot += (uint64_t)x.x * y.x + (uint64_t)x.y * y.y + (uint64_t)x.z * y.z + (uint64_t)x.w * y.w;
            }
          } else {
            for (int j = lane; j < w; j += 64) dot += (uint64_t)dense1(sb, c0 + j) * img[j];
          }
          dot = wave_sum_u64(dot);
          valueAB = (double)dot;
        } else {
          double A, B;
          seq_row_sums(tv, a, b, c0, w, A, B, valueAB);  // every lane (uniform result)
          den = __dmul_rn(__dsqrt_rn(A), __dsqrt_rn(B));
          if (den == 0.0) continue;
        }
        if (lane == 0) s_sim[i] = java_min(s_sim[i], __ddiv_rn(valueAB, den));  // (this wave owns s_sim[i])
      }
    }
    __syncthreads();
    if (EST) {
      for (int i = tid; i < cnt; i += kItemThreads) s_sim[i] = cosine_finish(s_sim[i], weighted);
      __syncthreads();
      if (tid == 0) est.add(s_sim, s_pref, cnt);  // preference order: the tiles ascend, the tile in order
    } else {
      for (int i = tid; i < cnt; i += kItemThreads) g.out_sims[li * nr + j0 + i] = cosine_finish(s_sim[i], weighted);
    }
    __syncthreads();  // s_sim / s_pref are read before the next tile overwrites them
  }
  if (EST && tid == 0) g.out_est[li] = est.finish(g.use_capper, g.lo, g.hi);
}

// ---- the wide route: widths whose image is past the LDS budget ----

// pair i of lc x nr: (left[i / nr], right[i % nr])
__global__ void k_item_pairs(const int64_t* left, const int64_t* right, int64_t nr, int64_t m, int64_t* qrows,
                             int64_t* rows) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    qrows[i] = left[i / nr];
    rows[i] = right[i % nr];
  }
}

// item_estimate_one per left owner over its row of similarities [lc][nr]
__global__ void k_item_reduce(const double* sims, const float* prefs, int64_t nr, int64_t lc, int use_capper, float lo,
                              float hi, float* out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < lc; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = item_estimate_one(sims + i * nr, prefs, nr, use_capper, lo, hi);
}

// userSimilarity(left[i], right[j]) for i < lc, j < nr into d_sims[i * nr + j]
// through k_pair_cosine (lc * nr <= kItemRoutePairs)
static int pairs_route(cms_handle* h, const int64_t* d_left, int64_t lc, const int64_t* d_right, int64_t nr,
                       DevBuf& pairs, double* d_sims, hipStream_t st) {
  const int64_t m = lc * nr;
  if (m <= 0) return CMS_OK;
  CMS_HIP(pairs.ensure(sizeof(int64_t) * 2 * (size_t)m));
  int64_t* q = pairs.as<int64_t>();
  const unsigned grid = (unsigned)std::min<int64_t>((m + 255) / 256, 4096);
  hipLaunchKernelGGL(k_item_pairs, dim3(grid), dim3(256), 0, st, d_left, d_right, nr, m, q, q + m);
  CMS_HIP(hipGetLastError());
  return pair_cosines_many(h, q, q + m, m, d_sims, st);
}

static size_t image_bytes(const cms_handle* h) { return ((size_t)h->p.width * 4 + 15) / 16 * 16; }

int item_block(cms_handle* h, QueryCtx& c, hipStream_t st, bool timed, const int64_t* left, int64_t nl,
               const int64_t* right, int64_t nr, double* out) {
  if (nl <= 0 || nr <= 0) return CMS_OK;
  if (nl >= (int64_t(1) << 31)) return set_error(CMS_E_PARAM, "too many left owners in one block");
  // c.q: left rows then right rows; c.o: the block
  CMS_HIP(c.q.ensure(sizeof(int64_t) * (size_t)(nl + nr)));
  CMS_HIP(c.o.ensure(sizeof(double) * (size_t)nl * (size_t)nr));
  int64_t* d_left = c.q.as<int64_t>();
  int64_t* d_right = d_left + nl;
  CMS_HIP(hipMemcpyAsync(d_left, left, sizeof(int64_t) * (size_t)nl, hipMemcpyHostToDevice, st));
  CMS_HIP(hipMemcpyAsync(d_right, right, sizeof(int64_t) * (size_t)nr, hipMemcpyHostToDevice, st));
  {
    TimedScope ts(h, "item_block", timed);
    if (h->p.width <= kItemMaxWidth) {
      ItemArgs g{};
      g.left = d_left;
      g.right = d_right;
      g.nr = nr;
      g.out_sims = c.o.as<double>();
      const int64_t ntiles = (nr + kItemTile - 1) / kItemTile;
      hipLaunchKernelGGL(k_item_block<false>, dim3((unsigned)nl, (unsigned)std::min<int64_t>(ntiles, 65535)),
                         dim3(kItemThreads), image_bytes(h), st, h->tview(), h->d_norm, h->d_norm_sqrt, h->hp, h->n,
                         (int)h->p.weighting, g);
      CMS_HIP(hipGetLastError());
    } else {
      const int64_t step = std::max<int64_t>(1, kItemRoutePairs / nr);
      for (int64_t l0 = 0; l0 < nl; l0 += step)
        if (int rc = pairs_route(h, d_left + l0, std::min(step, nl - l0), d_right, nr, c.r, c.o.as<double>() + l0 * nr, st))
          return rc;
    }
  }
  CMS_HIP(hipMemcpyAsync(out, c.o.ptr, sizeof(double) * (size_t)nl * (size_t)nr, hipMemcpyDeviceToHost, st));
  CMS_HIP(hipStreamSynchronize(st));
  return CMS_OK;
}

int item_estimates(cms_handle* h, QueryCtx& c, hipStream_t st, bool timed, int64_t n, const int64_t* pref_off,
                   const int64_t* pref_rows, const float* pref_vals, const int64_t* cand_off, const int64_t* cand,
                   int use_capper, float lo, float hi, float* out) {
  const int64_t M = pref_off[n], Q = cand_off[n];
  if (Q <= 0) return CMS_OK;
  if (Q >= (int64_t(1) << 31)) return set_error(CMS_E_PARAM, "too many candidate items in one batch");
  // c.q: candidate rows; c.z: candidate -> user; c.y: preference offsets;
  // c.r: preferred rows; c.x: preference values; c.o: estimates
  std::vector<int32_t> cand_user((size_t)Q);
  for (int64_t u = 0; u < n; ++u)
    for (int64_t i = cand_off[u]; i < cand_off[u + 1]; ++i) cand_user[(size_t)i] = (int32_t)u;
  CMS_HIP(c.q.ensure(sizeof(int64_t) * (size_t)Q));
  CMS_HIP(c.z.ensure(sizeof(int32_t) * (size_t)Q));
  CMS_HIP(c.y.ensure(sizeof(int64_t) * (size_t)(n + 1)));
  CMS_HIP(c.r.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(M, 1)));
  CMS_HIP(c.x.ensure(sizeof(float) * (size_t)std::max<int64_t>(M, 1)));
  CMS_HIP(c.o.ensure(sizeof(float) * (size_t)Q));
  CMS_HIP(hipMemcpyAsync(c.q.ptr, cand, sizeof(int64_t) * (size_t)Q, hipMemcpyHostToDevice, st));
  CMS_HIP(hipMemcpyAsync(c.z.ptr, cand_user.data(), sizeof(int32_t) * (size_t)Q, hipMemcpyHostToDevice, st));
  CMS_HIP(hipMemcpyAsync(c.y.ptr, pref_off, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
  if (M > 0) {
    CMS_HIP(hipMemcpyAsync(c.r.ptr, pref_rows, sizeof(int64_t) * (size_t)M, hipMemcpyHostToDevice, st));
    CMS_HIP(hipMemcpyAsync(c.x.ptr, pref_vals, sizeof(float) * (size_t)M, hipMemcpyHostToDevice, st));
  }
  DevBuf pairs, sims;  // (the wide route's scratch, call-local)
  {
    TimedScope ts(h, "item_estimate", timed);
    if (h->p.width <= kItemMaxWidth) {
      ItemArgs g{};
      g.left = c.q.as<int64_t>();
      g.right = c.r.as<int64_t>();
      g.left_user = c.z.as<int32_t>();
      g.pref_off = c.y.as<int64_t>();
      g.pref_vals = c.x.as<float>();
      g.use_capper = use_capper;
      g.lo = lo;
      g.hi = hi;
      g.out_est = c.o.as<float>();
      hipLaunchKernelGGL(k_item_block<true>, dim3((unsigned)Q, 1), dim3(kItemThreads), image_bytes(h), st, h->tview(),
                         h->d_norm, h->d_norm_sqrt, h->hp, h->n, (int)h->p.weighting, g);
      CMS_HIP(hipGetLastError());
    } else {
      // per user: chunks of candidates x all preferences through k_pair_cosine, then the reduction
      for (int64_t u = 0; u < n; ++u) {
        const int64_t P = pref_off[u + 1] - pref_off[u], C = cand_off[u + 1] - cand_off[u];
        if (C == 0) continue;
        const int64_t step = std::max<int64_t>(1, kItemRoutePairs / std::max<int64_t>(P, 1));
        for (int64_t c0 = 0; c0 < C; c0 += step) {
          const int64_t lc = std::min(step, C - c0);
          CMS_HIP(sims.ensure(sizeof(double) * (size_t)std::max<int64_t>(lc * P, 1)));
          const int64_t* d_left = c.q.as<int64_t>() + cand_off[u] + c0;
          if (int rc = pairs_route(h, d_left, lc, c.r.as<int64_t>() + pref_off[u], P, pairs, sims.as<double>(), st))
            return rc;
          const unsigned grid = (unsigned)std::min<int64_t>((lc + 255) / 256, 4096);
          hipLaunchKernelGGL(k_item_reduce, dim3(grid), dim3(256), 0, st, sims.as<double>(),
                             c.x.as<float>() + pref_off[u], P, lc, use_capper, lo, hi,
                             c.o.as<float>() + cand_off[u] + c0);
          CMS_HIP(hipGetLastError());
        }
      }
    }
  }
  CMS_HIP(hipMemcpyAsync(out, c.o.ptr, sizeof(float) * (size_t)Q, hipMemcpyDeviceToHost, st));
  CMS_HIP(hipStreamSynchronize(st));
  return CMS_OK;
}

}  // namespace cms
