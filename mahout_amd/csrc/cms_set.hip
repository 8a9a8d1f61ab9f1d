// cms_set.hip -- the set similarities of a handle's DataModel: co-occurrence,
// Tanimoto coefficient, city block and log-likelihood (cms_set.h states the
// semantics and what is exact).  All four are functions of how many entries two
// lists share and of the two list lengths; no preference value, unit or float
// is read.  The attached model's two CSRs serve both faces as they serve the
// co-rated similarities (CommonSide, cms_exact_model.h): of a side only off,
// key, xoff, xlist, n and num are read.  The sketch table is neither read nor
// written.
//
//   - k_set_tile<MEASURE>: one workgroup of 512 threads per (query list, tile
//     of T candidate lists).  LDS holds [T] u32 counts on the dynamic base and
//     nothing else: 64 KiB at the default T = 16384, so two workgroups share a
//     CU.  The counts are cleared with 16-byte stores; the query's entries are
//     dealt to the eight waves; a wave binary-searches the entry's cross list
//     for the tile's first candidate (not at all in the first tile) and its
//     lanes walk to the tile's last one, each lane loading one 4-byte list
//     index and issuing one returnless LDS add per posting entry.  The list
//     indices of one cross list are distinct, so the 64 adds of one wave
//     instruction never meet in a cell.  A count is at most the query's length,
//     below 2^31, and cannot wrap.  After the barrier every thread finishes its
//     candidates through set_finish<MEASURE>, the lengths taken from off, into
//     the f64 [Q][n] slab.  Every list takes this kernel: there is no
//     eligibility, no sequential route and no re-scored column;
//   - k_set_pairs<MEASURE>: one thread per pair, set_intersection_size (a
//     key-only merge join) and the same set_finish, addressed by CommonPairArgs
//     as k_common_pairs is.  It serves the elementwise and one-against-many
//     calls;
//   - the top-k is launch_top_k on the slab, self_col the query's own index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cms_exact_model.h"
#include "cms_set.h"

namespace cms {

constexpr int kSetThreads = 512;  // 8 waves; two workgroups per CU at the default tile
constexpr int kSetPairThreads = 256;
constexpr int64_t kSetChunkMax = 16384;  // queries per slab chunk (the tile grid is chunk x tiles)

// ---- the tile kernel ----
// block b: candidate tile b % ntiles of query b / ntiles (qidx: its list index)
template <int MEASURE>
__global__ __launch_bounds__(kSetThreads) void k_set_tile(CommonSide v, const int64_t* qidx, int32_t T, int64_t ntiles,
                                                          int32_t owner_side, double* slab, int64_t ld) {
  extern __shared__ __attribute__((aligned(16))) unsigned int set_cnt[];
  const int64_t q = blockIdx.x / ntiles;
  const int64_t x = qidx[q];
  const int64_t c0 = (blockIdx.x % ntiles) * T;
  const int64_t c1 = min(v.n, c0 + (int64_t)T);
  uint4* cnt4 = reinterpret_cast<uint4*>(set_cnt);  // T is a multiple of 64
  for (int i = threadIdx.x; i < T / 4; i += kSetThreads) cnt4[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const int64_t xlo = v.off[x], xhi = v.off[x + 1];
  const int lane = threadIdx.x & 63;
  for (int64_t p = xlo + (threadIdx.x >> 6); p < xhi; p += kSetThreads >> 6) {
    const int32_t key = v.key[p];
    int64_t a = v.xoff[key];
    const int64_t hi = v.xoff[key + 1];
    if (c0 > 0) {
      for (int64_t b = hi; a < b;) {  // the cross list's first entry at or past the tile's first candidate
        const int64_t mid = (a + b) >> 1;
        if (v.xlist[mid] < c0) a = mid + 1;
        else b = mid;
      }
    }
    for (int64_t t = a + lane; t < hi; t += 64) {
      const int64_t r = v.xlist[t];
      if (r >= c1) break;
      atomicAdd(&set_cnt[(int)(r - c0)], 1u);
    }
  }
  __syncthreads();
  const int64_t n1 = xhi - xlo;
  for (int i = threadIdx.x; i < (int)(c1 - c0); i += kSetThreads) {
    const int64_t c = c0 + i;
    slab[q * ld + c] = set_finish<MEASURE>((int64_t)set_cnt[i], n1, v.off[c + 1] - v.off[c], v.num, owner_side);
  }
}

// ---- the pair kernel ----
template <int MEASURE>
__global__ __launch_bounds__(kSetPairThreads) void k_set_pairs(CommonSide v, CommonPairArgs g, int32_t owner_side) {
  const int64_t total = g.cross ? g.n1 * g.n2 : g.n1;
  for (int64_t t = blockIdx.x * (int64_t)kSetPairThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kSetPairThreads) {
    int64_t x, y, o;
    if (g.cross) {
      int64_t i = t / g.n2;
      const int64_t j = t - i * g.n2;
      if (g.sel) i = g.sel[i];
      x = g.i1[i];
      y = g.i2 ? g.i2[j] : j;
      o = i * g.ld + (g.scatter ? y : j);
    } else {
      x = g.i1[t];
      y = g.i2[t];
      o = t;
    }
    const int64_t xlo = v.off[x], nx = v.off[x + 1] - xlo;
    const int64_t ylo = v.off[y], ny = v.off[y + 1] - ylo;
    const int64_t k = set_intersection_size(v.key + xlo, nx, v.key + ylo, ny);
    g.out[o] = set_finish<MEASURE>(k, nx, ny, v.num, owner_side);
  }
}

// ---- host side ----

template <int MEASURE>
static int launch_set_pairs_as(cms_handle* h, const CommonSide& v, const CommonPairArgs& g, int64_t total,
                               int32_t owner_side, const char* scope) {
  const int64_t grid = std::min<int64_t>((total + kSetPairThreads - 1) / kSetPairThreads, (int64_t)h->num_cus * 32);
  TimedScope ts(h, scope);
  hipLaunchKernelGGL(k_set_pairs<MEASURE>, dim3((unsigned)grid), dim3(kSetPairThreads), 0, h->stream, v, g, owner_side);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

template <int MEASURE>
static int launch_set_tile_as(cms_handle* h, const CommonSide& v, const int64_t* d_q, int64_t qc, int T, int64_t ntiles,
                              int32_t owner_side, double* slab) {
  static bool attr_set[64] = {};  // per device: the default tile's counts are the whole 64 KiB
  if (!attr_set[h->device & 63]) {
    (void)hipFuncSetAttribute((const void*)k_set_tile<MEASURE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)sizeof(uint32_t) * kSetTileDefault);
    attr_set[h->device & 63] = true;
  }
  TimedScope ts(h, "set_tile");
  hipLaunchKernelGGL(k_set_tile<MEASURE>, dim3((unsigned)(qc * ntiles)), dim3(kSetThreads), sizeof(uint32_t) * (size_t)T,
                     h->stream, v, d_q, (int32_t)T, ntiles, owner_side, slab, v.n);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int set_pairs_device(cms_handle* h, int32_t measure, int32_t side, const CommonPairArgs& g, const char* scope) {
  const int64_t total = g.cross ? g.n1 * g.n2 : g.n1;
  if (total <= 0) return CMS_OK;
  const CommonSide v = common_side(h, side);
  const int32_t owner_side = side == CMS_SIDE_OWNER;
  switch (measure) {
    case kSetCooccurrence: return launch_set_pairs_as<kSetCooccurrence>(h, v, g, total, owner_side, scope);
    case kSetTanimoto: return launch_set_pairs_as<kSetTanimoto>(h, v, g, total, owner_side, scope);
    case kSetCityBlock: return launch_set_pairs_as<kSetCityBlock>(h, v, g, total, owner_side, scope);
    default: return launch_set_pairs_as<kSetLogLikelihood>(h, v, g, total, owner_side, scope);
  }
}

int set_pair_call(cms_handle* h, int32_t measure, int32_t side, const int64_t* i1, int64_t n1, const int64_t* i2,
                  int64_t n2, bool cross, double* out) {
  ExactModel& m = *h->exact;
  const int64_t total = cross ? n1 * n2 : n1;
  if (total <= 0) return CMS_OK;
  int rc;
  if ((rc = upload(h, m.q1, i1, (size_t)n1)) || (rc = upload(h, m.q2, i2, (size_t)n2))) return rc;
  CMS_HIP(m.out.ensure(sizeof(double) * (size_t)total));
  const CommonPairArgs g{m.q1.as<int64_t>(), m.q2.as<int64_t>(), nullptr, n1, n2, cross ? 1 : 0, 0, m.out.as<double>(), n2};
  if ((rc = set_pairs_device(h, measure, side, g, "set_pairs"))) return rc;
  CMS_HIP(hipMemcpyAsync(out, m.out.ptr, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

int set_top_k(cms_handle* h, int32_t measure, int32_t side, const int64_t* idx, int64_t nq, int32_t k, int64_t* d_ids,
              double* d_scores, int32_t* d_counts) {
  ExactModel& m = *h->exact;
  const CommonSide v = common_side(h, side);
  const int32_t owner_side = side == CMS_SIDE_OWNER;
  const int64_t n = v.n;  // the slab's columns
  if (n == 0) return CMS_OK;
  const int T = set_tile_for(h->tune.set_tile);
  const int64_t ntiles = (n + T - 1) / T;
  const int64_t chunk = std::min<int64_t>({slab_rows_for(n), kSetChunkMax, (int64_t(1) << 31) / ntiles - 1});
  CMS_HIP(h->ws_slab.ensure(sizeof(double) * (size_t)(std::min(chunk, nq) * n)));
  CMS_HIP(m.q1.ensure(sizeof(int64_t) * (size_t)std::min(chunk, nq)));
  double* slab = h->ws_slab.as<double>();
  // the IDs of the slab's columns: the owners', or the item keys
  const int64_t* col_ids = owner_side ? h->d_owner_ids : m.d_ids.as<int64_t>();
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t qc = std::min(chunk, nq - q0);
    CMS_HIP(hipMemcpyAsync(m.q1.ptr, idx + q0, sizeof(int64_t) * (size_t)qc, hipMemcpyHostToDevice, h->stream));
    const int64_t* d_q = m.q1.as<int64_t>();
    int rc;
    switch (measure) {
      case kSetCooccurrence: rc = launch_set_tile_as<kSetCooccurrence>(h, v, d_q, qc, T, ntiles, owner_side, slab); break;
      case kSetTanimoto: rc = launch_set_tile_as<kSetTanimoto>(h, v, d_q, qc, T, ntiles, owner_side, slab); break;
      case kSetCityBlock: rc = launch_set_tile_as<kSetCityBlock>(h, v, d_q, qc, T, ntiles, owner_side, slab); break;
      default: rc = launch_set_tile_as<kSetLogLikelihood>(h, v, d_q, qc, T, ntiles, owner_side, slab); break;
    }
    if (rc) return rc;
    std::vector<TopQuery> qs((size_t)qc);
    for (int64_t q = 0; q < qc; ++q) qs[(size_t)q] = TopQuery{q, idx[q0 + q], q0 + q};
    // (launch_top_k synchronises the stream: qs may go)
    if ((rc = launch_top_k(h, slab, qs, k, nullptr, d_ids, d_scores, d_counts, n, col_ids))) return rc;
  }
  return CMS_OK;
}

}  // namespace cms
