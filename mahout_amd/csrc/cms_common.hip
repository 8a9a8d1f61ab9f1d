// cms_common.hip -- the co-rated similarities of a handle's DataModel:
// uncentered cosine, Pearson correlation and Euclidean distance over the
// entries two preference lists have in COMMON (AbstractSimilarity
// .userSimilarity / .itemSimilarity; cms_common.h states the semantics and why
// the integer route is the reference's value bit for bit).  The attached model
// (exact_attach) holds both CSRs -- owner to (item, unit, float) and item to
// (owner row, unit, float) -- so one kernel text serves both faces: a SIDE is
// the pair (own lists, cross lists), the user side passing (off, item, unit;
// ioff, irow, iunit) and the item side passing them swapped.  The sketch table
// is neither read nor written.
//
//   - k_common_tile<MEASURE>: one workgroup per (query list, tile of T
//     candidate lists).  LDS holds the candidates' cells as separate arrays
//     sized by the measure at compile time: [T] u64 per wide sum, then [T] u32
//     counts, on the 16-byte-aligned dynamic base (T is a multiple of 64, so
//     every array is aligned to its type).  Euclidean: sum of (x_u - y_u)^2 and
//     the count, 12 B per candidate; uncentered: S_xy, S_xx, S_yy and the
//     count, 28 B; Pearson adds S_x and S_y, 44 B.  The query's entries are
//     dealt to the waves; a wave binary-searches the entry's cross list for the
//     tile's first candidate and its lanes walk to the tile's last one, each
//     lane adding its terms with LDS atomics (64-bit for the sums, 32-bit for
//     the count).  A (query entry, candidate) pair is met by exactly one lane.
//     After the barrier every thread finishes its candidates through
//     common_finish<MEASURE> into the f64 [Q][n] slab;
//   - k_common_pairs<MEASURE>: one thread per pair, common_merge_join (the
//     reference's own loop over the floats) and the same common_finish.  It
//     scores every pair, eligible or not, and serves the elementwise and
//     one-against-many calls, a query that is not common-eligible (scored
//     whole; its tile blocks leave at once) and the non-eligible candidates'
//     columns of every query, re-scored after the tile pass;
//   - the top-k is launch_top_k on the slab, self_col the query's own index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cms_common.h"
#include "cms_exact_model.h"

namespace cms {

constexpr int kCommonThreads = 512;  // 8 waves; two workgroups per CU at the default tiles
constexpr int kCommonPairThreads = 256;
constexpr int64_t kCommonChunkMax = 16384;  // queries per slab chunk (the tile grid is chunk x tiles)

// ---- the tile kernel ----
// block b: candidate tile b % ntiles of query b / ntiles (qidx: its list index)
template <int MEASURE>
__global__ __launch_bounds__(kCommonThreads) void k_common_tile(CommonSide v, const int64_t* qidx, int32_t T,
                                                                int64_t ntiles, double* slab, int64_t ld) {
  extern __shared__ __attribute__((aligned(16))) unsigned char common_lds[];
  constexpr int kWide = MEASURE == kCommonEuclidean ? 1 : MEASURE == kCommonUncentered ? 3 : 5;
  static_assert(kWide * 8 + 4 == (MEASURE == kCommonEuclidean ? 12 : MEASURE == kCommonUncentered ? 28 : 44),
                "common_cell_bytes");
  // Euclidean: [0] the squared differences.  Else [0] S_xy, [1] S_xx, [2] S_yy, Pearson [3] S_x, [4] S_y.
  unsigned long long* wide = reinterpret_cast<unsigned long long*>(common_lds);
  unsigned int* cnt = reinterpret_cast<unsigned int*>(wide + (size_t)kWide * T);
  const int64_t q = blockIdx.x / ntiles;
  const int64_t x = qidx[q];
  if (v.U[x] >= kCommonEligible) return;  // scored whole by k_common_pairs
  const int64_t c0 = (blockIdx.x % ntiles) * T;
  const int64_t c1 = min(v.n, c0 + (int64_t)T);
  for (int i = threadIdx.x; i < kWide * T; i += kCommonThreads) wide[i] = 0ULL;
  for (int i = threadIdx.x; i < T; i += kCommonThreads) cnt[i] = 0u;
  __syncthreads();
  const int64_t xlo = v.off[x], xhi = v.off[x + 1];
  const int lane = threadIdx.x & 63;
  for (int64_t p = xlo + (threadIdx.x >> 6); p < xhi; p += kCommonThreads >> 6) {
    const int32_t key = v.key[p];
    const int32_t xu = v.unit[p];
    int64_t a = v.xoff[key];
    const int64_t hi = v.xoff[key + 1];
    for (int64_t b = hi; a < b;) {  // the cross list's first entry at or past the tile's first candidate
      const int64_t mid = (a + b) >> 1;
      if (v.xlist[mid] < c0) a = mid + 1;
      else b = mid;
    }
    for (int64_t t = a + lane; t < hi; t += 64) {
      const int64_t r = v.xlist[t];
      if (r >= c1) break;
      const int32_t yu = v.xunit[t];
      const int i = (int)(r - c0);
      if constexpr (MEASURE == kCommonEuclidean) {
        atomicAdd(&wide[i], (unsigned long long)common_term_d2(xu, yu));
      } else {
        atomicAdd(&wide[i], (unsigned long long)common_term_xy(xu, yu));
        atomicAdd(&wide[T + i], (unsigned long long)common_term_sq(xu));
        atomicAdd(&wide[2 * T + i], (unsigned long long)common_term_sq(yu));
        if constexpr (MEASURE == kCommonPearson) {
          atomicAdd(&wide[3 * T + i], (unsigned long long)common_term_lin(xu));
          atomicAdd(&wide[4 * T + i], (unsigned long long)common_term_lin(yu));
        }
      }
      atomicAdd(&cnt[i], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (int)(c1 - c0); i += kCommonThreads) {
    const int64_t c = c0 + i;
    CommonSums s;
    if constexpr (MEASURE == kCommonEuclidean)
      s = common_cells_to_sums(0, 0, 0, 0, 0, wide[i], cnt[i], v.shift);
    else if constexpr (MEASURE == kCommonUncentered)
      s = common_cells_to_sums(wide[i], 0, 0, wide[T + i], wide[2 * T + i], 0, cnt[i], v.shift);
    else
      s = common_cells_to_sums(wide[i], wide[3 * T + i], wide[4 * T + i], wide[T + i], wide[2 * T + i], 0, cnt[i],
                               v.shift);
    slab[q * ld + c] = common_finish<MEASURE>(s, xhi - xlo, v.off[c + 1] - v.off[c], v.num, v.weighted);
  }
}

// ---- the pair kernel ----
// (CommonPairArgs, cms_exact_model.h: elementwise, or cross with optional scatter)
template <int MEASURE>
__global__ __launch_bounds__(kCommonPairThreads) void k_common_pairs(CommonSide v, CommonPairArgs g) {
  const int64_t total = g.cross ? g.n1 * g.n2 : g.n1;
  for (int64_t t = blockIdx.x * (int64_t)kCommonPairThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kCommonPairThreads) {
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
    const CommonSums s = common_merge_join(v.key + xlo, v.val + xlo, nx, v.key + ylo, v.val + ylo, ny);
    g.out[o] = common_finish<MEASURE>(s, nx, ny, v.num, v.weighted);
  }
}

// ---- host side ----

template <int MEASURE>
static int launch_pairs_as(cms_handle* h, const CommonSide& v, const CommonPairArgs& g, int64_t total,
                           const char* scope) {
  const int64_t grid =
      std::min<int64_t>((total + kCommonPairThreads - 1) / kCommonPairThreads, (int64_t)h->num_cus * 32);
  TimedScope ts(h, scope);
  hipLaunchKernelGGL(k_common_pairs<MEASURE>, dim3((unsigned)grid), dim3(kCommonPairThreads), 0, h->stream, v, g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int common_pairs_device(cms_handle* h, int32_t measure, int32_t side, const CommonPairArgs& g, const char* scope) {
  const int64_t total = g.cross ? g.n1 * g.n2 : g.n1;
  if (total <= 0) return CMS_OK;
  const CommonSide v = common_side(h, side);
  switch (measure) {
    case kCommonUncentered: return launch_pairs_as<kCommonUncentered>(h, v, g, total, scope);
    case kCommonPearson: return launch_pairs_as<kCommonPearson>(h, v, g, total, scope);
    default: return launch_pairs_as<kCommonEuclidean>(h, v, g, total, scope);
  }
}

static int launch_pairs(cms_handle* h, int32_t measure, int32_t side, const CommonPairArgs& g) {
  return common_pairs_device(h, measure, side, g, "common_pairs");
}

template <int MEASURE>
static int launch_tile_as(cms_handle* h, const CommonSide& v, const int64_t* d_q, int64_t qc, int T, int64_t ntiles,
                          double* slab) {
  static bool attr_set[64] = {};  // per device: the default tile's cells are nearly the whole 64 KiB
  if (!attr_set[h->device & 63]) {
    (void)hipFuncSetAttribute((const void*)k_common_tile<MEASURE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              common_cell_bytes(MEASURE) * common_tile_default(MEASURE));
    attr_set[h->device & 63] = true;
  }
  TimedScope ts(h, "common_tile");
  hipLaunchKernelGGL(k_common_tile<MEASURE>, dim3((unsigned)(qc * ntiles)), dim3(kCommonThreads),
                     (size_t)common_cell_bytes(MEASURE) * (size_t)T, h->stream, v, d_q, (int32_t)T, ntiles, slab, v.n);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int common_key_index(cms_handle* h, int64_t key, int64_t* index) {
  const std::vector<int64_t>& ids = h->exact->ids;
  const auto it = std::lower_bound(ids.begin(), ids.end(), key);
  if (it == ids.end() || *it != key) return set_error(CMS_E_NO_SUCH_ID, "no such key %lld in the attached model", (long long)key);
  *index = it - ids.begin();
  return CMS_OK;
}

int common_pair_call(cms_handle* h, int32_t measure, int32_t side, const int64_t* i1, int64_t n1, const int64_t* i2,
                     int64_t n2, bool cross, double* out) {
  ExactModel& m = *h->exact;
  const int64_t total = cross ? n1 * n2 : n1;
  if (total <= 0) return CMS_OK;
  int rc;
  if ((rc = upload(h, m.q1, i1, (size_t)n1)) || (rc = upload(h, m.q2, i2, (size_t)n2))) return rc;
  CMS_HIP(m.out.ensure(sizeof(double) * (size_t)total));
  CommonPairArgs g{m.q1.as<int64_t>(), m.q2.as<int64_t>(), nullptr, n1, n2, cross ? 1 : 0, 0, m.out.as<double>(), n2};
  if ((rc = launch_pairs(h, measure, side, g))) return rc;
  CMS_HIP(hipMemcpyAsync(out, m.out.ptr, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

int common_top_k(cms_handle* h, int32_t measure, int32_t side, const int64_t* idx, int64_t nq, int32_t k,
                 int64_t* d_ids, double* d_scores, int32_t* d_counts) {
  ExactModel& m = *h->exact;
  const CommonSide v = common_side(h, side);
  const int s = side == CMS_SIDE_OWNER ? 0 : 1;
  const int64_t n = v.n;  // the slab's columns
  if (n == 0) return CMS_OK;
  const int T = common_tile_for(measure, h->tune.common_tile);
  const int64_t ntiles = (n + T - 1) / T;
  const int64_t chunk = std::min<int64_t>({slab_rows_for(n), kCommonChunkMax, (int64_t(1) << 31) / ntiles - 1});
  CMS_HIP(h->ws_slab.ensure(sizeof(double) * (size_t)(std::min(chunk, nq) * n)));
  CMS_HIP(m.q1.ensure(sizeof(int64_t) * (size_t)std::min(chunk, nq)));
  CMS_HIP(m.sel.ensure(sizeof(int64_t) * (size_t)std::min(chunk, nq)));
  double* slab = h->ws_slab.as<double>();
  // the IDs of the slab's columns: the owners', or the item keys
  const int64_t* col_ids = side == CMS_SIDE_OWNER ? h->d_owner_ids : m.d_ids.as<int64_t>();
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t qc = std::min(chunk, nq - q0);
    CMS_HIP(hipMemcpyAsync(m.q1.ptr, idx + q0, sizeof(int64_t) * (size_t)qc, hipMemcpyHostToDevice, h->stream));
    std::vector<int64_t> sel;  // the chunk's queries that are not common-eligible
    for (int64_t q = 0; q < qc; ++q)
      if (m.h_cseq[s][(size_t)idx[q0 + q]]) sel.push_back(q);
    int rc = CMS_OK;
    if ((int64_t)sel.size() < qc) {
      switch (measure) {
        case kCommonUncentered:
          rc = launch_tile_as<kCommonUncentered>(h, v, m.q1.as<int64_t>(), qc, T, ntiles, slab);
          break;
        case kCommonPearson:
          rc = launch_tile_as<kCommonPearson>(h, v, m.q1.as<int64_t>(), qc, T, ntiles, slab);
          break;
        default:
          rc = launch_tile_as<kCommonEuclidean>(h, v, m.q1.as<int64_t>(), qc, T, ntiles, slab);
          break;
      }
      if (rc) return rc;
    }
    if (!sel.empty()) {  // whole queries of the sequential route
      CMS_HIP(hipMemcpyAsync(m.sel.ptr, sel.data(), sizeof(int64_t) * sel.size(), hipMemcpyHostToDevice, h->stream));
      CommonPairArgs g{m.q1.as<int64_t>(), nullptr, m.sel.as<int64_t>(), (int64_t)sel.size(), n, 1, 0, slab, n};
      if ((rc = launch_pairs(h, measure, side, g))) return rc;
    }
    if (m.n_cseq[s] > 0 && (int64_t)sel.size() < qc) {  // the non-eligible candidates' columns of every query
      CommonPairArgs g{m.q1.as<int64_t>(), m.cseq[s].as<int64_t>(), nullptr, qc, m.n_cseq[s], 1, 1, slab, n};
      if ((rc = launch_pairs(h, measure, side, g))) return rc;
    }
    std::vector<TopQuery> qs((size_t)qc);
    for (int64_t q = 0; q < qc; ++q) qs[(size_t)q] = TopQuery{q, idx[q0 + q], q0 + q};
    // (launch_top_k synchronises the stream: sel and qs may go)
    if ((rc = launch_top_k(h, slab, qs, k, nullptr, d_ids, d_scores, d_counts, n, col_ids))) return rc;
  }
  return CMS_OK;
}

}  // namespace cms
