// cms_exact.hip -- the exact CosineSimilarity of a handle's DataModel.
//
// CosineSimilarity.userSimilarity (T/impl/similarity/CosineSimilarity.java:44-103)
// is the full-norm cosine over the raw preferences: the quantity CosineCM's
// sketch cosine approximates.  A handle may carry its owners' DataModel
// (exact_attach) beside the sketch table, which this file never reads or
// writes:
//
//   - the host validates the CSR, picks the shift s (exact_shift_for), forms
//     every owner's units, sum of squared units U, sequential sumX2 and its
//     square root, and the item-side index -- item to (owner row ascending,
//     unit), GenericDataModel.transposed() with the keys remapped to dense item
//     indices; the float values stay on the owner side, where the sequential
//     route reads them;
//   - k_exact_tile: one workgroup per (query row, tile of T candidate rows).
//     The tile's dots are i64 cells in LDS; the query's preferences are dealt
//     to the waves, a wave walks one item's posting list from the tile's first
//     row (binary search) to its last, its lanes adding x_unit * y_unit into
//     the candidates' cells with LDS atomics.  After a barrier every thread
//     finishes its candidates through exact_finish into the [Q][n] slab;
//   - k_exact_pairs: one thread per pair, the merge join of the two ascending
//     lists in the reference's order (exact_merge_join), the same exact_finish.
//     It serves the explicit-pair calls, a query row that is not
//     integer-eligible (scored whole), and the non-eligible candidate columns
//     of every query, re-scored after the tile pass;
//   - the top-k is launch_top_k on the slab, as the sketch paths call it.
//
// Why the tile's value is the reference's, bit for bit: for two owners with
// U < 2^53 every partial sum the reference forms is an integer multiple of
// 2^-2s of magnitude below 2^53, so no addition rounds and
// ldexp((double) dot, -2s) is sumXY in any order; the rest is correctly rounded
// operations on the same operands.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "cms_exact.h"
#include "cms_internal.h"

namespace cms {

constexpr int kExactThreads = 512;      // 8 waves; two workgroups per CU at the default tile
constexpr int kExactPairThreads = 256;
constexpr int64_t kExactChunkMax = 16384;  // query rows per slab chunk (the tile grid is chunk x tiles)

struct ExactModel {
  int64_t n = 0, npairs = 0, nitems = 0;
  int shift = kExactNoShift;
  std::vector<uint8_t> h_seq;  // [n] 1: not integer-eligible
  int64_t n_seq = 0;
  DevBuf off, item, val, unit;  // owner side: [n + 1] i64, [np] dense item (i32), float, unit (i32)
  DevBuf ioff, irow, iunit;     // item side: [nitems + 1] i64, [np] owner row ascending (i32), unit (i32)
  DevBuf U, root;               // [n] saturating sum of squared units (u64), Math.sqrt(sumX2) (f64)
  DevBuf seq_rows;              // [n_seq] the non-eligible rows (i64)
  DevBuf q1, q2, sel, out;      // a call's rows, selected queries and results
};

struct ExactView {
  const int64_t* off;
  const int32_t* item;
  const float* val;
  const int32_t* unit;
  const int64_t* ioff;
  const int32_t* irow;
  const int32_t* iunit;
  const uint64_t* U;
  const double* root;
  int64_t n;
  int32_t shift, weighted;
};

static ExactView exact_view(const cms_handle* h) {
  const ExactModel& m = *h->exact;
  return ExactView{m.off.as<int64_t>(),   m.item.as<int32_t>(),  m.val.as<float>(), m.unit.as<int32_t>(),
                   m.ioff.as<int64_t>(),  m.irow.as<int32_t>(),  m.iunit.as<int32_t>(), m.U.as<uint64_t>(),
                   m.root.as<double>(),   m.n, m.shift, (int32_t)h->p.weighting};
}

// ---- the tile kernel ----
// block b: candidate tile b % ntiles of query b / ntiles (qrows: its owner row)
__global__ __launch_bounds__(kExactThreads) void k_exact_tile(ExactView v, const int64_t* qrows, int32_t T,
                                                              int64_t ntiles, double* slab, int64_t ld) {
  extern __shared__ unsigned long long exact_cells[];
  const int64_t q = blockIdx.x / ntiles;
  const int64_t x = qrows[q];
  if (v.U[x] >= kExactEligible) return;  // scored whole by k_exact_pairs
  const int64_t c0 = (blockIdx.x % ntiles) * T;
  const int64_t c1 = min(v.n, c0 + (int64_t)T);
  for (int i = threadIdx.x; i < T; i += kExactThreads) exact_cells[i] = 0ULL;
  __syncthreads();
  const int64_t xlo = v.off[x], xhi = v.off[x + 1];
  const int lane = threadIdx.x & 63;
  for (int64_t p = xlo + (threadIdx.x >> 6); p < xhi; p += kExactThreads >> 6) {
    const int32_t it = v.item[p];
    const int64_t xu = v.unit[p];
    int64_t a = v.ioff[it];
    const int64_t hi = v.ioff[it + 1];
    for (int64_t b = hi; a < b;) {  // the posting list's first row at or past the tile's
      const int64_t mid = (a + b) >> 1;
      if (v.irow[mid] < c0) a = mid + 1;
      else b = mid;
    }
    for (int64_t t = a + lane; t < hi; t += 64) {
      const int64_t r = v.irow[t];
      if (r >= c1) break;
      atomicAdd(&exact_cells[r - c0], (unsigned long long)(xu * (int64_t)v.iunit[t]));
    }
  }
  __syncthreads();
  const double rootX = v.root[x];
  for (int64_t i = threadIdx.x; i < c1 - c0; i += kExactThreads) {
    const int64_t c = c0 + i;
    const double sumXY = exact_dot_to_sum((int64_t)exact_cells[i], v.shift);
    slab[q * ld + c] = exact_finish(sumXY, rootX, v.root[c], xhi - xlo, v.off[c + 1] - v.off[c], v.weighted);
  }
}

// ---- the pair kernel ----
// elementwise: out[t] = userSimilarity(r1[t], r2[t]), t < n1.
// cross: query i (sel[i'] when sel is given, i' < n1) against column j < n2
// (owner row r2[j]; r2 null: row j) into out[i * ld + j], or, scattered, into
// out[i * ld + r2[j]] (the slab's column of that owner).
struct ExactPairArgs {
  const int64_t* r1;
  const int64_t* r2;
  const int64_t* sel;
  int64_t n1, n2;
  int32_t cross, scatter;
  double* out;
  int64_t ld;
};

__global__ __launch_bounds__(kExactPairThreads) void k_exact_pairs(ExactView v, ExactPairArgs g) {
  const int64_t total = g.cross ? g.n1 * g.n2 : g.n1;
  for (int64_t t = blockIdx.x * (int64_t)kExactPairThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kExactPairThreads) {
    int64_t x, y, o;
    if (g.cross) {
      int64_t i = t / g.n2;
      const int64_t j = t - i * g.n2;
      if (g.sel) i = g.sel[i];
      x = g.r1[i];
      y = g.r2 ? g.r2[j] : j;
      o = i * g.ld + (g.scatter ? y : j);
    } else {
      x = g.r1[t];
      y = g.r2[t];
      o = t;
    }
    const int64_t xlo = v.off[x], nx = v.off[x + 1] - xlo;
    const int64_t ylo = v.off[y], ny = v.off[y + 1] - ylo;
    const double sumXY = exact_merge_join(v.item + xlo, v.val + xlo, nx, v.item + ylo, v.val + ylo, ny);
    g.out[o] = exact_finish(sumXY, v.root[x], v.root[y], nx, ny, v.weighted);
  }
}

static int launch_pairs(cms_handle* h, const ExactPairArgs& g) {
  const int64_t total = g.cross ? g.n1 * g.n2 : g.n1;
  if (total <= 0) return CMS_OK;
  const int64_t grid = std::min<int64_t>((total + kExactPairThreads - 1) / kExactPairThreads, (int64_t)h->num_cus * 32);
  TimedScope ts(h, "exact_pairs");
  hipLaunchKernelGGL(k_exact_pairs, dim3((unsigned)grid), dim3(kExactPairThreads), 0, h->stream, exact_view(h), g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

// ---- host side ----

void exact_release(cms_handle* h) {
  delete h->exact;
  h->exact = nullptr;
}

static int exact_tile_rows(const cms_handle* h) { return exact_tile_for(h->tune.exact_tile); }

// (the host array must stay alive until the stream is synchronised)
template <class T>
static int upload(cms_handle* h, DevBuf& b, const T* v, size_t count) {
  CMS_HIP(b.ensure(sizeof(T) * count));
  if (count > 0) CMS_HIP(hipMemcpyAsync(b.ptr, v, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
  return CMS_OK;
}
template <class T>
static int upload(cms_handle* h, DevBuf& b, const std::vector<T>& v) {
  return upload(h, b, v.data(), v.size());
}

int exact_attach(cms_handle* h, const int64_t* off, const int64_t* keys, const float* vals) {
  const int64_t n = h->n;
  if (!exact_valid_csr(n, off, keys))
    return set_error(CMS_E_PARAM,
                     "cms_exact_attach_csr: offsets must start at 0 and never decrease, and a row's keys must be "
                     "strictly ascending");
  const int64_t np = off[n];
  std::unique_ptr<ExactModel> m(new (std::nothrow) ExactModel());
  if (!m) return set_error(CMS_E_OOM, "host allocation failed");
  m->n = n;
  m->npairs = np;
  m->shift = exact_shift_for(vals, np);
  // getItemIDs(): the keys in ascending order are the dense item indices, so a
  // row's items ascend as its keys do
  std::vector<int64_t> ids(keys, keys + np);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  if (ids.size() > (size_t)INT32_MAX) return set_error(CMS_E_PARAM, "cms_exact_attach_csr: more than 2^31 - 1 items");
  m->nitems = (int64_t)ids.size();
  std::vector<int32_t> item((size_t)np), unit((size_t)np, 0);
  std::vector<int64_t> ioff((size_t)m->nitems + 1, 0);
  for (int64_t t = 0; t < np; ++t) {
    item[(size_t)t] = (int32_t)(std::lower_bound(ids.begin(), ids.end(), keys[t]) - ids.begin());
    ++ioff[(size_t)item[(size_t)t] + 1];
    if (m->shift != kExactNoShift) unit[(size_t)t] = exact_unit(vals[t], m->shift);
  }
  for (int64_t i = 0; i < m->nitems; ++i) ioff[(size_t)i + 1] += ioff[(size_t)i];
  std::vector<uint64_t> U((size_t)n);
  std::vector<double> root((size_t)n);
  std::vector<int64_t> seq_rows;
  m->h_seq.assign((size_t)n, 0);
  std::vector<int32_t> irow((size_t)np), iunit((size_t)np);
  {
    std::vector<int64_t> fill(ioff.begin(), ioff.end() - 1);
    for (int64_t r = 0; r < n; ++r) {  // rows in ascending order: every posting list ascends
      double sum2;
      exact_owner_sums(vals, off[r], off[r + 1], m->shift, U[(size_t)r], sum2, root[(size_t)r]);
      if (U[(size_t)r] >= kExactEligible) {
        m->h_seq[(size_t)r] = 1;
        seq_rows.push_back(r);
      }
      for (int64_t t = off[r]; t < off[r + 1]; ++t) {
        const int64_t at = fill[(size_t)item[(size_t)t]]++;
        irow[(size_t)at] = (int32_t)r;
        iunit[(size_t)at] = unit[(size_t)t];
      }
    }
  }
  m->n_seq = (int64_t)seq_rows.size();
  int rc;
  {
    TimedScope ts(h, "exact_attach");
    (void)((rc = upload(h, m->off, off, (size_t)n + 1)) || (rc = upload(h, m->val, vals, (size_t)np)) ||
           (rc = upload(h, m->item, item)) || (rc = upload(h, m->unit, unit)) || (rc = upload(h, m->ioff, ioff)) ||
           (rc = upload(h, m->irow, irow)) || (rc = upload(h, m->iunit, iunit)) || (rc = upload(h, m->U, U)) ||
           (rc = upload(h, m->root, root)) || (rc = upload(h, m->seq_rows, seq_rows)));
  }
  const hipError_t synced = hipStreamSynchronize(h->stream);  // whatever was queued is done with the host arrays
  if (rc) return rc;
  CMS_HIP(synced);
  exact_release(h);
  h->exact = m.release();
  return CMS_OK;
}

int exact_pair_call(cms_handle* h, const int64_t* r1, int64_t n1, const int64_t* r2, int64_t n2, bool cross,
                    double* out) {
  ExactModel& m = *h->exact;
  const int64_t total = cross ? n1 * n2 : n1;
  if (total <= 0) return CMS_OK;
  CMS_HIP(m.q1.ensure(sizeof(int64_t) * (size_t)n1));
  CMS_HIP(m.q2.ensure(sizeof(int64_t) * (size_t)n2));
  CMS_HIP(m.out.ensure(sizeof(double) * (size_t)total));
  CMS_HIP(hipMemcpyAsync(m.q1.ptr, r1, sizeof(int64_t) * (size_t)n1, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(m.q2.ptr, r2, sizeof(int64_t) * (size_t)n2, hipMemcpyHostToDevice, h->stream));
  ExactPairArgs g{m.q1.as<int64_t>(), m.q2.as<int64_t>(), nullptr, n1, n2, cross ? 1 : 0, 0, m.out.as<double>(), n2};
  if (int rc = launch_pairs(h, g)) return rc;
  CMS_HIP(hipMemcpyAsync(out, m.out.ptr, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

int exact_top_k_rows(cms_handle* h, const int64_t* rows, int64_t nq, int32_t k, int64_t* d_ids, double* d_scores,
                     int32_t* d_counts) {
  ExactModel& m = *h->exact;
  const int64_t n = h->n;
  const int T = exact_tile_rows(h);
  const int64_t ntiles = (n + T - 1) / T;
  const int64_t chunk = std::min<int64_t>({slab_rows_for(n), kExactChunkMax, (int64_t(1) << 31) / ntiles - 1});
  CMS_HIP(h->ws_slab.ensure(sizeof(double) * (size_t)(std::min(chunk, nq) * n)));
  CMS_HIP(m.q1.ensure(sizeof(int64_t) * (size_t)std::min(chunk, nq)));
  CMS_HIP(m.sel.ensure(sizeof(int64_t) * (size_t)std::min(chunk, nq)));
  double* slab = h->ws_slab.as<double>();
  static bool attr_set[64] = {};  // per device: the default tile's cells are the whole 64 KiB
  if (!attr_set[h->device & 63]) {
    (void)hipFuncSetAttribute((const void*)k_exact_tile, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint64_t) * kExactTile));
    attr_set[h->device & 63] = true;
  }
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t qc = std::min(chunk, nq - q0);
    CMS_HIP(hipMemcpyAsync(m.q1.ptr, rows + q0, sizeof(int64_t) * (size_t)qc, hipMemcpyHostToDevice, h->stream));
    std::vector<int64_t> sel;  // the chunk's queries that are not integer-eligible
    for (int64_t q = 0; q < qc; ++q)
      if (m.h_seq[(size_t)rows[q0 + q]]) sel.push_back(q);
    if ((int64_t)sel.size() < qc) {
      TimedScope ts(h, "exact_tile");
      hipLaunchKernelGGL(k_exact_tile, dim3((unsigned)(qc * ntiles)), dim3(kExactThreads), sizeof(uint64_t) * (size_t)T,
                         h->stream, exact_view(h), m.q1.as<int64_t>(), (int32_t)T, ntiles, slab, n);
      CMS_HIP(hipGetLastError());
    }
    int rc;
    if (!sel.empty()) {  // whole rows of the sequential route
      CMS_HIP(hipMemcpyAsync(m.sel.ptr, sel.data(), sizeof(int64_t) * sel.size(), hipMemcpyHostToDevice, h->stream));
      ExactPairArgs g{m.q1.as<int64_t>(), nullptr, m.sel.as<int64_t>(), (int64_t)sel.size(), n, 1, 0, slab, n};
      if ((rc = launch_pairs(h, g))) return rc;
    }
    if (m.n_seq > 0 && (int64_t)sel.size() < qc) {  // the non-eligible candidates' columns of every query
      ExactPairArgs g{m.q1.as<int64_t>(), m.seq_rows.as<int64_t>(), nullptr, qc, m.n_seq, 1, 1, slab, n};
      if ((rc = launch_pairs(h, g))) return rc;
    }
    std::vector<TopQuery> qs((size_t)qc);
    for (int64_t q = 0; q < qc; ++q) qs[(size_t)q] = TopQuery{q, rows[q0 + q], q0 + q};
    // (launch_top_k synchronises the stream: sel and qs may go)
    if ((rc = launch_top_k(h, slab, qs, k, nullptr, d_ids, d_scores, d_counts))) return rc;
  }
  return CMS_OK;
}

}  // namespace cms
