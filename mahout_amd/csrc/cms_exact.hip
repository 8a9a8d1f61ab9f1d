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
//   - the top-k is launch_top_k on the slab, as the sketch paths call it;
//   - k_exact_estimate: GenericUserBasedRecommender.doEstimatePreference over
//     the raw preferences (the sim == null branch), one workgroup per (user,
//     tile of T candidate slots) -- see the kernel.
//
// Why the tile's value is the reference's, bit for bit: for two owners with
// U < 2^53 every partial sum the reference forms is an integer multiple of
// 2^-2s of magnitude below 2^53, so no addition rounds and
// ldexp((double) dot, -2s) is sumXY in any order; the rest is correctly rounded
// operations on the same operands.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <vector>

#include "cms_exact.h"
#include "cms_exact_plan.h"
#include "cms_internal.h"
#include "cms_ref.h"

namespace cms {

constexpr int kExactThreads = 512;      // 8 waves; two workgroups per CU at the default tile
constexpr int kExactPairThreads = 256;
constexpr int kExactEstThreads = 256;   // three workgroups per CU at the default tile (48 KiB each)
constexpr int64_t kExactChunkMax = 16384;  // query rows per slab chunk (the tile grid is chunk x tiles)

struct ExactModel {
  int64_t n = 0, npairs = 0, nitems = 0;
  int shift = kExactNoShift;
  std::vector<uint8_t> h_seq;  // [n] 1: not integer-eligible
  std::vector<int64_t> ids;    // [nitems] getItemIDs(): the keys, sorted and unique (key -> dense item index)
  std::vector<int64_t> h_off, h_keys;  // the attached CSR's offsets and keys: the DataModel of the recommend call
  int64_t n_seq = 0;
  DevBuf off, item, val, unit;  // owner side: [n + 1] i64, [np] dense item (i32), float, unit (i32)
  DevBuf ioff, irow, iunit;     // item side: [nitems + 1] i64, [np] owner row ascending (i32), unit (i32)
  DevBuf U, root;               // [n] saturating sum of squared units (u64), Math.sqrt(sumX2) (f64)
  DevBuf seq_rows;              // [n_seq] the non-eligible rows (i64)
  DevBuf q1, q2, sel, out;      // a call's rows, selected queries and results
  DevBuf e_urow, e_nboff, e_slot, e_tiles, e_est;  // an estimate batch: users' rows, neighbour offsets, plan, estimates
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

// ---- the estimate kernel ----
// GenericUserBasedRecommender.doEstimatePreference with sim == null
// (T/impl/recommender/GenericUserBasedRecommender.java:134-184) for the
// candidate slots of one (user, tile): the neighbourhood is walked in the
// caller's order (:147); the user itself is skipped (:148); pref is the
// neighbour's raw float for the item, an absent item being no data point and
// a present 0.0 being one (:159-161); theSimilarity is sims[j], the exact
// userSimilarity(user, neighbour) of k_exact_pairs, skipped when NaN
// (:162-163); per data point ItemEstimate::add of that one element (:164-166)
// and at the end ItemEstimate::finish (:172-183).
//
// Block b holds tile b's slots in LDS: their dense item indices, ascending,
// and an ItemEstimate each (preference, total, count), zeroed.  The neighbours
// are taken one after another by the whole workgroup.  The neighbour's item
// list ascends as the slots do: a binary search finds its first item at or
// past the tile's first slot, the threads walk the list from there to the
// tile's last item, and each thread looks its item up among the slots (binary
// search in LDS) and, on a hit, adds its data point to that slot.  A
// neighbour's items are distinct, so one slot is touched by one thread per
// neighbour: no atomics, and no sum depends on which thread ran when.  The
// barrier between two neighbours keeps every slot's sums in neighbourhood
// order.  The work is the neighbours' list lengths within the tile's range,
// times the log of the tile.
struct ExactEstArgs {
  const int64_t* urow;      // [n] the users' owner rows
  const int64_t* nb_off;    // [n + 1] user u's neighbours: nb_row / sims [nb_off[u], nb_off[u + 1])
  const int64_t* nb_row;    // the neighbours' owner rows
  const double* sims;       // userSimilarity(user, neighbour)
  const ExactEstTile* tiles;
  const int32_t* slot_item;  // [S]
  float* est;                // [S]
  int32_t T, use_capper;
  float lo, hi;
};

__global__ __launch_bounds__(kExactEstThreads) void k_exact_estimate(ExactView v, ExactEstArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char exact_est_lds[];
  double* preference = reinterpret_cast<double*>(exact_est_lds);
  double* total = preference + g.T;
  int32_t* slot = reinterpret_cast<int32_t*>(total + g.T);
  int32_t* count = slot + g.T;
  const ExactEstTile tile = g.tiles[blockIdx.x];
  const int len = tile.len;  // >= 1
  for (int i = threadIdx.x; i < len; i += kExactEstThreads) {
    slot[i] = g.slot_item[tile.lo + i];
    preference[i] = 0.0;
    total[i] = 0.0;
    count[i] = 0;
  }
  __syncthreads();
  const int32_t first = slot[0], last = slot[len - 1];
  const int64_t x = g.urow[tile.user];
  const int64_t jhi = g.nb_off[tile.user + 1];
  for (int64_t j = g.nb_off[tile.user]; j < jhi; ++j) {
    const int64_t y = g.nb_row[j];
    const double s = g.sims[j];
    if (y == x || s != s) continue;  // the same for every thread: no slot is touched, no barrier is owed
    int64_t a = v.off[y];
    const int64_t hi = v.off[y + 1];
    for (int64_t b = hi; a < b;) {  // the neighbour's first item at or past the tile's
      const int64_t mid = (a + b) >> 1;
      if (v.item[mid] < first) a = mid + 1;
      else b = mid;
    }
    for (int64_t t = a + threadIdx.x; t < hi; t += kExactEstThreads) {
      const int32_t it = v.item[t];
      if (it > last) break;
      int lo = 0;
      for (int up = len; lo < up;) {
        const int mid = (lo + up) >> 1;
        if (slot[mid] < it) lo = mid + 1;
        else up = mid;
      }
      if (lo < len && slot[lo] == it) {
        ItemEstimate e;
        e.preference = preference[lo];
        e.total = total[lo];
        e.count = count[lo];
        const float pref = v.val[t];
        e.add(&s, &pref, 1);
        preference[lo] = e.preference;
        total[lo] = e.total;
        count[lo] = e.count;
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < len; i += kExactEstThreads) {
    ItemEstimate e;
    e.preference = preference[i];
    e.total = total[i];
    e.count = count[i];
    g.est[tile.lo + i] = e.finish(g.use_capper, g.lo, g.hi);
  }
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
  m->h_off.assign(off, off + n + 1);
  m->h_keys.assign(keys, keys + np);
  m->ids = std::move(ids);
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

void exact_host_csr(const cms_handle* h, const int64_t** off, const int64_t** keys) {
  *off = h->exact->h_off.data();
  *keys = h->exact->h_keys.data();
}

int exact_estimate_batch(cms_handle* h, int64_t n, const int64_t* user_rows, const int64_t* nb_offsets,
                         const int64_t* nb_rows, const int64_t* item_offsets, const int64_t* item_keys,
                         int32_t use_capper, float cap_min, float cap_max, float* out) {
  ExactModel& m = *h->exact;
  const int64_t M = nb_offsets[n], Q = item_offsets[n];
  if (Q == 0) return CMS_OK;
  const int T = exact_est_tile_for(h->tune.exact_est_tile);
  ExactEstPlan plan;
  exact_plan_estimates(m.ids, n, item_offsets, item_keys, T, plan, [](int64_t users, auto f) {
    parallel_users(users, (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), f);
  });
  const size_t S = plan.slot_item.size();
  std::vector<float> est(S);
  if (S > 0) {
    // userSimilarity(user, neighbour) of every pair of the batch (:162): one elementwise launch
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
      ExactPairArgs pg{m.q1.as<int64_t>(), m.q2.as<int64_t>(), nullptr, M, M, 0, 0, m.out.as<double>(), M};
      if ((rc = launch_pairs(h, pg))) return rc;
      ExactEstArgs g{m.e_urow.as<int64_t>(),       m.e_nboff.as<int64_t>(), m.q2.as<int64_t>(),  m.out.as<double>(),
                     m.e_tiles.as<ExactEstTile>(), m.e_slot.as<int32_t>(),  m.e_est.as<float>(), (int32_t)T,
                     use_capper,                   cap_min,                 cap_max};
      {
        TimedScope ts(h, "exact_estimate");
        hipLaunchKernelGGL(k_exact_estimate, dim3((unsigned)plan.tiles.size()), dim3(kExactEstThreads),
                           (size_t)kExactEstSlotBytes * (size_t)T, h->stream, exact_view(h), g);
        CMS_HIP(hipGetLastError());
      }
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
