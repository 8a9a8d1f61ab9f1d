// cms_threshold.hip -- threshold neighbourhoods over a similarity slab on gfx950.
//
// ThresholdUserNeighborhood.getUserNeighborhood
// (T/impl/neighborhood/ThresholdUserNeighborhood.java:86-94) walks the other
// users in DataModel.getUserIDs() order -- ascending ID, i.e. ascending owner
// row -- and keeps those with !Double.isNaN(s) && s >= threshold.  The answer
// is a list of unknown length per query, so the top-k's fixed [rows][k]
// machinery does not apply; the selection here reads the same [query][n] fp64
// slabs and emits a CSR in owner row order, with no atomics and no sort:
//   k_thr_mark     one wave per 64 slab columns of a query: the wave's ballot
//                  is one u64 word of the query's mask (position space);
//   k_thr_rowmask  (permuted slabs) one wave per 64 owner rows: lane r reads
//                  bit inv[r] of the position mask, the ballot is the mask in
//                  row space;
//   k_thr_scan     one workgroup per query: exclusive scan of the words'
//                  popcounts -> per-word offsets and the query's count;
//   k_thr_fill     one lane per mask word: its set bits, in order, to
//                  base[query] + word offset + rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "cms_internal.h"

namespace cms {

constexpr int kThrThreads = 256;  // 4 waves
constexpr int kThrWaves = kThrThreads / 64;

// Wave task t = (query q = t / nw, mask word wi = t % nw).  Without a
// permutation (inv null) the mask is already in row space and the popcounts
// are written here.
__global__ __launch_bounds__(kThrThreads) void k_thr_mark(const double* __restrict__ slab, int64_t ld, int64_t n,
                                                          int64_t nw, const TopQuery* __restrict__ queries,
                                                          int64_t nq, double threshold, int has_perm,
                                                          uint64_t* __restrict__ mask, uint32_t* __restrict__ wcnt) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = blockIdx.x * (int64_t)kThrWaves + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kThrWaves;
  const int64_t tasks = nq * nw;
  for (int64_t t = wave; t < tasks; t += stride) {  // wave-uniform
    const int64_t q = t / nw, wi = t - q * nw;
    const TopQuery Q = queries[q];
    const int64_t c = wi * 64 + lane;
    bool keep = false;
    if (c < n) {
      const double v = slab[Q.slab_row * ld + c];
      keep = v == v && v >= threshold && c != Q.self_col;
    }
    const uint64_t word = __ballot(keep);
    if (lane == 0) {
      mask[t] = word;
      if (!has_perm) wcnt[t] = (uint32_t)__popcll(word);
    }
  }
}

// Position-space mask -> row-space mask (owner row r sits at column inv[r]).
__global__ __launch_bounds__(kThrThreads) void k_thr_rowmask(const uint64_t* __restrict__ pmask, int64_t n, int64_t nw,
                                                             int64_t nq, const uint32_t* __restrict__ inv,
                                                             uint64_t* __restrict__ rmask,
                                                             uint32_t* __restrict__ wcnt) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = blockIdx.x * (int64_t)kThrWaves + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kThrWaves;
  const int64_t tasks = nq * nw;
  for (int64_t t = wave; t < tasks; t += stride) {
    const int64_t q = t / nw, wi = t - q * nw;
    const int64_t r = wi * 64 + lane;
    bool keep = false;
    if (r < n) {
      const uint32_t p = inv[r];
      keep = (pmask[q * nw + (p >> 6)] >> (p & 63u)) & 1ull;
    }
    const uint64_t word = __ballot(keep);
    if (lane == 0) {
      rmask[t] = word;
      wcnt[t] = (uint32_t)__popcll(word);
    }
  }
}

// wcnt[q][*] -> its exclusive scan in place, count[q] = the total.
__global__ __launch_bounds__(kThrThreads) void k_thr_scan(uint32_t* __restrict__ wcnt, int64_t nw,
                                                          uint32_t* __restrict__ count) {
  __shared__ uint32_t wsum[kThrWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t* w = wcnt + blockIdx.x * nw;
  uint32_t carry = 0;
  for (int64_t b = 0; b < nw; b += kThrThreads) {
    const int64_t i = b + tid;
    const uint32_t v = i < nw ? w[i] : 0u;
    uint32_t s = v;  // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(s, o, 64);
      if (lane >= o) s += u;
    }
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kThrWaves; ++k) {
      const uint32_t x = wsum[k];
      if (k < wv) before += x;
      total += x;
    }
    if (i < nw) w[i] = carry + before + s - v;
    carry += total;
    __syncthreads();  // wsum is rewritten by the next chunk
  }
  if (tid == 0) count[blockIdx.x] = carry;
}

// One lane per mask word.  base[q]: the query's first slot in the staging
// arrays.  inv null: columns are rows.  out_scores null: IDs only.
__global__ __launch_bounds__(kThrThreads) void k_thr_fill(const double* __restrict__ slab, int64_t ld, int64_t nw,
                                                          const TopQuery* __restrict__ queries, int64_t nq,
                                                          const uint64_t* __restrict__ rmask,
                                                          const uint32_t* __restrict__ woff,
                                                          const int64_t* __restrict__ base,
                                                          const uint32_t* __restrict__ inv,
                                                          const int64_t* __restrict__ owner_ids,
                                                          int64_t* __restrict__ out_ids,
                                                          double* __restrict__ out_scores) {
  const int64_t tasks = nq * nw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tasks; t += (int64_t)gridDim.x * blockDim.x) {
    uint64_t word = rmask[t];
    if (!word) continue;
    const int64_t q = t / nw, wi = t - q * nw;
    const double* sc = slab + queries[q].slab_row * ld;
    int64_t o = base[q] + woff[t];
    while (word) {
      const int64_t row = wi * 64 + __builtin_ctzll(word);
      word &= word - 1;
      out_ids[o] = owner_ids ? owner_ids[row] : row;
      if (out_scores) out_scores[o] = sc[inv ? (int64_t)inv[row] : row];
      ++o;
    }
  }
}

namespace {

unsigned wave_grid(int64_t tasks) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((tasks + kThrWaves - 1) / kThrWaves, int64_t(1) << 20));
}

// The selection's scratch and bookkeeping of one threshold_rows call.
struct ThrJob {
  cms_handle* h;
  double threshold;
  int64_t nw;                 // mask words per query
  const uint32_t* d_inv = nullptr;  // owner row -> slab column (permuted slabs)
  DevBuf inv, pmask, rmask, wcnt, count, base, stage;
  std::vector<uint32_t> h_count;
  std::vector<int64_t> h_base;
  // per output slot: list length and where the list was written (entries
  // land in processing order; finish() restores query order)
  std::vector<int64_t> len, at;
  int64_t running = 0;
  bool in_order = true;
  int64_t next_pos = 0;
  int64_t* out_ids;
  double* out_scores;
  int64_t capacity;
};

// One chunk: the slab holds the similarities of the queries qs.
int select_chunk(ThrJob& J, const double* slab, const std::vector<TopQuery>& qs) {
  cms_handle* h = J.h;
  const int64_t nqc = (int64_t)qs.size();
  if (nqc == 0) return CMS_OK;
  const int64_t n = h->n, nw = J.nw, tasks = nqc * nw;
  CMS_HIP(h->ws_topq.ensure(sizeof(TopQuery) * (size_t)nqc));
  CMS_HIP(hipMemcpyAsync(h->ws_topq.ptr, qs.data(), sizeof(TopQuery) * (size_t)nqc, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(J.rmask.ensure(sizeof(uint64_t) * (size_t)tasks));
  CMS_HIP(J.wcnt.ensure(sizeof(uint32_t) * (size_t)tasks));
  CMS_HIP(J.count.ensure(sizeof(uint32_t) * (size_t)nqc));
  if (J.d_inv) CMS_HIP(J.pmask.ensure(sizeof(uint64_t) * (size_t)tasks));
  const TopQuery* dq = h->ws_topq.as<TopQuery>();
  {
    TimedScope ts(h, "threshold_select");
    hipLaunchKernelGGL(k_thr_mark, dim3(wave_grid(tasks)), dim3(kThrThreads), 0, h->stream, slab, n, n, nw, dq, nqc,
                       J.threshold, J.d_inv ? 1 : 0, J.d_inv ? J.pmask.as<uint64_t>() : J.rmask.as<uint64_t>(),
                       J.wcnt.as<uint32_t>());
    if (J.d_inv)
      hipLaunchKernelGGL(k_thr_rowmask, dim3(wave_grid(tasks)), dim3(kThrThreads), 0, h->stream,
                         J.pmask.as<uint64_t>(), n, nw, nqc, J.d_inv, J.rmask.as<uint64_t>(), J.wcnt.as<uint32_t>());
    hipLaunchKernelGGL(k_thr_scan, dim3((unsigned)nqc), dim3(kThrThreads), 0, h->stream, J.wcnt.as<uint32_t>(), nw,
                       J.count.as<uint32_t>());
    CMS_HIP(hipGetLastError());
  }
  J.h_count.resize((size_t)nqc);
  CMS_HIP(hipMemcpyAsync(J.h_count.data(), J.count.ptr, sizeof(uint32_t) * (size_t)nqc, hipMemcpyDeviceToHost,
                         h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));  // (also: the host query list and ws_topq may be reused)
  J.h_base.resize((size_t)nqc);
  int64_t chunk_total = 0;
  for (int64_t q = 0; q < nqc; ++q) {
    const int64_t pos = qs[(size_t)q].out_pos;
    J.h_base[(size_t)q] = chunk_total;
    J.len[(size_t)pos] = J.h_count[(size_t)q];
    J.at[(size_t)pos] = J.running + chunk_total;
    chunk_total += J.h_count[(size_t)q];
    if (pos != J.next_pos) J.in_order = false;
    J.next_pos = pos + 1;
  }
  const int64_t start = J.running;
  J.running += chunk_total;
  if (!J.out_ids || J.running > J.capacity || chunk_total == 0) return CMS_OK;  // count only
  const size_t cells = (size_t)chunk_total;
  if (J.stage.ensure((sizeof(int64_t) + (J.out_scores ? sizeof(double) : 0)) * cells) != hipSuccess)
    return set_error(CMS_E_OOM, "threshold neighbours: no device memory for a chunk's %lld entries",
                     (long long)chunk_total);
  CMS_HIP(J.base.ensure(sizeof(int64_t) * (size_t)nqc));
  CMS_HIP(hipMemcpyAsync(J.base.ptr, J.h_base.data(), sizeof(int64_t) * (size_t)nqc, hipMemcpyHostToDevice, h->stream));
  int64_t* s_ids = J.stage.as<int64_t>();
  double* s_sc = J.out_scores ? reinterpret_cast<double*>(s_ids + cells) : nullptr;
  {
    TimedScope ts(h, "threshold_select");
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tasks + kThrThreads - 1) / kThrThreads, 1 << 20));
    hipLaunchKernelGGL(k_thr_fill, dim3(g), dim3(kThrThreads), 0, h->stream, slab, n, nw, dq, nqc,
                       J.rmask.as<uint64_t>(), J.wcnt.as<uint32_t>(), J.base.as<int64_t>(), J.d_inv, h->d_owner_ids,
                       s_ids, s_sc);
    CMS_HIP(hipGetLastError());
  }
  CMS_HIP(hipMemcpyAsync(J.out_ids + start, s_ids, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, h->stream));
  if (s_sc) CMS_HIP(hipMemcpyAsync(J.out_scores + start, s_sc, sizeof(double) * cells, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));  // h_base and the staging buffer are reused
  return CMS_OK;
}

// offsets and *total from the per-query lengths; lists that were written in
// another order than the queries' (permuted tiles) move to their places.
int finish(ThrJob& J, int64_t nq, int64_t* offsets, int64_t* total) {
  offsets[0] = 0;
  for (int64_t i = 0; i < nq; ++i) offsets[i + 1] = offsets[i] + J.len[(size_t)i];
  *total = offsets[nq];
  if (!J.out_ids || *total > J.capacity || J.in_order || *total == 0) return CMS_OK;
  const size_t cells = (size_t)*total;
  int64_t* ti = new (std::nothrow) int64_t[cells];
  double* tsc = J.out_scores ? new (std::nothrow) double[cells] : nullptr;
  if (!ti || (J.out_scores && !tsc)) {
    delete[] ti;
    delete[] tsc;
    return set_error(CMS_E_OOM, "host allocation failed");
  }
  std::memcpy(ti, J.out_ids, sizeof(int64_t) * cells);
  if (tsc) std::memcpy(tsc, J.out_scores, sizeof(double) * cells);
  for (int64_t i = 0; i < nq; ++i) {
    const size_t m = (size_t)J.len[(size_t)i];
    if (!m) continue;
    std::memcpy(J.out_ids + offsets[i], ti + J.at[(size_t)i], sizeof(int64_t) * m);
    if (tsc) std::memcpy(J.out_scores + offsets[i], tsc + J.at[(size_t)i], sizeof(double) * m);
  }
  delete[] ti;
  delete[] tsc;
  return CMS_OK;
}

}  // namespace

// Threshold neighbourhoods of the owner rows rows[0, nq) (any order, repeats
// allowed): offsets [nq + 1] and *total always; the lists (host arrays, owner
// row order within a list) while they fit capacity.  out_ids null: counts only.
int threshold_rows(cms_handle* h, const int64_t* rows, int64_t nq, double threshold, int64_t* offsets,
                   int64_t* out_ids, double* out_scores, int64_t capacity, int64_t* total) {
  const int64_t n = h->n;
  int rc = CMS_OK;
  ThrJob J{h, threshold, (n + 63) / 64};
  J.out_ids = out_ids;
  J.out_scores = out_scores;
  J.capacity = capacity;
  J.len.assign((size_t)nq, 0);
  J.at.assign((size_t)nq, 0);
  const int64_t chunk = h->tune.threshold_slab_rows > 0 ? h->tune.threshold_slab_rows : slab_rows_for(n);
  if (h->per_owner) {
    if ((rc = po_require_shapes(h, nullptr, 0))) return rc;
  } else if (mfma_eligible(h) && (rc = cosine_prepare(h))) {
    return rc;
  }
  if (!h->per_owner && mfma_eligible(h) && h->n_inexact_rows == 0) {
    // MFMA slabs over runs of the PERMUTED 128-row tiles that hold a requested position
    std::vector<uint32_t> inv32((size_t)n);
    for (int64_t r = 0; r < n; ++r) inv32[(size_t)r] = (uint32_t)h->h_inv[(size_t)r];
    CMS_HIP(J.inv.ensure(sizeof(uint32_t) * (size_t)n));
    CMS_HIP(hipMemcpyAsync(J.inv.ptr, inv32.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    J.d_inv = J.inv.as<uint32_t>();
    std::vector<std::pair<int64_t, int64_t>> q((size_t)nq);  // (position, output slot)
    for (int64_t i = 0; i < nq; ++i) q[(size_t)i] = {h->h_inv[(size_t)rows[i]], i};
    std::sort(q.begin(), q.end());
    std::vector<int64_t> tiles;
    for (const auto& e : q)
      if (tiles.empty() || tiles.back() != e.first / 128) tiles.push_back(e.first / 128);
    const int64_t max_run = std::min<int64_t>(chunk, (int64_t)tiles.size() * 128);
    CMS_HIP(h->ws_slab.ensure(sizeof(double) * (size_t)(max_run * n)));
    size_t ti = 0, qi = 0;
    while (ti < tiles.size()) {
      size_t tj = ti + 1;
      while (tj < tiles.size() && tiles[tj] == tiles[tj - 1] + 1 && (int64_t)(tj - ti + 1) * 128 <= chunk) ++tj;
      const int64_t q0 = tiles[ti] * 128;
      const int64_t qc = std::min<int64_t>(n - q0, (int64_t)(tj - ti) * 128);
      if ((rc = cosine_slab(h, q0, qc, h->ws_slab.as<double>()))) return rc;
      std::vector<TopQuery> qs;
      for (; qi < q.size() && q[qi].first < q0 + qc; ++qi)
        qs.push_back(TopQuery{q[qi].first - q0, q[qi].first, q[qi].second});
      if ((rc = select_chunk(J, h->ws_slab.as<double>(), qs))) return rc;
      ti = tj;
    }
    return finish(J, nq, offsets, total);
  }
  // the other producers: the query rows in chunks, columns are owner rows
  const int64_t qb = std::max<int64_t>(1, std::min<int64_t>(nq, chunk));
  CMS_HIP(h->ws_slab.ensure(sizeof(double) * (size_t)(qb * n)));
  double* slab = h->ws_slab.as<double>();
  const bool pair_rows = !h->per_owner && !h->f64;
  CMS_HIP(h->ws_query.ensure(sizeof(int64_t) * (size_t)(pair_rows ? n : qb)));
  if (pair_rows) {  // the pair kernel's candidate list: every owner row
    std::vector<int64_t> all((size_t)n);
    for (int64_t i = 0; i < n; ++i) all[(size_t)i] = i;
    CMS_HIP(hipMemcpyAsync(h->ws_query.ptr, all.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
  }
  for (int64_t r0 = 0; r0 < nq; r0 += qb) {
    const int64_t rcnt = std::min(qb, nq - r0);
    std::vector<TopQuery> qs((size_t)rcnt);
    for (int64_t q = 0; q < rcnt; ++q) qs[(size_t)q] = TopQuery{q, rows[r0 + q], r0 + q};
    if (h->per_owner) {
      CMS_HIP(hipMemcpyAsync(h->ws_query.ptr, rows + r0, sizeof(int64_t) * (size_t)rcnt, hipMemcpyHostToDevice,
                             h->stream));
      if ((rc = po_pair_cosines(h, h->ws_query.as<int64_t>(), rcnt, nullptr, n, slab))) return rc;
    } else if (h->f64) {
      for (int64_t q = 0; q < rcnt;) {  // runs of consecutive rows share a launch
        int64_t e = q + 1;
        while (e < rcnt && rows[r0 + e] == rows[r0 + e - 1] + 1) ++e;
        if ((rc = f64_slab(h, rows[r0 + q], e - q, slab + q * n))) return rc;
        q = e;
      }
    } else {
      for (int64_t q = 0; q < rcnt; ++q)
        if ((rc = pair_cosines(h, rows[r0 + q], h->ws_query.as<int64_t>(), n, slab + q * n))) return rc;
    }
    if ((rc = select_chunk(J, slab, qs))) return rc;
  }
  return finish(J, nq, offsets, total);
}

}  // namespace cms
