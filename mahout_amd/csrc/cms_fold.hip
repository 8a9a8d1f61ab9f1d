// cms_fold.hip -- the kernels of cms_fold_table: a live u32 table folded to a
// narrower width w' that divides its own w.
//
// The hash is ((a key + b) mod p) mod w, and (s mod w) mod w' = s mod w' for
// every divisor w' of w, so T'[r][i][j'] = the sum of T[r][i][j] over
// j = j' (mod w') is the table the same stream builds at width w'.  The driver
// (cms_checkpoint.hip fold_plan / fold_pack_payload) goes compaction's route:
// scan, ckpt::compact_form and the payload offsets on the host, pack.  Both
// kernels are one workgroup per owner row over a persistent grid and read every
// stored source byte once; neither holds a row at more than its folded width.
//
//   k_fold_scan  the folded row's largest counter (2^32 when a folded counter
//                reaches it) and whether every sketch row sums to the row mass
//   k_fold_pack  the folded row in its target form at its place in the payload,
//                and the payload checksum of what it stores
//
// Dense source rows where w' % 16 == 0 never touch LDS: folded group g (16
// counters) of a sketch row is the sum of the source groups g + k w'/16 for
// k < w / w'; a lane takes a folded group, walks its source groups and adds in
// registers.  Neighbouring lanes take neighbouring groups, so each step of the
// walk is one coalesced load across the wavefront.  A list source, a list
// target and widths with w' % 16 != 0 go through an LDS image of the folded
// sketch row, u32 [w']: at w' <= w / 2 that is at most the 2 w bytes
// k_compact_pack's image takes (w' == w is compaction itself: the driver sends
// it to k_compact_scan / k_compact_pack).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cms_checkpoint.h"
#include "cms_internal.h"
#include "cms_rows.h"

namespace cms {
namespace {

using namespace ckpt;
using namespace rows;

// Folded counters [jf, jf + 16) of the sketch row whose source counters start
// at `base` (a multiple of 16, as jf and wf): the sum over k < K of the source
// groups at base + jf + k wf.  True when a sum passed 2^32 - 1 (only u32
// source rows can: K narrow counters stay far below it).
__device__ __forceinline__ bool fold_group(const RowSrc& s, int64_t base, int K, int wf, uint32_t (&v)[16]) {
  bool over = false;
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = 0u;
  for (int k = 0; k < K; ++k) {
    uint32_t x[16];
    src16(s, base + (int64_t)k * wf, x);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t t = v[q] + x[q];
      over |= t < x[q];
      v[q] = t;
    }
  }
  return over;
}

// Sketch row rr of the dense row r (source s) added into the zeroed image
// lc[0, wf): counter j to j mod wf.  Returns the lane's part of the sketch
// row's sum; over: an image word passed 2^32 - 1.
__device__ __forceinline__ unsigned long long image_add_dense(const TableView& tv, const RowSrc& s, int64_t r, int rr,
                                                               int wf, uint32_t* lc, bool& over) {
  const int w = tv.w;
  unsigned long long sum = 0;
  if ((w & 15) == 0) {
    for (int g = threadIdx.x; g < (w >> 4); g += 256) {
      uint32_t x[16];
      src16(s, (int64_t)rr * w + 16 * g, x);
      int jf = (16 * g) % wf;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (x[q]) {
          over |= atomicAdd(&lc[jf], x[q]) + x[q] < x[q];
          sum += x[q];
        }
        if (++jf == wf) jf = 0;
      }
    }
  } else {  // (no forms at such a width: u16 and u32 rows, counter by counter)
    for (int j = threadIdx.x; j < w; j += 256) {
      const uint32_t x = tv.get(r, (int64_t)rr * w + j);
      if (x) {
        over |= atomicAdd(&lc[j % wf], x) + x < x;
        sum += x;
      }
    }
  }
  return sum;
}

constexpr unsigned long long kOver = 1ull << 32;  // the scan's largest counter, saturated

// out[r] = (largest folded counter of row r, saturated at 2^32 - 1; bit 0: every
// sketch row sums to the row mass -- asked only of rows whose mass is in
// [1, list_mass_max], as in k_compact_scan -- bit 1: a folded counter reached
// 2^32).  lc: wf zeroed words, left zeroed after every row.
__global__ __launch_bounds__(256) void k_fold_scan(TableView tv, const uint64_t* mass, int64_t n, int depth, int wf,
                                                   uint64_t list_mass_max, uint2* out) {
  extern __shared__ uint32_t lc[];
  __shared__ unsigned long long s_red[4];
  __shared__ unsigned long long s_max[4];
  const int w = tv.w;
  const int K = w / wf;
  const int G = wf >> 4;  // folded groups per sketch row (the register path: wf % 16 == 0)
  for (int j = threadIdx.x; j < wf; j += 256) lc[j] = 0u;
  __syncthreads();
  auto umax = [](unsigned long long a, unsigned long long b) { return a > b ? a : b; };
  auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const RowSrc s = row_src(tv, r);  // (uniform over the workgroup)
    const uint64_t M = mass[r];
    unsigned long long mx = 0;
    uint32_t eq = 0;
    if (s.p == nullptr) {
      // the shared zero row: nothing is read
    } else if (s.f == kFormList) {
      // folded counter (rr, b) = the entries of sketch row rr congruent to b: the
      // count an entry's atomic returns, plus one, passes through every value up to it
      const uint16_t* e = reinterpret_cast<const uint16_t*>(s.p);
      const uint32_t m = e[0];
      for (int rr = 0; rr < depth; ++rr) {
        for (uint32_t t = threadIdx.x; t < m; t += 256) {
          const uint32_t b = e[1 + (uint32_t)rr * m + t];
          if (b < (uint32_t)w) mx = umax(mx, (unsigned long long)atomicAdd(&lc[b % (uint32_t)wf], 1u) + 1u);
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < m; t += 256) {  // only the words the entries touched
          const uint32_t b = e[1 + (uint32_t)rr * m + t];
          if (b < (uint32_t)w) lc[b % (uint32_t)wf] = 0u;
        }
        __syncthreads();
      }
      mx = block_reduce(mx, s_max, umax);
      eq = (uint64_t)m == M;  // every sketch row of a list has m entries
    } else {
      const bool sums = M >= 1 && M <= list_mass_max;
      bool all = sums;
      if ((wf & 15) == 0 && !sums) {  // only the maximum is asked for: the folded row's d G groups flat over the lanes
        for (int i = threadIdx.x; i < depth * G; i += 256) {
          const int rr = i / G, g = i - rr * G;
          uint32_t v[16];
          if (fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v)) mx = kOver;
#pragma unroll
          for (int q = 0; q < 16; ++q) mx = umax(mx, v[q]);
        }
      } else if ((wf & 15) == 0) {
        for (int rr = 0; rr < depth; ++rr) {
          unsigned long long sum = 0;
          for (int g = threadIdx.x; g < G; g += 256) {
            uint32_t v[16];
            if (fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v)) mx = kOver;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              mx = umax(mx, v[q]);
              sum += v[q];
            }
          }
          all = all && block_reduce(sum, s_red, add) == M;
        }
      } else {
        for (int rr = 0; rr < depth; ++rr) {
          bool over = false;
          const unsigned long long sum = image_add_dense(tv, s, r, rr, wf, lc, over);
          if (over) mx = kOver;
          __syncthreads();
          for (int j = threadIdx.x; j < wf; j += 256) {
            mx = umax(mx, lc[j]);
            lc[j] = 0u;
          }
          if (sums) all = all && block_reduce(sum, s_red, add) == M;
          __syncthreads();
        }
      }
      mx = block_reduce(mx, s_max, umax);
      eq = all;
    }
    if (threadIdx.x == 0) out[r] = make_uint2(mx >= kOver ? 0xFFFFFFFFu : (uint32_t)mx, eq | (mx >= kOver ? 2u : 0u));
  }
}

// Row r folded to width wf in its target form tform[r] (kRow*) at payload +
// dst[r]; out[0] += the checksum of the bytes stored.  The payload was zeroed:
// pad bytes stay zero.  A list row's key count is its mass (compact_form: every
// sketch row sums to it); entries past it are never written, whatever the
// counters say.  lc: wf words.
__global__ __launch_bounds__(256) void k_fold_pack(TableView tv, const uint64_t* mass, const uint8_t* tform,
                                                   const uint64_t* dst, int64_t n, int depth, int wf, uint8_t* payload,
                                                   unsigned long long* out) {
  extern __shared__ uint32_t lc[];
  __shared__ unsigned long long s_red[4];
  __shared__ uint32_t s_wave[4];
  const int w = tv.w;
  const int K = w / wf;
  const int G = wf >> 4;
  const bool groups = (wf & 15) == 0;
  unsigned long long acc = 0;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int tf = tform[r];  // (uniform over the workgroup, as every branch below)
    const RowSrc s = row_src(tv, r);
    if (tf == kRowZero || s.p == nullptr) continue;
    uint8_t* row = payload + dst[r];
    const bool src_list = s.f == kFormList;
    const int tb = target_bits(tf);
    if (!src_list && tf != kRowList && groups) {  // dense -> dense in registers
      for (int i = threadIdx.x; i < depth * G; i += 256) {
        const int rr = i / G, g = i - rr * G;
        uint32_t v[16];
        fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v);
        store_group(row, (int64_t)rr * wf + 16 * g, v, tb, acc);
      }
      continue;
    }
    const uint32_t m = (uint32_t)mass[r];  // (a list target's key count)
    uint16_t* e = reinterpret_cast<uint16_t*>(row);
    if (tf == kRowList && threadIdx.x == 0) {
      e[0] = (uint16_t)m;
      acc += m;
    }
    const int chunk = (wf + 255) >> 8;  // consecutive buckets per lane: a list's entries come out ascending
    const int j0 = min(wf, (int)threadIdx.x * chunk), j1 = min(wf, j0 + chunk);
    for (int rr = 0; rr < depth; ++rr) {  // a sketch row at a time through the image
      for (int j = threadIdx.x; j < wf; j += 256) lc[j] = 0u;
      __syncthreads();
      if (src_list) {
        const uint16_t* se = reinterpret_cast<const uint16_t*>(s.p);
        const uint32_t sm = se[0];
        for (uint32_t t = threadIdx.x; t < sm; t += 256) {
          const uint32_t b = se[1 + (uint32_t)rr * sm + t];
          if (b < (uint32_t)w) atomicAdd(&lc[b % (uint32_t)wf], 1u);
        }
      } else {
        bool over = false;  // (the scan refused a row that passes 2^32)
        (void)image_add_dense(tv, s, r, rr, wf, lc, over);
      }
      __syncthreads();
      if (tf == kRowList) {
        uint32_t cnt = 0;
        for (int j = j0; j < j1; ++j) cnt += lc[j];
        uint32_t at = block_scan_exclusive(cnt, s_wave);
        for (int j = j0; j < j1; ++j) {
          for (uint32_t c = lc[j]; c > 0 && at < m; --c, ++at) {
            const uint32_t idx = 1u + (uint32_t)rr * m + at;
            e[idx] = (uint16_t)j;
            acc += (unsigned long long)j << (16 * (idx & 3u));
          }
        }
      } else if (groups) {
        for (int g = threadIdx.x; g < G; g += 256) {
          uint32_t v[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) v[q] = lc[16 * g + q];
          store_group(row, (int64_t)rr * wf + 16 * g, v, tb, acc);
        }
      } else {  // (no forms at such a width: u16 or u32 counters)
        for (int j = threadIdx.x; j < wf; j += 256) store_counter(row, (int64_t)rr * wf + j, lc[j], tb, acc);
      }
      __syncthreads();  // the image is read before the next sketch row replaces it
    }
  }
  auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
  const unsigned long long total = block_reduce(acc, s_red, add);
  if (threadIdx.x == 0 && total) atomicAdd(out, total);
}

unsigned rows_grid(const cms_handle* h) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(h->n, (int64_t)h->num_cus * 8));
}

// wf <= w / 2 <= 16384: the image is at most 64 KiB, beside the kernels' few
// static words past the 64 KiB a kernel gets unasked.
void allow_lds() {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)k_fold_scan, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fold_pack, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    return true;
  }();
  (void)attr;
}

}  // namespace

int fold_scan(cms_handle* h, int32_t wf, uint64_t list_mass_max, uint2* d_scan) {
  if (wf < 1 || wf > h->p.width / 2 || h->p.width % wf) return set_error(CMS_E_PARAM, "fold_scan: width %d", (int)wf);
  allow_lds();
  TimedScope ts(h, "fold_scan");
  hipLaunchKernelGGL(k_fold_scan, dim3(rows_grid(h)), dim3(256), sizeof(uint32_t) * (size_t)wf, h->stream, h->tview(),
                     h->d_row_mass, h->n, (int)h->p.depth, (int)wf, list_mass_max, d_scan);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int fold_pack(cms_handle* h, int32_t wf, const uint8_t* d_tform, const uint64_t* d_dst, uint8_t* d_payload,
              uint64_t payload_bytes, unsigned long long* d_sum) {
  if (wf < 1 || wf > h->p.width / 2 || h->p.width % wf) return set_error(CMS_E_PARAM, "fold_pack: width %d", (int)wf);
  allow_lds();
  TimedScope ts(h, "fold_pack");
  if (payload_bytes) CMS_HIP(hipMemsetAsync(d_payload, 0, (size_t)payload_bytes, h->stream));
  hipLaunchKernelGGL(k_fold_pack, dim3(rows_grid(h)), dim3(256), sizeof(uint32_t) * (size_t)wf, h->stream, h->tview(),
                     h->d_row_mass, d_tform, d_dst, h->n, (int)h->p.depth, (int)wf, d_payload, d_sum);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

}  // namespace cms
