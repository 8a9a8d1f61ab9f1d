// cms_compact.hip -- the kernels of cms_compact_table: every owner row
// re-stored in the narrowest form its counters need now.
//
// The driver (cms_checkpoint.hip compact_table) packs the live table,
// re-formed, into a checkpoint-format payload beside it, verifies that payload
// with the loader's own pass, and restores it through restore_layout /
// k_ckpt_unpack.  Two kernels are new, both one workgroup per owner row over a
// persistent grid:
//
//   k_compact_scan  reads each row once in whatever form it is in and writes
//                   its largest counter and whether every sketch row sums to
//                   the row mass (asked only of rows small enough to become a
//                   list).  The host applies ckpt::compact_form to these.
//   k_compact_pack  re-encodes each row from its current form into its target
//                   form at its place in the payload: dense -> dense at 16
//                   counters per lane, anything -> list through an LDS image
//                   of the sketch row and a block-wide exclusive scan (lane t
//                   writes its buckets c[j] times from its scan offset), list
//                   -> dense through the same image.  It accumulates the
//                   payload checksum of what it stores.
//
// The LDS image holds one sketch row as u16 halves (2 w bytes, at most 64 KiB):
// it is used only when the source or the target is a list, both rows of mass
// below 2^16, so no counter passes a half.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cms_checkpoint.h"
#include "cms_internal.h"
#include "cms_rows.h"

namespace cms {
namespace {

using namespace ckpt;
using namespace rows;

// out[r] = (largest counter of row r, 1 when every sketch row sums to the row
// mass).  The sums are taken only of rows whose mass is in [1, list_mass_max]:
// no other row can become a list (list_mass_max 0: none can).  lc: lds_words
// zeroed words, the u16 counts of a list's sketch row.
__global__ __launch_bounds__(256) void k_compact_scan(TableView tv, const uint64_t* mass, int64_t n, int depth,
                                                      uint64_t list_mass_max, int lds_words, uint2* out) {
  extern __shared__ uint32_t lc[];
  __shared__ unsigned long long s_red[4];
  __shared__ uint32_t s_max[4];
  const int w = tv.w;
  const bool groups = (w & 15) == 0;
  for (int j = threadIdx.x; j < lds_words; j += 256) lc[j] = 0u;
  __syncthreads();
  auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const RowSrc s = row_src(tv, r);  // (uniform over the workgroup)
    const uint64_t M = mass[r];
    uint32_t mx = 0, eq = 0;
    if (s.p == nullptr) {
      // the shared zero row: every counter is zero
    } else if (s.f == kFormList) {
      // counter (rr, b) = the entries of sketch row rr equal to b: the count an
      // entry's atomic returns, plus one, passes through every value up to it
      const uint16_t* e = reinterpret_cast<const uint16_t*>(s.p);
      const uint32_t m = e[0];
      for (int rr = 0; rr < depth; ++rr) {
        for (uint32_t t = threadIdx.x; t < m; t += 256) {
          const uint32_t b = e[1 + (uint32_t)rr * m + t];
          if (b < (uint32_t)w && (int)(b >> 1) < lds_words) {
            const uint32_t sh = (b & 1u) * 16u;
            mx = umax(mx, ((atomicAdd(&lc[b >> 1], 1u << sh) >> sh) & 0xFFFFu) + 1u);
          }
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < m; t += 256) {  // only the words the entries touched
          const uint32_t b = e[1 + (uint32_t)rr * m + t];
          if (b < (uint32_t)w && (int)(b >> 1) < lds_words) lc[b >> 1] = 0u;
        }
        __syncthreads();
      }
      mx = block_reduce(mx, s_max, umax);
      eq = (uint64_t)m == M;  // every sketch row of a list has m entries
    } else {
      const bool sums = M >= 1 && M <= list_mass_max;
      bool all = sums;
      if (!sums && groups) {  // only the maximum is asked for: the row's d w / 16 groups flat over the lanes
        for (int64_t g = threadIdx.x; g < (tv.dw >> 4); g += 256) {
          uint32_t v[16];
          src16(s, 16 * g, v);
#pragma unroll
          for (int q = 0; q < 16; ++q) mx = umax(mx, v[q]);
        }
      }
      for (int rr = 0; rr < depth && (sums || !groups); ++rr) {
        unsigned long long sum = 0;
        if (groups) {
          for (int g = threadIdx.x; g < (w >> 4); g += 256) {
            uint32_t v[16];
            src16(s, (int64_t)rr * w + 16 * g, v);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              mx = umax(mx, v[q]);
              sum += v[q];
            }
          }
        } else {  // (no forms at such a width: u16 and u32 rows, counter by counter)
          for (int j = threadIdx.x; j < w; j += 256) {
            const uint32_t v = tv.get(r, (int64_t)rr * w + j);
            mx = umax(mx, v);
            sum += v;
          }
        }
        if (sums) all = all && block_reduce(sum, s_red, add) == M;
      }
      mx = block_reduce(mx, s_max, umax);
      eq = all;
    }
    if (threadIdx.x == 0) out[r] = make_uint2(mx, eq);
  }
}

__device__ __forceinline__ uint32_t lds_half(const uint32_t* lc, int j) { return (lc[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu; }

// Sketch row rr of the row at s as u16 halves in lc[0, w / 2) (w % 32 == 0:
// only shapes with forms have lists).  Ends with the workgroup synchronised.
__device__ __forceinline__ void expand_row(const RowSrc& s, int rr, int w, uint32_t* lc) {
  if (s.f == kFormList) {
    const uint16_t* e = reinterpret_cast<const uint16_t*>(s.p);
    const uint32_t m = e[0];
    for (int j = threadIdx.x; j < (w >> 1); j += 256) lc[j] = 0u;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < m; t += 256) {
      const uint32_t b = e[1 + (uint32_t)rr * m + t];
      if (b < (uint32_t)w) atomicAdd(&lc[b >> 1], 1u << ((b & 1u) * 16u));
    }
  } else {
    for (int g = threadIdx.x; g < (w >> 4); g += 256) {
      uint32_t v[16];
      src16(s, (int64_t)rr * w + 16 * g, v);
#pragma unroll
      for (int q = 0; q < 8; ++q) lc[8 * g + q] = (v[2 * q] & 0xFFFFu) | (v[2 * q + 1] << 16);
    }
  }
  __syncthreads();
}

// Row r in its target form tform[r] (kRow*) at payload + dst[r]; out[0] += the
// checksum of the bytes stored.  The payload was zeroed: pad bytes stay zero.
// A list row's key count is its mass (compact_form: every sketch row sums to
// it); entries past it are never written, whatever the counters say.
__global__ __launch_bounds__(256) void k_compact_pack(TableView tv, const uint64_t* mass, const uint8_t* tform,
                                                      const uint64_t* dst, int64_t n, int depth, int lds_words,
                                                      uint8_t* payload, unsigned long long* out) {
  extern __shared__ uint32_t lc[];
  __shared__ unsigned long long s_red[4];
  __shared__ uint32_t s_wave[4];
  const int w = tv.w;
  const int64_t dw = tv.dw;
  const bool groups = (w & 15) == 0;
  unsigned long long acc = 0;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int tf = tform[r];  // (uniform over the workgroup, as every branch below)
    const RowSrc s = row_src(tv, r);
    if (tf == kRowZero || s.p == nullptr) continue;
    uint8_t* row = payload + dst[r];
    const bool src_list = s.f == kFormList;
    if (tf == kRowList) {
      if (2 * lds_words < w) continue;  // (the driver sends no list to a shape without the image)
      const uint32_t m = (uint32_t)mass[r];
      uint16_t* e = reinterpret_cast<uint16_t*>(row);
      if (threadIdx.x == 0) {
        e[0] = (uint16_t)m;
        acc += m;
      }
      const int chunk = (w + 255) >> 8;  // consecutive buckets per lane: the entries come out ascending
      const int j0 = min(w, (int)threadIdx.x * chunk), j1 = min(w, j0 + chunk);
      for (int rr = 0; rr < depth; ++rr) {
        expand_row(s, rr, w, lc);
        uint32_t cnt = 0;
        for (int j = j0; j < j1; ++j) cnt += lds_half(lc, j);
        uint32_t at = block_scan_exclusive(cnt, s_wave);
        for (int j = j0; j < j1; ++j) {
          for (uint32_t c = lds_half(lc, j); c > 0 && at < m; --c, ++at) {
            const uint32_t idx = 1u + (uint32_t)rr * m + at;
            e[idx] = (uint16_t)j;
            acc += (unsigned long long)j << (16 * (idx & 3u));
          }
        }
        __syncthreads();  // the image is read before the next sketch row replaces it
      }
      continue;
    }
    const int tb = tf == kRowU1 ? 1 : tf == kRowU2 ? 2 : tf == kRowU4 ? 4 : tf == kRowU8 ? 8 : tf == kRowU16 ? 16 : 32;
    if (!groups) {  // (no forms at such a width: u16 or u32 counters from u16 or u32 counters)
      for (int64_t j = threadIdx.x; j < dw; j += 256) {
        const uint32_t v = tv.get(r, j);
        if (tb == 16) {
          *reinterpret_cast<uint16_t*>(row + 2 * j) = (uint16_t)v;
          acc += (unsigned long long)(v & 0xFFFFu) << (8 * (int)((2 * j) & 7));
        } else {
          *reinterpret_cast<uint32_t*>(row + 4 * j) = v;
          acc += (unsigned long long)v << (8 * (int)((4 * j) & 7));
        }
      }
      continue;
    }
    if (!src_list) {  // dense -> dense: the row's d w / 16 groups flat over the lanes, whatever the width
      for (int64_t g = threadIdx.x; g < (dw >> 4); g += 256) {
        uint32_t v[16];
        src16(s, 16 * g, v);
        store_group(row, 16 * g, v, tb, acc);
      }
      continue;
    }
    if (2 * lds_words < w) continue;
    for (int rr = 0; rr < depth; ++rr) {  // list -> dense: a sketch row at a time through the image
      expand_row(s, rr, w, lc);
      for (int g = threadIdx.x; g < (w >> 4); g += 256) {
        uint32_t v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = lds_half(lc, 16 * g + q);
        store_group(row, (int64_t)rr * w + 16 * g, v, tb, acc);
      }
      __syncthreads();
    }
  }
  auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
  const unsigned long long total = block_reduce(acc, s_red, add);
  if (threadIdx.x == 0 && total) atomicAdd(out, total);
}

int lds_words_for(const cms_handle* h) {  // a list row can be stored, or built, at this shape
  return h->forms_ok && (size_t)h->dw * 2 <= 80 * 1024 ? h->p.width / 2 : 0;
}
unsigned rows_grid(const cms_handle* h) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(h->n, (int64_t)h->num_cus * 8));
}


// At d = 1 a shape with lists has up to 32768 halves: 64 KiB of image beside
// the kernels' few static words, past the 64 KiB a kernel gets unasked.
void allow_lds() {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)k_compact_scan, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    (void)hipFuncSetAttribute((const void*)k_compact_pack, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    return true;
  }();
  (void)attr;
}

}  // namespace

int compact_scan(cms_handle* h, uint64_t list_mass_max, uint2* d_scan) {
  const int lw = lds_words_for(h);
  allow_lds();
  TimedScope ts(h, "compact_scan");
  hipLaunchKernelGGL(k_compact_scan, dim3(rows_grid(h)), dim3(256), sizeof(uint32_t) * (size_t)lw, h->stream, h->tview(),
                     h->d_row_mass, h->n, (int)h->p.depth, list_mass_max, lw, d_scan);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int compact_pack(cms_handle* h, const uint8_t* d_tform, const uint64_t* d_dst, uint8_t* d_payload, uint64_t payload_bytes,
                 unsigned long long* d_sum) {
  const int lw = lds_words_for(h);
  allow_lds();
  TimedScope ts(h, "compact_pack");
  if (payload_bytes) CMS_HIP(hipMemsetAsync(d_payload, 0, (size_t)payload_bytes, h->stream));
  hipLaunchKernelGGL(k_compact_pack, dim3(rows_grid(h)), dim3(256), sizeof(uint32_t) * (size_t)lw, h->stream, h->tview(),
                     h->d_row_mass, d_tform, d_dst, h->n, (int)h->p.depth, lw, d_payload, d_sum);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

}  // namespace cms
