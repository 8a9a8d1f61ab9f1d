// cms_fold.hip -- the kernels that re-encode every owner row of a live u32
// table at a width w' that divides its own w: cms_fold_table (w' < w) and
// cms_compact_table (w' == w, K = w / w' = 1: nothing folds and every row is
// re-stored in its narrowest form).  DESIGN.md 4.12.
//
// The hash is ((a key + b) mod p) mod w, and (s mod w) mod w' = s mod w' for
// every divisor w' of w, so T'[r][i][j'] = the sum of T[r][i][j] over
// j = j' (mod w') is the table the same stream builds at width w'.  The driver
// (cms_checkpoint.hip fold_plan / fold_payload) scans, applies
// ckpt::compact_form and lays the payload out on the host, and packs.  Both
// kernels are one workgroup per owner row over a persistent grid and read every
// stored source byte once; neither holds a row at more than its folded width.
//
//   k_fold_scan  the folded row's largest counter (2^32 when a folded counter
//                reaches it) and whether every sketch row sums to the row mass
//                (asked only of rows small enough to become a list)
//   k_fold_pack  the folded row in its target form at its place in the payload,
//                and the payload checksum of what it stores
//
// Dense source rows into dense target rows never touch LDS.  Where
// w' % 16 == 0, folded group g (16 counters) of a sketch row is the sum of the
// source groups g + k w'/16 for k < K; a lane takes a folded group, walks its
// source groups and adds in registers.  Neighbouring lanes take neighbouring
// groups, so each step of the walk is one coalesced load across the wavefront
// (at K == 1 the walk is the row's groups flat over the lanes).  At other
// widths, which have no forms, a lane takes a folded counter the same way.
//
// A list source or a list target goes through an LDS image of the folded
// sketch row as u16 halves, (w' + 1) / 2 words and at most 64 KiB: a list has
// at most 2^16 - 1 keys and a list target a mass below that, so no folded
// counter of either passes a half.  The scan alone counts a folding list
// (K >= 2) in whole words, w' <= w / 2 of them: the half's shifts and mask sit
// on the one dependent chain of its atomic and cost fold_scan 2.6 % at
// config 3, and the words are no more LDS than the scan took before.
//
// Both kernels are compiled twice from the one source, kFolds false for
// w' == w: with K == 1 known to the compiler the accumulators of the fold are
// no registers at all, and the compaction keeps the six (scan) and four (pack)
// waves per SIMD that a run-time K costs it.
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

// The same for one counter of row r (shapes without forms: u16 and u32 rows,
// no group of 16 is whole): the sum of the source counters at j + k wf.
__device__ __forceinline__ uint32_t fold_counter(const TableView& tv, int64_t r, int64_t j, int K, int wf, bool& over) {
  uint32_t v = 0;
  for (int k = 0; k < K; ++k) {
    const uint32_t x = tv.get(r, j + (int64_t)k * wf);
    v += x;
    over |= v < x;
  }
  return v;
}

// where bucket b of a source row folds to
__device__ __forceinline__ uint32_t fold_bucket(uint32_t b, int K, int wf) { return K == 1 ? b : b % (uint32_t)wf; }

__device__ __forceinline__ uint32_t lds_half(const uint32_t* lc, int j) { return (lc[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu; }

constexpr unsigned long long kOver = 1ull << 32;  // the scan's largest counter, saturated

// out[r] = (largest folded counter of row r, saturated at 2^32 - 1; bit 0: every
// sketch row sums to the row mass -- asked only of rows whose mass is in
// [1, list_mass_max]: no other row can become a list (list_mass_max 0: none
// can) -- bit 1: a folded counter reached 2^32).  lc: lds_words zeroed words,
// the counts of a list's folded sketch row (u16 halves at K == 1, whole words
// when folding), left zeroed after every row.
template <bool kFolds>
__global__ __launch_bounds__(256) void k_fold_scan(TableView tv, const uint64_t* mass, int64_t n, int depth, int wf,
                                                   uint64_t list_mass_max, int lds_words, uint2* out) {
  extern __shared__ uint32_t lc[];
  __shared__ unsigned long long s_red[4];
  __shared__ unsigned long long s_max[4];
  const int w = tv.w;
  const int K = kFolds ? w / wf : 1;
  const int G = wf >> 4;  // folded groups per sketch row
  const bool groups = (wf & 15) == 0;
  for (int j = threadIdx.x; j < lds_words; j += 256) lc[j] = 0u;
  __syncthreads();
  auto umax = [](auto a, decltype(a) b) { return a > b ? a : b; };
  auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const RowSrc s = row_src(tv, r);  // (uniform over the workgroup)
    const uint64_t M = mass[r];
    uint32_t mx = 0, eq = 0;
    bool over = false;
    if (s.p == nullptr) {
      // the shared zero row: nothing is read
    } else if (s.f == kFormList) {
      // folded counter (rr, b) = the entries of sketch row rr congruent to b: the
      // count an entry's atomic returns, plus one, passes through every value up to it
      const uint16_t* e = reinterpret_cast<const uint16_t*>(s.p);
      const uint32_t m = e[0];
      for (int rr = 0; rr < depth; ++rr) {
        for (uint32_t t = threadIdx.x; t < m; t += 256) {
          const uint32_t b = e[1 + (uint32_t)rr * m + t], bf = fold_bucket(b, K, wf);
          const uint32_t cell = kFolds ? bf : bf >> 1, sh = kFolds ? 0u : (bf & 1u) * 16u;
          if (b < (uint32_t)w && (int)cell < lds_words)
            mx = umax(mx, ((atomicAdd(&lc[cell], 1u << sh) >> sh) & (kFolds ? ~0u : 0xFFFFu)) + 1u);
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < m; t += 256) {  // only the words the entries touched
          const uint32_t b = e[1 + (uint32_t)rr * m + t], bf = fold_bucket(b, K, wf);
          const uint32_t cell = kFolds ? bf : bf >> 1;
          if (b < (uint32_t)w && (int)cell < lds_words) lc[cell] = 0u;
        }
        __syncthreads();
      }
      eq = (uint64_t)m == M;  // every sketch row of a list has m entries
    } else {
      const bool sums = M >= 1 && M <= list_mass_max;
      bool all = sums;
      if (groups && !sums) {  // only the maximum is asked for: the folded row's d G groups flat over the lanes
        for (int i = threadIdx.x; i < depth * G; i += 256) {
          const int rr = i / G, g = i - rr * G;
          uint32_t v[16];
          over |= fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v);
#pragma unroll
          for (int q = 0; q < 16; ++q) mx = umax(mx, v[q]);
        }
      }
      for (int rr = 0; rr < depth && (sums || !groups); ++rr) {
        unsigned long long sum = 0;
        if (groups) {
          for (int g = threadIdx.x; g < G; g += 256) {
            uint32_t v[16];
            over |= fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              mx = umax(mx, v[q]);
              sum += v[q];
            }
          }
        } else {
          for (int j = threadIdx.x; j < wf; j += 256) {
            const uint32_t v = fold_counter(tv, r, (int64_t)rr * w + j, K, wf, over);
            mx = umax(mx, v);
            sum += v;
          }
        }
        if (sums) all = all && block_reduce(sum, s_red, add) == M;
      }
      eq = all;
    }
    const unsigned long long top = block_reduce(over ? kOver : (unsigned long long)mx, s_max, umax);
    if (threadIdx.x == 0) out[r] = make_uint2(top >= kOver ? 0xFFFFFFFFu : (uint32_t)top, eq | (top >= kOver ? 2u : 0u));
  }
}

// Sketch row rr of the row at s, folded to width wf, as u16 halves in
// lc[0, (wf + 1) / 2): a list's entries by atomics, a dense row (wf % 32 == 0:
// it becomes a list, and only shapes with forms have lists) a folded group at
// a time.  Ends with the workgroup synchronised.
__device__ __forceinline__ void fold_row_image(const RowSrc& s, int rr, int w, int K, int wf, uint32_t* lc) {
  if (s.f == kFormList) {
    const uint16_t* e = reinterpret_cast<const uint16_t*>(s.p);
    const uint32_t m = e[0];
    for (int j = threadIdx.x; j < ((wf + 1) >> 1); j += 256) lc[j] = 0u;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < m; t += 256) {
      const uint32_t b = e[1 + (uint32_t)rr * m + t], bf = fold_bucket(b, K, wf);
      if (b < (uint32_t)w) atomicAdd(&lc[bf >> 1], 1u << ((bf & 1u) * 16u));
    }
  } else {
    for (int g = threadIdx.x; g < (wf >> 4); g += 256) {
      uint32_t v[16];
      fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v);
#pragma unroll
      for (int q = 0; q < 8; ++q) lc[8 * g + q] = (v[2 * q] & 0xFFFFu) | (v[2 * q + 1] << 16);
    }
  }
  __syncthreads();
}

// The image as sketch row rr of the list at e (key count m): a lane takes
// consecutive buckets and writes bucket j c[j] times from its exclusive-scan
// offset, so the entries come out ascending; none is written past m, whatever
// the counters say.
__device__ __forceinline__ void emit_list(const uint32_t* lc, int wf, int rr, uint32_t m, uint16_t* e, uint32_t* s_wave,
                                          unsigned long long& acc) {
  const int chunk = (wf + 255) >> 8;
  const int j0 = min(wf, (int)threadIdx.x * chunk), j1 = min(wf, j0 + chunk);
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
}

// Row r folded to width wf in its target form tform[r] (kRow*) at payload +
// dst[r]; out[0] += the checksum of the bytes stored.  The payload was zeroed:
// pad bytes stay zero.  A list row's key count is its mass (compact_form: every
// sketch row sums to it).  lc: lds_words words.
template <bool kFolds>
__global__ __launch_bounds__(256) void k_fold_pack(TableView tv, const uint64_t* mass, const uint8_t* tform,
                                                   const uint64_t* dst, int64_t n, int depth, int wf, int lds_words,
                                                   uint8_t* payload, unsigned long long* out) {
  extern __shared__ uint32_t lc[];
  __shared__ unsigned long long s_red[4];
  __shared__ uint32_t s_wave[4];
  const int w = tv.w;
  const int K = kFolds ? w / wf : 1;
  const int G = wf >> 4;
  const bool groups = (wf & 15) == 0;
  unsigned long long acc = 0;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int tf = tform[r];  // (uniform over the workgroup, as every branch below)
    const RowSrc s = row_src(tv, r);
    if (tf == kRowZero || s.p == nullptr) continue;
    uint8_t* row = payload + dst[r];
    const int tb = target_bits(tf);
    if (s.f != kFormList && tf != kRowList) {  // dense -> dense in registers
      if (groups) {
        for (int i = threadIdx.x; i < depth * G; i += 256) {
          const int rr = i / G, g = i - rr * G;
          uint32_t v[16];
          fold_group(s, (int64_t)rr * w + 16 * g, K, wf, v);
          store_group(row, (int64_t)rr * wf + 16 * g, v, tb, acc);
        }
      } else {
        bool over = false;  // (the scan refused a row that passes 2^32)
        for (int rr = 0; rr < depth; ++rr)
          for (int j = threadIdx.x; j < wf; j += 256)
            store_counter(row, (int64_t)rr * wf + j, fold_counter(tv, r, (int64_t)rr * w + j, K, wf, over), tb, acc);
      }
      continue;
    }
    if (2 * lds_words < wf) continue;  // (the driver sends no list to a shape without the image)
    const uint32_t m = (uint32_t)mass[r];  // (a list target's key count)
    uint16_t* e = reinterpret_cast<uint16_t*>(row);
    if (tf == kRowList && threadIdx.x == 0) {
      e[0] = (uint16_t)m;
      acc += m;
    }
    for (int rr = 0; rr < depth; ++rr) {  // a sketch row at a time through the image
      fold_row_image(s, rr, w, K, wf, lc);
      if (tf == kRowList) {
        emit_list(lc, wf, rr, m, e, s_wave, acc);
      } else if (groups) {
        for (int g = threadIdx.x; g < G; g += 256) {
          uint32_t v[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) v[q] = lds_half(lc, 16 * g + q);
          store_group(row, (int64_t)rr * wf + 16 * g, v, tb, acc);
        }
      } else {
        for (int j = threadIdx.x; j < wf; j += 256) store_counter(row, (int64_t)rr * wf + j, lds_half(lc, j), tb, acc);
      }
      __syncthreads();  // the image is read before the next sketch row replaces it
    }
  }
  auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
  const unsigned long long total = block_reduce(acc, s_red, add);
  if (threadIdx.x == 0 && total) atomicAdd(out, total);
}

// Words of the image: a sketch row folded to wf as halves where a source row
// (the handle holds lists) or a target row (compact_form gives lists at shape
// (depth, wf)) can be a list, else none.
int image_words(const cms_handle* h, int32_t wf) {
  const bool source = h->forms_ok && (size_t)h->dw * 2 <= 80 * 1024;
  const bool target = h->tune.forms && wf % 32 == 0 && (size_t)h->p.depth * wf * 2 <= 80 * 1024;
  return source || target ? (wf + 1) / 2 : 0;
}

unsigned rows_grid(const cms_handle* h) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(h->n, (int64_t)h->num_cus * 8));
}

// At d = 1 a shape with lists has up to 32768 halves: 64 KiB of image beside
// the kernels' few static words, past the 64 KiB a kernel gets unasked.
void allow_lds() {
  static bool attr = [] {
    for (const void* k : {(const void*)k_fold_scan<false>, (const void*)k_fold_scan<true>, (const void*)k_fold_pack<false>,
                          (const void*)k_fold_pack<true>})
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    return true;
  }();
  (void)attr;
}

int check_width(const cms_handle* h, int32_t wf, const char* what) {
  if (wf < 1 || wf > h->p.width || h->p.width % wf) return set_error(CMS_E_PARAM, "%s: width %d", what, (int)wf);
  return CMS_OK;
}

}  // namespace

int fold_scan(cms_handle* h, int32_t wf, uint64_t list_mass_max, uint2* d_scan) {
  if (int rc = check_width(h, wf, "fold_scan")) return rc;
  // (the scan counts a folding list in whole words, wf <= w / 2 of them: no half to select on its one dependent chain)
  const int lw = wf == h->p.width ? image_words(h, wf) : 2 * image_words(h, wf);
  allow_lds();
  TimedScope ts(h, wf == h->p.width ? "compact_scan" : "fold_scan");
  hipLaunchKernelGGL(wf == h->p.width ? k_fold_scan<false> : k_fold_scan<true>, dim3(rows_grid(h)), dim3(256), sizeof(uint32_t) * (size_t)lw, h->stream, h->tview(),
                     h->d_row_mass, h->n, (int)h->p.depth, (int)wf, list_mass_max, lw, d_scan);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int fold_pack(cms_handle* h, int32_t wf, const uint8_t* d_tform, const uint64_t* d_dst, uint8_t* d_payload,
              uint64_t payload_bytes, unsigned long long* d_sum) {
  if (int rc = check_width(h, wf, "fold_pack")) return rc;
  const int lw = image_words(h, wf);
  allow_lds();
  TimedScope ts(h, wf == h->p.width ? "compact_pack" : "fold_pack");
  if (payload_bytes) CMS_HIP(hipMemsetAsync(d_payload, 0, (size_t)payload_bytes, h->stream));
  hipLaunchKernelGGL(wf == h->p.width ? k_fold_pack<false> : k_fold_pack<true>, dim3(rows_grid(h)), dim3(256), sizeof(uint32_t) * (size_t)lw, h->stream, h->tview(),
                     h->d_row_mass, d_tform, d_dst, h->n, (int)h->p.depth, (int)wf, lw, d_payload, d_sum);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

}  // namespace cms
