// cms_retract.hip -- pairs taken out of a live sketch table (cms_retract,
// cms_retract_device_rows): DoubleCountMinSketch.update(key, -val) for pairs
// that were ingested, so the table is the remaining stream's, counter for
// counter.  The reference states removals and changed values in
// FileDataModel's update files (T/impl/model/file/FileDataModel.java:493-527)
// and rebuilds every sketch; cms_subtract_table takes a whole saved image out.
// This path costs what the batch costs: no kernel here sweeps the table's
// counters and no buffer of table size exists -- only O(num_owners) passes
// over per-owner scalars (pair counts, offsets, batch masses) and O(pairs x
// depth) counter reads and writes.
//
// Grouping by owner: a batch of kPartitionPairs pairs or more goes through
// partition_to_csr, the route k_ingest_sorted uses; a smaller one through a
// counting sort of its own (k_retract_count, a scan, k_retract_scatter: three
// small launches instead of the partition's fifteen, and per-owner atomics
// that a small batch does not contend on).  Then
//   k_retract_plan     per owner: its run class, from its pair count
//   k_retract_wave<W>  runs of <= kRetractWaveRun pairs, one wave per owner:
//                      a lane holds a pair and its bucket of sketch row i,
//                      equal buckets are combined across the wave
//                      (retract_combine), the leader of each bucket compares
//                      the summed decrement with the live counter
//                      (TableView::get: any form, lists included) -- work
//                      proportional to pairs x depth, independent of w
//   k_retract_image<W> longer runs, one workgroup per owner: an LDS image of
//                      decrements -- all d sketch rows at once when d x w
//                      counters fit kImageWords, so the run is read and hashed
//                      once; else as many rows (or, past kImageWords buckets,
//                      as wide a tile of one row) as fit -- filled with LDS
//                      atomics, then swept over its non-zero buckets
// W = false is the check, and stores nothing to the table.  The MASS rule
// first: the run's summed decrement (a wave or workgroup reduction, kept in
// delta[] for the write pass) against row_mass; an owner that fails it is
// reported (64-bit atomicMin of its row) and skipped, so every sum the COUNTER
// rule then forms is below 2^32.  Only when both rules hold for the whole
// batch does anything change: the live list rows that lose entries are
// rewritten densely (widen_rows, as the subtraction does), the owners are
// marked for cms_top_k_refresh, and W = true takes each combined decrement out
// with one table_sub and the run's mass out of row_mass.  The check passed on
// the sums, so no borrow crosses a packed field and lanes that share a word
// subtract safely.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "cms_device.h"
#include "cms_internal.h"
#include "cms_retract.h"

namespace cms {

namespace {

static_assert(kRetractBadRow == kFlagBadRow && kRetractBadValue == kFlagBadValue, "the ingest's flag bits");

constexpr int64_t kPartitionPairs = 32768;  // from here on the partition groups the batch (as ingest_coo_device's sorted path)
constexpr int kImageWords = 24576;          // u32 counters of one LDS image (96 KiB)
constexpr int kImageThreads = 1024;

// out[] of a call (u64 words)
enum : int { kOutFlags = 0, kOutMassRow = 1, kOutCounterRow = 2, kOutLists = 3, kOutWave = 4, kOutImage = 5, kOutWords = 6 };
enum : unsigned long long { kBadMass = 1, kBadCounter = 2, kAnyMass = 4 };

// counter c of row r -= dec: the sibling of table_add (cms_ingest.hip).  A
// packed form takes dec << shift off the aligned word with one atomic; the
// caller's check bounded dec by the field's value, so no borrow leaves it.
__device__ __forceinline__ void table_sub(const TableView& tv, int64_t r, int64_t c, uint32_t dec) {
  const int32_t s = tv.hidx[r];
  if (s >= 0) {
    atomicSub(tv.hot + (int64_t)s * tv.dw + c, dec);
    return;
  }
  if (s == kFormList) return;  // (widen_rows rewrote every list row that loses entries)
  if (s == kFormU16) {
    const int64_t g = tv.base(r) + c;  // (the row's base is even: 64-B aligned)
    atomicSub(reinterpret_cast<uint32_t*>(tv.t16) + (g >> 1), dec << ((uint32_t)(g & 1) << 4));
    return;
  }
  uint32_t* w32 = reinterpret_cast<uint32_t*>(tv.row16(r));
  if (s == kFormU8) atomicSub(w32 + (c >> 2), dec << ((uint32_t)(c & 3) << 3));
  else if (s == kFormU2) atomicSub(w32 + (c >> 4), dec << ((uint32_t)(c & 15) << 1));
  else if (s == kFormU1) atomicSub(w32 + (c >> 5), dec << (uint32_t)(c & 31));
  else atomicSub(w32 + (c >> 3), dec << ((uint32_t)(c & 7) << 2));
}

__global__ void k_retract_validate(const int64_t* rows, const float* val, int64_t np, int64_t nrows, int fb,
                                   uint32_t* flags) {
  uint32_t f = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x)
    f |= retract_validate_pair(rows, val, i, nrows, fb);
  if (f) atomicOr(flags, f);
}

// ---- the counting sort of a small batch (rows are validated: every row is in [0, nrows)) ----

__global__ void k_retract_count(const int64_t* row, int64_t np, uint32_t* cnt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&cnt[row[i]], 1u);
}

// cnt[r] pairs of owner r land in perm[off[r], off[r + 1]): k_retract_count
// counted exactly the pairs this kernel places, so every slot is inside the range
__global__ void k_retract_scatter(const int64_t* row, int64_t np, const uint32_t* off, uint32_t* cnt, uint32_t* perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = row[i];
    const uint32_t k = atomicSub(&cnt[r], 1u);  // k in [1, count]
    const uint32_t pos = off[r] + k - 1u;
    if (k >= 1u && pos < off[r + 1]) perm[pos] = (uint32_t)i;
  }
}

// The batch grouped by owner: owner r's pairs are positions [lo(r), hi(r)).
// Behind the partition a position is a pair of the grouped arrays (tokens in
// keys.tok, values in val); behind the counting sort it names a pair of the
// caller's arrays through perm.
struct Batch {
  const int64_t* off64;   // partition_to_csr's offsets [n + 1], or null
  const uint32_t* off32;  // the counting sort's offsets [n + 1]
  const uint32_t* perm;   // the counting sort's order (null behind the partition)
  Keys keys;
  const float* val;
  __device__ __forceinline__ int64_t lo(int64_t r) const { return off64 ? off64[r] : (int64_t)off32[r]; }
  __device__ __forceinline__ int64_t hi(int64_t r) const { return off64 ? off64[r + 1] : (int64_t)off32[r + 1]; }
  __device__ __forceinline__ int64_t pair(int64_t p) const { return perm ? (int64_t)perm[p] : p; }
};

// Each workgroup appends its owners to the two run lists with one atomic per
// list (one atomic per owner on one word costs more than the runs themselves).
__global__ __launch_bounds__(256) void k_retract_plan(int64_t n, Batch b, int32_t* wave_list, int32_t* image_list,
                                                      unsigned long long* out) {
  __shared__ uint32_t scr[256 / 64 + 1];
  __shared__ unsigned long long s_base[2];
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {  // (uniform)
    const int64_t r = base + threadIdx.x;
    const int64_t c = r < n ? b.hi(r) - b.lo(r) : 0;
    const uint32_t is_wave = c > 0 && c <= kRetractWaveRun, is_image = c > kRetractWaveRun;
    uint32_t tot_w, tot_i;
    const uint32_t at_w = block_excl_scan_u32(is_wave, scr, &tot_w);
    const uint32_t at_i = block_excl_scan_u32(is_image, scr, &tot_i);
    if (threadIdx.x == 0) {
      s_base[0] = tot_w ? atomicAdd(out + kOutWave, (unsigned long long)tot_w) : 0ULL;
      s_base[1] = tot_i ? atomicAdd(out + kOutImage, (unsigned long long)tot_i) : 0ULL;
    }
    __syncthreads();
    if (is_wave) wave_list[s_base[0] + at_w] = (int32_t)r;
    if (is_image) image_list[s_base[1] + at_i] = (int32_t)r;
    __syncthreads();  // s_base is read before the next round sets it
  }
}

// After the check pass: whether any run takes anything out, and how many live
// list rows lose entries (one atomic per wave that has something to say).
__global__ void k_retract_summary(int64_t n, const uint64_t* delta, const int32_t* hidx, unsigned long long* out) {
  uint32_t lists = 0, any = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    if (delta[r] == 0) continue;
    any = 1;
    lists += hidx[r] == kFormList;
  }
  lists = wave_sum_u32(lists);
  any = wave_sum_u32(any);
  if ((threadIdx.x & 63) == 0) {
    if (any) atomicOr(out + kOutFlags, (unsigned long long)kAnyMass);
    if (lists) atomicAdd(out + kOutLists, (unsigned long long)lists);
  }
}

// the widening of the live list rows that lose entries: bound = the row's own
// mass (widen_rows then picks the narrowest dense form that holds it), 0 for
// every other row (not listed)
__global__ void k_retract_list_bounds(int64_t n, const uint64_t* delta, const uint64_t* mass, const int32_t* hidx,
                                      uint64_t* bound, uint32_t* cbound) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const bool hit = delta[r] != 0 && hidx[r] == kFormList;
    bound[r] = hit ? mass[r] : 0ULL;
    if (hit) cbound[r] = 0u;
  }
}

// The mass rule of one run, by its first lane / thread (mass: the run's summed
// decrement; live null: an empty handle, every live mass is 0).  Returns
// whether the counter rule may go on with this run.
__device__ __forceinline__ bool mass_rule(int64_t r, uint64_t mass, const uint64_t* live, uint64_t* delta,
                                          unsigned long long* out, bool first) {
  const bool ok = mass <= (live ? live[r] : 0ULL);
  if (first) {
    delta[r] = mass;
    if (!ok) {  // (a refusal: the only atomics of the rule)
      atomicOr(out + kOutFlags, (unsigned long long)kBadMass);
      atomicMin(out + kOutMassRow, (unsigned long long)r);
    }
  }
  return ok && mass != 0;
}

template <bool kWrite>
__global__ __launch_bounds__(256) void k_retract_wave(const int32_t* list, const unsigned long long* count_p, Batch b,
                                                      HashParams hp, TableView tv, uint64_t* row_mass, uint64_t* delta,
                                                      unsigned long long* out) {
  const int lane = threadIdx.x & 63;
  const int64_t count = (int64_t)*count_p;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t idx = wave; idx < count; idx += nwaves) {  // (uniform across the wave)
    const int64_t r = list[idx];
    const int64_t p0 = b.lo(r);
    const int c = (int)min(b.hi(r) - p0, (int64_t)kRetractWaveRun);
    uint32_t dec = 0;
    uint64_t kp = 0;
    if (lane < c) {
      const int64_t pi = b.pair(p0 + lane);
      retract_dec(b.val, pi, hp.frac_bits, dec);
      kp = b.keys.at(pi);
    }
    if (kWrite) {
      if (delta[r] == 0) continue;  // every value of the run is zero
    } else {
      uint64_t mass = dec;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mass += __shfl_xor(mass, o, 64);
      if (!mass_rule(r, mass, row_mass, delta, out, lane == 0)) continue;
    }
    bool bad = false;
    for (int i = 0; i < hp.depth; ++i) {
      const uint32_t bk = lane < c ? bucket(hp, i, kp) : 0xFFFFFFFFu;
      uint64_t sum;
      const bool leader = retract_combine(
          lane, bk, c, [&](int s) { return (uint32_t)__shfl((int)bk, s, 64); },
          [&](int s) { return (uint32_t)__shfl((int)dec, s, 64); }, sum);
      if (lane < c && leader && sum != 0 && bk < hp.width) {
        const int64_t cell = (int64_t)i * hp.width + bk;
        if (kWrite) table_sub(tv, r, cell, (uint32_t)sum);
        else if (retract_under(sum, tv.get(r, cell))) bad = true;
      }
    }
    if (kWrite) {
      if (lane == 0) row_mass[r] -= delta[r];
    } else if (bad) {
      atomicOr(out + kOutFlags, (unsigned long long)kBadCounter);
      atomicMin(out + kOutCounterRow, (unsigned long long)r);
    }
  }
}

// rows: sketch rows per image (rows x tw <= kImageWords); tw: the image's
// buckets per sketch row (w, or a tile of kImageWords of a wider row).
template <bool kWrite>
__global__ __launch_bounds__(kImageThreads) void k_retract_image(const int32_t* list, const unsigned long long* count_p,
                                                                 Batch b, HashParams hp, TableView tv, uint64_t* row_mass,
                                                                 uint64_t* delta, unsigned long long* out, int rows,
                                                                 uint32_t tw) {
  extern __shared__ uint32_t img[];  // [rows][tw]
  __shared__ uint64_t red[kImageThreads / 64];
  const int64_t count = (int64_t)*count_p;
  const uint32_t w = hp.width;
  for (int64_t idx = blockIdx.x; idx < count; idx += gridDim.x) {
    const int64_t r = list[idx];
    const int64_t p0 = b.lo(r), c = b.hi(r) - p0;
    if (kWrite) {
      if (delta[r] == 0) continue;  // (uniform: one value for the workgroup)
    } else {
      uint64_t part = 0;
      for (int64_t j = threadIdx.x; j < c; j += kImageThreads) {
        uint32_t dec;
        retract_dec(b.val, b.pair(p0 + j), hp.frac_bits, dec);
        part = sat_add(part, (uint64_t)dec);
      }
      const uint64_t mass = block_sum_u64_sat(part, red);  // (the same sum in every thread)
      if (!mass_rule(r, mass, row_mass, delta, out, threadIdx.x == 0)) continue;
    }
    bool bad = false;
    for (int i0 = 0; i0 < hp.depth; i0 += rows) {
      const int nr = min(rows, hp.depth - i0);
      for (uint32_t t0 = 0; t0 < w; t0 += tw) {
        const uint32_t cw = min(w - t0, tw);
        for (uint32_t j = threadIdx.x; j < (uint32_t)nr * tw; j += kImageThreads) img[j] = 0u;
        __syncthreads();
        for (int64_t j = threadIdx.x; j < c; j += kImageThreads) {
          const int64_t pi = b.pair(p0 + j);
          uint32_t dec;
          retract_dec(b.val, pi, hp.frac_bits, dec);
          if (dec == 0) continue;
          const uint64_t kp = b.keys.at(pi);
          for (int ii = 0; ii < nr; ++ii) {
            const uint32_t e = bucket(hp, i0 + ii, kp);
            if (e < w && e >= t0 && e - t0 < cw) atomicAdd(&img[(uint32_t)ii * tw + (e - t0)], dec);
          }
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < (uint32_t)nr * tw; j += kImageThreads) {
          const uint32_t sum = img[j];
          if (sum == 0) continue;
          const uint32_t ii = j / tw, col = j - ii * tw;
          if (col >= cw) continue;
          const int64_t cell = (int64_t)(i0 + (int)ii) * w + t0 + col;
          if (kWrite) table_sub(tv, r, cell, sum);
          else if (retract_under(sum, tv.get(r, cell))) bad = true;
        }
        __syncthreads();  // the sweep ends before the next image is zeroed
      }
    }
    if (kWrite) {
      if (threadIdx.x == 0) row_mass[r] -= delta[r];
    } else if (bad) {
      atomicOr(out + kOutFlags, (unsigned long long)kBadCounter);
      atomicMin(out + kOutCounterRow, (unsigned long long)r);
    }
  }
}

unsigned grid_over(int64_t items, int64_t per_block, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap));
}

long long owner_name(const cms_handle* h, unsigned long long row, bool by_id) {
  return by_id && row < h->h_owner_ids.size() ? (long long)h->h_owner_ids[(size_t)row] : (long long)row;
}

}  // namespace

int retract_validate(cms_handle* h, const int64_t* d_rows, const float* d_val, int64_t np) {
  if (np <= 0 || (!d_rows && !d_val)) return CMS_OK;
  hipLaunchKernelGGL(k_retract_validate, dim3(grid_over(np, 256, 8192)), dim3(256), 0, h->stream, d_rows, d_val, np, h->n,
                     h->hp.frac_bits, h->d_flags);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int retract_coo_device(cms_handle* h, const int64_t* d_row, const int64_t* d_key, const float* d_val, int64_t np,
                       bool by_id) {
  if (np <= 0) return CMS_OK;
  const int64_t n = h->n;
  if (np >= (int64_t(1) << 31) || n >= (int64_t(1) << 31) - 1)
    return set_error(CMS_E_PARAM, "cms_retract: a batch takes fewer than 2^31 pairs and owners (split it: each call is all-or-nothing)");
  const char* who = by_id ? "owner ID" : "owner row";
  const bool part = np >= kPartitionPairs;

  // scratch: [delta u64 n | out u64 | cnt u32 n+1] zeroed together, then the run lists and (counting sort) the
  // offsets, the scan's block sums and the grouped order
  const int64_t nb = (n + 1 + 4095) / 4096 + 1;  // scan_exclusive_u32: tiles of 4096
  const size_t o_delta = 0, o_out = o_delta + sizeof(uint64_t) * (size_t)n, o_cnt = o_out + sizeof(uint64_t) * kOutWords;
  const size_t zero_bytes = o_cnt + (part ? 0 : sizeof(uint32_t) * (size_t)(n + 1));
  const size_t o_wl = (zero_bytes + 15) & ~size_t(15), o_il = o_wl + sizeof(int32_t) * (size_t)n;
  const size_t o_off = o_il + sizeof(int32_t) * (size_t)n, o_bsum = o_off + sizeof(uint32_t) * (size_t)(n + 1);
  const size_t o_perm = o_bsum + sizeof(uint32_t) * (size_t)nb;
  const size_t total = part ? o_off : o_perm + sizeof(uint32_t) * (size_t)np;
  CMS_HIP(h->ws_retract.ensure(total));
  uint8_t* ws = h->ws_retract.as<uint8_t>();
  uint64_t* delta = reinterpret_cast<uint64_t*>(ws + o_delta);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(ws + o_out);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + o_cnt);
  int32_t* wave_list = reinterpret_cast<int32_t*>(ws + o_wl);
  int32_t* image_list = reinterpret_cast<int32_t*>(ws + o_il);
  uint32_t* off32 = reinterpret_cast<uint32_t*>(ws + o_off);
  uint32_t* bsum = reinterpret_cast<uint32_t*>(ws + o_bsum);
  uint32_t* perm = reinterpret_cast<uint32_t*>(ws + o_perm);

  unsigned long long res[kOutWords] = {};
  const unsigned gp = grid_over(np, 256, 16384), gn = grid_over(n, 256, 8192);
  int rc;
  // the image: every sketch row at once when d x w fits, else the rows (or the tile of one row) that fit
  const int64_t w = h->p.width;
  const uint32_t tw = (uint32_t)std::min<int64_t>(w, kImageWords);
  const int rows = (int)std::max<int64_t>(1, std::min<int64_t>(h->p.depth, kImageWords / tw));
  const size_t lds = sizeof(uint32_t) * (size_t)rows * tw;
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)k_retract_image<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint32_t) * kImageWords));
    (void)hipFuncSetAttribute((const void*)k_retract_image<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(uint32_t) * kImageWords));
    return true;
  }();
  (void)attr;
  Batch batch{};
  // the run counts stay on the device: the grids are sized by what the batch can hold
  const unsigned gw = grid_over(std::min(np, n), 4, (int64_t)h->num_cus * 8);
  const unsigned gi = grid_over(np / (kRetractWaveRun + 1), 1, (int64_t)h->num_cus);
  const uint64_t* live = h->empty ? nullptr : h->d_row_mass;
  const bool images = np > kRetractWaveRun;  // (a batch this small has no long run)
  auto launch = [&](bool write) -> int {
    if (write) {
      if (images)
        hipLaunchKernelGGL(k_retract_image<true>, dim3(gi), dim3(kImageThreads), lds, h->stream, image_list, out + kOutImage,
                           batch, h->hp, h->tview(), h->d_row_mass, delta, out, rows, tw);
      hipLaunchKernelGGL(k_retract_wave<true>, dim3(gw), dim3(256), 0, h->stream, wave_list, out + kOutWave, batch, h->hp,
                         h->tview(), h->d_row_mass, delta, out);
    } else {
      if (images)
        hipLaunchKernelGGL(k_retract_image<false>, dim3(gi), dim3(kImageThreads), lds, h->stream, image_list, out + kOutImage,
                           batch, h->hp, h->tview(), const_cast<uint64_t*>(live), delta, out, rows, tw);
      hipLaunchKernelGGL(k_retract_wave<false>, dim3(gw), dim3(256), 0, h->stream, wave_list, out + kOutWave, batch, h->hp,
                         h->tview(), const_cast<uint64_t*>(live), delta, out);
    }
    CMS_HIP(hipGetLastError());
    return CMS_OK;
  };
  {
    TimedScope ts(h, "retract_check");
    CMS_HIP(hipMemsetAsync(ws, 0, zero_bytes, h->stream));
    CMS_HIP(hipMemsetAsync(out + kOutMassRow, 0xFF, 2 * sizeof(uint64_t), h->stream));  // the two atomicMin words
    if (part) {
      int64_t* coff;
      uint32_t* ctok;
      float* cval;
      if ((rc = partition_to_csr(h, d_row, d_key, d_val, np, &coff, &ctok, &cval))) return rc;
      batch = Batch{coff, nullptr, nullptr, Keys{d_key, ctok}, cval};
    } else {
      hipLaunchKernelGGL(k_retract_count, dim3(gp), dim3(256), 0, h->stream, d_row, np, cnt);
      CMS_HIP(hipGetLastError());
      if ((rc = scan_exclusive_u32(h, cnt, off32, n + 1, bsum))) return rc;
      hipLaunchKernelGGL(k_retract_scatter, dim3(gp), dim3(256), 0, h->stream, d_row, np, off32, cnt, perm);
      batch = Batch{nullptr, off32, perm, Keys{d_key, nullptr}, d_val};
    }
    hipLaunchKernelGGL(k_retract_plan, dim3(gn), dim3(256), 0, h->stream, n, batch, wave_list, image_list, out);
    CMS_HIP(hipGetLastError());
    // ---- the mass rule and the counter rule: no store to the table ----
    if ((rc = launch(false))) return rc;
    hipLaunchKernelGGL(k_retract_summary, dim3(grid_over(n, 256 * 16, 256)), dim3(256), 0, h->stream, n, delta, h->d_hidx, out);
    CMS_HIP(hipGetLastError());
    CMS_HIP(hipMemcpyAsync(res, out, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    if (res[kOutFlags] & kBadMass)
      return set_error(CMS_E_OVERFLOW, "%s %lld: the batch takes out more than the owner's mass (the pairs are no part of this table's stream)",
                       who, owner_name(h, res[kOutMassRow], by_id));
    if (res[kOutFlags] & kBadCounter)
      return set_error(CMS_E_OVERFLOW, "%s %lld: a counter would fall below zero (the pairs are no part of this table's stream)",
                       who, owner_name(h, res[kOutCounterRow], by_id));
    if (!(res[kOutFlags] & kAnyMass)) return CMS_OK;  // every value was zero: nothing changes, not even the state
  }

  // ---- every check has passed: the first write follows ----
  if (res[kOutLists] != 0) {  // live list rows that lose entries are rewritten densely, as the subtraction does
    CMS_HIP(h->ws_bound.ensure(sizeof(uint64_t) * (size_t)n));
    hipLaunchKernelGGL(k_retract_list_bounds, dim3(gn), dim3(256), 0, h->stream, n, delta, h->d_row_mass, h->d_hidx,
                       h->ws_bound.as<uint64_t>(), h->d_cbound);
    CMS_HIP(hipGetLastError());
    if ((rc = widen_rows(h, h->ws_bound.as<uint64_t>(), nullptr, false))) return rc;
  }
  if (h->rf_valid && (rc = refresh_mark(h, d_row, np))) return rc;  // cms_top_k_refresh stays incremental
  {
    TimedScope ts(h, "retract_apply");
    if ((rc = launch(true))) return rc;
  }
  CMS_HIP(hipStreamSynchronize(h->stream));
  // "ingested, not finalized", the state a subtraction leaves; cms_finalize re-derives norms and row maxima
  h->norms_valid = false;
  h->finalized = false;
  h->stale_possible = true;
  return CMS_OK;
}

}  // namespace cms
