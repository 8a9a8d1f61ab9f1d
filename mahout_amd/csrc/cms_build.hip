// cms_build.hip -- LDS-staged sketch-row build (the sketch-update hot kernel).
//
// Input: CSR keys grouped by owner row (the DataModel layout, or the output of
// the COO partition in cms_ingest.hip).  One workgroup builds one owner's
// d x w sketch one sketch row at a time in LDS:
//   - the owner's keys are read once (cached in registers across the d sketch
//     rows when the owner has <= 1024 keys, otherwise streamed in batches of
//     four loads per thread) and reduced mod p once;
//   - every update of sketch row r is an LDS atomic add at h_r(key)
//     (DoubleCountMinSketch.update, T/impl/common/DoubleCountMinSketch.java:72-80);
//   - the finished row leaves LDS as 16-byte coalesced stores, the same pass
//     zeroes the LDS slot for row r+1 and accumulates sum(c^2) (the valueA of
//     DoubleCountMinSketch.cosine :131-138) -- so the table is written exactly
//     once, zero fill included, and the norms cost no extra HBM pass.
// Hot owners (more than kSlice keys) are split into slices built by separate
// workgroups; a slice adds its LDS row into the (pre-zeroed) table row with
// 256-byte coalesced atomics and a small pass derives the hot rows' norms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "cms_device.h"
#include "cms_internal.h"

namespace cms {

#ifdef CMS_BUILD_CHEAPHASH  // bound analysis only: a trivial hash instead of the exact mod-p one
#define bucket(hp, d, kp) ((uint32_t)(((kp) >> (d)) & (hp).wmask))
#endif
#ifdef CMS_BUILD_GATHERHASH  // bound analysis only: the row's bucket gathered from a per-key table
#define bucket(hp, d, kp) \
  ((uint32_t)(((&(hp).gtab[(kp) & 0xFFFFFFu].x)[((d) >> 1) & 3] >> (((d) & 1) << 4)) & (hp).wmask))
#endif

struct HotInfo {
  int64_t row;
  int32_t nslices;
  int32_t e0;  // first extra slice (extra_map index) of the row
};

constexpr int kKeyRegs = 4;

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));  // keys cached per thread: owners up to 1024 keys are read once

// 8 byte counters (each < 16) of two words -> 8 nibbles, counter k in bits 4k:
// x | x >> 4 puts counters 0|1 in byte 0 and 2|3 in byte 2; one v_perm_b32
// gathers bytes 0 and 2 of both words.
__device__ __forceinline__ uint32_t nibbles8(uint32_t lo, uint32_t hi) {
  return __builtin_amdgcn_perm(hi | (hi >> 4), lo | (lo >> 4), 0x06040200u);
}

// Rows with more than `split` keys are hot (u32 slot, built in slices of
// `slice` keys); slices [first, ns) of each are listed in extra_map (first =
// 1: slice 0 is built by the row's own k_build_rows block; first = 0: every
// slice by k_build_slices).
__global__ void k_build_plan(const int64_t* lo_, const int64_t* hi_, int64_t nrows, int64_t split, int64_t slice,
                             int first, int32_t* row_hot, HotInfo* hot, int2* extra_map,
                             uint32_t* counters /* [0]=hot rows [1]=mapped slices */, uint64_t* norm, uint32_t* rowmax,
                             int depth) {
  const int lane = (int)__lane_id();
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < nrows; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = base + threadIdx.x;
    const int64_t c = r < nrows ? hi_[r] - lo_[r] : 0;
    const bool is_hot = c > split;
    if (r < nrows && !is_hot) row_hot[r] = -1;
    int32_t ns = 0;
    uint32_t hidx = 0, e0 = 0;
    if (is_hot) {
      ns = (int32_t)((c + slice - 1) / slice);
      // one 64-bit atomic claims the hot index (low word) and the mapped slices (high word)
      const unsigned long long old =
          atomicAdd(reinterpret_cast<unsigned long long*>(counters), ((unsigned long long)(ns - first) << 32) | 1ULL);
      hidx = (uint32_t)old;
      e0 = (uint32_t)(old >> 32);
      hot[hidx] = HotInfo{r, ns, (int32_t)e0};
      row_hot[r] = (int32_t)hidx;
      for (int d = 0; d < depth; ++d) norm[r * depth + d] = 0;
      rowmax[r] = 0;
    }
    // the wave writes each hot row's slice map together (a Zipf head row has
    // hundreds of slices)
    unsigned long long m = __ballot(is_hot);
    while (m) {
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      const int32_t nsl = __builtin_amdgcn_readlane(ns, l);
      const uint32_t hl = (uint32_t)__builtin_amdgcn_readlane((int)hidx, l);
      const uint32_t el = (uint32_t)__builtin_amdgcn_readlane((int)e0, l);
      for (int32_t sl = first + lane; sl < nsl; sl += 64) extra_map[el + sl - first] = make_int2((int)hl, sl);
    }
  }
}

// Upper bound of every counter of each row after the coming build (the row's
// mass in counter units, old mass included when accumulating), and the rows
// whose keys are split over several workgroups (their slices add with u32
// atomics): both need a hot slot before the launch.
__global__ void k_row_bound_implicit(const int64_t* lo_, const int64_t* hi_, int64_t nrows, int fb, int64_t slice, const uint64_t* old_mass,
                                     uint64_t* bound, uint8_t* force) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = hi_[r] - lo_[r];
    bound[r] = ((uint64_t)c << fb) + (old_mass ? old_mass[r] : 0ULL);
    force[r] = c > slice ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_row_bound_values(const int64_t* lo_, const int64_t* hi_, const float* vals, int64_t nrows, int fb,
                                                          int64_t slice, const uint64_t* old_mass, uint64_t* bound,
                                                          uint8_t* force) {
  __shared__ uint64_t red[4];
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    uint64_t s = 0;
    for (int64_t i = lo_[r] + threadIdx.x; i < hi_[r]; i += 256) {
      uint32_t inc;
      if (load_inc(vals, i, inc, fb)) s += inc;  // bad values are flagged by the build itself
    }
    s = block_sum_u64_sat(s, red);
    if (threadIdx.x == 0) {
      bound[r] = sat_add(s, old_mass ? old_mass[r] : 0ULL);
      force[r] = (hi_[r] - lo_[r]) > slice ? 1 : 0;
    }
  }
}

// An owner of a fresh build whose every counter is provably below 2^8 (its
// mass bound) and whose keys fit the register cache: built whole in LDS by
// k_build_lists / k_build_nibbles / k_build_bytes (not by k_build_rows).
constexpr int64_t kByteKeys = 64 * kKeyRegs;  // one wave's register cache (k_build_nibbles)
__device__ __forceinline__ bool byte_class(int32_t slot, int64_t nkeys, uint64_t bound) {
  return slot < 0 && nkeys <= kByteKeys && bound < 256;
}

// grid = emax + nrows: blocks [0, emax) build extra slices of hot owners (heavy
// work first), blocks [emax, emax + nrows) one owner each (slice 0 if hot).
// Store form of the narrow rows' write-out: 0 = 8-B stores (4 counters per
// lane), 1 = 16-B stores (8 counters per lane), 2 = 16-B non-temporal stores.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_row(uint4* p, uint4 v, int sv) {
  if (sv == 2) {
    const u32x4_t x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<u32x4_t*>(p));
  } else {
    *p = v;
  }
}

#ifdef CMS_NO_SLICE_PAIRS
constexpr bool kNoSlicePairs = true;
#else
constexpr bool kNoSlicePairs = false;
#endif
constexpr int kBuildStoreForm = 2;
constexpr size_t kFormLdsMax = 64 * 1024;  // byte-form owners: [d][w] bytes of LDS per workgroup  // 16-B non-temporal: config-3 build 20.4 -> 19.4 ms, config 2 ~1% (scripts/store_ab.sh)

// waves per SIMD the row and mid builds are compiled for: 6 (up to 80 VGPRs,
// no spills) -- at 8 (64 VGPRs) both spilled a few registers and the config-3
// build scope took 7.21-7.25 ms against 6.80-6.82 ms at 6 (6.88-6.94 at 7)
constexpr int kBuildWaves = 6;
template <int SV>
__global__ __launch_bounds__(kBuildThreads) __attribute__((amdgpu_waves_per_eu(kBuildWaves, 8))) void k_build_rows(
    const int64_t* lo_, const int64_t* hi_, Keys keys, const float* vals, int64_t nrows, HashParams hp,
    int64_t slice,
    const int32_t* row_hot, const HotInfo* hot, const int2* extra_map, const uint32_t* counters, int64_t emax,
    TableView tv, uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax, uint32_t* flags, int accumulate,
    int slices_done, const uint64_t* bound, int forms, int skip_untouched, int32_t* hidx_w, uint32_t* cbound,
    const int32_t* rows_list, const uint32_t* rows_cnt) {
  extern __shared__ __align__(16) uint32_t lds[];  // one sketch row [w] u32, or a byte-form owner's [d][w] u8
  __shared__ unsigned long long s_norm[CMS_MAX_DEPTH];
  __shared__ unsigned long long s_mass;
  __shared__ uint32_t s_max;  // largest counter of the row (limb count of the all-pairs operands)
  const int w = (int)hp.width;
  const int64_t dw = (int64_t)hp.depth * w;
  const int tid = threadIdx.x;

  int64_t row, lo, hi;
  bool atomic_mode;
  if (blockIdx.x < emax) {
    if (slices_done || blockIdx.x >= counters[1]) return;  // slices_done: k_build_slices built them
#ifdef CMS_BUILD_NOSLICES  // bound analysis only: hot rows' extra slices skipped
    return;
#endif
    int2 m = extra_map[blockIdx.x];
    row = hot[m.x].row;
    lo = lo_[row] + (int64_t)m.y * slice;
    hi = min(hi_[row], lo + slice);
    atomic_mode = true;
  } else {
    row = (int64_t)blockIdx.x - emax;
    if (rows_list) {  // only the listed rows (the slot rows; the others have kernels of their own)
      if (row >= (int64_t)*rows_cnt) return;
      row = rows_list[row];
    }
    lo = lo_[row];
    atomic_mode = row_hot[row] >= 0;
    if (atomic_mode && slices_done) return;  // a split row: all its slices ran in k_build_slices
    hi = atomic_mode ? lo + slice : hi_[row];
    // accumulating into a live table with current norms: a row without keys
    // keeps its counters, norms and form (a form row may only be touched
    // after widen_rows made it u16)
    if (skip_untouched && hi_[row] == lo) return;
  }
#ifdef CMS_BUILD_NOKEYS  // bound analysis only: the write path alone
  hi = lo;
#endif
  // a hot row (slot) is u32, any other row u16 (promote_rows ran before the launch)
  const int32_t slot = tv.hidx[row];
  uint32_t* dst = slot >= 0 ? tv.hot + (int64_t)slot * dw : nullptr;
  uint16_t* dst16 = tv.row16(row);
  const bool load_old = accumulate && !atomic_mode;
  if (tid < CMS_MAX_DEPTH) s_norm[tid] = 0ULL;
  if (tid == 0) {
    s_mass = 0ULL;
    s_max = 0u;
  }
  uint32_t vmax = 0;

  // keys of small owners: read and reduced once for all d sketch rows
  const bool cached = (hi - lo) <= (int64_t)kBuildThreads * kKeyRegs;
  // Byte forms: a fresh narrow owner whose mass (so every counter) stays
  // below 2^8 is built by k_build_nibbles (4-bit rows) or, when a counter
  // reaches 16, by k_build_bytes (u8 rows) -- both launched after this kernel.
  if (forms && !atomic_mode && !load_old && byte_class(slot, hi - lo, bound[row])) return;
  uint64_t kp[kKeyRegs];
  uint32_t ik[kKeyRegs];
  uint64_t mass = 0;
  bool badv = false;
  if (cached) {
#pragma unroll
    for (int k = 0; k < kKeyRegs; ++k) {
      int64_t i = lo + tid + (int64_t)k * kBuildThreads;
      kp[k] = 0;
      ik[k] = 0;
      if (i < hi) {
        uint32_t inc;
        if (!load_inc(vals, i, inc, hp.frac_bits)) {
          badv = true;
          inc = 0;
        }
        kp[k] = keys.at(i);
        ik[k] = inc;
        mass += inc;
      }
    }
  }
  {
  // LDS slot for sketch row 0 (the old counters when accumulating)
  for (int j = tid; j < w; j += kBuildThreads) lds[j] = load_old ? (dst ? dst[j] : (uint32_t)dst16[j]) : 0u;
  __syncthreads();

  // Narrow rows of a fresh build pair their sketch rows: every counter of such
  // a row is below 2^16 (promote_rows guarantees it), so row d counts in the
  // low and row d+1 in the high half of the same LDS word without a carry
  // between them -- d = 5 takes three update/write-out phases instead of five.
  // A slice of a split (hot) row with unit increments counts at most
  // slice << frac_bits < 2^16 per bucket, so it pairs its sketch rows the same
  // way and walks its (uncached) keys ceil(d/2) times instead of d times.
  const bool slice_pairs = atomic_mode && !vals && (slice << hp.frac_bits) < 65536 && !kNoSlicePairs;
  const bool pair_rows = ((!dst && !load_old && !atomic_mode) || slice_pairs) && (w & 3) == 0;
  for (int d = 0; d < hp.depth;) {
    const bool two = pair_rows && d + 1 < hp.depth;
    // ---- updates of sketch row d (and d+1) ----
    if (cached) {
#pragma unroll
      for (int k = 0; k < kKeyRegs; ++k)
        if (ik[k]) {
          atomicAdd(&lds[bucket(hp, d, kp[k])], ik[k]);
          if (two) atomicAdd(&lds[bucket(hp, d + 1, kp[k])], ik[k] << 16);
        }
    } else {
      for (int64_t base = lo; base < hi; base += 4 * kBuildThreads) {
        uint64_t kk[4];
        uint32_t inc4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int64_t i = base + tid + (int64_t)u * kBuildThreads;
          kk[u] = i < hi ? keys.at(i) : 0;
          inc4[u] = 0;
          if (i < hi) {
            uint32_t inc;
            if (!load_inc(vals, i, inc, hp.frac_bits)) {
              badv = true;
              inc = 0;
            }
            inc4[u] = inc;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (inc4[u]) {
            const uint64_t kr = kk[u];
            atomicAdd(&lds[bucket(hp, d, kr)], inc4[u]);
            if (two) atomicAdd(&lds[bucket(hp, d + 1, kr)], inc4[u] << 16);
          }
          if (d == 0) mass += inc4[u];
        }
      }
    }
    lds_barrier();  // LDS order only: the write-out stores stay in flight
    // ---- write-out of row d, zero/load the slot for row d+1, sum of squares ----
    const int64_t rofs = (int64_t)d * w;
    const bool more = load_old && d + 1 < hp.depth;
    if (atomic_mode && two) {  // paired slice rows: low halves row d, high halves row d + 1
      for (int j = tid; j < w; j += kBuildThreads) {
        const uint32_t v = lds[j];
        lds[j] = 0u;
        if (v & 0xFFFFu) atomicAdd(dst + rofs + j, v & 0xFFFFu);
        if (v >> 16) atomicAdd(dst + rofs + w + j, v >> 16);
      }
    } else if (atomic_mode) {  // slices of a split row: always a hot (u32) row
      for (int j = tid; j < w; j += kBuildThreads) {
        uint32_t v = lds[j];
        lds[j] = 0u;
#ifdef CMS_BUILD_NOSLICEADD  // bound analysis only: the slices' global atomics skipped
        if (v == 0xFFFFFFFFu)
#endif
        if (v) atomicAdd(dst + rofs + j, v);
      }
    } else if (two && SV > 0 && (w & 7) == 0) {
      // as below, 8 counters (16 B) per lane and row per store
      uint4* l4 = reinterpret_cast<uint4*>(lds);
      uint4* da = reinterpret_cast<uint4*>(dst16 + rofs);
      uint4* db = reinterpret_cast<uint4*>(dst16 + rofs + w);
      uint32_t sqa = 0, sqb = 0;
      u16x2 pm = {0, 0};
      for (int j = tid; j < (w >> 3); j += kBuildThreads) {
        const uint4 v = l4[2 * j], u = l4[2 * j + 1];
        l4[2 * j] = make_uint4(0, 0, 0, 0);
        l4[2 * j + 1] = make_uint4(0, 0, 0, 0);
        const uint32_t a0 = __builtin_amdgcn_perm(v.y, v.x, 0x05040100u), a1 = __builtin_amdgcn_perm(v.w, v.z, 0x05040100u);
        const uint32_t a2 = __builtin_amdgcn_perm(u.y, u.x, 0x05040100u), a3 = __builtin_amdgcn_perm(u.w, u.z, 0x05040100u);
        const uint32_t b0 = __builtin_amdgcn_perm(v.y, v.x, 0x07060302u), b1 = __builtin_amdgcn_perm(v.w, v.z, 0x07060302u);
        const uint32_t b2 = __builtin_amdgcn_perm(u.y, u.x, 0x07060302u), b3 = __builtin_amdgcn_perm(u.w, u.z, 0x07060302u);
        store_row(da + j, make_uint4(a0, a1, a2, a3), SV);
        store_row(db + j, make_uint4(b0, b1, b2, b3), SV);
        const u16x2 pa0 = __builtin_bit_cast(u16x2, a0), pa1 = __builtin_bit_cast(u16x2, a1);
        const u16x2 pa2 = __builtin_bit_cast(u16x2, a2), pa3 = __builtin_bit_cast(u16x2, a3);
        const u16x2 pb0 = __builtin_bit_cast(u16x2, b0), pb1 = __builtin_bit_cast(u16x2, b1);
        const u16x2 pb2 = __builtin_bit_cast(u16x2, b2), pb3 = __builtin_bit_cast(u16x2, b3);
        sqa = __builtin_amdgcn_udot2(pa0, pa0, sqa, false);
        sqa = __builtin_amdgcn_udot2(pa1, pa1, sqa, false);
        sqa = __builtin_amdgcn_udot2(pa2, pa2, sqa, false);
        sqa = __builtin_amdgcn_udot2(pa3, pa3, sqa, false);
        sqb = __builtin_amdgcn_udot2(pb0, pb0, sqb, false);
        sqb = __builtin_amdgcn_udot2(pb1, pb1, sqb, false);
        sqb = __builtin_amdgcn_udot2(pb2, pb2, sqb, false);
        sqb = __builtin_amdgcn_udot2(pb3, pb3, sqb, false);
        const u16x2 ma = __builtin_elementwise_max(__builtin_elementwise_max(pa0, pa1), __builtin_elementwise_max(pa2, pa3));
        const u16x2 mb = __builtin_elementwise_max(__builtin_elementwise_max(pb0, pb1), __builtin_elementwise_max(pb2, pb3));
        pm = __builtin_elementwise_max(pm, __builtin_elementwise_max(ma, mb));
      }
      vmax = max(vmax, max((uint32_t)pm.x, (uint32_t)pm.y));
      sqa = wave_sum_u32(sqa);
      sqb = wave_sum_u32(sqb);
      if ((tid & 63) == 0) {
        atomicAdd(&s_norm[d], (unsigned long long)sqa);
        atomicAdd(&s_norm[d + 1], (unsigned long long)sqb);
      }
    } else if (two) {
      // rows d and d+1 leave LDS together; squares by v_dot2_u32_u16 on the
      // packed store words: a narrow row's sum of squares is at most
      // mass * max < 2^32, so u32 partial sums are exact
      uint4* l4 = reinterpret_cast<uint4*>(lds);
      uint2* da = reinterpret_cast<uint2*>(dst16 + rofs);
      uint2* db = reinterpret_cast<uint2*>(dst16 + rofs + w);
      uint32_t sqa = 0, sqb = 0;
      u16x2 pm = {0, 0};
      for (int j = tid; j < (w >> 2); j += kBuildThreads) {
        const uint4 v = l4[j];
        l4[j] = make_uint4(0, 0, 0, 0);
        const uint32_t a0 = __builtin_amdgcn_perm(v.y, v.x, 0x05040100u), a1 = __builtin_amdgcn_perm(v.w, v.z, 0x05040100u);
        const uint32_t b0 = __builtin_amdgcn_perm(v.y, v.x, 0x07060302u), b1 = __builtin_amdgcn_perm(v.w, v.z, 0x07060302u);
        da[j] = make_uint2(a0, a1);
        db[j] = make_uint2(b0, b1);
        const u16x2 pa0 = __builtin_bit_cast(u16x2, a0), pa1 = __builtin_bit_cast(u16x2, a1);
        const u16x2 pb0 = __builtin_bit_cast(u16x2, b0), pb1 = __builtin_bit_cast(u16x2, b1);
        sqa = __builtin_amdgcn_udot2(pa0, pa0, sqa, false);
        sqa = __builtin_amdgcn_udot2(pa1, pa1, sqa, false);
        sqb = __builtin_amdgcn_udot2(pb0, pb0, sqb, false);
        sqb = __builtin_amdgcn_udot2(pb1, pb1, sqb, false);
        pm = __builtin_elementwise_max(pm, __builtin_elementwise_max(__builtin_elementwise_max(pa0, pa1),
                                                                     __builtin_elementwise_max(pb0, pb1)));
      }
      vmax = max(vmax, max((uint32_t)pm.x, (uint32_t)pm.y));
      sqa = wave_sum_u32(sqa);
      sqb = wave_sum_u32(sqb);
      if ((tid & 63) == 0) {
        atomicAdd(&s_norm[d], (unsigned long long)sqa);
        atomicAdd(&s_norm[d + 1], (unsigned long long)sqb);
      }
    } else {
      uint64_t sq = 0;
      // 16-B u32 stores for slots, 8-B u16 stores for narrow rows (when the
      // row offset keeps them aligned); the next sketch row's old counters
      // are loaded into the slot as it is drained
      const bool vec = (w & 3) == 0 && (dst != nullptr || (tv.base(row) & 3) == 0);
      if (vec && !dst && !more && SV > 0 && (w & 7) == 0 && (tv.base(row) & 7) == 0) {
        // narrow row, fresh build, 16-B stores (8 counters per lane)
        uint4* l4 = reinterpret_cast<uint4*>(lds);
        uint4* d4 = reinterpret_cast<uint4*>(dst16 + rofs);
        uint32_t sq32 = 0;
        u16x2 pm = {0, 0};
        for (int j = tid; j < (w >> 3); j += kBuildThreads) {
          const uint4 v = l4[2 * j], u = l4[2 * j + 1];
          l4[2 * j] = make_uint4(0, 0, 0, 0);
          l4[2 * j + 1] = make_uint4(0, 0, 0, 0);
          const uint32_t a0 = __builtin_amdgcn_perm(v.y, v.x, 0x05040100u), a1 = __builtin_amdgcn_perm(v.w, v.z, 0x05040100u);
          const uint32_t a2 = __builtin_amdgcn_perm(u.y, u.x, 0x05040100u), a3 = __builtin_amdgcn_perm(u.w, u.z, 0x05040100u);
          store_row(d4 + j, make_uint4(a0, a1, a2, a3), SV);
          const u16x2 pa0 = __builtin_bit_cast(u16x2, a0), pa1 = __builtin_bit_cast(u16x2, a1);
          const u16x2 pa2 = __builtin_bit_cast(u16x2, a2), pa3 = __builtin_bit_cast(u16x2, a3);
          sq32 = __builtin_amdgcn_udot2(pa0, pa0, sq32, false);
          sq32 = __builtin_amdgcn_udot2(pa1, pa1, sq32, false);
          sq32 = __builtin_amdgcn_udot2(pa2, pa2, sq32, false);
          sq32 = __builtin_amdgcn_udot2(pa3, pa3, sq32, false);
          pm = __builtin_elementwise_max(pm, __builtin_elementwise_max(__builtin_elementwise_max(pa0, pa1),
                                                                       __builtin_elementwise_max(pa2, pa3)));
        }
        vmax = max(vmax, max((uint32_t)pm.x, (uint32_t)pm.y));
        sq = sq32;
      } else if (vec && !dst && !more) {
        // narrow row, fresh build (the common case): every counter < 2^16, so
        // the squares are full-rate 24-bit products and no sum can saturate
        uint4* l4 = reinterpret_cast<uint4*>(lds);
        uint2* d2 = reinterpret_cast<uint2*>(dst16 + rofs);
        uint32_t sq32 = 0;  // < 2^32: see the paired write-out
        u16x2 pm = {0, 0};
        for (int j = tid; j < (w >> 2); j += kBuildThreads) {
          const uint4 v = l4[j];
          l4[j] = make_uint4(0, 0, 0, 0);
          const uint32_t a0 = __builtin_amdgcn_perm(v.y, v.x, 0x05040100u), a1 = __builtin_amdgcn_perm(v.w, v.z, 0x05040100u);
#ifdef CMS_BUILD_NOWRITE  // bound analysis only: no table stores
          if (v.x == 0xFFFFFFFFu)
#endif
          d2[j] = make_uint2(a0, a1);
          const u16x2 pa0 = __builtin_bit_cast(u16x2, a0), pa1 = __builtin_bit_cast(u16x2, a1);
          sq32 = __builtin_amdgcn_udot2(pa0, pa0, sq32, false);
          sq32 = __builtin_amdgcn_udot2(pa1, pa1, sq32, false);
          pm = __builtin_elementwise_max(pm, __builtin_elementwise_max(pa0, pa1));
        }
        vmax = max(vmax, max((uint32_t)pm.x, (uint32_t)pm.y));
        sq = sq32;
      } else if (vec) {
        uint4* l4 = reinterpret_cast<uint4*>(lds);
        for (int j = tid; j < (w >> 2); j += kBuildThreads) {
          const uint4 v = l4[j];
          uint4 nv = make_uint4(0, 0, 0, 0);
          if (more) {
            if (dst) {
              nv = reinterpret_cast<const uint4*>(dst + rofs + w)[j];
            } else {
              const ushort4 o = reinterpret_cast<const ushort4*>(dst16 + rofs + w)[j];
              nv = make_uint4(o.x, o.y, o.z, o.w);
            }
          }
          l4[j] = nv;
#ifdef CMS_BUILD_NOWRITE  // bound analysis only: no table stores
          if (v.x == 0xFFFFFFFFu)
#endif
          if (dst) reinterpret_cast<uint4*>(dst + rofs)[j] = v;
          else reinterpret_cast<ushort4*>(dst16 + rofs)[j] = make_ushort4((unsigned short)v.x, (unsigned short)v.y,
                                                                          (unsigned short)v.z, (unsigned short)v.w);
          vmax = max(vmax, max(max(v.x, v.y), max(v.z, v.w)));
          sq = sat_add(sq, (uint64_t)v.x * v.x);
          sq = sat_add(sq, (uint64_t)v.y * v.y);
          sq = sat_add(sq, (uint64_t)v.z * v.z);
          sq = sat_add(sq, (uint64_t)v.w * v.w);
        }
      } else {
        for (int j = tid; j < w; j += kBuildThreads) {
          const uint32_t v = lds[j];
          lds[j] = more ? (dst ? dst[rofs + w + j] : (uint32_t)dst16[rofs + w + j]) : 0u;
          if (dst) dst[rofs + j] = v;
          else dst16[rofs + j] = (uint16_t)v;
          vmax = max(vmax, v);
          sq = sat_add(sq, (uint64_t)v * v);
        }
      }
      // per-thread sums stay far below 2^64 for counters < 2^26; anything at or
      // above 2^53 only has to stay >= 2^53 (inexact regime), so clamp.
      sq = wave_sum_u64_sat(sq);
      if (sq > (1ULL << 60)) sq = 1ULL << 60;
      if ((tid & 63) == 0) atomicAdd(&s_norm[d], (unsigned long long)sq);
    }
    lds_barrier();  // LDS order only: the write-out stores stay in flight
    d += two ? 2 : 1;
  }
  }  // sketch-row loop

  if (badv) atomicOr(flags, kFlagBadValue);
  mass = wave_sum_u64_sat(mass);
  if ((tid & 63) == 0 && mass) atomicAdd(&s_mass, (unsigned long long)mass);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
  if ((tid & 63) == 0 && vmax) atomicMax(&s_max, vmax);
  __syncthreads();
  if (!atomic_mode && tid < hp.depth) norm[row * hp.depth + tid] = s_norm[tid];
  if (!atomic_mode && tid == 0) rowmax[row] = s_max;
  if (tid == 0) {
    uint64_t tm = s_mass;
    if (!atomic_mode) {
      uint64_t m = accumulate ? row_mass[row] + tm : tm;
      row_mass[row] = m;
      if (m >= (1ULL << 32)) atomicOr(flags, kFlagOverflow);
    } else if (tm) {
      unsigned long long old = atomicAdd((unsigned long long*)&row_mass[row], (unsigned long long)tm);
      if (old + tm >= (1ULL << 32)) atomicOr(flags, kFlagOverflow);
    }
  }
}

// Owner classes of a fresh build with forms: rows holding a u32 slot (split
// owners and masses >= 2^16: k_build_rows), byte-class rows (k_build_nibbles
// finds them itself) and the rest, the mid class (k_build_mid), in two lists:
// the CACHED owners (their keys fit k_build_mid's registers) and the STREAMED
// ones, those above kStreamBigKeys keys first (a persistent grid that starts
// the long owners first ends with the short ones).
// Rows of chunks of kClassChunk owners per workgroup: the class lists are
// gathered in LDS (wave-aggregated LDS counters) and reserved with one global
// atomic per chunk and list -- with one atomic per wave the list counters
// took ~200 us of contention at 1M owners.
//
// A mid list is TWO-ENDED: cnt[0] owners from the front of its cap entries,
// cnt[1] more from the back.  The streamed list holds the long owners in
// front and the others behind; the cached list holds the cached owners behind
// and takes in front the streamed owners that the one-pass kernel sends back
// (and the list rows that k_build_mid_lists sends back).  The cached owners
// that k_build_mid_lists builds (mid_list_row, where that kernel exists) have
// a one-ended list of their own.
constexpr int kMidThreads = 256;  // threads per owner (a workgroup) of the row-at-a-time mid build
constexpr int64_t kMidCachedKeys = (int64_t)kMidThreads * kKeyRegs;
constexpr int64_t kStreamBigKeys = 4096;
__device__ __forceinline__ int32_t list2_at(const int32_t* list, uint32_t cap, uint32_t nfront, uint32_t i) {
  return i < nfront ? list[i] : list[cap - 1u - (i - nfront)];
}
// A byte-class owner's first form: 1-bit rows up to bit_keys keys
// (Tunables::bit_keys, 64), 2-bit up to crumb_keys (256), else 4-bit
__host__ __device__ __forceinline__ int nib_first_bits(int64_t m, int w, int bit_keys, int crumb_keys) {
  return (m <= bit_keys && (w & 127) == 0) ? 1 : (m <= crumb_keys && (w & 63) == 0) ? 2 : 4;
}
// ... stored as a list row: unit increments, at most list_keys keys, and the
// list (2 + 2 d m bytes) no larger than the dense row it would take first
__host__ __device__ __forceinline__ bool nib_list_row(int64_t m, int w, int d, bool weighted, int frac_bits,
                                                      int bit_keys, int crumb_keys, int list_keys) {
  return m <= list_keys && !weighted && frac_bits == 0 &&
         2 + 2 * (int64_t)d * m <= ((int64_t)d * w * nib_first_bits(m, w, bit_keys, crumb_keys)) / 8;
}
// A cached mid owner stored as a list row (while no counter passes 255): unit
// increments, at most list_keys keys (kMidListKeys, or 0 without lists), d m
// entries within the list's 8192, and the list smaller than even the 4-bit
// row.  mid_rows, k_build_classes and k_build_mid_lists decide by this.
__host__ __device__ __forceinline__ bool mid_list_row(int64_t m, int w, int d, bool weighted, int frac_bits,
                                                      int list_keys) {
  return m <= list_keys && !weighted && frac_bits == 0 && (int64_t)d * m <= 8192 &&
         2 + 2 * (int64_t)d * m < (int64_t)d * w / 2;
}
// counters of the class lists (one zeroed block per build)
enum {
  kCntSlot = 0,
  kCntMid = 1 /* front, back */,
  kCntStream = 3 /* front, back */,
  kCntTicket = 5,
  kCntMidLists = 6,
  kCntWords = 8
};
constexpr int kClassChunk = 4096;
// mid_lists_keys: kMidListKeys where k_build_mid_lists runs in this build (its
// owners then leave the cached list for mid_lists), else 0
__global__ __launch_bounds__(256) void k_build_classes(const int64_t* lo_, const int64_t* hi_, int64_t nrows,
                                                       const int32_t* hidx, const uint64_t* bound, int32_t* slot_list,
                                                       int32_t* mid_list, int32_t* stream_list, uint32_t* cnt,
                                                       int32_t* mid_lists, int mid_lists_keys, int d, int w) {
  // two-ended, as the lists they feed (an owner is in one class): slot
  // rows from the front of s_own and cached owners from its back, long
  // streamed owners from the front of s_str and short ones from its back
  __shared__ int32_t s_own[kClassChunk], s_str[kClassChunk], s_lst[kClassChunk];
  __shared__ uint32_t s_n[5], s_b[5];  // slot, cached, streamed long, streamed short, cached list rows
  const int lane = (int)__lane_id();
  const int tid = threadIdx.x;
  const uint32_t cap = (uint32_t)nrows;
  const unsigned long long below = (1ULL << lane) - 1ULL;
  for (int64_t r0 = (int64_t)blockIdx.x * kClassChunk; r0 < nrows; r0 += (int64_t)gridDim.x * kClassChunk) {
    if (tid < 5) s_n[tid] = 0;
    __syncthreads();
    for (int64_t r = r0 + tid; r < r0 + kClassChunk; r += 256) {  // (whole waves: the ballots)
      bool is[5] = {false, false, false, false, false};
      if (r < nrows) {
        const int32_t sl = hidx[r];
        const int64_t m = hi_[r] - lo_[r];
        is[0] = sl >= 0;
        const bool is_mid = !is[0] && !byte_class(sl, m, bound[r]);
        const bool cached = is_mid && m <= kMidCachedKeys;
        is[4] = cached && mid_list_row(m, w, d, false, 0, mid_lists_keys);
        is[1] = cached && !is[4];
        is[2] = is_mid && m > kStreamBigKeys;
        is[3] = is_mid && !cached && !is[2];
      }
      unsigned long long mk[5];
      uint32_t b[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        mk[k] = __ballot(is[k]);
        if (lane == 0 && mk[k]) b[k] = atomicAdd(&s_n[k], (uint32_t)__popcll(mk[k]));
        b[k] = (uint32_t)__shfl((int)b[k], 0, 64) + (uint32_t)__popcll(mk[k] & below);
      }
      if (is[0]) s_own[b[0]] = (int32_t)r;
      if (is[1]) s_own[kClassChunk - 1 - b[1]] = (int32_t)r;
      if (is[2]) s_str[b[2]] = (int32_t)r;
      if (is[3]) s_str[kClassChunk - 1 - b[3]] = (int32_t)r;
      if (is[4]) s_lst[b[4]] = (int32_t)r;
    }
    __syncthreads();
    if (tid < 5) {
      const int ci = tid == 0 ? kCntSlot : tid == 1 ? kCntMid + 1 : tid == 4 ? kCntMidLists : kCntStream + tid - 2;
      s_b[tid] = s_n[tid] ? atomicAdd(&cnt[ci], s_n[tid]) : 0u;
    }
    __syncthreads();
    for (uint32_t i = tid; i < s_n[0]; i += 256) slot_list[s_b[0] + i] = s_own[i];
    for (uint32_t i = tid; i < s_n[1]; i += 256) mid_list[cap - 1u - (s_b[1] + i)] = s_own[kClassChunk - 1 - i];
    for (uint32_t i = tid; i < s_n[2]; i += 256) stream_list[s_b[2] + i] = s_str[i];
    for (uint32_t i = tid; i < s_n[3]; i += 256) stream_list[cap - 1u - (s_b[3] + i)] = s_str[kClassChunk - 1 - i];
    for (uint32_t i = tid; i < s_n[4]; i += 256) mid_lists[s_b[4] + i] = s_lst[i];
    __syncthreads();
  }
}

// Mid-class owners (narrow, more than 256 keys or a mass >= 256): one
// workgroup per owner, in the narrowest form that holds it -- 4-bit first,
// u8 when a counter reaches 16, u16 when one reaches 256 (each escalation
// restarts the owner; the wider layout overwrites every byte the narrower one
// wrote).  The 4-bit attempt counts ALL d sketch rows at once in a [d][w]
// 4-bit LDS image (d*w/2 bytes, 20 KB at config 3), so each key is read and
// hashed once; its sums of squares come from reading the image back (v_dot4
// of the nibbles) as it is stored.  The u8 / u16 attempts go one sketch row
// at a time (a w- or 2w-byte image), the returning LDS adds giving each
// row's sum of squares.  A persistent grid walks the device-side list.
// mid owners of up to this many keys (the register-cached ones) may be list rows
constexpr int kMidListKeys = kBuildThreads * kKeyRegs;
// keys per thread in flight per step of an uncached owner's row pass
constexpr int kMidRowKeys = 4;
// mid_rows is the body of k_build_mid<SV, D, kMidThreads> (the kernel follows
// mid_streamed below): the cached owners, and the streamed ones that are
// weighted, do not start at u8 or passed 255 in mid_streamed's image.
template <int SV, int D, int MT>
__device__ __forceinline__ void mid_rows(
    const int64_t* lo_, const int64_t* hi_, const Keys& keys, const float* vals, const HashParams& hp,
    const int32_t* list, const uint32_t* list_cnt, uint32_t cap, const TableView& tv, int32_t* hidx_w,
    uint32_t* cbound, uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax, uint32_t* flags, int list_keys,
    int u4_keys, int u8_keys) {
  static_assert(MT == kMidThreads, "one instantiation per depth");
  constexpr int MTH = MT;        // threads per owner (a workgroup)
  constexpr int MKR = kKeyRegs;  // key registers per thread: 1024 keys cached per owner
  extern __shared__ __align__(16) uint32_t lds[];  // one sketch row of up to w u16 counters, or the [d][w] 4-bit image
  __shared__ unsigned long long s_norm[CMS_MAX_DEPTH];
  __shared__ unsigned long long s_mass;
  __shared__ uint32_t s_max, s_ovf;
  const int tid = threadIdx.x;
  const int w = (int)hp.width;
  const uint32_t nfront = list_cnt[0], count = nfront + list_cnt[1];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const int64_t row = list2_at(list, cap, nfront, li);
    const int64_t lo = lo_[row], hi = hi_[row];
    const bool cached = (hi - lo) <= (int64_t)MTH * MKR;
    uint64_t kp[MKR];
    uint32_t ik[MKR];
    uint64_t mass = 0;
    bool badv = false;
    if (cached) {
#pragma unroll
      for (int k = 0; k < MKR; ++k) {
        const int64_t i = lo + tid + (int64_t)k * MTH;
        kp[k] = 0;
        ik[k] = 0;
        if (i < hi) {
          uint32_t inc;
          if (!load_inc(vals, i, inc, hp.frac_bits)) {
            badv = true;
            inc = 0;
          }
          kp[k] = keys.at(i);
          ik[k] = inc;
          mass += inc;
        }
      }
    }
    uint4* d4 = reinterpret_cast<uint4*>(tv.row16(row));  // the row's slot (64-B aligned)
    // a LIST row (cms_internal.h kFormList) when the owner's keys sit in
    // registers, increments are units, and the list beats even the 4-bit row:
    // the counting below then only yields the norms and the maximum, and the
    // keys' buckets leave instead of the image (u16 counters -- a count past
    // 255 -- keep the dense row)
    const int64_t m = hi - lo;
    const bool as_list = cached && mid_list_row(m, w, hp.depth, vals != nullptr, hp.frac_bits, list_keys);
    uint16_t* lst = tv.row16(row);
    int level = -1;  // the form that holds the owner: 0 4-bit, 1 u8, 2 u16 (the class bound keeps every counter < 2^16)
    uint32_t vmax = 0;
    // the first form tried (Tunables::mid_u4_keys / mid_u8_keys); a list row
    // leaves its entries in the 4-bit pass, so it always takes that pass
    // ... unless k_build_mid_lists sent it back (the cached owners in front
    // of the list): a counter passed 255, so the u16 rows at once
    const int start = cached && li < nfront ? 2 : as_list || m <= u4_keys ? 0 : m <= u8_keys ? 1 : 2;
    bool mass_pending = !cached;  // uncached keys: the mass is summed by the first pass over them
    // ALL sketch rows in one key pass in a [d][w] 4-bit image.  (A [d][w] u8
    // image after a 4-bit overflow -- a Zipf key set repeats its popular keys,
    // and config 3 has 40K u8 owners -- measured slower: its 40 KB per
    // workgroup halve the owners in flight, build 6.55 -> 7.01 ms.)
    if (start == 0) {
      constexpr int ab = 4;
      const int lga = 3;  // log2(counters per word)
      const uint32_t capa = (1u << ab) - 1u;
      const int nq_all = (int)((int64_t)hp.depth * w * ab >> 7);  // uint4 of the [d][w] image
      uint4* l4 = reinterpret_cast<uint4*>(lds);
      for (int j = tid; j < nq_all; j += MTH) l4[j] = make_uint4(0, 0, 0, 0);
      if (tid < CMS_MAX_DEPTH) s_norm[tid] = 0ULL;
      if (tid == 0) {
        s_max = 0u;
        s_ovf = 0u;
        s_mass = 0ULL;
      }
      __syncthreads();
      bool ovf = false;
      vmax = 0;
      // a list row at an unrolled depth takes its sums of squares from the
      // adds (2 c inc + inc^2 per update, telescoping to sum c^2) instead of
      // reading the image back: nothing of it is stored
      constexpr int kSq = D > 0 ? D : 1;
      uint32_t sqr[kSq];
#pragma unroll
      for (int d = 0; d < kSq; ++d) sqr[d] = 0u;
      const bool tele = D > 0 && as_list;
      // lt >= 0: the key's list index -- a list row's entries leave during
      // the count (a count past 255 later rewrites the slot as u16 rows)
      auto add_all = [&](uint64_t kr, uint32_t inc, int64_t lt) {
        each_bucket<D>(hp, kr, [&](int d, uint32_t bk) {
          if (lt >= 0) lst[1 + (int64_t)d * m + lt] = (uint16_t)bk;
          const uint32_t c = (uint32_t)d * (uint32_t)w + bk;
          const uint32_t sh = (c & ((1u << lga) - 1u)) * (uint32_t)ab;
          const uint32_t old = (atomicAdd(&lds[c >> lga], inc << sh) >> sh) & capa;
          const uint32_t nv = old + inc;
          ovf |= nv > capa || inc > capa;  // carried into the next counter: a wider form
          vmax = max(vmax, nv);
          if (D > 0) sqr[D > 0 ? d : 0] += (2u * old + inc) * inc;
        });
      };
      if (cached) {
#pragma unroll
        for (int k = 0; k < MKR; ++k)
          if (ik[k]) add_all(kp[k], ik[k], as_list ? (int64_t)(tid + k * MTH) : int64_t(-1));
      } else {
        // the next step's key loads go out before this step's keys are added
        constexpr int64_t kStep = 4 * MTH;
        uint64_t nx[4];
        auto fetch = [&](int64_t base) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int64_t i = base + tid + (int64_t)u * MTH;
            nx[u] = i < hi ? keys.raw(i) : 0ULL;
          }
        };
        fetch(lo);
        for (int64_t base = lo; base < hi; base += kStep) {
          uint64_t kk[4];
          uint32_t inc4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            kk[u] = nx[u];
            const int64_t i = base + tid + (int64_t)u * MTH;
            inc4[u] = 0;
            if (i < hi) {
              uint32_t inc;
              if (!load_inc(vals, i, inc, hp.frac_bits)) {
                badv = true;
                inc = 0;
              }
              inc4[u] = inc;
            }
          }
          if (base + kStep < hi) fetch(base + kStep);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (inc4[u]) add_all(keys.resolve(kk[u]), inc4[u], -1);
            mass += inc4[u];
          }
        }
        mass_pending = false;
      }
      if (__ballot(ovf) && (tid & 63) == 0) s_ovf = 1u;
      __syncthreads();
      const bool fits = s_ovf == 0u;
      __syncthreads();  // every thread has read s_ovf before the row passes reset it
      if (fits) level = 0;
      if (fits && tele) {
#pragma unroll
        for (int d = 0; d < kSq; ++d) {
          const uint32_t sq = wave_sum_u32(sqr[d]);
          if ((tid & 63) == 0 && sq) atomicAdd(&s_norm[d], (unsigned long long)sq);
        }
        level = 3;  // a list row, norms done: no read-back
      }
    }
    if (level == 3) level = 0;
    else if (level == 0) {
      // read the image back: each sketch row's sum of squares (v_dot4 of its
      // low and high nibbles) as its rows leave for the slot
      const uint4* l4 = reinterpret_cast<const uint4*>(lds);
      const int nq = w >> 5;  // uint4 per 4-bit sketch row
      for (int d = 0; d < hp.depth; ++d) {
        uint32_t sq = 0;  // <= row mass * max counter < 2^32
        for (int j = tid; j < nq; j += MTH) {
          const uint4 v = l4[d * nq + j];
          const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t lo4 = x[q] & 0x0F0F0F0Fu, hi4 = (x[q] >> 4) & 0x0F0F0F0Fu;
            sq = __builtin_amdgcn_udot4(lo4, lo4, sq, false);
            sq = __builtin_amdgcn_udot4(hi4, hi4, sq, false);
          }
#ifdef CMS_BUILD_NOWRITE  // bound analysis only: no table stores
          if (false)
#endif
          if (!as_list) store_row(d4 + d * nq + j, v, SV);
        }
        sq = wave_sum_u32(sq);
        if ((tid & 63) == 0 && sq) atomicAdd(&s_norm[d], (unsigned long long)sq);
      }
    }
    // the 4-bit image overflowed (or was skipped): one sketch row at a time, u8 then u16
    if (level < 0) level = start > 1 ? 2 : 1;
    else level = -level - 1;  // done: mark so the row passes are skipped
    for (;;) {
      if (level < 0) break;  // the 4-bit image held every counter
      const int bits = 4 << level;
      const int lg = 3 - level;          // log2(counters per word)
      const uint32_t cap = (1u << bits) - 1u;
      const int nq = (w * bits) >> 7;    // uint4 per sketch row (w % 32 == 0)
      uint4* l4 = reinterpret_cast<uint4*>(lds);
      if (tid < CMS_MAX_DEPTH) s_norm[tid] = 0ULL;
      if (tid == 0) {
        s_max = 0u;
        s_ovf = 0u;
        s_mass = 0ULL;  // (added once, after the last pass; the 4-bit pass may not have run)
      }
      vmax = 0;
      for (int d = 0; d < hp.depth; ++d) {
        for (int j = tid; j < nq; j += MTH) l4[j] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        uint64_t sq = 0;
        bool ovf = false;
        auto add = [&](uint64_t kr, uint32_t inc) {
          const uint32_t c = bucket(hp, d, kr);
          const uint32_t sh = (c & ((1u << lg) - 1u)) * (uint32_t)bits;
          const uint32_t old = (atomicAdd(&lds[c >> lg], inc << sh) >> sh) & cap;
          const uint32_t nv = old + inc;
          ovf |= nv > cap || inc > cap;  // carried into the next counter: a wider form
          sq += (uint64_t)(2u * old + inc) * inc;
          vmax = max(vmax, nv);
        };
        if (cached) {
#pragma unroll
          for (int k = 0; k < MKR; ++k)
            if (ik[k]) add(kp[k], ik[k]);
        } else {
          for (int64_t base = lo; base < hi; base += kMidRowKeys * MTH) {
            uint64_t kk[kMidRowKeys];
            uint32_t inc4[kMidRowKeys];
#pragma unroll
            for (int u = 0; u < kMidRowKeys; ++u) {
              const int64_t i = base + tid + (int64_t)u * MTH;
              kk[u] = i < hi ? keys.at(i) : 0;
              inc4[u] = 0;
              if (i < hi) {
                uint32_t inc;
                if (!load_inc(vals, i, inc, hp.frac_bits)) {
                  badv = true;
                  inc = 0;
                }
                inc4[u] = inc;
              }
            }
#pragma unroll
            for (int u = 0; u < kMidRowKeys; ++u) {
              if (inc4[u]) add(kk[u], inc4[u]);
              if (mass_pending) mass += inc4[u];
            }
          }
          mass_pending = false;  // summed once, by row 0 of the first pass
        }
        sq = wave_sum_u64_sat(sq);
        if ((tid & 63) == 0 && sq) atomicAdd(&s_norm[d], (unsigned long long)sq);
        if (__ballot(ovf) && (tid & 63) == 0) s_ovf = 1u;
        __syncthreads();
        if (s_ovf) break;  // uniform: escalate
#ifdef CMS_BUILD_NOWRITE  // bound analysis only: no table stores
        if (false)
#endif
        if (!(as_list && level == 1))  // a list row's entries left in the 4-bit pass
          for (int j = tid; j < nq; j += MTH) store_row(d4 + d * nq + j, l4[j], SV);
        __syncthreads();  // the image is read out before the next sketch row zeroes it
      }
      if (!s_ovf || level == 2) break;
      __syncthreads();
      ++level;
    }
    if (level < 0) level = -level - 1;
    if (badv) atomicOr(flags, kFlagBadValue);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
    if ((tid & 63) == 0 && vmax) atomicMax(&s_max, vmax);
    mass = wave_sum_u64_sat(mass);
    if ((tid & 63) == 0 && mass) atomicAdd(&s_mass, (unsigned long long)mass);
    __syncthreads();
    if (tid < hp.depth) norm[row * hp.depth + tid] = s_norm[tid];
    const bool listed = as_list && level <= 1;
    if (tid == 0) {
      rowmax[row] = s_max;
      row_mass[row] = s_mass;
      if (s_mass >= (1ULL << 32)) atomicOr(flags, kFlagOverflow);
      if (listed) lst[0] = (uint16_t)m;
      hidx_w[row] = listed ? kFormList : level == 0 ? kFormU4 : level == 1 ? kFormU8 : kFormU16;
      cbound[row] = s_max;
    }
    __syncthreads();  // shared sums consumed before the next owner
  }
}

// The branch-free row hash (RowHash) in k_build_slices and mid_streamed; the
// bound-analysis hashes live in each_bucket, so those builds keep it.
#if defined(CMS_BUILD_CHEAPHASH) || defined(CMS_BUILD_GATHERHASH)
constexpr bool kRowHash = false;
#else
constexpr bool kRowHash = true;
#endif

// One pass of a workgroup of T threads over the keys [lo, end), PER keys a
// thread a step: the next step's loads (load(i), a raw key of type R) are
// issued before this step's keys go to f, so a load's latency hides behind
// the previous keys' hashes and LDS adds.  f runs for live keys only (a raw
// key may be any value) and returns whether the key is still to be done: those
// keys go to g after the step's last f, in a rolled loop, so the rare route's
// code stands once and outside the unrolled keys (NoRedo for g: f does every
// key itself, its answer is not read).
struct NoRedo {};
template <typename R, int PER, int T, typename L, typename F, typename G>
__device__ __forceinline__ void key_pass(int64_t lo, int64_t end, int tid, L&& load, F&& f, G&& g) {
  constexpr int64_t kStep = (int64_t)PER * T;
  R nx[PER];
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int64_t i = base + tid + (int64_t)u * T;
      nx[u] = i < end ? load(i) : R(0);
    }
  };
  if (lo < end) fetch(lo);
  for (int64_t base = lo; base < end; base += kStep) {
    R kk[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) kk[u] = nx[u];
    if (base + kStep < end) fetch(base + kStep);
    const int live = (int)min(end - base, kStep);  // (uniform) keys of this step
    if constexpr (std::is_same<typename std::decay<G>::type, NoRedo>::value) {
#pragma unroll
      for (int u = 0; u < PER; ++u)
        if (tid < live - u * T) f(kk[u]);
    } else {
      uint32_t left = 0;
#pragma unroll
      for (int u = 0; u < PER; ++u)
        if (tid < live - u * T && f(kk[u])) left |= 1u << u;
      if (left) {
#pragma unroll 1
        for (int u = 0; u < PER; ++u) {
          if (!((left >> u) & 1u)) continue;
          R k = kk[0];
#pragma unroll
          for (int j = 1; j < PER; ++j) k = j == u ? kk[j] : k;
          g(k);
        }
      }
    }
  }
}

// STREAMED mid owners (more than kMidCachedKeys keys) of a unit-increment
// build: ONE key pass for all d sketch rows, the shape of k_build_slices on a
// [d][w] u8 image (d*w bytes, 40 KB at config 3).  mid_rows walks such an
// owner's keys d times, one sketch row each, every step's loads waited for
// before its keys are hashed; here the tokens are fetched a step ahead and
// each key is hashed once for all d rows (RowHash, or each_bucket where it
// does not apply).  512 threads per image:
// four images fill a CU's LDS, and with 256 threads they were 16 waves per CU
// (the k_build_image experiment, which also swept its image for the few
// hundred keys of a cached owner); four 512-thread workgroups are the CU's
// whole wave budget, and only owners above 1024 keys pay the sweep.
// The image takes all the dynamic LDS and the kernel has no static LDS (a
// word of static LDS would cost the fourth image of a CU): the workgroup's
// reductions and its next ticket go through the image's own words after the
// sweep has read them.
// A counter that passes 255 carries into the neighbouring byte (or out of
// its word), which takes 255 (or 256) off the image's byte sum: the sweep sums
// the bytes, and an owner whose sum is not d times its key count is sent back
// (the front of the cached list, redo) for mid_rows' u16 rows.  The adds
// therefore need not return the old counter -- with returning adds and a flag
// per add the kernel spilled at 80 VGPRs.  An owner that does not start at u8
// (Tunables::mid_u4_keys / mid_u8_keys) is sent back too: the stored form of
// every owner is the one mid_rows alone gives it.  Workgroups take owners
// from a ticket counter: the owners' key counts span 16x.
constexpr int kStreamThreads = 512;
constexpr int kStreamPer = 2;  // keys per thread per step (the next step's loads in flight; 4 spilled at 64 VGPRs)
// LDS words the reductions need: the next ticket, then per wave d sums of squares, a maximum and a byte sum
constexpr int kStreamRedWords = 1 + (kStreamThreads / 64) * (CMS_MAX_DEPTH + 2);
template <int SV, int D>
__device__ __forceinline__ void mid_streamed(const int64_t* lo_, const int64_t* hi_, const Keys& keys,
                                             const HashParams& hp, const int32_t* list, const uint32_t* list_cnt,
                                             uint32_t cap, const TableView& tv, int32_t* hidx_w, uint32_t* cbound,
                                             uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax, int32_t* redo,
                                             uint32_t* redo_cnt, uint32_t* ticket, int u4_keys, int u8_keys) {
  extern __shared__ __align__(16) uint32_t lds[];  // the [d][w] u8 image (at least kStreamRedWords words)
  constexpr int T = kStreamThreads;
  constexpr int NW = T / 64;
  constexpr int RS = CMS_MAX_DEPTH + 2;  // reduction words per wave
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int w = (int)hp.width;
  const int depth = D > 0 ? D : hp.depth;
  const int nq = w >> 4;  // uint4 per u8 sketch row (w % 32 == 0)
  const uint32_t nfront = list_cnt[0], count = nfront + list_cnt[1];
  uint4* l4 = reinterpret_cast<uint4*>(lds);
  uint32_t* red = lds + 1;
  if (tid == 0) lds[0] = atomicAdd(ticket, 1u);
  __syncthreads();
  uint32_t li = lds[0];
  while (li < count) {  // (uniform)
    __syncthreads();  // the ticket and the last owner's sums are read before the image is zeroed
    const int64_t row = list2_at(list, cap, nfront, li);
    const int64_t lo = lo_[row], hi = hi_[row];
    const int64_t m = hi - lo;
    const bool u8_start = m > u4_keys && m <= u8_keys;  // else mid_rows' owner
    uint32_t mine = 0;  // lane r holds its wave's sum of squares of sketch row r
    uint32_t bytes = 0;  // sum of the image's bytes: d * m unless a counter passed 255
    u16x2 pm = {0, 0};
    if (u8_start) {
      for (int j = tid; j < depth * nq; j += T) l4[j] = make_uint4(0, 0, 0, 0);
      __syncthreads();
      auto add = [&](int r, uint32_t bk) {
        const uint32_t c = (uint32_t)r * (uint32_t)w + bk;
        atomicAdd(&lds[c >> 2], 1u << ((c & 3u) << 3));
      };
      // k_build_slices' key pass on the u8 image: a key's D rows by RowHash
      // (cms_hash.h), then its D adds back to back -- the word of counter
      // (r, bk) is at byte r * w + (bk & ~3) (w % 32 == 0), the shift of its
      // byte takes the low five bits of bk << 3.  RowHash's constants stay
      // scalar here: in vector registers the kernel spilled at its 64 VGPRs,
      // and so it did with a key pass of its own for tokens, for CSR keys or
      // for the shapes RowHash does not cover -- ONE pass, the three routes
      // behind scalar branches per key (the last with its rows rolled).
      constexpr int DR = D > 0 ? D : 1;
      const RowHash<DR> rh(hp);
      const bool fast = kRowHash && D > 0 && hp.fastq, tok = keys.tok != nullptr;  // (kernel-uniform)
      key_pass<uint64_t, kStreamPer, T>(
          lo, hi, tid, [&](int64_t i) { return keys.raw(i); },
          [&](uint64_t raw) {
            if (!fast) {  // any depth, any width
              each_bucket<(kRowHash ? 0 : D)>(hp, keys.resolve(raw), add);
              return false;
            }
            uint32_t bk[DR];
            uint32_t k = (uint32_t)raw;    // a token below kTokEscape is the reduced key
            bool again = k >= kTokEscape;  // (an escaped one is resolved in the redo)
            if (!tok) {
              const uint64_t kp = reduce_key((int64_t)raw);
              k = (uint32_t)kp;
              again = kp >= kRowHashKeyEnd;
            }
            if (rh.rows32(k, bk) || again) {  // the redo: about 1 key in 6,500, and every key that is no u32
              const uint64_t kp = keys.resolve(raw);
#pragma unroll 1
              for (int r = 0; r < D; ++r) add(r, bucket(hp, r, kp));
              return false;
            }
#pragma unroll
            for (int r = 0; r < D; ++r)
              atomicAdd(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + ((uint32_t)r * (uint32_t)w + (bk[r] & ~3u))),
                        1u << ((bk[r] << 3) & 31u));
            return false;
          },
          NoRedo{});  // (the redo in place: the kernel has no register left for key_pass' second loop)
      __syncthreads();
      // the image leaves as it is (an owner that overflowed is rewritten whole
      // by mid_rows); each sketch row's sum of squares by v_dot4 of its bytes,
      // the largest counter by packed u16 maxima of the even and the odd bytes
      uint4* d4 = reinterpret_cast<uint4*>(tv.row16(row));  // the row's slot (64-B aligned)
      auto sweep_row = [&](int r) {
        uint32_t sq = 0;  // <= 255 * the key count < 2^32
        for (int j = tid; j < nq; j += T) {
          const uint4 v = l4[r * nq + j];
          const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            sq = __builtin_amdgcn_udot4(x[q], x[q], sq, false);
            bytes = __builtin_amdgcn_udot4(x[q], 0x01010101u, bytes, false);
            pm = __builtin_elementwise_max(pm, __builtin_elementwise_max(__builtin_bit_cast(u16x2, x[q] & 0x00FF00FFu),
                                                                         __builtin_bit_cast(u16x2, (x[q] >> 8) & 0x00FF00FFu)));
          }
          store_row(d4 + r * nq + j, v, SV);
        }
        sq = wave_sum_u32(sq);
        if (lane == r) mine = sq;
      };
#pragma unroll 1
      for (int r = 0; r < depth; ++r) sweep_row(r);
    }
    uint32_t vmax = max((uint32_t)pm.x, (uint32_t)pm.y);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
    bytes = wave_sum_u32(bytes);  // <= d * m < 2^32
    __syncthreads();  // the image is read out: its first words take the reductions
    if (lane < depth) red[wv * RS + lane] = mine;
    if (lane == 0) {
      red[wv * RS + CMS_MAX_DEPTH] = vmax;
      red[wv * RS + CMS_MAX_DEPTH + 1] = bytes;
    }
    if (tid == 0) lds[0] = atomicAdd(ticket, 1u);
    __syncthreads();
    uint32_t mx = 0, total = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      mx = max(mx, red[k * RS + CMS_MAX_DEPTH]);
      total += red[k * RS + CMS_MAX_DEPTH + 1];
    }
    if (!u8_start || total != (uint32_t)depth * (uint32_t)m) {
      if (tid == 0) redo[atomicAdd(redo_cnt, 1u)] = (int32_t)row;
    } else {
      if (tid < depth) {
        uint64_t s = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) s += red[k * RS + tid];
        norm[row * depth + tid] = s;
      }
      if (tid == 0) {
        rowmax[row] = mx;
        row_mass[row] = (uint64_t)m;  // unit increments
        hidx_w[row] = kFormU8;
        cbound[row] = mx;
      }
    }
    li = lds[0];
  }
}

// The mid-class kernel: MT == kMidThreads walks a list with mid_rows (a
// persistent grid with a fixed stride), MT == kStreamThreads takes a streamed
// list's owners by ticket with mid_streamed.  One name for both: profiles and
// the benchmark's kernel patterns are keyed on it.
template <int SV, int D, int MT>
// mid_rows, 4 waves per SIMD: the key prefetch needs more than the 80 VGPRs
// of 6 (it spilled there); the build measured the same (profiles/r04/ab_*_s5).
// mid_streamed, 8: four 512-thread workgroups per CU.
__global__ __launch_bounds__(MT) __attribute__((amdgpu_waves_per_eu(MT == kStreamThreads ? 8 : 4, 8))) void k_build_mid(
    const int64_t* lo_, const int64_t* hi_, Keys keys, const float* vals, HashParams hp,
    const int32_t* list, const uint32_t* list_cnt /* front, back */, uint32_t cap, TableView tv, int32_t* hidx_w,
    uint32_t* cbound, uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax, uint32_t* flags, int list_keys,
    int u4_keys, int u8_keys, int32_t* redo, uint32_t* redo_cnt, uint32_t* ticket) {
  if constexpr (MT == kStreamThreads)
    mid_streamed<SV, D>(lo_, hi_, keys, hp, list, list_cnt, cap, tv, hidx_w, cbound, row_mass, norm, rowmax, redo,
                        redo_cnt, ticket, u4_keys, u8_keys);
  else
    mid_rows<SV, D, MT>(lo_, hi_, keys, vals, hp, list, list_cnt, cap, tv, hidx_w, cbound, row_mass, norm, rowmax,
                        flags, list_keys, u4_keys, u8_keys);
}

// Byte-class owners (byte_class): ONE WAVE per owner, four owners per
// workgroup, each wave with its own w/2-byte LDS slot (4 KB at w = 8192).  The
// owner's keys are read once into registers; each sketch row in turn is
// counted in the slot as 1-, 2- or 4-bit counters (the narrowest form the
// owner's key count suggests, widened on overflow) and leaves as 16-B
// non-temporal stores of the slot itself (no packing).  The LDS adds
// return the old counter, so each sketch row's sum of squares (2 c inc +
// inc^2 per update, telescoping to the exact sum) and the row maximum come out
// of the update pass.  With 4 KB per owner 32 owners are in flight per CU
// (the wave limit), against 8 with a whole-sketch 20 KB image per workgroup
// (config 3: 5.1 ms for this kernel with 4-bit rows only, 3.1 ms with 1- and
// 2-bit rows, which halve and quarter the row bytes).  A counter that would pass 15 (a
// repeated key, a collision, an increment >= 16) is detected by its add; the
// owner is queued for k_build_bytes, which rewrites its whole slot, norms and
// maximum as a u8 row.  Waves never wait on each other (no workgroup barrier):
// one wave's LDS operations execute in program order.
constexpr int kMidGridPerCu = 8;  // persistent k_build_mid workgroups per CU
constexpr int kNibWaves = 4;
// owners with at most Tunables::bit_keys (64) keys try 1-bit rows first, with
// at most crumb_keys (256) 2-bit rows (nib_first_bits; nib_list_row: the list rows)

// Compact layout of a fresh build (row_layout): each row's arena capacity in
// 128-B units, by what its class's kernel can store -- a hot row nothing (its
// counters are u32 slot rows), a byte-class row its list entries or its u8
// image (k_build_nibbles' forms up to k_build_bytes' u8 rows), any other row
// (the mid class, or every row without forms) a whole u16 slot (kCapU16).
__global__ void k_row_caps(const int64_t* lo_, const int64_t* hi_, int64_t n, const uint64_t* bound,
                           const int32_t* hidx, int forms, int weighted, int frac_bits, int d, int w, int bit_keys,
                           int crumb_keys, int list_keys, uint32_t* caps) {
  const int64_t dw = (int64_t)d * w;
  const uint32_t full = (uint32_t)(slot_units(dw) / kRowAlign);
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = hidx[r];
    const int64_t m = hi_[r] - lo_[r];
    uint32_t c = full;
    if (s >= 0) {
      c = 0;
    } else if (forms && byte_class(s, m, bound[r])) {
      const int64_t u16s = nib_list_row(m, w, d, weighted != 0, frac_bits, bit_keys, crumb_keys, list_keys)
                               ? 1 + (int64_t)d * m  // [0] = m, then the d x m entries
                               : dw / 2;             // the u8 image
      c = (uint32_t)((u16s + kRowAlign - 1) / kRowAlign);
    }
    caps[r] = c;
  }
}

// One byte-class owner by one wave (k_build_nibbles).
template <int SV>
__device__ __forceinline__ void nib_owner(
    int64_t row, uint32_t* lds, const int64_t* lo_, const int64_t* hi_, const Keys& keys, const float* vals,
    const HashParams& hp, const int32_t* row_hot, const uint64_t* bound, const TableView& tv, int32_t* hidx_w,
    uint32_t* cbound, uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax, uint32_t* flags, int32_t* redo,
    uint32_t* redo_cnt, int bit_keys, int crumb_keys, int list_keys, int lists_done) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t lo = lo_[row], hi = hi_[row];
  if (row_hot[row] >= 0 || !byte_class(tv.hidx[row], hi - lo, bound[row])) return;
  const int w = (int)hp.width;
  // lists_done: k_build_lists has built the list rows
  if (lists_done && nib_list_row(hi - lo, w, hp.depth, vals != nullptr, hp.frac_bits, bit_keys, crumb_keys, list_keys))
    return;
  uint64_t kp[kKeyRegs];
  uint32_t ik[kKeyRegs];
  uint32_t mass = 0;
  bool badv = false;
#pragma unroll
  for (int k = 0; k < kKeyRegs; ++k) {
    const int64_t i = lo + lane + (int64_t)k * 64;
    kp[k] = 0;
    ik[k] = 0;
    if (i < hi) {
      uint32_t inc;
      if (!load_inc(vals, i, inc, hp.frac_bits)) {
        badv = true;
        inc = 0;
      }
      kp[k] = keys.at(i);
      ik[k] = inc;
      mass += inc;
    }
  }
  // 1-bit counters first for owners of <= bit_keys keys, 2-bit for <=
  // crumb_keys (most byte-class owners: no counter reaches 4), 4-bit for the
  // rest; an add that overflows the form restarts the owner one form wider
  // (the wider rows overwrite every byte the narrower ones wrote), and past 15
  // the owner goes to k_build_bytes (u8)
  const int64_t m = hi - lo;
  // list rows (cms_internal.h kFormList): unit increments, at most list_keys
  // keys; counted as 4-bit in LDS for the norms and the maximum only, the
  // entries leave as the owner's buckets (nib_first_bits / nib_list_row: the
  // compact layout sizes the row by the same rule, k_row_caps)
  int bits = nib_first_bits(m, w, bit_keys, crumb_keys);
  const bool as_list = nib_list_row(m, w, hp.depth, vals != nullptr, hp.frac_bits, bit_keys, crumb_keys, list_keys);
  if (as_list) bits = 4;
  uint16_t* lst = tv.row16(row);  // list row: [0] = m, then [d][m] buckets
  uint4* slot4 = reinterpret_cast<uint4*>(lds) + wv * (w >> 5);  // w/2 bytes per wave (the 4-bit row)
  uint32_t* slot = lds + wv * (w >> 3);
  uint4* d4 = reinterpret_cast<uint4*>(tv.row16(row));  // the row's u16 slot (64-B aligned)
  uint32_t vmax = 0;
  bool ovf = false;
  for (;;) {
    const int lg = bits == 1 ? 5 : bits == 2 ? 4 : 3;  // log2(counters per 32-bit word)
    const uint32_t cap = (1u << bits) - 1u;
    const int nq = (w * bits) >> 7;   // uint4 per sketch row
    vmax = 0;
    ovf = false;
    for (int d = 0; d < hp.depth; ++d) {
      for (int j = lane; j < nq; j += 64) slot4[j] = make_uint4(0, 0, 0, 0);
      uint32_t sq = 0;
#pragma unroll
      for (int k = 0; k < kKeyRegs; ++k)
        if (ik[k]) {
          const uint32_t c = bucket(hp, d, kp[k]);
          const uint32_t sh = (c & ((1u << lg) - 1u)) * (uint32_t)bits;
          const uint32_t old = (atomicAdd(&slot[c >> lg], ik[k] << sh) >> sh) & cap;
          const uint32_t nv = old + ik[k];
          ovf |= nv > cap || ik[k] > cap;  // the add carried into the next counter: a wider form
          sq += (2u * old + ik[k]) * ik[k];
          vmax = max(vmax, nv);
          if (as_list) lst[1 + (int64_t)d * m + lane + 64 * k] = (uint16_t)c;
        }
      if (__ballot(ovf)) break;  // uniform: escalate (the slot is zeroed by the next owner's first row)
      sq = wave_sum_u32(sq);  // <= mass * 15
#ifdef CMS_BUILD_NOWRITE  // bound analysis only: no table stores
      if (false)
#endif
      if (!as_list)
        for (int j = lane; j < nq; j += 64) store_row(d4 + d * nq + j, slot4[j], SV);
      if (lane == 0) norm[row * hp.depth + d] = sq;
    }
    if (!__ballot(ovf) || bits == 4) break;
    bits *= 2;
  }
  if (as_list && lane == 0) lst[0] = (uint16_t)m;
  if (badv) atomicOr(flags, kFlagBadValue);
  if (__ballot(ovf)) {  // to k_build_bytes; a list row (~row) stays one there: its counters are < 2^8 (m < 2^8)
    if (lane == 0) redo[atomicAdd(redo_cnt, 1u)] = as_list ? ~(int32_t)row : (int32_t)row;
    return;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
  mass = wave_sum_u32(mass);  // < 2^8 (byte class)
  if (lane == 0) {
    rowmax[row] = vmax;
    row_mass[row] = mass;
    hidx_w[row] = as_list ? kFormList : bits == 1 ? kFormU1 : bits == 2 ? kFormU2 : kFormU4;
    cbound[row] = vmax;
  }
}


// Grid: one owner per wave (the row loop below runs once).
// The second parameter is only ever 0 and unused: it stays so that the
// kernel's name does (profiles and the benchmark's kernel patterns are keyed on it)
template <int SV, int>
__global__ __launch_bounds__(64 * kNibWaves) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_build_nibbles(
    const int64_t* lo_, const int64_t* hi_, Keys keys, const float* vals, int64_t nrows, HashParams hp,
    const int32_t* row_hot, const uint64_t* bound, TableView tv, int32_t* hidx_w, uint32_t* cbound, uint64_t* row_mass,
    uint64_t* norm, uint32_t* rowmax, uint32_t* flags, int32_t* redo, uint32_t* redo_cnt, int bit_keys,
    int crumb_keys, int list_keys, int lists_done) {
  extern __shared__ __align__(16) uint32_t lds[];  // [kNibWaves][w / 8] words: one sketch row of nibbles per wave
  const int64_t nw = (int64_t)gridDim.x * kNibWaves;
  for (int64_t row = (int64_t)blockIdx.x * kNibWaves + (threadIdx.x >> 6); row < nrows; row += nw)
    nib_owner<SV>(row, lds, lo_, hi_, keys, vals, hp, row_hot, bound, tv, hidx_w, cbound, row_mass, norm, rowmax, flags,
                  redo, redo_cnt, bit_keys, crumb_keys, list_keys, lists_done);
}

// The byte-class owners that nib_list_row makes list rows, on a fresh build
// with unit increments at a power-of-two width (hp.fastq) and depth D: what
// nib_owner gives them -- [0] = m, the [d][m] entries in key order, the norms
// and the maximum from 4-bit counts in the wave's LDS slot, ~row to
// k_build_bytes when a counter passes 15 -- without the generic kernel's
// forms, weights and escalation.  Each key is hashed once for all D rows (one
// fp64 conversion, bucket_q's usual route on constants in scalar registers;
// the rare other routes repeat the key through bucket()), its entries
// stored as they are produced and kept packed two to a register for the row
// passes, which issue all of a sketch row's adds before they read an old
// counter (one LDS wait per sketch row) and store zero to the words they
// added into (the slot is zeroed whole once per wave).  The grid is resident
// and wave g takes rows g, g + G, ...: the next owner's spans are loaded
// before the current owner's hashes and its first 64 keys before the row
// passes, so the two dependent global round trips overlap work.  SV is
// unused (a list row has no dense stores); it keeps the name in line with
// the other build kernels.
// Wave-wide sum and maximum by DPP row operations: six VALU instructions and
// a v_readlane, against six LDS round trips (ds_bpermute) of the __shfl_xor
// form.  Quads, half rows and rows of 16 lanes fold in place, row_bcast15
// carries rows 0 and 2 into rows 1 and 3, row_bcast31 rows 0-1 into rows 2-3:
// lane 63 holds the result.
template <typename F>
__device__ __forceinline__ uint32_t wave_fold_dpp(uint32_t v, F f) {
  v = f(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v = f(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v = f(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));  // row_half_mirror
  v = f(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));  // row_mirror
  v = f(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false)); // row_bcast15 into rows 1, 3 (0 elsewhere)
  v = f(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false)); // row_bcast31 into rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// k_build_lists' row passes for an owner of NS live key slots (the slots
// below the last are full): the D sketch rows counted one after another as
// 4-bit counters in the wave's slot.  A lane past the owner's last key adds 0
// to word 0 (its packed buckets are 0), so no add sits under a branch and the
// row's adds are all in flight before the first old counter is read.  Returns
// whether a counter passed 15 (the owner then ends: wave-uniform).
template <int D, int NS>
__device__ __forceinline__ bool list_rows(uint32_t* slot, const uint32_t (&pk)[kKeyRegs][(D + 1) / 2], int lane,
                                          int m, uint32_t (&sq)[3], uint32_t& vmax) {
  const uint32_t tail = lane + 64 * (NS - 1) < m ? 1u : 0u;  // the last slot's lane holds a key
  bool ovf = false;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    uint32_t c[NS], old[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      c[k] = (pk[k][r >> 1] >> ((r & 1) << 4)) & 0xFFFFu;
      old[k] = atomicAdd(&slot[c[k] >> 3], (k < NS - 1 ? 1u : tail) << ((c[k] & 7u) << 2));
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const uint32_t live = k < NS - 1 ? 1u : tail;
      const uint32_t o = (old[k] >> ((c[k] & 7u) << 2)) & 15u;
      const uint32_t nv = (o + 1u) * live;
      ovf |= nv > 15u;  // the add carried into the next counter
      sq[r >> 1] += ((2u * o + 1u) * live) << ((r & 1) << 4);  // 2 c + 1 per unit add: telescopes to the exact sum of squares
      vmax = max(vmax, nv);
      // zero to just the words added into, after every lane's add of this row
      // (one wave's LDS operations execute in order): 0.87 ms alone against
      // 1.14 ms with the slot zeroed whole by 16-B stores before every row
      slot[c[k] >> 3] = 0u;
    }
    if (__ballot(ovf)) return true;
  }
  return false;
}

template <int SV, int D>
__global__ __launch_bounds__(64 * kNibWaves) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_build_lists(
    const int64_t* lo_, const int64_t* hi_, Keys keys, int64_t nrows, HashParams hp, const int32_t* row_hot,
    const uint64_t* bound, TableView tv, int32_t* hidx_w, uint32_t* cbound, uint64_t* row_mass, uint64_t* norm,
    uint32_t* rowmax, int32_t* redo, uint32_t* redo_cnt, int bit_keys, int crumb_keys, int list_keys) {
  static_assert(D > 0 && D <= 6, "three registers of packed 16-bit sums");
  extern __shared__ __align__(16) uint32_t lds[];  // [kNibWaves][w / 8] words: one sketch row of nibbles per wave
  constexpr int P = (D + 1) / 2;  // registers of a key's packed buckets
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = (int)hp.width;
  uint32_t* slot = lds + wv * (w >> 3);
  for (int j = lane; j < (w >> 3); j += 64) slot[j] = 0u;
  const int64_t nw = (int64_t)gridDim.x * kNibWaves;
  // what bucket_q's usual route needs of the D rows, six scalar registers a
  // row (through each_bucket<D> the whole HashParams rows stayed live, spilled,
  // and came back with some twenty-five v_readlane per hash)
  double qa[D], qb[D];
  uint32_t am[D], bm[D];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    qa[r] = hp.qa[r];
    qb[r] = hp.qb[r];
    am[r] = (uint32_t)hp.ap[r] & hp.wmask;
    bm[r] = (uint32_t)hp.bp[r];
  }
  // an owner's key count if this kernel builds it, else -1
  auto owner = [&](int64_t m, int32_t hot, int32_t form, uint64_t bnd) -> int {
    return hot < 0 && byte_class(form, m, bnd) && nib_list_row(m, w, D, false, 0, bit_keys, crumb_keys, list_keys)
               ? (int)m
               : -1;
  };
  int64_t row = (int64_t)blockIdx.x * kNibWaves + wv;
  if (row >= nrows) return;
  int64_t lo = lo_[row];
  int m = owner(hi_[row] - lo, row_hot[row], tv.hidx[row], bound[row]);
  uint64_t raw0 = lane < m ? keys.raw(lo + lane) : 0ULL;
  for (;;) {
    const int64_t nrow = row + nw;
    const bool more = nrow < nrows;
    int64_t nlo = 0, nhi = 0;
    int32_t nhot = 0, nform = 0;
    uint64_t nbound = 0;
    if (more) {  // (all five loads in flight together)
      nlo = lo_[nrow];
      nhi = hi_[nrow];
      nhot = row_hot[nrow];
      nform = tv.hidx[nrow];
      nbound = bound[nrow];
    }
    uint32_t pk[kKeyRegs][P];  // bucket r of key slot k: bits 16 (r & 1) of pk[k][r >> 1]
    uint16_t* lst = nullptr;
    if (m >= 0) {
      lst = tv.row16(row);  // [0] = m, then [d][m] buckets
      uint64_t raw[kKeyRegs];
      raw[0] = raw0;
#pragma unroll
      for (int k = 1; k < kKeyRegs; ++k) raw[k] = lane + 64 * k < m ? keys.raw(lo + lane + 64 * k) : 0ULL;
#pragma unroll
      for (int k = 0; k < kKeyRegs; ++k) {
#pragma unroll
        for (int q = 0; q < P; ++q) pk[k][q] = 0u;
        if (lane + 64 * k < m) {
          uint16_t* e = lst + 1 + lane + 64 * k;
          const uint64_t kp = keys.resolve(raw[k]);
          const double kf = (double)(uint32_t)kp;
          const uint32_t km = (uint32_t)kp & hp.wmask;
          bool redo_key = (kp >> 32) != 0;
#pragma unroll
          for (int r = 0; r < D; ++r) {  // bucket_q without its margin branch
            const double y = fma(qa[r], kf, qb[r]);
            const double fl = floor(y);
            const double fr = y - fl;
            redo_key |= !(fr >= kQEps && fr <= 1.0 - kQEps);
            const uint32_t q = (uint32_t)__double_as_longlong(fl + 4503599627370496.0);
            const uint32_t c = (__umul24(am[r], km) + bm[r] + __umul24(q, 25u)) & hp.wmask;
            e[r * m] = (uint16_t)c;
            pk[k][r >> 1] |= c << ((r & 1) << 4);
          }
          if (redo_key) {  // a hash in bucket_q's margin (1 in 30,000) or a key >= 2^32: the key's rows again, by bucket()
#pragma unroll 1
            for (int r = 0; r < D; ++r) {
              const uint32_t c = bucket(hp, r, kp);
              e[r * m] = (uint16_t)c;
#pragma unroll
              for (int q = 0; q < P; ++q)
                if ((r >> 1) == q)
                  pk[k][q] = (r & 1) ? (pk[k][q] & 0xFFFFu) | (c << 16) : (pk[k][q] & 0xFFFF0000u) | c;
            }
          }
        }
      }
    }
    int nm = -1;
    uint64_t nraw0 = 0ULL;
    if (more) {
      nm = owner(nhi - nlo, nhot, nform, nbound);
      if (lane < nm) nraw0 = keys.raw(nlo + lane);
    }
    if (m >= 0) {
      // per sketch row: the exact sum of squares (2 c + 1 per unit add,
      // telescoping) as 16-bit fields, two rows to a register: a lane's sum is
      // below 4 * 31, the wave's below 2^13
      uint32_t sq[3] = {0u, 0u, 0u};
      uint32_t vmax = 0;
      const int ns = (m + 63) >> 6;  // live key slots (uniform): the row passes have no branch per slot
      const bool ovf = ns == 1   ? list_rows<D, 1>(slot, pk, lane, m, sq, vmax)
                       : ns == 2 ? list_rows<D, 2>(slot, pk, lane, m, sq, vmax)
                       : ns == 3 ? list_rows<D, 3>(slot, pk, lane, m, sq, vmax)
                       : ns == 4 ? list_rows<D, 4>(slot, pk, lane, m, sq, vmax)
                                 : false;
      if (lane == 0) lst[0] = (uint16_t)m;
      if (ovf) {  // to k_build_bytes, which keeps the list (~row) and rewrites entries, norms and maximum
        if (lane == 0) redo[atomicAdd(redo_cnt, 1u)] = ~(int32_t)row;
      } else {
#pragma unroll
        for (int q = 0; q < P; ++q) sq[q] = wave_fold_dpp(sq[q], [](uint32_t a, uint32_t b) { return a + b; });
        vmax = wave_fold_dpp(vmax, [](uint32_t a, uint32_t b) { return max(a, b); });  // (0 is neutral for both)
        if (lane < D) {
          uint32_t s = 0;
#pragma unroll
          for (int r = 0; r < D; ++r)
            if (lane == r) s = (sq[r >> 1] >> ((r & 1) << 4)) & 0xFFFFu;
          norm[row * D + lane] = s;
        }
        if (lane == 0) {
          rowmax[row] = vmax;
          row_mass[row] = (uint64_t)m;  // unit increments
          hidx_w[row] = kFormList;
          cbound[row] = vmax;
        }
      }
    }
    if (!more) break;
    row = nrow;
    lo = nlo;
    m = nm;
    raw0 = nraw0;
  }
}

// The cached mid owners that mid_list_row makes list rows (256 to 1024 keys
// at config 3), under k_build_lists' conditions -- unit increments, a
// power-of-two width (hp.fastq), depth D -- and in its shape: ONE WAVE per
// owner, no barrier and no pass over w.  The result needs the keys' buckets
// in key order, each sketch row's sum of squares and the largest counter.
// Each key is hashed once for all D rows (the six hash scalars a row and the
// redo_key route of k_build_lists), its entries stored as they are produced
// and kept packed two to a register, up to kMidListSlots key slots a lane.
// The wave's LDS slot holds one sketch row of w u8 counters: per sketch row
// every add of the owner is issued before an old counter is read (a lane past
// the last key adds 0 to a word of its own), 2 old + 1 per add telescopes to the sum of
// squares (32 bits a row: a lane's sixteen adds reach 16 * 511), and zero is
// stored to just the words added into once the row's adds are all issued.  A
// counter that would pass 255 carries inside a word the row clears anyway;
// the owner then leaves its rows (wave-uniform) for the front of the cached
// list, where mid_rows builds its u16 rows -- the form mid_rows alone gives
// it.  The grid is resident and wave g takes list entries g, g + G, ...: the
// entry is read two owners ahead, the next owner's spans and place before the
// hashes, its first key slot before the row passes.  SV is unused.
constexpr int kMidListWaves = 4;       // waves per workgroup, each with a slot of its own
constexpr int kMidListSlots = 16;      // key slots per lane: kMidListKeys keys in registers
constexpr int kMidListGroup = 4;       // key slots whose loads are in flight together; the row passes go by whole groups
constexpr int kMidListSlotMax = 8192;  // widest sketch row it takes: 32 KB of LDS per workgroup, four workgroups per CU
static_assert(64 * kMidListSlots == kMidListKeys && kMidListSlots % kMidListGroup == 0, "every cached list row fits");

// Its row passes for an owner of ns live key slots (uniform: a scalar branch
// per slot, none per lane).  Bit k of `live`: the lane's key slot k holds a key.
template <int D>
__device__ __forceinline__ bool mid_list_rows(uint32_t* slot, const uint32_t (&pk)[kMidListSlots][(D + 1) / 2],
                                              uint32_t live, int ns, uint32_t (&sq)[D], uint32_t& vmax) {
  bool ovf = false;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    uint32_t old[kMidListSlots];
#pragma unroll
    for (int k = 0; k < kMidListSlots; ++k)
      if (k < ns) {
        const uint32_t c = (pk[k][r >> 1] >> ((r & 1) << 4)) & 0xFFFFu;
        old[k] = atomicAdd(&slot[c >> 2], ((live >> k) & 1u) << ((c & 3u) << 3));
      }
#pragma unroll
    for (int k = 0; k < kMidListSlots; ++k)
      if (k < ns) {
        // (the bucket unpacked again: kept from the adds, the sixteen addresses
        // and shifts spilled beside the packed buckets and the old counters)
        uint32_t p = pk[k][r >> 1];
        asm volatile("" : "+v"(p));
        const uint32_t c = (p >> ((r & 1) << 4)) & 0xFFFFu;
        const uint32_t lv = (live >> k) & 1u;
        const uint32_t o = (old[k] >> ((c & 3u) << 3)) & 255u;
        const uint32_t nv = (o + 1u) * lv;
        ovf |= nv > 255u;  // the add carried into the next counter (or out of the word)
        sq[r] += (2u * o + 1u) * lv;
        vmax = max(vmax, nv);
        // zero to just the words added into, after every lane's add of this
        // row (one wave's LDS operations execute in order): 388 us alone
        // against 399 us with the slot zeroed whole before every row
        slot[c >> 2] = 0u;
      }
    if (__ballot(ovf)) return true;
  }
  return false;
}

template <int SV, int D>
__global__ __launch_bounds__(64 * kMidListWaves) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_build_mid_lists(
    const int64_t* lo_, const int64_t* hi_, Keys keys, HashParams hp, const int32_t* list, const uint32_t* list_cnt,
    TableView tv, int32_t* hidx_w, uint32_t* cbound, uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax,
    int32_t* redo, uint32_t* redo_cnt) {
  extern __shared__ __align__(16) uint32_t lds[];  // [kMidListWaves][w / 4] words: one sketch row of u8 counters per wave
  constexpr int P = (D + 1) / 2;  // registers of a key's packed buckets
  constexpr int NSL = kMidListSlots, GS = kMidListGroup, NGR = NSL / GS;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = (int)hp.width;
  uint32_t* slot = lds + wv * (w >> 2);
  for (int j = lane; j < (w >> 2); j += 64) slot[j] = 0u;
  const uint32_t count = list_cnt[0];
  // a lane past the owner's last key adds 0 to a word of its own (the lanes of
  // one wave adding to one word would take their turns)
  const uint32_t idle = ((4u * (uint32_t)lane) & hp.wmask) * 0x10001u;
  double qa[D], qb[D];  // (k_build_lists: what bucket_q's usual route needs, six scalar registers a row)
  uint32_t am[D], bm[D];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    qa[r] = hp.qa[r];
    qb[r] = hp.qb[r];
    am[r] = (uint32_t)hp.ap[r] & hp.wmask;
    bm[r] = (uint32_t)hp.bp[r];
  }
  // a fixed stride over the list: 388 us alone against 1227 us with every
  // wave drawing its entries from one ticket counter (a wave's owner is a few
  // microseconds of work; the owners' key counts span only 4x)
  const uint32_t stride = gridDim.x * kMidListWaves;  // (count + 2 stride < 2^32)
  const uint32_t li = blockIdx.x * kMidListWaves + wv;
  if (li >= count) return;
  int32_t row = list[li];
  int32_t row1 = li + stride < count ? list[li + stride] : -1;
  uint32_t li2 = li + 2u * stride;
  int64_t lo = lo_[row];
  int m = (int)(hi_[row] - lo);
  int64_t base = tv.base(row);
  uint64_t raw0 = lane < m ? keys.raw(lo + lane) : 0ULL;
  for (;;) {
    const int32_t row2 = li2 < count ? list[li2] : -1;
    li2 += stride;
    int64_t nlo = 0, nhi = 0, nbase = 0;
    if (row1 >= 0) {  // (the three loads in flight together)
      nlo = lo_[row1];
      nhi = hi_[row1];
      nbase = tv.base(row1);
    }
    uint16_t* lst = tv.t16 + base;  // [0] = m, then [d][m] buckets
    uint32_t pk[NSL][P];            // bucket r of key slot k: bits 16 (r & 1) of pk[k][r >> 1]
    {
      uint64_t cur[GS], nxt[GS];
      cur[0] = raw0;
#pragma unroll
      for (int j = 1; j < GS; ++j) cur[j] = lane + 64 * j < m ? keys.raw(lo + lane + 64 * j) : 0ULL;
#pragma unroll
      for (int g = 0; g < NGR; ++g) {
#pragma unroll
        for (int j = 0; j < GS; ++j) nxt[j] = 0ULL;
        if (g + 1 < NGR && 64 * GS * (g + 1) < m) {  // (uniform) the next group's keys before this group's hashes
#pragma unroll
          for (int j = 0; j < GS; ++j) {
            const int t = lane + 64 * (GS * (g + 1) + j);
            if (t < m) nxt[j] = keys.raw(lo + t);
          }
        }
#pragma unroll
        for (int j = 0; j < GS; ++j)
#pragma unroll
          for (int q = 0; q < P; ++q) pk[GS * g + j][q] = idle;
        if (64 * GS * g < m) {  // (uniform)
#pragma unroll
          for (int j = 0; j < GS; ++j) {
            const int k = GS * g + j;
            if (lane + 64 * k < m) {
              uint16_t* e = lst + 1 + lane + 64 * k;
              const uint64_t kp = keys.resolve(cur[j]);
              const double kf = (double)(uint32_t)kp;
              const uint32_t km = (uint32_t)kp & hp.wmask;
              bool redo_key = (kp >> 32) != 0;
#pragma unroll
              for (int q = 0; q < P; ++q) pk[k][q] = 0u;
#pragma unroll
              for (int r = 0; r < D; ++r) {  // bucket_q without its margin branch
                const double y = fma(qa[r], kf, qb[r]);
                const double fl = floor(y);
                const double fr = y - fl;
                redo_key |= !(fr >= kQEps && fr <= 1.0 - kQEps);
                const uint32_t q = (uint32_t)__double_as_longlong(fl + 4503599627370496.0);
                const uint32_t c = (__umul24(am[r], km) + bm[r] + __umul24(q, 25u)) & hp.wmask;
                e[r * m] = (uint16_t)c;
                pk[k][r >> 1] |= c << ((r & 1) << 4);
              }
              if (redo_key) {  // a hash in bucket_q's margin or a key >= 2^32: the key's rows again, by bucket()
#pragma unroll 1
                for (int r = 0; r < D; ++r) {
                  const uint32_t c = bucket(hp, r, kp);
                  e[r * m] = (uint16_t)c;
#pragma unroll
                  for (int q = 0; q < P; ++q)
                    if ((r >> 1) == q)
                      pk[k][q] = (r & 1) ? (pk[k][q] & 0xFFFFu) | (c << 16) : (pk[k][q] & 0xFFFF0000u) | c;
                }
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < GS; ++j) cur[j] = nxt[j];
      }
    }
    int nm = 0;
    uint64_t nraw0 = 0ULL;
    if (row1 >= 0) {
      nm = (int)(nhi - nlo);
      if (lane < nm) nraw0 = keys.raw(nlo + lane);
    }
    uint32_t sq[D];
#pragma unroll
    for (int r = 0; r < D; ++r) sq[r] = 0u;
    uint32_t vmax = 0;
    const int nf = min(max((m - lane + 63) >> 6, 0), NSL);  // the lane's key slots
    const uint32_t live = (1u << nf) - 1u;
    const int ns = (m + 63) >> 6;  // live key slots (uniform)
    const bool ovf = mid_list_rows<D>(slot, pk, live, ns, sq, vmax);
    if (ovf) {  // to mid_rows, which rewrites the whole slot as u16 rows
      if (lane == 0) redo[atomicAdd(redo_cnt, 1u)] = row;
    } else {
#pragma unroll
      for (int r = 0; r < D; ++r) sq[r] = wave_fold_dpp(sq[r], [](uint32_t a, uint32_t b) { return a + b; });
      vmax = wave_fold_dpp(vmax, [](uint32_t a, uint32_t b) { return max(a, b); });  // (0 is neutral for both)
      if (lane < D) {
        uint32_t s = 0;
#pragma unroll
        for (int r = 0; r < D; ++r)
          if (lane == r) s = sq[r];
        norm[(int64_t)row * D + lane] = s;
      }
      if (lane == 0) {
        lst[0] = (uint16_t)m;
        rowmax[row] = vmax;
        row_mass[row] = (uint64_t)m;  // unit increments
        hidx_w[row] = kFormList;
        cbound[row] = vmax;
      }
    }
    if (row1 < 0) break;
    row = row1;
    lo = nlo;
    m = nm;
    base = nbase;
    raw0 = nraw0;
    row1 = row2;
  }
}

// The byte-class owners a counter >= 16 sent back from k_build_nibbles: the
// same one-pass build on a [d][w] u8 image (dw bytes of LDS), stored as u8
// rows -- or, for a list row (listed as ~row), its entries written whole and
// the list kept (the compact layout sized it as a list; a list holds any
// counter below 2^8).  A persistent grid walks the device-side list (no host
// count).
template <int SV>
__global__ __launch_bounds__(kBuildThreads) void k_build_bytes(
    const int64_t* lo_, const int64_t* hi_, Keys keys, const float* vals, HashParams hp,
    const int32_t* list, const uint32_t* list_cnt, TableView tv, int32_t* hidx_w, uint32_t* cbound,
    uint64_t* row_mass, uint64_t* norm, uint32_t* rowmax, uint32_t* flags) {
  extern __shared__ __align__(16) uint32_t lds[];  // [d][w] bytes
  __shared__ unsigned long long s_norm[CMS_MAX_DEPTH];
  __shared__ uint32_t s_max, s_mass;
  const int tid = threadIdx.x;
  const int w = (int)hp.width;
  const int64_t dw = (int64_t)hp.depth * w;
  const uint32_t count = *list_cnt;
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const bool keep_list = list[li] < 0;
    const int64_t row = keep_list ? ~(int64_t)list[li] : (int64_t)list[li];
    const int64_t lo = lo_[row], hi = hi_[row];
    uint16_t* lst = tv.row16(row);  // list row: [0] = m (k_build_nibbles wrote it), then [d][m] buckets
    if (tid < CMS_MAX_DEPTH) s_norm[tid] = 0ULL;
    if (tid == 0) {
      s_max = 0u;
      s_mass = 0u;
    }
    uint64_t kp[kKeyRegs];
    uint32_t ik[kKeyRegs];
    uint32_t mass = 0;
    bool badv = false;
#pragma unroll
    for (int k = 0; k < kKeyRegs; ++k) {
      const int64_t i = lo + tid + (int64_t)k * kBuildThreads;
      kp[k] = 0;
      ik[k] = 0;
      if (i < hi) {
        uint32_t inc;
        if (!load_inc(vals, i, inc, hp.frac_bits)) {
          badv = true;
          inc = 0;
        }
        kp[k] = keys.at(i);
        ik[k] = inc;
        mass += inc;
      }
    }
    const int nq = (int)(dw >> 4);  // uint4 words of the byte image
    uint4* l4 = reinterpret_cast<uint4*>(lds);
    for (int j = tid; j < nq; j += kBuildThreads) l4[j] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    uint32_t vmax = 0;
    for (int d = 0; d < hp.depth; ++d) {
      uint32_t sq = 0;
#pragma unroll
      for (int k = 0; k < kKeyRegs; ++k)
        if (ik[k]) {
          const uint32_t bk = bucket(hp, d, kp[k]);
          const uint32_t c = (uint32_t)d * (uint32_t)w + bk;
          if (keep_list) lst[1 + (int64_t)d * (hi - lo) + tid + (int64_t)k * kBuildThreads] = (uint16_t)bk;
          const uint32_t sh = (c & 3u) << 3;
          const uint32_t old = (atomicAdd(&lds[c >> 2], ik[k] << sh) >> sh) & 255u;  // < 2^8: no carry
          sq += (2u * old + ik[k]) * ik[k];
          vmax = max(vmax, old + ik[k]);
        }
      sq = wave_sum_u32(sq);  // <= mass * 255 < 2^16
      if ((tid & 63) == 0 && sq) atomicAdd(&s_norm[d], (unsigned long long)sq);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
    if ((tid & 63) == 0 && vmax) atomicMax(&s_max, vmax);
    mass = wave_sum_u32(mass);
    if ((tid & 63) == 0 && mass) atomicAdd(&s_mass, mass);
    __syncthreads();
    uint4* d4 = reinterpret_cast<uint4*>(lst);
#ifdef CMS_BUILD_NOWRITE  // bound analysis only: no table stores
    if (false)
#endif
    if (!keep_list)
      for (int j = tid; j < nq; j += kBuildThreads) store_row(d4 + j, l4[j], SV);
    if (badv) atomicOr(flags, kFlagBadValue);
    if (tid < hp.depth) norm[row * hp.depth + tid] = s_norm[tid];
    if (tid == 0) {
      rowmax[row] = s_max;
      row_mass[row] = s_mass;
      hidx_w[row] = keep_list ? kFormList : kFormU8;
      cbound[row] = s_max;
    }
    __syncthreads();  // the image and the shared sums are consumed before the next owner
  }
}

// Hot (split) owners with unit increments: one workgroup per SLICE of up to
// kHotSlice keys, all d sketch rows counted at once in an LDS image of u16
// counters ([d][w] u16: a slice of < 2^16 >> frac_bits unit increments cannot
// carry out of one), so each key is read and hashed ONCE (k_build_rows walks
// a slice's keys once per pair of sketch rows).  The image is added into the
// owner's u32 slot row (zeroed by promote_rows, or the old counters of an
// accumulating build) with 64-bit global atomics, two adjacent counters per
// add: a counter stays below its row mass < 2^32, so the low half never
// carries into the high one.  Bigger slices than k_build_rows' mean fewer
// dense slice images added into the slots.  No static LDS: two 80 KB images
// share a CU at d = 5, w = 8192.
constexpr int kSliceThreads = 512;
// a fresh build's single-slice owners store their slot rows whole (no slot
// zeroing, no 64-bit slot atomics; norms from the same pass)
constexpr bool kWholeSlices = true;
constexpr int64_t kHotSlice = 65535;  // keys per slice (u16 image, frac_bits 0)
// D: the depth when it is 4 or 5 (rows unrolled: RowHash at a power-of-two
// width, else each_bucket), else 0
template <int D>
__global__ __launch_bounds__(kSliceThreads) void k_build_slices(const int64_t* lo_, const int64_t* hi_, Keys keys,
                                                                HashParams hp, int64_t slice, const HotInfo* hot,
                                                                const int2* smap, const uint32_t* counters,
                                                                TableView tv, uint64_t* row_mass, uint32_t* flags,
                                                                int whole, uint64_t* norm, uint32_t* rowmax) {
  extern __shared__ __align__(16) uint32_t lds[];  // [d * w / 2] words, two u16 counters each
  const uint32_t nsl = counters[1];
  if (blockIdx.x >= nsl) return;
  const int tid = threadIdx.x;
  // a Zipf head owner has hundreds of slices, adjacent in smap: workgroups
  // take the slices in a strided order (a prime stride is a bijection unless
  // it divides the count) so the ones running together belong to many owners
  // and their row adds do not all land on one 160 KB slot row at once
  const uint32_t stride = (nsl % 7919u) ? 7919u : 7907u;
  const uint32_t sidx = (uint32_t)(((uint64_t)blockIdx.x * stride) % nsl);  // the mapped slice
  const int2 m = smap[sidx];
  const int64_t row = hot[m.x].row;
  const int64_t lo = lo_[row] + (int64_t)m.y * slice;
  const int64_t end = min(hi_[row], lo + slice);
  const int w = (int)hp.width;
  const int64_t dw = (int64_t)hp.depth * w;
  const int words = (int)(dw >> 1);
  uint4* l4 = reinterpret_cast<uint4*>(lds);
  for (int j = tid; j < (words >> 2); j += kSliceThreads) l4[j] = make_uint4(0, 0, 0, 0);
  for (int j = (words & ~3) + tid; j < words; j += kSliceThreads) lds[j] = 0u;
  __syncthreads();
  const uint32_t one = 1u << hp.frac_bits;
  // eight keys per thread per step (4: the same time, profiles/r04/ab_*_s5);
  // the next step's eight loads are issued before this step's keys are
  // hashed, so a key load's latency is hidden behind the previous keys' d x 8
  // hashes and LDS adds
  constexpr int kPer = 8;
  auto add = [&](int r, uint32_t bk) {
    const uint32_t c = (uint32_t)r * (uint32_t)w + bk;
#ifdef CMS_BUILD_NOLDSADD  // bound analysis only: hashes kept live, no LDS adds
    if (c == 0xFFFFFFFFu)
#endif
    atomicAdd(&lds[c >> 1], one << ((c & 1u) << 4));
  };
  if (kRowHash && D > 0 && hp.fastq) {  // (kernel-uniform)
    // a key's D rows hashed branch-free into registers (RowHash, cms_hash.h),
    // one branch per key, then its D adds back to back: the word of counter
    // (r, bk) is at byte r * 2w | ((bk << 1) & ~3) (w is a power of two) and
    // the shift of its half takes the low five bits of bk << 4
    constexpr int DR = D > 0 ? D : 1;
    RowHash<DR> rh(hp);
    rh.vgpr();
    const uint32_t w2 = 2u * (uint32_t)w;
    auto add_rows = [&](const uint32_t (&bk)[DR]) {
#pragma unroll
      for (int r = 0; r < D; ++r) {
        uint32_t* p = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + ((uint32_t)r * w2 | ((bk[r] << 1) & ~3u)));
#ifdef CMS_BUILD_NOLDSADD
        if (bk[r] == 0xFFFFFFFFu)
#endif
        atomicAdd(p, one << ((bk[r] << 4) & 31u));
      }
    };
    auto redo_key = [&](uint64_t kp) {  // about 1 key in 6,500, and every key that is no u32
#pragma unroll 1
      for (int r = 0; r < D; ++r) add(r, bucket(hp, r, kp));
    };
    if (keys.tok) {
      // a token below kTokEscape is the reduced key, a u32 below 2^31; an
      // escaped one is resolved (from the batch's keys) in the redo
      const uint32_t* tok = keys.tok;
      key_pass<uint32_t, kPer, kSliceThreads>(
          lo, end, tid, [&](int64_t i) { return tok[i]; },
          [&](uint32_t t) {
            uint32_t bk[DR];
            if (rh.rows32(t, bk) || t >= kTokEscape) return true;
            add_rows(bk);
            return false;
          },
          [&](uint32_t t) { redo_key(keys.resolve(t)); });
    } else {
      const int64_t* key = keys.key;
      key_pass<int64_t, kPer, kSliceThreads>(
          lo, end, tid, [&](int64_t i) { return key[i]; },
          [&](int64_t k) {
            uint32_t bk[DR];
            if (rh.rows(reduce_key(k), bk)) return true;
            add_rows(bk);
            return false;
          },
          [&](int64_t k) { redo_key(reduce_key(k)); });
    }
  } else {
    key_pass<uint64_t, kPer, kSliceThreads>(
        lo, end, tid, [&](int64_t i) { return keys.raw(i); },
        [&](uint64_t raw) {
          each_bucket<D>(hp, keys.resolve(raw), add);
          return false;
        },
        NoRedo{});
  }
  __syncthreads();
  if (whole && hot[m.x].nslices == 1) {
    // the owner's only slice, in a fresh build: its slot row is the image
    // itself (the slot was not zeroed), stored whole as u32 counters with
    // 16-B non-temporal stores; its sums of squares and largest counter come
    // from the same pass (k_hot_norms skips it)
    u32x4_t* o4 = reinterpret_cast<u32x4_t*>(tv.hot + (int64_t)tv.hidx[row] * dw);
    const uint2* s2 = reinterpret_cast<const uint2*>(lds);
    uint32_t vmax = 0;
    for (int r = 0; r < hp.depth; ++r) {
      uint64_t sq = 0;
      const int q0 = r * (w >> 2), q1 = q0 + (w >> 2);  // uint4 of u32 counters (4 per) of sketch row r
      for (int q = q0 + tid; q < q1; q += kSliceThreads) {
        const uint2 v = s2[q];  // four u16 counters
        const uint32_t c0 = v.x & 0xFFFFu, c1 = v.x >> 16, c2 = v.y & 0xFFFFu, c3 = v.y >> 16;
        sq += (uint64_t)c0 * c0 + (uint64_t)c1 * c1 + (uint64_t)c2 * c2 + (uint64_t)c3 * c3;
        vmax = max(max(vmax, max(c0, c1)), max(c2, c3));
        const u32x4_t x = {c0, c1, c2, c3};
        __builtin_nontemporal_store(x, o4 + q);
      }
      sq = wave_sum_u64_sat(sq);  // (no static LDS: two 80 KB images share a CU)
      if ((tid & 63) == 0 && sq) atomicAdd((unsigned long long*)&norm[row * hp.depth + r], (unsigned long long)sq);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
    if ((tid & 63) == 0 && vmax) atomicMax(&rowmax[row], vmax);
  } else {
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(tv.hot + (int64_t)tv.hidx[row] * dw);
    // the slices of one owner start their sweep at different 512-B-aligned
    // offsets of the slot row (same-address atomics from many workgroups queue)
    const int units = (words + 63) >> 6;
    const int rot = (int)(((uint32_t)m.y * 2654435761u >> 8) % (uint32_t)units) << 6;
    for (int jj = tid; jj < words; jj += kSliceThreads) {
      const int j = jj + rot < words ? jj + rot : jj + rot - words;
      const uint32_t v = lds[j];
#ifdef CMS_BUILD_NOSLICEADD  // bound analysis only: the slices' global atomics skipped
      if (v == 0xFFFFFFFFu)
#endif
      if (v) atomicAdd(dst + j, (unsigned long long)(v & 0xFFFFu) | ((unsigned long long)(v >> 16) << 32));
    }
  }
  if (tid == 0) {
    const uint64_t tm = (uint64_t)(end - lo) * one;
    const unsigned long long old = atomicAdd((unsigned long long*)&row_mass[row], (unsigned long long)tm);
    if (old + tm >= (1ULL << 32)) atomicOr(flags, kFlagOverflow);
  }
}

// Sum of squares of the hot rows after every slice landed; grid (<= 256, depth,
// chunks of 1024), blocks striding over the hot rows the plan counted (the
// host's bound on them is loose, and empty blocks still cost launch time).
// Norms and maxima of the hot (u32 slot) rows: one workgroup per (row,
// sketch row) at a time, the whole w counters in 16-byte loads (eight in
// flight per thread at w = 8192), one block reduction per sketch row.
// whole_slices (0 or 1): single-slice rows already have their norms
// (k_build_slices stored them whole) and are skipped.
__global__ __launch_bounds__(256) void k_hot_norms(const HotInfo* hot, const uint32_t* counters, HashParams hp,
                                                   TableView tv, uint64_t* norm, uint32_t* rowmax, int whole_slices) {
  __shared__ uint64_t red[4];
  const uint32_t nhot = counters[0];
  const int d = blockIdx.y;
  const int w = (int)hp.width;
  for (uint32_t hb = blockIdx.x; hb < nhot; hb += gridDim.x) {
    if (hot[hb].nslices <= whole_slices) continue;  // (uniform per block; a hot row has at least one slice)
    const int64_t row = hot[hb].row;
    const uint32_t* p = tv.hot + (int64_t)tv.hidx[row] * tv.dw + (int64_t)d * w;  // split rows are slots
    uint64_t sq = 0;
    uint32_t vmax = 0;
    if ((w & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
      const uint4* p4 = reinterpret_cast<const uint4*>(p);
      for (int j = threadIdx.x; j < (w >> 2); j += 256) {
        const uint4 v = p4[j];
        sq = sat_add(sq, (uint64_t)v.x * v.x + (uint64_t)v.y * v.y);
        sq = sat_add(sq, (uint64_t)v.z * v.z + (uint64_t)v.w * v.w);
        vmax = max(vmax, max(max(v.x, v.y), max(v.z, v.w)));
      }
    } else {
      for (int j = threadIdx.x; j < w; j += 256) {
        sq = sat_add(sq, (uint64_t)p[j] * p[j]);
        vmax = max(vmax, p[j]);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
    if ((threadIdx.x & 63) == 0 && vmax) atomicMax(&rowmax[row], vmax);
    uint64_t tot = block_sum_u64_sat(sq, red);
    if (tot > (1ULL << 60)) tot = 1ULL << 60;
    if (threadIdx.x == 0) atomicAdd((unsigned long long*)&norm[row * hp.depth + d], (unsigned long long)tot);
  }
}

int row_bounds(cms_handle* h, const int64_t* d_lo, const int64_t* d_hi, const float* d_val, const uint64_t* old_mass,
               int64_t slice, uint64_t* bound, uint8_t* force) {
  const int64_t n = h->n;
  if (d_val)
    hipLaunchKernelGGL(k_row_bound_values, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(n, 65536))),
                       dim3(256), 0, h->stream, d_lo, d_hi, d_val, n, h->hp.frac_bits, slice, old_mass, bound, force);
  else
    hipLaunchKernelGGL(k_row_bound_implicit, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096))),
                       dim3(256), 0, h->stream, d_lo, d_hi, n, h->hp.frac_bits, slice, old_mass, bound, force);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int ingest_csr_device(cms_handle* h, const int64_t* d_off, const int64_t* d_key, const float* d_val, int64_t npairs) {
  h->rf_valid = false;  // CSR batches do not mark touched owners: the next refresh is a full job
  return ingest_spans_device(h, d_off, d_off + 1, d_key, nullptr, d_val, npairs);
}

int ingest_spans_device(cms_handle* h, const int64_t* d_lo, const int64_t* d_hi, const int64_t* d_key,
                        const uint32_t* d_tok, const float* d_val, int64_t npairs) {
  const Keys keys{d_key, d_tok};
  const int64_t n = h->n;
  int rc0;
  const int accumulate = h->empty ? 0 : 1;
  // Rows with more than kSplit keys are hot: a u32 slot, built in slices.
  // kSplit: 8192 keys, or 16384 for rows of 8192+ counters (config 3: build
  // 19.4 -> 18.5 ms; config 2 prefers 8192).
  int64_t kSplit = cms::kSlice;
  if (h->p.width >= 8192) kSplit *= 2;
  if (h->tune.split_keys > 0) kSplit = h->tune.split_keys;
  // Unit increments whose [d][w] u16 image fits a workgroup's LDS: the
  // slices (every one, slice 0 included) run on k_build_slices, kHotSlice
  // keys each, one key pass.  Otherwise (weighted increments, wide shapes)
  // k_build_rows builds slices of kSplit keys, a pass per pair of sketch rows.
  const size_t img_lds = (size_t)h->dw * 2;
  const bool fast_slices = !d_val && (h->dw % 8) == 0 && img_lds <= 80 * 1024 && h->hp.frac_bits < 16;
  const int64_t kSliceKeys = fast_slices ? (kHotSlice >> h->hp.frac_bits) : kSplit;
  // a fresh build: single-slice owners store their slot rows whole
  // (k_build_slices), so their slots are not zeroed by the promotion
  const int whole_slices =
      kWholeSlices && fast_slices && !accumulate && (h->p.width % 4) == 0 ? 1 : 0;
  const int64_t max_hot = std::min<int64_t>(n, npairs / kSplit + 1);
  const int64_t emax = npairs / kSliceKeys + max_hot + 1;  // mapped slices
  const size_t sz_rowhot = (sizeof(int32_t) * (size_t)n + 15) & ~size_t(15);
  const size_t sz_hot = (sizeof(HotInfo) * (size_t)max_hot + 15) & ~size_t(15);
  const size_t sz_extra = sizeof(int2) * (size_t)emax;
  CMS_HIP(h->ws_hot.ensure(sz_rowhot + sz_hot + sz_extra + 64));
  char* base = h->ws_hot.as<char>();
  int32_t* row_hot = reinterpret_cast<int32_t*>(base);
  HotInfo* hot = reinterpret_cast<HotInfo*>(base + sz_rowhot);
  int2* extra_map = reinterpret_cast<int2*>(base + sz_rowhot + sz_hot);
  uint32_t* counters = h->d_flags + 4;  // [4..7]: hot rows, mapped slices (one u64 atomic), spare
  // A fresh unit-increment build right after a partition that marked its
  // spans (ingest_coo): the plan below needs only the spans, so it runs on
  // the side stream beside the partition's last scatter (h->stream swapped
  // for the section; joined back before the build reads the keys).
  struct PlanSide {
    cms_handle* h;
    bool on = false;
    void end() {
      if (!on) return;
      on = false;
      std::swap(h->stream, h->side_stream);
      h->plan_side_active = false;
      if (hipEventRecord(h->ev_plan, h->side_stream) == hipSuccess) (void)hipStreamWaitEvent(h->stream, h->ev_plan, 0);
    }
    ~PlanSide() { end(); }
  } plan_side{h};
  if (h->spans_event && !accumulate && !d_val && h->side_stream) {
    h->spans_event = false;
    CMS_HIP(hipStreamWaitEvent(h->side_stream, h->ev_spans, 0));
    std::swap(h->stream, h->side_stream);
    h->plan_side_active = true;  // nothing in the section may launch on h->side_stream (it is the main stream now)
    plan_side.on = true;
  }
  CMS_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), h->stream));
  // table layout: rows that could reach 2^16, and split rows, get u32 slots
  {
    TimedScope ts(h, "build_plan");
    if (!accumulate && (rc0 = reset_table_layout(h))) return rc0;
    DevBuf& bound = h->ws_bound;
    DevBuf& force = h->ws_force;
    CMS_HIP(bound.ensure(sizeof(uint64_t) * (size_t)std::max<int64_t>(n, 1)));
    CMS_HIP(force.ensure((size_t)std::max<int64_t>(n, 1)));
    if ((rc0 = row_bounds(h, d_lo, d_hi, d_val, accumulate ? h->d_row_mass : nullptr, kSplit, bound.as<uint64_t>(),
                          force.as<uint8_t>())))
      return rc0;
    // A fresh build with implicit (unit) increments: a row needs a slot when
    // it is split (more than kSplit keys: at most npairs / (kSplit + 1) rows)
    // or its mass reaches 2^16 (at most total / 2^16 rows; with
    // 2^(16 - s) > kSplit keys such a row is split anyway) -- a bound the host
    // knows without reading anything back.  Reserving costs slot memory, so
    // only a bound worth at most 2 GB of slots takes this path; a larger job
    // reads the count back.
    int64_t max_new = -1;
    if (!accumulate && !d_val && h->hp.frac_bits < 16) {
      const int64_t split = npairs / (kSplit + 1) + 1;
      const int64_t heavy = (int64_t)(((uint64_t)npairs << h->hp.frac_bits) / kNarrowLimit);
      const int64_t slots = (int64_t(1) << (16 - h->hp.frac_bits)) > kSplit ? split : split + heavy;
      if ((double)slots * (double)h->dw * 4.0 <= 2.0e9) max_new = slots;
    }
    // a fresh build's single-slice owners store their slot rows whole
    // (k_build_slices): their slots are not zeroed first
    const uint64_t whole_bound = whole_slices ? (uint64_t)kSliceKeys << h->hp.frac_bits : 0;
    if ((rc0 = promote_rows(h, bound.as<uint64_t>(), force.as<uint8_t>(), accumulate != 0, max_new, whole_bound)))
      return rc0;
    // accumulating: every touched u8 / nibble row becomes u16 first (the build
    // adds into u16 or u32 rows); untouched rows are skipped by the build when
    // their norms are current, otherwise every form row is widened
    if (accumulate &&
        (rc0 = widen_rows(h, h->norms_valid ? bound.as<uint64_t>() : nullptr, h->d_row_mass, true, d_lo, d_hi)))
      return rc0;
  }
  {
    TimedScope ts(h, "build_plan");
    unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_build_plan, dim3(grid), dim3(256), 0, h->stream, d_lo, d_hi, n, kSplit, kSliceKeys,
                       fast_slices ? 0 : 1, row_hot, hot, extra_map, counters, h->d_norm, h->d_rowmax, h->p.depth);
    CMS_HIP(hipGetLastError());
  }
  // fresh builds may store byte forms: the whole [d][w] byte image in LDS
  const int forms = h->forms_ok && !accumulate && (size_t)h->dw <= kFormLdsMax ? 1 : 0;
  if (h->compact && !accumulate) {
    // the compact layout: capacities by class, their scan, the arena sized
    // (the one read-back of the build; beside the last scatter when the
    // plan runs on the side stream)
    TimedScope ts(h, "build_plan");
    CMS_HIP(h->ws_layout.ensure(sizeof(uint32_t) * (size_t)(2 * n + n / 4096 + 16)));
    uint32_t* caps = h->ws_layout.as<uint32_t>();
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_row_caps, dim3(grid), dim3(256), 0, h->stream, d_lo, d_hi, n, h->ws_bound.as<uint64_t>(),
                       h->d_hidx, forms, d_val ? 1 : 0, h->hp.frac_bits, h->p.depth, h->p.width, h->tune.bit_keys,
                       h->tune.crumb_keys, lists_allowed(h) ? h->tune.list_keys : 0, caps);
    CMS_HIP(hipGetLastError());
    if ((rc0 = row_layout(h, caps, caps + n))) return rc0;
  }
  plan_side.end();
  const int skip_untouched = accumulate && h->norms_valid ? 1 : 0;
  const size_t lds = sizeof(uint32_t) * (size_t)((h->p.width + 3) & ~3);
  // k_build_rows: with fast slices it builds only the unsplit slot rows
  const int64_t row_emax = fast_slices ? 0 : emax;
  const int slices_done = fast_slices ? 1 : 0;
  bool hot_norms_done = false;
  auto launch_hot_norms = [&]() -> int {
    TimedScope ts(h, "hot_norms");
    dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(max_hot, 1024)), (unsigned)h->p.depth);
    hipLaunchKernelGGL(k_hot_norms, grid, dim3(256), 0, h->stream, hot, counters, h->hp, h->tview(), h->d_norm,
                       h->d_rowmax, whole_slices);
    CMS_HIP(hipGetLastError());
    hot_norms_done = true;
    return CMS_OK;
  };
  {
    TimedScope ts(h, "build_rows");
    auto kern = k_build_rows<kBuildStoreForm>;
    // the split owners' slices, on the handle's stream (after the side stream
    // forks, so they overlap the byte and mid classes)
    auto launch_slices = [&]() -> int {
      if (!fast_slices) return CMS_OK;
#ifdef CMS_BUILD_SKIP_SLICES  // bound analysis only: the split owners' slices not built (wrong table)
      return CMS_OK;
#endif
      static bool attr = [] {
        for (const void* f : {(const void*)k_build_slices<0>, (const void*)k_build_slices<4>,
                              (const void*)k_build_slices<5>})
          (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        return true;
      }();
      (void)attr;
      auto kslices = h->p.depth == 5 ? k_build_slices<5> : h->p.depth == 4 ? k_build_slices<4> : k_build_slices<0>;
      hipLaunchKernelGGL(kslices, dim3((unsigned)emax), dim3(kSliceThreads), img_lds, h->stream, d_lo, d_hi,
                         keys, h->hp, kSliceKeys, hot, extra_map, counters, h->tview(), h->d_row_mass, h->d_flags,
                         whole_slices, h->d_norm, h->d_rowmax);
      CMS_HIP(hipGetLastError());
      return CMS_OK;
    };
    if (forms) {
      // owner classes: slot rows -> k_build_slices / k_build_rows (the
      // handle's stream), byte rows -> k_build_nibbles (+ k_build_bytes for
      // the ones a counter >= 16 sends back) and mid rows -> k_build_mid on the
      // side stream, so the classes' kernels overlap (their tails no longer
      // leave CUs idle)
      CMS_HIP(h->ws_blist.ensure(sizeof(int32_t) * (size_t)(4 * n + kCntWords)));
      int32_t* slot_list = h->ws_blist.as<int32_t>();
      int32_t* mid_list = slot_list + n;     // two-ended: sent-back streamed owners and list rows, cached owners
      int32_t* stream_list = mid_list + n;   // two-ended: owners above kStreamBigKeys keys, the others
      int32_t* mid_lists = stream_list + n;  // the cached owners of k_build_mid_lists
      uint32_t* lcnt = reinterpret_cast<uint32_t*>(mid_lists + n);  // kCnt*
      CMS_HIP(h->ws_plist.ensure(sizeof(int32_t) * (size_t)(n + 1)));
      int32_t* redo = h->ws_plist.as<int32_t>();
      uint32_t* redo_cnt = reinterpret_cast<uint32_t*>(redo + n);
      // the byte class's list rows in a kernel of their own where it exists:
      // unit increments, a power-of-two width, an unrolled depth
#if defined(CMS_BUILD_CHEAPHASH) || defined(CMS_BUILD_GATHERHASH)  // (those replace bucket(), which it does not call)
      const int lists_done = 0;
#else
      const int lists_done = !d_val && h->hp.frac_bits == 0 && h->hp.fastq && lists_allowed(h) &&
                                     (h->p.depth == 4 || h->p.depth == 5)
                                 ? 1
                                 : 0;
#endif
      // ... and the cached mid owners' (k_build_mid_lists), while a wave's
      // slot of w u8 counters leaves LDS for four waves per SIMD
      const bool mid_lists_done = lists_done && h->p.width <= kMidListSlotMax;
      CMS_HIP(hipMemsetAsync(lcnt, 0, kCntWords * sizeof(uint32_t), h->stream));
      CMS_HIP(hipMemsetAsync(redo_cnt, 0, sizeof(uint32_t), h->stream));
      hipLaunchKernelGGL(k_build_classes,
                         dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kClassChunk - 1) / kClassChunk, 1024))),
                         dim3(256), 0, h->stream, d_lo, d_hi, n, h->d_hidx, h->ws_bound.as<uint64_t>(), slot_list,
                         mid_list, stream_list, lcnt, mid_lists, mid_lists_done ? kMidListKeys : 0, h->p.depth,
                         h->p.width);
      CMS_HIP(hipGetLastError());
      if (h->plan_side_active) return set_error(CMS_E_STATE, "internal: side stream used while swapped for the plan");
      hipStream_t side = h->side_stream ? h->side_stream : h->stream;
#ifdef CMS_BUILD_SERIAL  // bound analysis only: the classes' kernels one after another (isolated durations)
      side = h->stream;
#endif
      // once the side stream has forked, every exit (error returns included)
      // joins it back: the caller's next work on h->stream may reuse or free
      // the buffers the side kernels are still writing
      // the mid class on a third stream (Tunables::build_streams == 3)
      const hipStream_t side2 = side != h->stream && h->tune.build_streams >= 3 ? h->side_stream2 : side;
      struct SideJoin {
        cms_handle* h;
        hipStream_t side, side2;
        bool armed = false;
        ~SideJoin() {
          if (armed && hipEventRecord(h->ev_join2, side) == hipSuccess)
            (void)hipStreamWaitEvent(h->stream, h->ev_join2, 0);
          if (armed && side2 != side && hipEventRecord(h->ev_join3, side2) == hipSuccess)
            (void)hipStreamWaitEvent(h->stream, h->ev_join3, 0);
        }
      } join{h, side, side2};
      if (side != h->stream) {
        CMS_HIP(hipEventRecord(h->ev_fork2, h->stream));
        CMS_HIP(hipStreamWaitEvent(side, h->ev_fork2, 0));
        if (side2 != side) CMS_HIP(hipStreamWaitEvent(side2, h->ev_fork2, 0));
        join.armed = true;
      }
      const int64_t nib_blocks = (n + kNibWaves - 1) / kNibWaves;
      const size_t nib_lds = (size_t)kNibWaves * (size_t)h->p.width / 2;
      // the cached mid owners' list rows first on the byte class's stream: the
      // cached k_build_mid on the other side stream waits for them, since it
      // builds the owners they send back
      if (mid_lists_done) {
        auto kml = h->p.depth == 5 ? k_build_mid_lists<kBuildStoreForm, 5> : k_build_mid_lists<kBuildStoreForm, 4>;
        const size_t ml_lds = (size_t)kMidListWaves * (size_t)h->p.width;
        if (h->mid_lists_wgs_per_cu <= 0) {  // a grid that is resident whole (wave g takes list entries g, g + G, ...)
          int per_cu = 0;
          CMS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kml, 64 * kMidListWaves, ml_lds));
          h->mid_lists_wgs_per_cu = std::max(1, per_cu);
        }
        const int64_t ml_blocks = std::min<int64_t>((n + kMidListWaves - 1) / kMidListWaves,
                                                    (int64_t)h->num_cus * h->mid_lists_wgs_per_cu);
        hipLaunchKernelGGL(kml, dim3((unsigned)ml_blocks), dim3(64 * kMidListWaves), ml_lds, side, d_lo, d_hi, keys,
                           h->hp, (const int32_t*)mid_lists, (const uint32_t*)(lcnt + kCntMidLists), h->tview(),
                           h->d_hidx, h->d_cbound, h->d_row_mass, h->d_norm, h->d_rowmax, mid_list, lcnt + kCntMid);
        CMS_HIP(hipGetLastError());
        if (side2 != side) CMS_HIP(hipEventRecord(h->ev_mid_lists, side));
      }
      if (lists_done) {
        auto klists = h->p.depth == 5 ? k_build_lists<kBuildStoreForm, 5> : k_build_lists<kBuildStoreForm, 4>;
        // a grid that is resident whole (wave g takes rows g, g + G, ...):
        // 0.87 ms alone against 0.91 ms with one owner per wave
        if (h->lists_wgs_per_cu <= 0) {
          int per_cu = 0;
          CMS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, klists, 64 * kNibWaves, nib_lds));
          h->lists_wgs_per_cu = std::max(1, per_cu);
        }
        const int64_t lists_blocks = std::min<int64_t>(nib_blocks, (int64_t)h->num_cus * h->lists_wgs_per_cu);
        hipLaunchKernelGGL(klists, dim3((unsigned)lists_blocks), dim3(64 * kNibWaves), nib_lds, side, d_lo, d_hi, keys,
                           n, h->hp, row_hot, h->ws_bound.as<uint64_t>(), h->tview(), h->d_hidx, h->d_cbound,
                           h->d_row_mass, h->d_norm, h->d_rowmax, redo, redo_cnt, h->tune.bit_keys,
                           h->tune.crumb_keys, h->tune.list_keys);
      }
      // with unit increments a byte-class owner has at most 255 keys (its
      // bound): where every such key count makes a list row (config 3),
      // k_build_nibbles would only read each row's spans and return (0.28 ms)
      bool nibbles_idle = lists_done != 0;
      for (int64_t m = 0; nibbles_idle && m < kByteKeys; ++m)
        nibbles_idle = nib_list_row(m, h->p.width, h->p.depth, false, 0, h->tune.bit_keys, h->tune.crumb_keys,
                                    h->tune.list_keys);
      if (!nibbles_idle)
        hipLaunchKernelGGL((k_build_nibbles<kBuildStoreForm, 0>), dim3((unsigned)nib_blocks), dim3(64 * kNibWaves),
                           nib_lds, side, d_lo, d_hi, keys, d_val, n, h->hp, row_hot, h->ws_bound.as<uint64_t>(),
                           h->tview(), h->d_hidx, h->d_cbound, h->d_row_mass, h->d_norm, h->d_rowmax, h->d_flags,
                           redo, redo_cnt, h->tune.bit_keys, h->tune.crumb_keys,
                           lists_allowed(h) ? h->tune.list_keys : 0, lists_done);
      // LDS: the [d][w] 4-bit image, or one sketch row of u16 counters
      const size_t mid_lds = std::max<size_t>((size_t)h->p.width * 2, (size_t)h->dw / 2);
      auto kmid = h->p.depth == 5   ? k_build_mid<kBuildStoreForm, 5, kMidThreads>
                  : h->p.depth == 4 ? k_build_mid<kBuildStoreForm, 4, kMidThreads>
                                    : k_build_mid<kBuildStoreForm, 0, kMidThreads>;
      auto launch_mid = [&](auto kern, int threads, unsigned grid, size_t klds, const int32_t* list, uint32_t* cnt) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), klds, side2, d_lo, d_hi, keys, d_val, h->hp, list,
                           (const uint32_t*)cnt, (uint32_t)n, h->tview(), h->d_hidx, h->d_cbound, h->d_row_mass,
                           h->d_norm, h->d_rowmax, h->d_flags, lists_allowed(h) ? kMidListKeys : 0,
                           h->tune.mid_u4_keys, h->tune.mid_u8_keys, mid_list, lcnt + kCntMid, lcnt + kCntTicket);
      };
      const unsigned mid_grid = (unsigned)std::min<int64_t>(n, (int64_t)h->num_cus * kMidGridPerCu);
      // the streamed owners first (the long work), in one key pass each when
      // the increments are units (forms: the [d][w] u8 image fits kFormLdsMax);
      // then the cached owners behind the streamed ones sent back for u16 rows
      bool one_pass = !d_val && h->hp.frac_bits == 0;
#ifdef CMS_BUILD_NO_STREAMED  // bound analysis only: the streamed owners row at a time (k_build_mid once per list)
      one_pass = false;
#endif
      if (one_pass) {
        auto kstr = h->p.depth == 5   ? k_build_mid<kBuildStoreForm, 5, kStreamThreads>
                    : h->p.depth == 4 ? k_build_mid<kBuildStoreForm, 4, kStreamThreads>
                                      : k_build_mid<kBuildStoreForm, 0, kStreamThreads>;
        const size_t str_lds = std::max<size_t>((size_t)h->dw, sizeof(uint32_t) * kStreamRedWords);
        if (h->stream_wgs_per_cu <= 0) {  // a grid that is resident whole (workgroups take owners by ticket)
          int per_cu = 0;
          CMS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kstr, kStreamThreads, str_lds));
          h->stream_wgs_per_cu = std::max(1, per_cu);
        }
        launch_mid(kstr, kStreamThreads, (unsigned)std::min<int64_t>(n, (int64_t)h->num_cus * h->stream_wgs_per_cu),
                   str_lds, stream_list, lcnt + kCntStream);
      } else {
        launch_mid(kmid, kMidThreads, mid_grid, mid_lds, stream_list, lcnt + kCntStream);
      }
      if (mid_lists_done && side2 != side) CMS_HIP(hipStreamWaitEvent(side2, h->ev_mid_lists, 0));
      launch_mid(kmid, kMidThreads, mid_grid, mid_lds, mid_list, lcnt + kCntMid);
      hipLaunchKernelGGL(k_build_bytes<kBuildStoreForm>, dim3((unsigned)std::min<int64_t>(n, (int64_t)h->num_cus * 2)),
                         dim3(kBuildThreads), (size_t)h->dw, side, d_lo, d_hi, keys, d_val, h->hp, redo, redo_cnt,
                         h->tview(), h->d_hidx, h->d_cbound, h->d_row_mass, h->d_norm, h->d_rowmax, h->d_flags);
      CMS_HIP(hipGetLastError());
      if ((rc0 = launch_slices())) return rc0;
      // slot rows: at most the slots in use (host-known), plus the mapped slices
      const int64_t nslot = std::min<int64_t>(n, h->hot_used);
      hipLaunchKernelGGL(kern, dim3((unsigned)(row_emax + nslot)), dim3(kBuildThreads), lds, h->stream, d_lo, d_hi,
                         keys, d_val, n, h->hp, kSliceKeys, row_hot, hot, extra_map, counters, row_emax, h->tview(),
                         h->d_row_mass, h->d_norm, h->d_rowmax, h->d_flags, accumulate, slices_done,
                         h->ws_bound.as<uint64_t>(), forms, skip_untouched, h->d_hidx, h->d_cbound,
                         (const int32_t*)slot_list, (const uint32_t*)lcnt);
      CMS_HIP(hipGetLastError());
      // (k_hot_norms here, overlapping the side streams' tail, measured no
      // faster: it competes with them for the CUs)
      if (join.armed) {
        join.armed = false;
        CMS_HIP(hipEventRecord(h->ev_join2, side));
        CMS_HIP(hipStreamWaitEvent(h->stream, h->ev_join2, 0));
        if (side2 != side) {
          CMS_HIP(hipEventRecord(h->ev_join3, side2));
          CMS_HIP(hipStreamWaitEvent(h->stream, h->ev_join3, 0));
        }
      }
    } else {
      if ((rc0 = launch_slices())) return rc0;
      hipLaunchKernelGGL(kern, dim3((unsigned)(row_emax + n)), dim3(kBuildThreads), lds, h->stream, d_lo, d_hi, keys,
                         d_val, n, h->hp, kSliceKeys, row_hot, hot, extra_map, counters, row_emax, h->tview(),
                         h->d_row_mass, h->d_norm, h->d_rowmax, h->d_flags, accumulate, slices_done,
                         h->ws_bound.as<uint64_t>(), forms, skip_untouched, h->d_hidx, h->d_cbound,
                         (const int32_t*)nullptr, (const uint32_t*)nullptr);
      CMS_HIP(hipGetLastError());
    }
  }
  if (!hot_norms_done && (rc0 = launch_hot_norms())) return rc0;
  h->empty = false;
  h->norms_valid = true;  // build_rows + hot_norms wrote the norm of every row
  return CMS_OK;
}

}  // namespace cms
