// cms_rows.h -- device helpers shared by the kernels that re-encode whole owner
// rows, one workgroup of 256 lanes per row (cms_fold.hip: a row folded to a
// divisor width, or at its own width in its narrowest form).  Where a row's
// counters are now, 16 of them at a time out of any dense form and into
// any dense form, the payload checksum of what is stored, and the workgroup's
// reduce and scan.
#pragma once
#include <hip/hip_runtime.h>

#include "cms_checkpoint.h"
#include "cms_internal.h"

namespace cms {
namespace rows {

// where a row's counters are now: p null for an owner on the shared zero row;
// f the narrow form (kForm*, < 0), or 0 for the u32 counters of a hot slot
struct RowSrc {
  const uint8_t* p;
  int32_t f;
};
__device__ __forceinline__ RowSrc row_src(const TableView& tv, int64_t r) {
  const int32_t s = tv.hidx[r];
  if (s >= 0) return RowSrc{reinterpret_cast<const uint8_t*>(tv.hot + (int64_t)s * tv.dw), 0};
  const int64_t o = tv.off[r];
  if (o == 0) return RowSrc{nullptr, s};
  return RowSrc{reinterpret_cast<const uint8_t*>(tv.t16 + (o & ~kCapMask)), s};
}

// counters [j, j + 16) (j % 16 == 0) of a dense row
__device__ __forceinline__ void src16(const RowSrc& s, int64_t j, uint32_t (&v)[16]) {
  if (s.f >= 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 y = reinterpret_cast<const uint4*>(s.p + 4 * j)[k];
      v[4 * k] = y.x, v[4 * k + 1] = y.y, v[4 * k + 2] = y.z, v[4 * k + 3] = y.w;
    }
  } else {
    unpack16(s.f, s.p, j, v);
  }
}

// the workgroup's 256 values reduced; every lane returns the result
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* s_red, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o));
  __syncthreads();  // (s_red is free of its last use)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(s_red[0], s_red[1]), op(s_red[2], s_red[3]));
}

// exclusive prefix sum of v over the workgroup's 256 lanes
__device__ __forceinline__ uint32_t block_scan_exclusive(uint32_t v, uint32_t* s_wave) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int k = 0; k < wv; ++k) base += s_wave[k];
  return base + inc - v;
}

// ---- the packers: 16 counters at tb bits each into the row at `row`, and
// what the stored bytes add to the payload checksum (the sum of its
// little-endian u64 words: a store of k <= 8 bytes at an offset aligned to k
// adds its value shifted by the offset's place in the word; rows start on
// 16-byte boundaries) ----
__device__ __forceinline__ unsigned long long pair64(uint32_t lo, uint32_t hi) {
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
__device__ __forceinline__ void store_group(uint8_t* row, int64_t j, const uint32_t (&v)[16], int tb,
                                            unsigned long long& acc) {
  switch (tb) {
    case 1: {
      uint32_t x = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) x |= (v[q] & 1u) << q;
      const int64_t o = j >> 3;
      *reinterpret_cast<uint16_t*>(row + o) = (uint16_t)x;
      acc += (unsigned long long)x << (8 * (int)(o & 7));
      break;
    }
    case 2: {
      uint32_t x = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) x |= (v[q] & 3u) << (2 * q);
      const int64_t o = j >> 2;
      *reinterpret_cast<uint32_t*>(row + o) = x;
      acc += (unsigned long long)x << (8 * (int)(o & 7));
      break;
    }
    case 4: {
      uint32_t x[2] = {0, 0};
#pragma unroll
      for (int q = 0; q < 16; ++q) x[q >> 3] |= (v[q] & 15u) << (4 * (q & 7));
      *reinterpret_cast<uint2*>(row + (j >> 1)) = make_uint2(x[0], x[1]);
      acc += pair64(x[0], x[1]);
      break;
    }
    case 8: {
      uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < 16; ++q) x[q >> 2] |= (v[q] & 255u) << (8 * (q & 3));
      *reinterpret_cast<uint4*>(row + j) = make_uint4(x[0], x[1], x[2], x[3]);
      acc += pair64(x[0], x[1]) + pair64(x[2], x[3]);
      break;
    }
    case 16: {
      uint32_t x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = (v[2 * q] & 0xFFFFu) | (v[2 * q + 1] << 16);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        reinterpret_cast<uint4*>(row + 2 * j)[k] = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        acc += pair64(x[4 * k], x[4 * k + 1]) + pair64(x[4 * k + 2], x[4 * k + 3]);
      }
      break;
    }
    default: {  // u32 counters
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        reinterpret_cast<uint4*>(row + 4 * j)[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
        acc += pair64(v[4 * k], v[4 * k + 1]) + pair64(v[4 * k + 2], v[4 * k + 3]);
      }
      break;
    }
  }
}

// one counter at tb = 16 or 32 bits (shapes without forms: no group of 16 is whole)
__device__ __forceinline__ void store_counter(uint8_t* row, int64_t j, uint32_t v, int tb, unsigned long long& acc) {
  if (tb == 16) {
    *reinterpret_cast<uint16_t*>(row + 2 * j) = (uint16_t)v;
    acc += (unsigned long long)(v & 0xFFFFu) << (8 * (int)((2 * j) & 7));
  } else {
    *reinterpret_cast<uint32_t*>(row + 4 * j) = v;
    acc += (unsigned long long)v << (8 * (int)((4 * j) & 7));
  }
}

// bits per counter of a dense target form (ckpt::kRow*)
__device__ __forceinline__ int target_bits(int tf) {
  return tf == ckpt::kRowU1 ? 1 : tf == ckpt::kRowU2 ? 2 : tf == ckpt::kRowU4 ? 4 : tf == ckpt::kRowU8 ? 8
       : tf == ckpt::kRowU16 ? 16 : 32;
}

}  // namespace rows
}  // namespace cms
