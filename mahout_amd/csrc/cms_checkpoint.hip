// cms_checkpoint.hip -- checkpoint and restore of the sketch table
// (cms_save_table / cms_load_table and their device-image twins).
//
// The image (cms_checkpoint.h, DESIGN.md 3 "Checkpoint image") carries every
// owner row in the form the table stores it in -- a list row its 2 + 2 d m
// bytes, a 4-bit row d w / 2, a hot row its u32 counters -- so a config-3
// table leaves as the 2.65 GB it occupies, not as 164 GB of dense u32.  Save
// is a gather of the rows' stored bytes into one dense payload, load a
// scatter into a freshly laid-out arena (row_layout: no holes left by movers).
//
//   k_ckpt_dir     one pass over the owners: directory entry + source address
//   k_ckpt_pack    segmented copy driven by the DESTINATION: a workgroup takes
//                  a fixed 16 KB tile of the payload, finds the tile's first
//                  row by binary search, keeps the tile's row boundaries in
//                  LDS, and every lane moves 16-byte chunks.  A Zipf table has
//                  a few 160 KB hot rows and a million rows of about 1 KB: a
//                  workgroup per row would be unbalanced, a tile per
//                  workgroup is not.
//   k_ckpt_unpack  the same mapping in reverse; recomputes the checksum from
//                  what it read and validates list rows while copying
//   k_ckpt_expand  a handle without forms (CMS_NO_FORMS=1) receives narrow
//                  rows expanded to u16
//
// cms_merge_table adds an image into a live table (a count-min sketch is
// linear).  Every check precedes every write: k_ckpt_unpack<false> verifies
// the whole resident image without a store, then the in-place writers'
// promote / widen step prepares the live rows, then the image is applied.
// cms_subtract_table is the other half: image B's stream being a sub-stream of
// the live table's, table - B is the table of the remaining stream.  After the
// same verify pass a second pass compares every image counter with its live
// counter, in whatever form either row is in, and stores nothing; only then
// are live list rows rewritten densely (widen_rows) and the image subtracted.
// Adding, comparing and subtracting are one statement, instantiated by
// Apply::kAdd / kCheck / kSub:
//
//   k_ckpt_apply<Op>        dense image rows of any form against dense live
//                           rows of any form, on the unpack's source-driven
//                           tile mapping
//   k_ckpt_apply_lists<Op>  list image rows into dense live rows (kAdd, kSub),
//                           one workgroup per row, counted in LDS
//   k_ckpt_check_rows       the check of the rows where either side is a list
//
// The payload offsets are summed on the host from the directory's read-back
// (64-bit: 16-byte units of a 79 GB arena pass 2^32); the same read-back
// sizes the image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cms_checkpoint.h"
#include "cms_internal.h"

namespace cms {
namespace {

using namespace ckpt;

constexpr int kTileChunks = 1024;        // 16-byte chunks per workgroup tile (16 KB)
constexpr uint64_t kListBit = 1ull << 63;  // seg_len: the segment is a list row (validated by the unpack)
constexpr uint64_t kIoChunk = 64ull << 20;  // bytes per pinned staging buffer of the file path
enum : unsigned long long { kBadList = 1, kBadPad = 2, kBadDest = 4, kBadUnder = 8 };

// The rows that have stored bytes, in row order: payload byte offsets
// (off[nseg] = the payload's length), device addresses and lengths.
struct SegView {
  const uint64_t* off;   // [nseg + 1]
  const uint64_t* addr;  // [nseg]
  const uint64_t* len;   // [nseg] (| kListBit)
  int64_t nseg;
};

__global__ void k_ckpt_dir(TableView tv, const uint32_t* cbound, const uint64_t* mass, const double* t64, int64_t n,
                           int depth, int empty, DirEntry* dir, uint64_t* addr) {
  const int64_t dw = tv.dw;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    DirEntry e;
    e.form = kRowZero;
    e.cls = 0;
    e.rsv = 0;
    e.cbound = 0;
    e.len = 0;
    e.mass = mass[r];
    e.off = 0;
    uint64_t a = 0;
    if (empty) {
      // every counter is zero (the arrays below are stale)
    } else if (t64) {
      e.form = kRowF64;
      e.len = 8 * (uint64_t)dw;
      a = reinterpret_cast<uint64_t>(t64 + r * dw);
    } else {
      const int32_t s = tv.hidx[r];
      if (s >= 0) {
        e.form = kRowHot;
        e.len = 4 * (uint64_t)dw;
        a = reinterpret_cast<uint64_t>(tv.hot + (int64_t)s * dw);
      } else {
        const int64_t o = tv.off[r];
        e.cbound = cbound[r];
        if (o != 0) {  // (offset 0: the shared zero row)
          e.cls = (uint8_t)(o & kCapMask);
          a = reinterpret_cast<uint64_t>(tv.t16 + (o & ~kCapMask));
          if (s == kFormList) {
            e.form = kRowList;
            e.len = 2 + 2 * (uint64_t)depth * tv.list_m(r);
          } else {
            e.form = s == kFormU1 ? kRowU1 : s == kFormU2 ? kRowU2 : s == kFormU4 ? kRowU4 : s == kFormU8 ? kRowU8 : kRowU16;
            e.len = ((uint64_t)dw * (uint64_t)form_bits(s)) / 8;
          }
        }
      }
    }
    dir[r] = e;
    addr[r] = a;
  }
}

// ---- the tile mapping shared by pack and unpack ----

// The segments of the tile starting at chunk t0: first = the one holding its
// first byte, s_off[0 .. cnt) their payload offsets (a segment takes at least
// one chunk, so at most kTileChunks + 1 of them touch a tile).
__device__ __forceinline__ void tile_setup(const SegView& sv, uint64_t t0, uint64_t* s_off, int64_t& first, int& cnt) {
  const uint64_t pos = t0 * 16;
  int64_t lo = 0, hi = sv.nseg;  // first segment starting past pos
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sv.off[mid] <= pos) lo = mid + 1; else hi = mid;
  }
  first = lo - 1;  // (off[0] == 0 <= pos)
  cnt = (int)min<int64_t>(sv.nseg - first, kTileChunks + 1);
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) s_off[i] = sv.off[first + i];
  __syncthreads();
}
__device__ __forceinline__ int tile_find(const uint64_t* s_off, int cnt, uint64_t pos) {
  int lo = 0, hi = cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_off[mid] <= pos) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// 16 bytes of a row from p (4-byte aligned), of which rem (> 0, even) belong
// to the row: the others read as zero.  Arena rows are 128-byte aligned and
// take whole 128-byte units, so a list's last word is read inside its place;
// hot and fp64 rows are whole words.
__device__ __forceinline__ uint4 load16(const uint8_t* p, uint64_t rem) {
  if (rem >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4*>(p);
  const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = (uint64_t)(4 * k) < rem ? p32[k] : 0u;
    if (rem < 16 && (uint64_t)k == (rem >> 2) && (rem & 3)) w[k] &= (1u << (8 * (uint32_t)(rem & 3))) - 1u;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// the first rem (> 0, even) bytes of v to p (4-byte aligned): nothing past the row's end is written
__device__ __forceinline__ void store16(uint8_t* p, uint64_t rem, const uint4& v) {
  if (rem >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    *reinterpret_cast<uint4*>(p) = v;
    return;
  }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if ((uint64_t)(4 * k + 4) <= rem) reinterpret_cast<uint32_t*>(p)[k] = w[k];
    else if ((uint64_t)(4 * k + 2) <= rem) *reinterpret_cast<uint16_t*>(p + 4 * k) = (uint16_t)w[k];
  }
}
__device__ __forceinline__ unsigned long long sum16(const uint4& v) {
  return ((unsigned long long)v.x | ((unsigned long long)v.y << 32)) +
         ((unsigned long long)v.z | ((unsigned long long)v.w << 32));
}
// per-lane sums -> one atomic add per workgroup
__device__ __forceinline__ void block_add(unsigned long long acc, unsigned long long* s_red, unsigned long long* out) {
  s_red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_red[0]) atomicAdd(out, s_red[0]);
}

// Payload chunks [c0, c1) -> dst (chunk c0 at dst, 16-byte aligned); out[0] += their checksum.
__global__ __launch_bounds__(256) void k_ckpt_pack(SegView sv, uint64_t c0, uint64_t c1, uint8_t* dst,
                                                   unsigned long long* out) {
  __shared__ uint64_t s_off[kTileChunks + 1];
  __shared__ unsigned long long s_red[256];
  unsigned long long acc = 0;
  const uint64_t tiles = (c1 - c0 + kTileChunks - 1) / kTileChunks;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t t0 = c0 + t * kTileChunks, t1 = min<uint64_t>(t0 + (uint64_t)kTileChunks, c1);
    int64_t first;
    int cnt;
    tile_setup(sv, t0, s_off, first, cnt);
    for (uint64_t c = t0 + threadIdx.x; c < t1; c += 256) {
      const uint64_t pos = c * 16;
      const int i = tile_find(s_off, cnt, pos);
      const int64_t s = first + i;
      const uint64_t rel = pos - s_off[i];
      const uint64_t len = sv.len[s] & ~kListBit;
      uint4 v = make_uint4(0, 0, 0, 0);  // (padding stores zero)
      if (rel < len) v = load16(reinterpret_cast<const uint8_t*>(sv.addr[s]) + rel, len - rel);
      *reinterpret_cast<uint4*>(dst + (c - c0) * 16) = v;
      acc += sum16(v);
    }
    __syncthreads();  // the tile's boundaries are read before the next tile's replace them
  }
  block_add(acc, s_red, out);
}

// src (chunk c0 at src) -> the rows' new places; out[0] += the checksum of
// what was read, out[1] |= kBad*.  A list row's chunk is checked before it is
// stored: its leading u16 must be the key count its length implies and every
// entry a bucket (< width) -- the readers index LDS by these entries.  A chunk
// that fails is not stored.  kStore = false is the merge's verify pass: the
// same mapping, checksum and checks over an image, and no store at all.
template <bool kStore>
__global__ __launch_bounds__(256) void k_ckpt_unpack(SegView sv, uint64_t c0, uint64_t c1, const uint8_t* src, int depth,
                                                     int width, unsigned long long* out) {
  __shared__ uint64_t s_off[kTileChunks + 1];
  __shared__ unsigned long long s_red[256];
  unsigned long long acc = 0, bad = 0;
  const uint64_t tiles = (c1 - c0 + kTileChunks - 1) / kTileChunks;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t t0 = c0 + t * kTileChunks, t1 = min<uint64_t>(t0 + (uint64_t)kTileChunks, c1);
    int64_t first;
    int cnt;
    tile_setup(sv, t0, s_off, first, cnt);
    for (uint64_t c = t0 + threadIdx.x; c < t1; c += 256) {
      const uint64_t pos = c * 16;
      const int i = tile_find(s_off, cnt, pos);
      const int64_t s = first + i;
      const uint64_t rel = pos - s_off[i];
      const uint64_t lf = sv.len[s];
      const uint64_t len = lf & ~kListBit;
      const uint4 v = *reinterpret_cast<const uint4*>(src + (c - c0) * 16);
      acc += sum16(v);
      if (rel >= len) {  // (cannot happen with a validated directory)
        bad |= kBadPad;
        continue;
      }
      const uint64_t rem = len - rel;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      bool ok = true;
      if (rem < 16) {  // pad bytes are zero in a valid image
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if ((uint64_t)(2 * q) >= rem && ((w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu)) ok = false;
        if (!ok) bad |= kBadPad;
      }
      if (lf & kListBit) {
        const uint64_t e0 = rel >> 1, ne = len >> 1;
        const uint32_t m_want = (uint32_t)((len - 2) / (2 * (uint64_t)depth));
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const uint32_t e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e0 + q < ne && (e0 + q == 0 ? e != m_want : e >= (uint32_t)width)) {
            ok = false;
            bad |= kBadList;
          }
        }
      }
      if (kStore && ok) store16(reinterpret_cast<uint8_t*>(sv.addr[s]) + rel, rem, v);
    }
    __syncthreads();
  }
  if (bad) atomicOr(out + 1, bad);
  block_add(acc, s_red, out);
}

// One workgroup per listed row: the narrow image at src[i] (a validated copy
// of its payload bytes) expanded to u16 counters in the row's whole slot,
// which reset_rows_zero left zeroed.
__global__ __launch_bounds__(256) void k_ckpt_expand(const int32_t* rows, const uint64_t* src, const int32_t* form,
                                                     int64_t count, uint16_t* t16, int64_t su, int64_t dw, int w) {
  for (int64_t i = blockIdx.x; i < count; i += gridDim.x) {
    const int64_t r = rows[i];
    const uint8_t* p8 = reinterpret_cast<const uint8_t*>(src[i]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(t16 + su + r * su);
    const int32_t f = form[i];
    if (f == kFormList) {  // the list re-count: entry (sketch row t / m, bucket e) adds one
      const uint16_t* e = reinterpret_cast<const uint16_t*>(p8);
      const uint32_t m = e[0];
      const int64_t ne = (dw / w) * (int64_t)m;
      for (int64_t t = threadIdx.x; t < ne; t += 256) {
        const int64_t ci = (t / m) * w + e[1 + t];
        atomicAdd(dst + (ci >> 1), 1u << ((ci & 1) * 16));  // (a counter stays below 2^16: no carry)
      }
    } else {
      for (int64_t j = (int64_t)threadIdx.x * 16; j < dw; j += 256 * 16) {
        uint32_t v[16];
        unpack16(f, p8, j, v);
        pack16<2>(v, dst, j);
      }
    }
  }
}

// ---- apply: a group of image counters meets a live row (cms_merge_table, cms_subtract_table) ----
//
// The image row's form is independent of the live row's.  A group of N image
// counters (N = 16; 8 from a u16 chunk, 4 from a u32 chunk) faces N tb / 8
// whole bytes of the live row, aligned to their own size, that no other lane
// touches, and is applied in one of three ways:
//
//   kAdd    promote_rows and widen_rows ran first on the rows' bounds, so
//           every live row that receives anything is dense -- a 1-bit ... u16
//           row in a place that holds it, or a u32 hot slot -- and no field of
//           it carries: the N values packed into words, one integer add each
//   kCheck  the group is loaded and compared field by field; true when any
//           live field is below its image counter; nothing is stored
//   kSub    follows a check that passed for the whole image: every decrement
//           fits its field, so the packed words subtract with one integer
//           subtract each and no borrow crosses a field
//
// A subtraction promotes nothing, so a u32 image row can face a narrow live
// row.  That gives the one group below a byte -- four u32 image counters on a
// 1-bit live row, half a byte that the next lane's chunk shares: kSub takes it
// with an atomic on the aligned word.  An add never meets it (a u32 image row
// forces a hot live row) and has no such store.

enum class Apply { kAdd, kCheck, kSub };

struct ApplyDst {
  uint8_t* p;  // the live row's first byte
  int tb;      // bits per counter: a narrow form's 1 .. 16, 32 for a hot slot; 0: a list row, or the shared zero row
};
__device__ __forceinline__ ApplyDst apply_dst(const TableView& tv, int64_t r) {
  const int32_t s = tv.hidx[r];
  if (s >= 0) return ApplyDst{reinterpret_cast<uint8_t*>(tv.hot + (int64_t)s * tv.dw), 32};
  const int64_t o = tv.off[r];
  if (s == kFormList || o == 0) return ApplyDst{nullptr, 0};
  return ApplyDst{reinterpret_cast<uint8_t*>(tv.t16 + (o & ~kCapMask)), form_bits(s)};
}

// x (op)= y, word by word
template <Apply Op>
__device__ __forceinline__ void apply_word(uint32_t& x, uint32_t y) {
  if constexpr (Op == Apply::kAdd) x += y; else x -= y;
}

// counters [j, j + N) of the TB-bit row at p against v; the load and store shapes follow from TB N alone
template <int TB, int N, Apply Op>
__device__ __forceinline__ bool apply_fields(uint8_t* p, int64_t j, const uint32_t (&v)[N]) {
  constexpr int kBits = TB * N;
  constexpr uint32_t kMask = (1u << TB) - 1u;
  static_assert(kBits >= 8 || Op != Apply::kAdd, "a plain add below a byte would race with the neighbouring lane");
  uint8_t* q = p + ((j * TB) >> 3);
  bool under = false;
  if constexpr (kBits >= 32) {
    constexpr int kWords = kBits / 32, kPer = 32 / TB;
    uint32_t x[kWords];
    if constexpr (kWords % 4 == 0) {
#pragma unroll
      for (int k = 0; k < kWords; k += 4) {
        const uint4 y = reinterpret_cast<const uint4*>(q)[k / 4];
        x[k] = y.x, x[k + 1] = y.y, x[k + 2] = y.z, x[k + 3] = y.w;
      }
    } else if constexpr (kWords == 2) {
      const uint2 y = *reinterpret_cast<const uint2*>(q);
      x[0] = y.x, x[1] = y.y;
    } else {
      x[0] = *reinterpret_cast<const uint32_t*>(q);
    }
    if constexpr (Op == Apply::kCheck) {
#pragma unroll
      for (int k = 0; k < kWords; ++k)
#pragma unroll
        for (int c = 0; c < kPer; ++c) under |= ((x[k] >> (c * TB)) & kMask) < v[k * kPer + c];
    } else {
#pragma unroll
      for (int k = 0; k < kWords; ++k) {
        uint32_t pk = 0;
#pragma unroll
        for (int c = 0; c < kPer; ++c) pk |= v[k * kPer + c] << (c * TB);
        apply_word<Op>(x[k], pk);
      }
      if constexpr (kWords % 4 == 0) {
#pragma unroll
        for (int k = 0; k < kWords; k += 4) reinterpret_cast<uint4*>(q)[k / 4] = make_uint4(x[k], x[k + 1], x[k + 2], x[k + 3]);
      } else if constexpr (kWords == 2) {
        *reinterpret_cast<uint2*>(q) = make_uint2(x[0], x[1]);
      } else {
        *reinterpret_cast<uint32_t*>(q) = x[0];
      }
    }
  } else {
    const int sh = kBits < 8 ? (int)((j * TB) & 7) : 0;  // (4 bits: the low or the high half of the byte)
    if constexpr (Op == Apply::kCheck) {
      const uint32_t x = (kBits == 16 ? (uint32_t)*reinterpret_cast<const uint16_t*>(q) : (uint32_t)*q) >> sh;
#pragma unroll
      for (int c = 0; c < N; ++c) under |= ((x >> (c * TB)) & kMask) < v[c];
    } else {
      uint32_t pk = 0;
#pragma unroll
      for (int c = 0; c < N; ++c) pk |= v[c] << (c * TB);
      if constexpr (kBits == 16) {
        uint32_t x = *reinterpret_cast<const uint16_t*>(q);
        apply_word<Op>(x, pk);
        *reinterpret_cast<uint16_t*>(q) = (uint16_t)x;
      } else if constexpr (kBits == 8) {
        uint32_t x = *q;
        apply_word<Op>(x, pk);
        *q = (uint8_t)x;
      } else if (pk) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(q);
        atomicSub(reinterpret_cast<uint32_t*>(a & ~uintptr_t(3)), pk << (sh + 8 * (int)(a & 3)));
      }
    }
  }
  return under;
}

// counters [0, cnt) of the u32 row at d against v: a hot row's neighbour follows at once, so a partial group stops
// at cnt, and only a whole aligned group goes as uint4
template <int N, Apply Op>
__device__ __forceinline__ bool apply_hot(uint32_t* d, const uint32_t (&v)[N], int cnt) {
  bool under = false;
  if (cnt == N && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
#pragma unroll
    for (int k = 0; k < N; k += 4) {
      uint4 x = reinterpret_cast<uint4*>(d)[k / 4];
      if constexpr (Op == Apply::kCheck) {
        under |= x.x < v[k] || x.y < v[k + 1] || x.z < v[k + 2] || x.w < v[k + 3];
      } else {
        apply_word<Op>(x.x, v[k]), apply_word<Op>(x.y, v[k + 1]), apply_word<Op>(x.z, v[k + 2]), apply_word<Op>(x.w, v[k + 3]);
        reinterpret_cast<uint4*>(d)[k / 4] = x;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (k < cnt) {
        if constexpr (Op == Apply::kCheck) under |= d[k] < v[k];
        else apply_word<Op>(d[k], v[k]);
      }
  }
  return under;
}

// counters [j, j + cnt) of the live row against v[0 .. cnt) (j % N == 0; v past cnt is zero: a narrow row's last
// partial group leaves the slack of its own slot as it is).  True: kCheck found a live field below its image counter.
template <int N, Apply Op>
__device__ __forceinline__ bool apply_counters(const ApplyDst& dst, int64_t j, const uint32_t (&v)[N], int cnt) {
  switch (dst.tb) {
    case 32: return apply_hot<N, Op>(reinterpret_cast<uint32_t*>(dst.p) + j, v, cnt);
    case 16: return apply_fields<16, N, Op>(dst.p, j, v);
    case 8: return apply_fields<8, N, Op>(dst.p, j, v);
    case 4: return apply_fields<4, N, Op>(dst.p, j, v);
    case 2: return apply_fields<2, N, Op>(dst.p, j, v);
    case 1: return apply_fields<1, N, Op>(dst.p, j, v);
    default: return false;
  }
}

// counters [16 g, 16 g + 16) of a 16-byte chunk w of SB-bit counters; false: all zero
template <int SB>
__device__ __forceinline__ bool chunk_counters(const uint32_t (&w)[4], int g, uint32_t (&v)[16]) {
  uint32_t any = 0;
  if constexpr (SB == 8) {
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (w[q >> 2] >> ((q & 3) * 8)) & 255u;
    any = w[0] | w[1] | w[2] | w[3];
  } else if constexpr (SB == 4) {
    const uint32_t a = g ? w[2] : w[0], b = g ? w[3] : w[1];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = ((q < 8 ? a : b) >> ((q & 7) * 4)) & 15u;
    any = a | b;
  } else {
    const int i = SB == 2 ? g : g >> 1;
    uint32_t x = i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3];
    if constexpr (SB == 1) x = (x >> ((g & 1) * 16)) & 0xFFFFu;
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (x >> (q * SB)) & ((1u << SB) - 1u);
    any = x;
  }
  return any != 0;
}

// Dense image rows (1-bit ... u16, u32 hot, fp64) of the resident payload src
// against dense live rows, any of the six widths on either side:
// k_ckpt_unpack's source-driven mapping, where sv.addr[s] is the segment's
// owner row and a segment flagged kListBit is another kernel's, or applies
// nothing.  A lane takes one 16-byte chunk: 128 / sb counters of one row.
//   kAdd    t64: the fp64 table (then every segment is an fp64 row)
//   kCheck  out[1] |= kBadUnder and out[2] = min(out[2], owner row) where a
//           live counter is below the image's; no store to the table
// out[1] |= kBadDest when a live row is in no state for the operation: a list
// or the zero row (the driver's promote / widen step, or its row routing,
// makes that impossible), or for an add a narrow row under u32 counters.
template <Apply Op>
__global__ __launch_bounds__(256) void k_ckpt_apply(SegView sv, uint64_t c1, const uint8_t* src, TableView tv, double* t64,
                                                    unsigned long long* out) {
  __shared__ uint64_t s_off[kTileChunks + 1];
  unsigned long long bad = 0;
  const int64_t dw = tv.dw;
  const uint64_t tiles = (c1 + kTileChunks - 1) / kTileChunks;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t t0 = t * kTileChunks, t1 = min<uint64_t>(t0 + (uint64_t)kTileChunks, c1);
    int64_t first;
    int cnt;
    tile_setup(sv, t0, s_off, first, cnt);
    for (uint64_t c = t0 + threadIdx.x; c < t1; c += 256) {
      const uint64_t pos = c * 16;
      const int i = tile_find(s_off, cnt, pos);
      const int64_t s = first + i;
      const uint64_t rel = pos - s_off[i];
      const uint64_t len = sv.len[s];
      if ((len & kListBit) || rel >= len) continue;
      const int64_t r = (int64_t)sv.addr[s];
      const int rem = (int)min<uint64_t>(len - rel, 16);
      const uint4 x = *reinterpret_cast<const uint4*>(src + pos);
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
      if constexpr (Op == Apply::kAdd) {
        if (t64) {  // one correctly rounded add per counter (always done: x + 0.0 is not x for every x)
          double* d = t64 + r * dw + (int64_t)(rel >> 3);
          d[0] += __longlong_as_double((long long)((uint64_t)w[0] | ((uint64_t)w[1] << 32)));
          if (rem == 16) d[1] += __longlong_as_double((long long)((uint64_t)w[2] | ((uint64_t)w[3] << 32)));
          continue;
        }
      }
      if ((w[0] | w[1] | w[2] | w[3]) == 0) continue;  // (most chunks of a sparse 1- or 2-bit row)
      const ApplyDst dst = apply_dst(tv, r);
      const int sb = (int)((len * 8) / (uint64_t)dw);
      if (dst.tb == 0 || (Op == Apply::kAdd && sb == 32 && dst.tb != 32)) {
        bad |= kBadDest;
        continue;
      }
      bool under = false;
      uint32_t v[16];
      switch (sb) {
        case 32: {
          const uint32_t v4[4] = {w[0], w[1], w[2], w[3]};
          if constexpr (Op == Apply::kAdd)  // u32 -> u32 only
            apply_hot<4, Op>(reinterpret_cast<uint32_t*>(dst.p) + (int64_t)(rel >> 2), v4, rem >> 2);
          else
            under = apply_counters<4, Op>(dst, (int64_t)(rel >> 2), v4, rem >> 2);
          break;
        }
        case 16: {
          uint32_t v8[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v8[q] = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          under = apply_counters<8, Op>(dst, (int64_t)(rel >> 1), v8, rem >> 1);
          break;
        }
        case 8:
          chunk_counters<8>(w, 0, v);
          under = apply_counters<16, Op>(dst, (int64_t)rel, v, 16);
          break;
        case 4:
#pragma unroll 1
          for (int g = 0; g < 2; ++g)
            if (chunk_counters<4>(w, g, v)) under |= apply_counters<16, Op>(dst, (int64_t)rel * 2 + 16 * g, v, 16);
          break;
        case 2:
#pragma unroll 1
          for (int g = 0; g < 4; ++g)
            if (chunk_counters<2>(w, g, v)) under |= apply_counters<16, Op>(dst, (int64_t)rel * 4 + 16 * g, v, 16);
          break;
        case 1:
#pragma unroll 1
          for (int g = 0; g < 8; ++g)
            if (chunk_counters<1>(w, g, v)) under |= apply_counters<16, Op>(dst, (int64_t)rel * 8 + 16 * g, v, 16);
          break;
        default: bad |= kBadDest; break;
      }
      if constexpr (Op == Apply::kCheck) {
        if (under) {
          bad |= kBadUnder;
          atomicMin(out + 2, (unsigned long long)r);
        }
      }
    }
    __syncthreads();
  }
  if (bad) atomicOr(out + 1, bad);
}

// List image rows into dense live rows (kAdd, kSub): one workgroup per listed
// row (rows[i], its payload offset off[i] and key count lm[i] from the
// validated directory).  Shapes with lists have w % 32 == 0.  A list's entries
// scatter, so each sketch row is counted in LDS first, upward from zero in u16
// cells, two per word: a list holds at most kListMaxKeys = 1024 keys and the
// loader accepts any such list -- all of them may share a bucket -- so a count
// can pass 2^8 and stays below 2^16.  Then every lane takes groups of 16 cells,
// skipping the groups that counted nothing.  The workgroup owns the live row:
// no global atomics.  out[1] |= kBadDest for a live row that is a list or on
// the zero row (widen_rows rewrote those).  The verify pass checked every
// entry; the b < w test only keeps LDS safe should the caller's device image
// change under the call.
template <Apply Op>
__global__ __launch_bounds__(256) void k_ckpt_apply_lists(const int32_t* rows, const uint64_t* off, const uint32_t* lm,
                                                          int64_t count, const uint8_t* src, TableView tv, int depth,
                                                          unsigned long long* out) {
  static_assert(Op != Apply::kCheck, "the check of a list row is k_ckpt_check_rows'");
  extern __shared__ __align__(16) uint32_t lc[];  // [w / 2]
  const int w = tv.w;
  // The cells are zeroed once: the lane that finds counts in a group puts zeros back, so every sketch row of every
  // listed row starts from zero cells without another pass over all of them.
  for (int j = threadIdx.x; j < (w >> 1); j += 256) lc[j] = 0u;
  __syncthreads();
  for (int64_t i = blockIdx.x; i < count; i += gridDim.x) {
    const int64_t r = rows[i];
    const uint16_t* e = reinterpret_cast<const uint16_t*>(src + off[i]) + 1;
    const uint32_t m = lm[i];
    const ApplyDst dst = apply_dst(tv, r);
    if (dst.tb == 0) {  // (uniform over the workgroup)
      if (threadIdx.x == 0) atomicOr(out + 1, (unsigned long long)kBadDest);
      continue;
    }
    for (int rr = 0; rr < depth; ++rr) {
      for (uint32_t t = threadIdx.x; t < m; t += 256) {
        const uint32_t b = e[(uint32_t)rr * m + t];
        if (b < (uint32_t)w) atomicAdd(&lc[b >> 1], 1u << ((b & 1u) * 16u));
      }
      __syncthreads();
      for (int g = threadIdx.x; g < (w >> 4); g += 256) {
        uint4* cells = reinterpret_cast<uint4*>(lc) + 2 * g;  // the group's 16 cells
        const uint4 lo = cells[0], hi = cells[1];
        if ((lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0) continue;
        cells[0] = cells[1] = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = (q & 1) ? x[q >> 1] >> 16 : x[q >> 1] & 0xFFFFu;
        apply_counters<16, Op>(dst, (int64_t)rr * w + 16 * g, v, 16);
      }
      __syncthreads();  // the groups are read and zeroed before the next sketch row counts into them
    }
  }
}

// The live list rows about to be rewritten (bound[r] != 0: the row's own
// mass) give up their tracked bound, so k_widen_mark's new bound -- the old
// one plus bound[r] -- is the mass itself and picks the narrowest form that
// holds it; the rewrite leaves cbound[r] = the mass, still a bound.
__global__ void k_ckpt_list_bounds(const uint64_t* bound, uint32_t* cbound, int64_t n) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    if (bound[r]) cbound[r] = 0u;
}

// 16 counters [j, j + 16) (j % 16 == 0) of a dense row at p8: form f < 0 (cms_forms.h), or f >= 0: u32 counters
__device__ __forceinline__ void row_counters16(int32_t f, const uint8_t* p8, int64_t j, uint32_t (&v)[16]) {
  if (f >= 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 y = reinterpret_cast<const uint4*>(p8 + 4 * j)[k];
      v[4 * k] = y.x, v[4 * k + 1] = y.y, v[4 * k + 2] = y.z, v[4 * k + 3] = y.w;
    }
  } else {
    unpack16(f, p8, j, v);
  }
}

// The subtraction's check of the rows where either side is a list: one
// workgroup per listed row (rows[i], the image row's payload offset off[i],
// its form sform[i] -- kFormList, a narrow form, or 0 for u32 counters -- and
// a list's key count lm[i], all from the validated directory); no store to
// the table.  Per sketch row an LDS image of w u16 halves starts at the bias
// 2^14; every entry of a live list adds one to its bucket's half, every entry
// of an image list takes one off (a live list adds and an image list takes,
// hence the bias; either holds at most 1024 keys, so no carry or borrow leaves
// a half).  Then each lane takes groups of 16 counters: live = dense live
// counter (0 for a list) + half - bias, image = dense image counter (0 for a
// list); live < image anywhere: out[1] |= kBadUnder, out[2] = min(out[2],
// row).  out[1] |= kBadDest for a live row on the zero row.  The verify pass
// checked every image entry and the build or the loader every live one; the
// b < w tests only keep LDS safe.
__global__ __launch_bounds__(256) void k_ckpt_check_rows(const int32_t* rows, const uint64_t* off, const int32_t* sform,
                                                         const uint32_t* lm, int64_t count, const uint8_t* src, TableView tv,
                                                         int depth, unsigned long long* out) {
  extern __shared__ __align__(16) uint32_t lc[];  // [w / 2]
  constexpr uint32_t kBias = 0x4000u;
  const int w = tv.w;
  for (int64_t i = blockIdx.x; i < count; i += gridDim.x) {
    const int64_t r = rows[i];
    const int32_t sf = sform[i];
    const uint8_t* sp = src + off[i];
    const uint16_t* se = reinterpret_cast<const uint16_t*>(sp) + 1;
    const uint32_t sm = sf == kFormList ? lm[i] : 0u;
    const int32_t lf = tv.hidx[r];
    const bool live_list = lf == kFormList;
    const ApplyDst dst = apply_dst(tv, r);  // (tb == 0: a list, or the zero row)
    if (dst.tb == 0 && !live_list) {  // (uniform over the workgroup; the driver sends no such row)
      if (threadIdx.x == 0) atomicOr(out + 1, (unsigned long long)kBadDest);
      continue;
    }
    const uint32_t m_live = live_list ? tv.list_m(r) : 0u;
    const uint16_t* le = live_list ? tv.row16(r) + 1 : nullptr;
    bool under = false;
    for (int rr = 0; rr < depth; ++rr) {
      for (int j = threadIdx.x; j < (w >> 1); j += 256) lc[j] = kBias | (kBias << 16);
      __syncthreads();
      for (uint32_t t = threadIdx.x; t < sm; t += 256) {
        const uint32_t b = se[(uint32_t)rr * sm + t];
        if (b < (uint32_t)w) atomicSub(&lc[b >> 1], 1u << ((b & 1u) * 16u));
      }
      for (uint32_t t = threadIdx.x; t < m_live; t += 256) {
        const uint32_t b = le[(uint32_t)rr * m_live + t];
        if (b < (uint32_t)w) atomicAdd(&lc[b >> 1], 1u << ((b & 1u) * 16u));
      }
      __syncthreads();
      for (int g = threadIdx.x; g < (w >> 4); g += 256) {
        const int64_t j = (int64_t)rr * w + 16 * g;
        uint32_t x[8];  // the group's 16 halves
        uint32_t differs = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          x[k] = lc[8 * g + k];
          differs |= x[k] ^ (kBias | (kBias << 16));
        }
        auto half = [&](int q) { return (q & 1) ? x[q >> 1] >> 16 : x[q >> 1] & 0xFFFFu; };
        // One side at least is a list, so at most one dense group is loaded.  An image list only takes from
        // the bias and a live list only adds to it, so each comparison stays in 32 bits.
        uint32_t v[16];
        if (sf == kFormList) {
          if (!differs) continue;  // no net entry in this group: nothing is taken from it, the live group is not read
          if (live_list) {
#pragma unroll
            for (int q = 0; q < 16; ++q) under |= half(q) < kBias;
          } else {
            row_counters16(dst.tb == 32 ? 0 : lf, dst.p, j, v);
#pragma unroll
            for (int q = 0; q < 16; ++q) under |= v[q] < kBias - half(q);
          }
        } else {  // a dense image row against a live list: read whole, zero wherever the list has no entry
          row_counters16(sf, sp, j, v);
#pragma unroll
          for (int q = 0; q < 16; ++q) under |= v[q] > half(q) - kBias;
        }
      }
      __syncthreads();  // the halves are read before the next sketch row resets them
    }
    if (under) {
      atomicOr(out + 1, (unsigned long long)kBadUnder);
      atomicMin(out + 2, (unsigned long long)r);
    }
  }
}

// ---- host side ----

struct Guard {
  cms_handle* h;
  explicit Guard(cms_handle* hh) : h(hh) {
    h->mu.lock();
    (void)hipSetDevice(h->device);
  }
  ~Guard() { h->mu.unlock(); }
};

struct Image {
  Header hd;
  std::vector<int64_t> ids;
  std::vector<DirEntry> dir;
  std::vector<uint64_t> addr;  // [n] device address of each row's stored bytes (0: none)
};

struct Segs {
  std::vector<uint64_t> off, addr, len;
  DevBuf d_off, d_addr, d_len;
  SegView view() const { return SegView{d_off.as<uint64_t>(), d_addr.as<uint64_t>(), d_len.as<uint64_t>(), (int64_t)addr.size()}; }
  int upload(cms_handle* h) {
    const size_t k = addr.size();
    CMS_HIP(d_off.ensure(sizeof(uint64_t) * (k + 1)));
    CMS_HIP(d_addr.ensure(sizeof(uint64_t) * std::max<size_t>(k, 1)));
    CMS_HIP(d_len.ensure(sizeof(uint64_t) * std::max<size_t>(k, 1)));
    CMS_HIP(hipMemcpyAsync(d_off.ptr, off.data(), sizeof(uint64_t) * (k + 1), hipMemcpyHostToDevice, h->stream));
    if (k) {
      CMS_HIP(hipMemcpyAsync(d_addr.ptr, addr.data(), sizeof(uint64_t) * k, hipMemcpyHostToDevice, h->stream));
      CMS_HIP(hipMemcpyAsync(d_len.ptr, len.data(), sizeof(uint64_t) * k, hipMemcpyHostToDevice, h->stream));
    }
    CMS_HIP(hipStreamSynchronize(h->stream));
    return CMS_OK;
  }
};

// the rows with stored bytes, from a directory and the rows' device addresses
void build_segs(const Image& im, Segs& sg) {
  const int64_t n = im.hd.num_owners;
  sg.off.clear(), sg.addr.clear(), sg.len.clear();
  for (int64_t r = 0; r < n; ++r) {
    const DirEntry& e = im.dir[r];
    if (e.len == 0) continue;
    sg.off.push_back(e.off);
    sg.addr.push_back(im.addr[r]);
    sg.len.push_back(e.len | (e.form == kRowList ? kListBit : 0));
  }
  sg.off.push_back(im.hd.payload_bytes);
}

unsigned grid_for(cms_handle* h, uint64_t chunks) {
  const uint64_t tiles = (chunks + kTileChunks - 1) / kTileChunks;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)h->num_cus * 16));
}

void add_host_time(cms_handle* h, const char* name, std::chrono::steady_clock::time_point t0) {
  if (!h->timing) return;
  auto& a = h->timing_acc[name];
  a.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  a.launches += 1;
}

int check_saveable(cms_handle* h, const char* what) {
  if (h->per_owner)
    return set_error(CMS_E_STATE, "%s: a per-owner-shape handle keeps the DataModel, not a table", what);
  if (h->multi() && !h->merged)
    return set_error(CMS_E_STATE, "%s: a multi-rank handle holds the whole table only once merged (cms_finalize)", what);
  if (h->multi() && h->dlog_n > 0)  // batches the other ranks have not seen, and theirs not applied here
    return set_error(CMS_E_STATE, "%s: COO batches since the merge are not exchanged yet (cms_finalize)", what);
  return CMS_OK;
}

// The image of the handle's table but its payload: header, IDs, directory
// and each row's source address.
int plan_save(cms_handle* h, Image& im) {
  const int64_t n = h->n;
  CMS_HIP(hipStreamSynchronize(h->stream));
  DevBuf d_dir, d_addr;
  CMS_HIP(d_dir.ensure(sizeof(DirEntry) * (size_t)n));
  CMS_HIP(d_addr.ensure(sizeof(uint64_t) * (size_t)n));
  {
    TimedScope ts(h, "ckpt_dir");
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192));
    hipLaunchKernelGGL(k_ckpt_dir, dim3(g), dim3(256), 0, h->stream, h->tview(), h->d_cbound, h->d_row_mass,
                       h->f64 ? h->d_t64 : (const double*)nullptr, n, (int)h->p.depth, h->empty ? 1 : 0,
                       d_dir.as<DirEntry>(), d_addr.as<uint64_t>());
    CMS_HIP(hipGetLastError());
  }
  im.dir.resize((size_t)n);
  im.addr.resize((size_t)n);
  CMS_HIP(hipMemcpyAsync(im.dir.data(), d_dir.ptr, sizeof(DirEntry) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipMemcpyAsync(im.addr.data(), d_addr.ptr, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  uint64_t at = 0;
  for (int64_t r = 0; r < n; ++r) {
    im.dir[r].off = at;
    at += round16(im.dir[r].len);
  }
  Header& hd = im.hd;
  std::memset(&hd, 0, sizeof(hd));
  std::memcpy(hd.magic, kMagic, sizeof(kMagic));
  hd.version = kVersion;
  hd.depth = h->p.depth;
  hd.width = h->p.width;
  hd.counter_type = h->p.counter_type;
  hd.frac_bits = h->p.frac_bits;
  hd.num_owners = n;
  hd.pairs_ingested = h->pairs_ingested;
  hd.seed = h->p.seed;
  im.ids = h->h_owner_ids;
  hd.flags = im.ids.empty() ? 0 : kFlagOwnerIds;
  layout_sections(&hd);
  hd.payload_bytes = at;
  hd.file_bytes = hd.payload_off + at;
  for (int i = 0; i < h->p.depth; ++i) {
    hd.a[i] = h->a[i];
    hd.b[i] = h->b[i];
  }
  // the writer holds itself to the reader's rules
  if (const char* why = check_directory(hd, im.dir.data(), n))
    return set_error(CMS_E_STATE, "checkpoint: the table's directory is inconsistent (%s)", why);
  return CMS_OK;
}

int pack_range(cms_handle* h, const Segs& sg, uint64_t c0, uint64_t c1, uint8_t* d_dst, unsigned long long* d_out) {
  if (c1 <= c0) return CMS_OK;
  TimedScope ts(h, "ckpt_pack");
  hipLaunchKernelGGL(k_ckpt_pack, dim3(grid_for(h, c1 - c0)), dim3(256), 0, h->stream, sg.view(), c0, c1, d_dst, d_out);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

int unpack_range(cms_handle* h, const Segs& sg, uint64_t c0, uint64_t c1, const uint8_t* d_src,
                 unsigned long long* d_out) {
  if (c1 <= c0) return CMS_OK;
  TimedScope ts(h, "ckpt_unpack");
  hipLaunchKernelGGL(k_ckpt_unpack<true>, dim3(grid_for(h, c1 - c0)), dim3(256), 0, h->stream, sg.view(), c0, c1, d_src,
                     (int)h->p.depth, (int)h->p.width, d_out);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

// two pinned host buffers, two device staging buffers and their events (the file path)
struct Staging {
  void* pin[2] = {nullptr, nullptr};
  DevBuf dev[2];
  hipEvent_t ev_a[2] = {nullptr, nullptr}, ev_b[2] = {nullptr, nullptr};
  int init(uint64_t bytes, bool with_dev = true) {  // (the merge copies straight into its resident image)
    for (int i = 0; i < 2; ++i) {
      CMS_HIP(hipHostMalloc(&pin[i], (size_t)bytes, hipHostMallocDefault));
      if (with_dev) CMS_HIP(dev[i].ensure((size_t)bytes));
      CMS_HIP(hipEventCreateWithFlags(&ev_a[i], hipEventDisableTiming));
      CMS_HIP(hipEventCreateWithFlags(&ev_b[i], hipEventDisableTiming));
    }
    return CMS_OK;
  }
  ~Staging() {
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 2; ++i) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      if (ev_a[i]) (void)hipEventDestroy(ev_a[i]);
      if (ev_b[i]) (void)hipEventDestroy(ev_b[i]);
    }
  }
};

struct File {
  FILE* f = nullptr;
  ~File() {
    if (f) std::fclose(f);
  }
};

// the half-written path + ".tmp" never outlives a failed save (after the rename there is nothing to remove)
struct TmpRemover {
  std::string path;
  ~TmpRemover() { std::remove(path.c_str()); }
};

// body(f, ok) writes an image to path + ".tmp" (ok = false: a short write; its
// own status for any other failure); the file is closed and renamed to path
// only when all of it was written.  The time from open to close is "ckpt_io".
template <class Body>
int write_atomically(cms_handle* h, const char* path, Body&& body) {
  const std::string tmp = std::string(path) + ".tmp";
  TmpRemover cleanup{tmp};  // (declared before the file: it is closed first)
  File out;
  out.f = std::fopen(tmp.c_str(), "wb");
  if (!out.f) return set_error(CMS_E_PARAM, "cannot open %s for writing", tmp.c_str());
  const auto t_io = std::chrono::steady_clock::now();
  bool ok = true;
  if (int rc = body(out.f, ok)) return rc;
  const bool closed = std::fclose(out.f) == 0;
  out.f = nullptr;
  add_host_time(h, "ckpt_io", t_io);
  if (!ok || !closed) return set_error(CMS_E_PARAM, "short write to %s", tmp.c_str());
  if (std::rename(tmp.c_str(), path) != 0) return set_error(CMS_E_PARAM, "cannot rename %s to %s", tmp.c_str(), path);
  return CMS_OK;
}

// header, IDs (and the gap before the directory), directory: the image's first payload_off bytes
std::vector<uint8_t> image_head(const Image& im) {
  const Header& hd = im.hd;
  std::vector<uint8_t> head((size_t)hd.payload_off, 0);
  std::memcpy(head.data(), &hd, sizeof(hd));
  if (!im.ids.empty()) std::memcpy(head.data() + hd.ids_off, im.ids.data(), (size_t)hd.ids_bytes);
  std::memcpy(head.data() + hd.dir_off, im.dir.data(), (size_t)hd.dir_bytes);
  return head;
}

int save_file(cms_handle* h, const char* path) {
  Image im;
  int rc = plan_save(h, im);
  if (rc) return rc;
  Segs sg;
  build_segs(im, sg);
  if ((rc = sg.upload(h))) return rc;
  DevBuf d_out;
  CMS_HIP(d_out.ensure(2 * sizeof(unsigned long long)));
  CMS_HIP(hipMemsetAsync(d_out.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
  const Header& hd = im.hd;
  return write_atomically(h, path, [&](FILE* f, bool& ok) -> int {
    // header (its checksum follows the payload), IDs, directory
    const std::vector<uint8_t> head = image_head(im);
    ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
    // the payload through two pinned buffers: pack of chunk i + 1 (the handle's
    // stream) and D2H of chunk i (the side stream) run while the host writes
    // chunk i - 1
    const uint64_t total = hd.payload_bytes / 16, per = kIoChunk / 16;
    const uint64_t nchunks = (total + per - 1) / per;
    if (ok && nchunks > 0) {
      Staging st;
      if (int r = st.init(std::min(kIoChunk, hd.payload_bytes))) return r;
      for (uint64_t i = 0; i <= nchunks && ok; ++i) {
        if (i < nchunks) {
          const int b = (int)(i & 1);
          const uint64_t c0 = i * per, c1 = std::min(total, c0 + per);
          if (i >= 2) CMS_HIP(hipStreamWaitEvent(h->stream, st.ev_b[b], 0));  // the copy out of dev[b] is done
          if (int r = pack_range(h, sg, c0, c1, st.dev[b].as<uint8_t>(), d_out.as<unsigned long long>())) return r;
          CMS_HIP(hipEventRecord(st.ev_a[b], h->stream));
          CMS_HIP(hipStreamWaitEvent(h->side_stream, st.ev_a[b], 0));
          CMS_HIP(hipMemcpyAsync(st.pin[b], st.dev[b].ptr, (size_t)((c1 - c0) * 16), hipMemcpyDeviceToHost, h->side_stream));
          CMS_HIP(hipEventRecord(st.ev_b[b], h->side_stream));
        }
        if (i >= 1) {
          const uint64_t j = i - 1, c0 = j * per, c1 = std::min(total, c0 + per);
          CMS_HIP(hipEventSynchronize(st.ev_b[j & 1]));
          ok = std::fwrite(st.pin[j & 1], 16, (size_t)(c1 - c0), f) == c1 - c0;
        }
      }
    }
    unsigned long long res[2] = {0, 0};
    CMS_HIP(hipMemcpyAsync(res, d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    im.hd.checksum = res[0];
    ok = ok && std::fseek(f, 0, SEEK_SET) == 0 && std::fwrite(&im.hd, sizeof(im.hd), 1, f) == 1;
    return CMS_OK;
  });
}

int save_device(cms_handle* h, void* d_buf, int64_t capacity, int64_t* bytes) {
  Image im;
  int rc = plan_save(h, im);
  if (rc) return rc;
  *bytes = (int64_t)im.hd.file_bytes;
  if (!d_buf) return CMS_OK;  // (the size only)
  if ((uint64_t)capacity < im.hd.file_bytes)
    return set_error(CMS_E_PARAM, "device image needs %lld bytes, the buffer has %lld", (long long)im.hd.file_bytes,
                     (long long)capacity);
  if (reinterpret_cast<uintptr_t>(d_buf) & 15) return set_error(CMS_E_PARAM, "device image must be 16-byte aligned");
  Segs sg;
  build_segs(im, sg);
  if ((rc = sg.upload(h))) return rc;
  DevBuf d_out;
  CMS_HIP(d_out.ensure(2 * sizeof(unsigned long long)));
  CMS_HIP(hipMemsetAsync(d_out.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
  uint8_t* base = static_cast<uint8_t*>(d_buf);
  const Header& hd = im.hd;
  if ((rc = pack_range(h, sg, 0, hd.payload_bytes / 16, base + hd.payload_off, d_out.as<unsigned long long>()))) return rc;
  unsigned long long res[2] = {0, 0};
  CMS_HIP(hipMemcpyAsync(res, d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  im.hd.checksum = res[0];
  const std::vector<uint8_t> head = image_head(im);
  CMS_HIP(hipMemcpyAsync(base, head.data(), head.size(), hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

// ---- load ----

// what a load and a merge both need: one fixed-shape table that no rank shares
int check_receives_image(cms_handle* h, const char* what) {
  if (h->per_owner)
    return set_error(CMS_E_STATE, "%s: a per-owner-shape handle keeps the DataModel, not a table", what);
  if (h->comm || h->ext_comm || h->multi())
    return set_error(CMS_E_STATE, "%s: the handle has a communicator (the merge would sum every rank's copy)", what);
  return CMS_OK;
}

int check_loadable(cms_handle* h, const char* what) {
  if (int rc = check_receives_image(h, what)) return rc;
  if (!h->empty || h->pairs_ingested != 0)
    return set_error(CMS_E_STATE, "%s: the handle must be empty (new, or after cms_reset)", what);
  return CMS_OK;
}

int check_matches(cms_handle* h, const Header& hd) {
  if (hd.depth != h->p.depth || hd.width != h->p.width)
    return set_error(CMS_E_PARAM, "checkpoint shape d=%d w=%d, handle d=%d w=%d", hd.depth, hd.width, h->p.depth, h->p.width);
  if (hd.num_owners != h->n)
    return set_error(CMS_E_PARAM, "checkpoint of %lld owners, handle of %lld", (long long)hd.num_owners, (long long)h->n);
  if (hd.counter_type != h->p.counter_type) return set_error(CMS_E_PARAM, "checkpoint and handle differ in counter type");
  if (hd.frac_bits != h->p.frac_bits)
    return set_error(CMS_E_PARAM, "checkpoint frac_bits %d, handle %d", hd.frac_bits, h->p.frac_bits);
  return CMS_OK;
}

// header, IDs and directory of an image from its first payload_off bytes
int parse_head(const uint8_t* head, Image& im) {
  const Header& hd = im.hd;
  const int64_t n = hd.num_owners;
  if (hd.flags & kFlagOwnerIds) {
    im.ids.resize((size_t)n);
    std::memcpy(im.ids.data(), head + hd.ids_off, (size_t)hd.ids_bytes);
    if (const char* why = check_owner_ids(im.ids.data(), n)) return set_error(CMS_E_PARAM, "checkpoint: %s", why);
  }
  im.dir.resize((size_t)n);
  std::memcpy(im.dir.data(), head + hd.dir_off, (size_t)hd.dir_bytes);
  if (const char* why = check_directory(hd, im.dir.data(), n)) return set_error(CMS_E_PARAM, "checkpoint: %s", why);
  return CMS_OK;
}

// rows a handle without forms receives expanded to u16 (k_ckpt_expand)
struct Expand {
  std::vector<int32_t> rows, form;
  std::vector<uint64_t> src;
  DevBuf scratch, d_rows, d_form, d_src;
};

int32_t table_form(uint8_t f) {
  return f == kRowList ? kFormList : f == kRowU1 ? kFormU1 : f == kRowU2 ? kFormU2 : f == kRowU4 ? kFormU4
       : f == kRowU8 ? kFormU8 : kFormU16;
}

// Lays the validated directory's rows out in the (empty) handle: forms,
// bounds, masses, hot slots and arena places; im.addr[r] = where row r's
// stored bytes go.
int restore_layout(cms_handle* h, Image& im, Expand& ex) {
  const int64_t n = h->n, dw = h->dw;
  im.addr.assign((size_t)n, 0);
  std::vector<uint64_t> mass((size_t)n);
  for (int64_t r = 0; r < n; ++r) mass[r] = im.dir[r].mass;
  if (h->f64) {
    bool any_zero = false;
    for (int64_t r = 0; r < n; ++r) {
      any_zero |= im.dir[r].form == kRowZero;
      if (im.dir[r].form == kRowF64) im.addr[r] = reinterpret_cast<uint64_t>(h->d_t64 + r * dw);
    }
    if (any_zero) CMS_HIP(hipMemsetAsync(h->d_t64, 0, sizeof(double) * (size_t)n * (size_t)dw, h->stream));
    CMS_HIP(hipMemcpyAsync(h->d_row_mass, mass.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    return CMS_OK;
  }
  int rc = reset_rows_zero(h);  // every row narrow and zero, no hot slots
  if (rc) return rc;
  const int64_t su = slot_units(dw);
  std::vector<int32_t> hidx((size_t)n);
  std::vector<uint32_t> cb((size_t)n), caps((size_t)n, 0);
  std::vector<uint64_t> xoff;
  int64_t nhot = 0;
  uint64_t xbytes = 0;
  for (int64_t r = 0; r < n; ++r) {
    const DirEntry& e = im.dir[r];
    cb[r] = e.cbound;
    if (e.form == kRowHot) {
      hidx[r] = (int32_t)nhot++;  // the next hot slot in row order
      continue;
    }
    if (e.form == kRowZero) {
      hidx[r] = kFormU16;
      continue;
    }
    const bool expand = !h->forms_ok && e.form != kRowU16;  // a form this handle cannot hold
    hidx[r] = expand ? kFormU16 : table_form(e.form);
    if (expand) {
      ex.rows.push_back((int32_t)r);
      ex.form.push_back(table_form(e.form));
      xoff.push_back(xbytes);
      xbytes += round16(e.len);
    }
    // the row's capacity: its saved place class, and at least its stored bytes
    // (a byte-class list's place is sized by the list, not by a class)
    const int64_t units = std::max<int64_t>(class_units(e.cls, dw), ((int64_t)e.len + 1) / 2);
    caps[r] = (uint32_t)((units + kRowAlign - 1) / kRowAlign);
  }
  if ((rc = grow_hot(h, nhot))) return rc;
  h->hot_used = nhot;
  CMS_HIP(hipMemcpyAsync(h->d_hidx, hidx.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(h->d_cbound, cb.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(h->d_row_mass, mass.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  std::vector<int64_t> off((size_t)n);
  if (h->compact) {  // through row_layout: class_of_units re-derives each place's class
    CMS_HIP(h->ws_layout.ensure(sizeof(uint32_t) * (size_t)(2 * n + n / 4096 + 16)));
    uint32_t* d_caps = h->ws_layout.as<uint32_t>();
    CMS_HIP(hipMemcpyAsync(d_caps, caps.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if ((rc = row_layout(h, d_caps, d_caps + n))) return rc;
    CMS_HIP(hipMemcpyAsync(off.data(), h->d_off, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    // A place's class is the narrower of the class row_layout derives from its
    // size and the class its entry records.  For an image a handle saved the
    // two are equal (the place is no smaller than the recorded class's units
    // and no larger than the place it was saved from); an image written with
    // narrower classes -- the forms' own, as cms_compact_table and
    // build_checkpoint's defaults record them, 0 for a list -- stays as
    // written, so save -> load -> save reproduces it.  (A narrower class only
    // moves a row sooner: the place still holds what the class says.)
    bool differs = false;
    for (int64_t r = 0; r < n; ++r) {
      if (off[r] == 0) continue;
      const int64_t o = (off[r] & ~kCapMask) | std::min<int64_t>(off[r] & kCapMask, (int64_t)im.dir[r].cls);
      differs |= o != off[r];
      off[r] = o;
    }
    if (differs) CMS_HIP(hipMemcpyAsync(h->d_off, off.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  } else {  // whole slots at the identity offsets
    for (int64_t r = 0; r < n; ++r) off[r] = (su + r * su) | kCapU16;
  }
  CMS_HIP(hipStreamSynchronize(h->stream));
  if (!ex.rows.empty()) CMS_HIP(ex.scratch.ensure((size_t)xbytes));
  size_t xi = 0;
  for (int64_t r = 0; r < n; ++r) {
    const DirEntry& e = im.dir[r];
    if (e.len == 0) continue;
    if (e.form == kRowHot) {
      im.addr[r] = reinterpret_cast<uint64_t>(h->hot_tab.as<uint32_t>() + (int64_t)hidx[r] * dw);
    } else if (xi < ex.rows.size() && ex.rows[xi] == r) {
      ex.src.push_back(reinterpret_cast<uint64_t>(ex.scratch.as<uint8_t>() + xoff[xi]));
      im.addr[r] = ex.src.back();
      ++xi;
    } else {
      im.addr[r] = reinterpret_cast<uint64_t>(h->d_t16 + (off[r] & ~kCapMask));
    }
  }
  return CMS_OK;
}

int run_expand(cms_handle* h, Expand& ex) {
  const size_t k = ex.rows.size();
  if (k == 0) return CMS_OK;
  CMS_HIP(ex.d_rows.ensure(sizeof(int32_t) * k));
  CMS_HIP(ex.d_form.ensure(sizeof(int32_t) * k));
  CMS_HIP(ex.d_src.ensure(sizeof(uint64_t) * k));
  CMS_HIP(hipMemcpyAsync(ex.d_rows.ptr, ex.rows.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(ex.d_form.ptr, ex.form.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(ex.d_src.ptr, ex.src.data(), sizeof(uint64_t) * k, hipMemcpyHostToDevice, h->stream));
  TimedScope ts(h, "ckpt_unpack");
  hipLaunchKernelGGL(k_ckpt_expand, dim3((unsigned)std::min<size_t>(k, 65536)), dim3(256), 0, h->stream,
                     ex.d_rows.as<int32_t>(), ex.d_src.as<uint64_t>(), ex.d_form.as<int32_t>(), (int64_t)k, h->d_t16,
                     slot_units(h->dw), h->dw, (int)h->p.width);
  CMS_HIP(hipGetLastError());
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

// a refused or failed load leaves the handle as cms_reset does
int leave_empty(cms_handle* h) {
  (void)hipStreamSynchronize(h->side_stream);
  CMS_HIP(hipMemsetAsync(h->d_row_mass, 0, sizeof(uint64_t) * (size_t)h->n, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  h->empty = true;
  h->norms_valid = false;
  h->finalized = false;
  h->pairs_ingested = 0;
  h->merged = false;
  h->rf_valid = false;
  return CMS_OK;
}

// the verified image becomes the handle's table: "ingested, not finalized"
int commit_load(cms_handle* h, const Image& im, Expand& ex, const unsigned long long res[2]) {
  if (res[1] & kBadList) {
    (void)leave_empty(h);
    return set_error(CMS_E_PARAM, "checkpoint: a list row's key count or an entry is out of range");
  }
  if (res[1] & kBadPad) {
    (void)leave_empty(h);
    return set_error(CMS_E_PARAM, "checkpoint: padding bytes are not zero");
  }
  if (res[0] != im.hd.checksum) {
    (void)leave_empty(h);
    return set_error(CMS_E_PARAM, "checkpoint: payload checksum mismatch");
  }
  int rc = run_expand(h, ex);
  if (rc) {
    (void)leave_empty(h);
    return rc;
  }
  const Header& hd = im.hd;
  for (int i = 0; i < h->p.depth; ++i) {  // as cms_set_hash_params installs them
    h->a[i] = hd.a[i];
    h->b[i] = hd.b[i];
    h->hp.ap[i] = reduce_key(hd.a[i]);
    h->hp.bp[i] = reduce_key(hd.b[i]);
  }
  hash_finish(h->hp);
  h->p.seed = hd.seed;
  if (!im.ids.empty()) {  // as cms_set_owner_ids
    if (!h->d_owner_ids) CMS_HIP(hipMalloc(&h->d_owner_ids, sizeof(int64_t) * (size_t)h->n));
    CMS_HIP(hipMemcpy(h->d_owner_ids, im.ids.data(), sizeof(int64_t) * (size_t)h->n, hipMemcpyHostToDevice));
    h->h_owner_ids = im.ids;
  } else if (!h->h_owner_ids.empty()) {  // the saved table's owners are its rows
    h->h_owner_ids.clear();
    if (h->d_owner_ids) (void)hipFree(h->d_owner_ids);
    h->d_owner_ids = nullptr;
  }
  h->pairs_ingested = hd.pairs_ingested;
  h->empty = false;
  h->norms_valid = false;
  h->finalized = false;
  h->mfma_ready = false;
  h->i8blk_ready = false;
  h->rf_valid = false;
  h->merged = false;
  h->ext_merged = false;
  h->dlog_n = 0;
  h->stale_possible = true;
  return CMS_OK;
}

// the file at path opened and its header read and validated (the file is left just past the header)
int read_header_file(File& in, const char* path, Header& hd) {
  in.f = std::fopen(path, "rb");
  if (!in.f) return set_error(CMS_E_PARAM, "cannot open %s", path);
  if (std::fseek(in.f, 0, SEEK_END) != 0) return set_error(CMS_E_PARAM, "cannot seek in %s", path);
  const long long size = (long long)std::ftell(in.f);
  std::rewind(in.f);
  if (size < (long long)sizeof(Header) || std::fread(&hd, sizeof(Header), 1, in.f) != 1)
    return set_error(CMS_E_PARAM, "checkpoint %s: shorter than a checkpoint header", path);
  if (const char* why = check_header(hd, (uint64_t)size)) return set_error(CMS_E_PARAM, "checkpoint %s: %s", path, why);
  return CMS_OK;
}

// An image's head -- header, IDs, directory -- read from the file at path,
// validated and matched against the handle; the file is left at the payload.
int read_head_file(File& in, const char* path, cms_handle* h, Image& im) {
  int rc = read_header_file(in, path, im.hd);
  if (rc) return rc;
  if ((rc = check_matches(h, im.hd))) return rc;
  std::vector<uint8_t> head((size_t)im.hd.payload_off);
  std::rewind(in.f);
  if (std::fread(head.data(), 1, head.size(), in.f) != head.size())
    return set_error(CMS_E_PARAM, "checkpoint %s: short read", path);
  return parse_head(head.data(), im);
}

// The same of a device image of `bytes` bytes at d_buf (synchronises the handle's stream).
int read_head_device(const void* d_buf, int64_t bytes, cms_handle* h, Image& im) {
  if (bytes < (int64_t)sizeof(Header)) return set_error(CMS_E_PARAM, "checkpoint image: shorter than a checkpoint header");
  if (reinterpret_cast<uintptr_t>(d_buf) & 15) return set_error(CMS_E_PARAM, "device image must be 16-byte aligned");
  CMS_HIP(hipStreamSynchronize(h->stream));
  CMS_HIP(hipMemcpy(&im.hd, d_buf, sizeof(Header), hipMemcpyDeviceToHost));
  if (const char* why = check_header(im.hd, (uint64_t)bytes)) return set_error(CMS_E_PARAM, "checkpoint image: %s", why);
  if (int rc = check_matches(h, im.hd)) return rc;
  std::vector<uint8_t> head((size_t)im.hd.payload_off);
  CMS_HIP(hipMemcpy(head.data(), d_buf, head.size(), hipMemcpyDeviceToHost));
  if (std::memcmp(head.data(), &im.hd, sizeof(Header)) != 0)
    return set_error(CMS_E_PARAM, "checkpoint image changed while it was read");
  return parse_head(head.data(), im);
}

int load_file(cms_handle* h, const char* path) {
  int rc = check_loadable(h, "cms_load_table");
  if (rc) return rc;
  File in;
  Image im;
  if ((rc = read_head_file(in, path, h, im))) return rc;
  const Header& hd = im.hd;
  // ---- every host check has passed: the device part ----
  CMS_HIP(hipStreamSynchronize(h->stream));
  Expand ex;
  Segs sg;
  DevBuf d_out;
  unsigned long long res[2] = {0, 0};
  auto device_part = [&]() -> int {
    int r = restore_layout(h, im, ex);
    if (r) return r;
    build_segs(im, sg);
    if ((r = sg.upload(h))) return r;
    CMS_HIP(d_out.ensure(2 * sizeof(unsigned long long)));
    CMS_HIP(hipMemsetAsync(d_out.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
    // the mirror of save_file: the host reads chunk i + 1 while chunk i goes
    // H2D (side stream) and is scattered (the handle's stream)
    const uint64_t total = hd.payload_bytes / 16, per = kIoChunk / 16;
    const uint64_t nchunks = (total + per - 1) / per;
    if (nchunks > 0) {
      Staging st;
      if ((r = st.init(std::min(kIoChunk, hd.payload_bytes)))) return r;
      const auto t_io = std::chrono::steady_clock::now();
      for (uint64_t i = 0; i < nchunks; ++i) {
        const int b = (int)(i & 1);
        const uint64_t c0 = i * per, c1 = std::min(total, c0 + per);
        if (i >= 2) CMS_HIP(hipEventSynchronize(st.ev_a[b]));  // pin[b] has left the host
        if (std::fread(st.pin[b], 16, (size_t)(c1 - c0), in.f) != c1 - c0)
          return set_error(CMS_E_PARAM, "checkpoint %s: short read", path);
        if (i >= 2) CMS_HIP(hipStreamWaitEvent(h->side_stream, st.ev_b[b], 0));  // dev[b] has been scattered
        CMS_HIP(hipMemcpyAsync(st.dev[b].ptr, st.pin[b], (size_t)((c1 - c0) * 16), hipMemcpyHostToDevice, h->side_stream));
        CMS_HIP(hipEventRecord(st.ev_a[b], h->side_stream));
        CMS_HIP(hipStreamWaitEvent(h->stream, st.ev_a[b], 0));
        if ((r = unpack_range(h, sg, c0, c1, st.dev[b].as<uint8_t>(), d_out.as<unsigned long long>()))) return r;
        CMS_HIP(hipEventRecord(st.ev_b[b], h->stream));
      }
      CMS_HIP(hipStreamSynchronize(h->stream));
      add_host_time(h, "ckpt_io", t_io);
    }
    CMS_HIP(hipMemcpyAsync(res, d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    return CMS_OK;
  };
  if ((rc = device_part())) {
    (void)leave_empty(h);
    return rc;
  }
  return commit_load(h, im, ex, res);
}

int load_device(cms_handle* h, const void* d_buf, int64_t bytes) {
  int rc = check_loadable(h, "cms_load_table_device");
  if (rc) return rc;
  Image im;
  if ((rc = read_head_device(d_buf, bytes, h, im))) return rc;
  const Header& hd = im.hd;
  Expand ex;
  Segs sg;
  DevBuf d_out;
  unsigned long long res[2] = {0, 0};
  auto device_part = [&]() -> int {
    int r = restore_layout(h, im, ex);
    if (r) return r;
    build_segs(im, sg);
    if ((r = sg.upload(h))) return r;
    CMS_HIP(d_out.ensure(2 * sizeof(unsigned long long)));
    CMS_HIP(hipMemsetAsync(d_out.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
    if ((r = unpack_range(h, sg, 0, hd.payload_bytes / 16, static_cast<const uint8_t*>(d_buf) + hd.payload_off,
                          d_out.as<unsigned long long>())))
      return r;
    CMS_HIP(hipMemcpyAsync(res, d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    return CMS_OK;
  };
  if ((rc = device_part())) {
    (void)leave_empty(h);
    return rc;
  }
  return commit_load(h, im, ex, res);
}

// ---- merge ----

// The verify pass of a merge and of a subtraction: checksum, pad bytes and
// every list row over the resident payload, no store.  Leaves the image's
// segments in sg (a segment's address: its owner row, as k_ckpt_apply reads it)
// and d_out ([0] checksum, [1] kBad* flags, [2] an owner row) zeroed but [2],
// which is all ones.
int verify_resident(cms_handle* h, Image& im, const uint8_t* d_payload, Segs& sg, DevBuf& d_out) {
  const Header& hd = im.hd;
  const int64_t n = h->n;
  im.addr.resize((size_t)n);
  for (int64_t r = 0; r < n; ++r) im.addr[r] = (uint64_t)r;
  build_segs(im, sg);
  int rc = sg.upload(h);
  if (rc) return rc;
  unsigned long long res[2] = {0, 0};
  const uint64_t chunks = hd.payload_bytes / 16;
  CMS_HIP(d_out.ensure(3 * sizeof(unsigned long long)));
  CMS_HIP(hipMemsetAsync(d_out.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
  CMS_HIP(hipMemsetAsync(d_out.as<unsigned long long>() + 2, 0xFF, sizeof(unsigned long long), h->stream));
  if (chunks > 0) {
    TimedScope ts(h, "ckpt_verify");
    hipLaunchKernelGGL(k_ckpt_unpack<false>, dim3(grid_for(h, chunks)), dim3(256), 0, h->stream, sg.view(), (uint64_t)0,
                       chunks, d_payload, (int)h->p.depth, (int)h->p.width, d_out.as<unsigned long long>());
    CMS_HIP(hipGetLastError());
  }
  CMS_HIP(hipMemcpyAsync(res, d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  if (res[1] & kBadList) return set_error(CMS_E_PARAM, "checkpoint: a list row's key count or an entry is out of range");
  if (res[1] & kBadPad) return set_error(CMS_E_PARAM, "checkpoint: padding bytes are not zero");
  if (res[0] != hd.checksum) return set_error(CMS_E_PARAM, "checkpoint: payload checksum mismatch");
  return CMS_OK;
}

// the rows a one-workgroup-per-row kernel takes: owner row, the image row's form (kFormList, a narrow form, 0 for
// u32 counters), its payload offset and a list's key count
struct RowList {
  std::vector<int32_t> row, form;
  std::vector<uint64_t> off;
  std::vector<uint32_t> m;
  DevBuf d_row, d_form, d_off, d_m;
  void push(int64_t r, const DirEntry& e, int depth) {
    row.push_back((int32_t)r);
    form.push_back(e.form == kRowHot ? 0 : table_form(e.form));
    off.push_back(e.off);
    m.push_back(e.form == kRowList ? (uint32_t)((e.len - 2) / (2 * (uint64_t)depth)) : 0u);
  }
  int upload(cms_handle* h) {
    const size_t k = row.size();
    if (k == 0) return CMS_OK;
    CMS_HIP(d_row.ensure(sizeof(int32_t) * k));
    CMS_HIP(d_form.ensure(sizeof(int32_t) * k));
    CMS_HIP(d_off.ensure(sizeof(uint64_t) * k));
    CMS_HIP(d_m.ensure(sizeof(uint32_t) * k));
    CMS_HIP(hipMemcpyAsync(d_row.ptr, row.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, h->stream));
    CMS_HIP(hipMemcpyAsync(d_form.ptr, form.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, h->stream));
    CMS_HIP(hipMemcpyAsync(d_off.ptr, off.data(), sizeof(uint64_t) * k, hipMemcpyHostToDevice, h->stream));
    CMS_HIP(hipMemcpyAsync(d_m.ptr, m.data(), sizeof(uint32_t) * k, hipMemcpyHostToDevice, h->stream));
    return CMS_OK;
  }
};

// One merge or subtraction in flight: what the shared opening leaves, what
// the operation's own middle adds for the shared closing.  (The host arrays
// of the uploads live here until the last synchronisation.)
struct ApplyJob {
  std::vector<uint64_t> mass;  // the live masses, then the new ones
  Segs sg;                     // the image's segments (a segment's address: its owner row)
  DevBuf d_out;                // [0] checksum, [1] kBad* flags, [2] an owner row
  uint64_t chunks = 0;         // 16-byte chunks of the payload
  RowList lists;               // the image's list rows that the write pass applies
  std::vector<int64_t> touched;  // rows the image changes (the refresh marks them)
  DevBuf d_touched;
  std::vector<uint64_t> bound;  // the widen step's per-row bounds
  std::vector<uint8_t> force;   // the promote step's rows that must hold u32 counters
};

// The checks a merge and a subtraction share, in this order: the header-level
// compatibility, the mass rule of the operation, then the verify pass over
// the whole payload.  No write.
int apply_open(cms_handle* h, Apply op, Image& im, const uint8_t* d_payload, ApplyJob& job) {
  const Header& hd = im.hd;
  const int64_t n = h->n;
  if (const char* why = check_merge_params(hd, h->a, h->b, h->h_owner_ids.empty() ? nullptr : h->h_owner_ids.data(),
                                           im.ids.empty() ? nullptr : im.ids.data()))
    return set_error(CMS_E_PARAM, "checkpoint: %s", why);
  CMS_HIP(hipStreamSynchronize(h->stream));
  job.mass.assign((size_t)n, 0);
  if (!h->empty) CMS_HIP(hipMemcpy(job.mass.data(), h->d_row_mass, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (const char* why = op == Apply::kAdd ? check_merge_masses(hd, im.dir.data(), job.mass.data(), n)
                                          : check_subtract_masses(hd, im.dir.data(), job.mass.data(), n))
    return set_error(CMS_E_OVERFLOW, "%s", why);
  job.chunks = hd.payload_bytes / 16;
  return verify_resident(h, im, d_payload, job.sg, job.d_out);
}

// cms_top_k_refresh stays incremental after a delta merge or subtraction
int mark_touched(cms_handle* h, ApplyJob& job) {
  if (!h->rf_valid || job.touched.empty()) return CMS_OK;
  const size_t bytes = sizeof(int64_t) * job.touched.size();
  CMS_HIP(job.d_touched.ensure(bytes));
  CMS_HIP(hipMemcpyAsync(job.d_touched.ptr, job.touched.data(), bytes, hipMemcpyHostToDevice, h->stream));
  return refresh_mark(h, job.d_touched.as<int64_t>(), (int64_t)job.touched.size());
}

// One pass of the image over the live table: the dense rows' kernel over the
// segments as job.sg was last uploaded, then the listed rows' kernel over rl.
int launch_apply(cms_handle* h, Apply op, ApplyJob& job, RowList& rl, const uint8_t* d_payload) {
  if (int rc = rl.upload(h)) return rc;
  TimedScope ts(h, op == Apply::kAdd ? "ckpt_add" : op == Apply::kCheck ? "ckpt_subcheck" : "ckpt_sub");
  unsigned long long* d_out = job.d_out.as<unsigned long long>();
  if (job.chunks > 0) {
    const auto dense = op == Apply::kAdd     ? k_ckpt_apply<Apply::kAdd>
                       : op == Apply::kCheck ? k_ckpt_apply<Apply::kCheck>
                                             : k_ckpt_apply<Apply::kSub>;
    hipLaunchKernelGGL(dense, dim3(grid_for(h, job.chunks)), dim3(256), 0, h->stream, job.sg.view(), job.chunks, d_payload,
                       h->tview(), h->f64 ? h->d_t64 : (double*)nullptr, d_out);
  }
  if (!rl.row.empty()) {
    const dim3 g((unsigned)std::min<size_t>(rl.row.size(), 65536));
    const size_t lds = 2 * (size_t)h->p.width;  // u16 cells
    if (op == Apply::kCheck) {
      hipLaunchKernelGGL(k_ckpt_check_rows, g, dim3(256), lds, h->stream, rl.d_row.as<int32_t>(), rl.d_off.as<uint64_t>(),
                         rl.d_form.as<int32_t>(), rl.d_m.as<uint32_t>(), (int64_t)rl.row.size(), d_payload, h->tview(),
                         (int)h->p.depth, d_out);
    } else {
      const auto lists = op == Apply::kAdd ? k_ckpt_apply_lists<Apply::kAdd> : k_ckpt_apply_lists<Apply::kSub>;
      hipLaunchKernelGGL(lists, g, dim3(256), lds, h->stream, rl.d_row.as<int32_t>(), rl.d_off.as<uint64_t>(),
                         rl.d_m.as<uint32_t>(), (int64_t)rl.row.size(), d_payload, h->tview(), (int)h->p.depth, d_out);
    }
  }
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

// d_out read back ([1]: the kBad* flags, [2]: an owner row), after everything queued so far
int read_out(cms_handle* h, ApplyJob& job, unsigned long long (&res)[3]) {
  CMS_HIP(hipMemcpyAsync(res, job.d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

// The merge's own middle, the first write: the in-place writers' sequence
// (ingest_coo_device) -- per-row bounds, promote, widen -- so that every live
// row that receives anything is dense and no field of it carries.
int merge_prepare(cms_handle* h, const Image& im, ApplyJob& job) {
  const int64_t n = h->n;
  int rc;
  if (h->f64) {
    if (h->empty) {
      CMS_HIP(hipMemsetAsync(h->d_t64, 0, sizeof(double) * (size_t)n * (size_t)h->dw, h->stream));
      CMS_HIP(hipMemsetAsync(h->d_row_mass, 0, sizeof(uint64_t) * (size_t)n, h->stream));
    }
    for (int64_t r = 0; r < n; ++r)
      if (im.dir[r].len) job.touched.push_back(r);
    return CMS_OK;
  }
  Segs& sg = job.sg;
  std::vector<uint64_t>& bound = job.bound;
  bound.assign((size_t)n, 0);
  job.force.assign((size_t)n, 0);
  for (int64_t r = 0; r < n; ++r) {
    const DirEntry& e = im.dir[r];
    const uint64_t inc = merge_increment(e);
    if (inc == 0) continue;  // (nothing stored, or every stored counter is zero: mass 0)
    bound[r] = job.mass[r] + inc;
    job.force[r] = e.form == kRowHot;  // a live row that receives u32 counters holds u32 counters
    job.touched.push_back(r);
    if (e.form == kRowList) job.lists.push(r, e, im.hd.depth);
  }
  // rows that add nothing leave the segments: their live rows were not prepared for an add
  for (size_t s = 0, r = 0; s < sg.len.size(); ++s) {
    while (im.dir[r].len == 0) ++r;
    if (bound[r] == 0) sg.len[s] |= kListBit;  // (k_ckpt_apply skips list segments)
    ++r;
  }
  if ((rc = sg.upload(h))) return rc;
  if (h->empty) {  // as a COO batch into an empty table
    if ((rc = reset_rows_zero(h))) return rc;
    CMS_HIP(hipMemsetAsync(h->d_row_mass, 0, sizeof(uint64_t) * (size_t)n, h->stream));
    // (a handle that never built a row has never written its bounds: the widen step adds to them)
    CMS_HIP(hipMemsetAsync(h->d_cbound, 0, sizeof(uint32_t) * (size_t)n, h->stream));
    h->norms_valid = false;
  }
  CMS_HIP(h->ws_bound.ensure(sizeof(uint64_t) * (size_t)n));
  CMS_HIP(h->ws_force.ensure((size_t)n));
  CMS_HIP(hipMemcpyAsync(h->ws_bound.ptr, bound.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(h->ws_force.ptr, job.force.data(), (size_t)n, hipMemcpyHostToDevice, h->stream));
  if ((rc = promote_rows(h, h->ws_bound.as<uint64_t>(), h->ws_force.as<uint8_t>(), true))) return rc;
  return widen_rows(h, h->ws_bound.as<uint64_t>(), h->d_row_mass, false);
}

// The subtraction's own middle: the counter check over the whole image
// against the live rows as they are now -- list rows and all, no store -- and
// only then the first write, the dense rewrite of the live list rows that
// lose entries.  Leaves the segments routed for the write pass.
int subtract_prepare(cms_handle* h, const Image& im, const uint8_t* d_payload, ApplyJob& job) {
  const Header& hd = im.hd;
  const int64_t n = h->n;
  Segs& sg = job.sg;
  int rc;
  // the live rows' states (12 bytes per owner, read back once beside the masses)
  std::vector<int32_t> hidx((size_t)n);
  std::vector<int64_t> off((size_t)n);
  CMS_HIP(hipMemcpy(hidx.data(), h->d_hidx, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  CMS_HIP(hipMemcpy(off.data(), h->d_off, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  // The rows the image subtracts from, and which kernel takes each.  In the
  // check a row whose image or live side is a list goes to k_ckpt_check_rows;
  // in the write pass the live lists are dense, so only the image's lists go
  // to k_ckpt_apply_lists; every other row to k_ckpt_apply.  Rows that
  // subtract nothing leave the segments.
  RowList crows;  // the check's listed rows
  std::vector<uint64_t> len_check(sg.len), len_write(sg.len);
  bool live_lists = false;
  for (size_t s = 0, r = 0; s < sg.len.size(); ++s, ++r) {
    while (im.dir[r].len == 0) ++r;
    const DirEntry& e = im.dir[r];
    const bool img_list = e.form == kRowList;
    if (e.mass == 0 || (img_list && e.len <= 2)) {  // (every stored counter is zero)
      len_check[s] |= kListBit, len_write[s] |= kListBit;
      continue;
    }
    if (hidx[r] < 0 && off[r] == 0)  // (mass > 0 passed the mass rule, yet the owner has no counters)
      return set_error(CMS_E_STATE, "cms_subtract_table: owner row %lld has a mass and no counters", (long long)r);
    const bool live_list = hidx[r] == kFormList;
    job.touched.push_back((int64_t)r);
    if (img_list || live_list) {
      crows.push((int64_t)r, e, hd.depth);
      len_check[s] |= kListBit;
    }
    if (img_list) {
      job.lists.push((int64_t)r, e, hd.depth);
      len_write[s] |= kListBit;
    }
    if (live_list) {  // the row's own mass: widen_rows rewrites it densely
      if (job.bound.empty()) job.bound.assign((size_t)n, 0);
      job.bound[r] = job.mass[r];
      live_lists = true;
    }
  }
  // ---- the counter check: no store ----
  sg.len = len_check;
  if ((rc = sg.upload(h))) return rc;
  if ((rc = launch_apply(h, Apply::kCheck, job, crows, d_payload))) return rc;
  unsigned long long res[3] = {0, 0, 0};
  if ((rc = read_out(h, job, res))) return rc;
  if (res[1] & kBadDest) return set_error(CMS_E_STATE, "cms_subtract_table: a live row changed form under the call");
  if (res[1] & kBadUnder)
    return set_error(CMS_E_OVERFLOW, "owner row %lld: a counter would fall below zero (the image is no part of this table's stream)",
                     (long long)res[2]);

  // ---- every check has passed: the first write follows ----
  if (live_lists) {  // bound > 0 on a list row is a rewrite (widen_needed); every other row's bound is 0: not listed
    CMS_HIP(h->ws_bound.ensure(sizeof(uint64_t) * (size_t)n));
    CMS_HIP(hipMemcpyAsync(h->ws_bound.ptr, job.bound.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_ckpt_list_bounds, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192))),
                       dim3(256), 0, h->stream, h->ws_bound.as<uint64_t>(), h->d_cbound, n);
    CMS_HIP(hipGetLastError());
    if ((rc = widen_rows(h, h->ws_bound.as<uint64_t>(), nullptr, false))) return rc;
  }
  sg.len = len_write;
  return sg.upload(h);
}

// The image (head parsed and validated into im, payload resident at d_payload,
// 16-byte aligned) added into the live table, or subtracted from it (u32
// counters).  Every check precedes the first write: a refusal leaves the table
// as it was.
int apply_resident(cms_handle* h, Apply op, Image& im, const uint8_t* d_payload) {
  const Header& hd = im.hd;
  const int64_t n = h->n;
  const bool add = op == Apply::kAdd;
  ApplyJob job;
  int rc = apply_open(h, op, im, d_payload, job);
  if (rc) return rc;
  if (!add && h->empty) return CMS_OK;  // every mass of the image is zero: nothing to take out of no counters
  if ((rc = add ? merge_prepare(h, im, job) : subtract_prepare(h, im, d_payload, job))) return rc;
  if ((rc = mark_touched(h, job))) return rc;
  if ((rc = launch_apply(h, op, job, job.lists, d_payload))) return rc;
  for (int64_t r = 0; r < n; ++r)  // the true masses, not the bounds
    job.mass[r] = add ? job.mass[r] + im.dir[r].mass : job.mass[r] - im.dir[r].mass;
  CMS_HIP(hipMemcpyAsync(h->d_row_mass, job.mass.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  unsigned long long res[3] = {0, 0, 0};
  if ((rc = read_out(h, job, res))) return rc;
  // "ingested, not finalized", as after a COO batch; cms_finalize re-derives norms and row maxima
  if (add) {
    h->pairs_ingested += hd.pairs_ingested;
    h->empty = false;
  } else {
    h->pairs_ingested = h->pairs_ingested > hd.pairs_ingested ? h->pairs_ingested - hd.pairs_ingested : 0;
  }
  h->norms_valid = false;
  h->finalized = false;
  h->stale_possible = true;
  if (res[1] & kBadDest)
    return set_error(CMS_E_STATE, add ? "cms_merge_table: a live row was in no form to take its adds"
                                      : "cms_subtract_table: a live row was in no form to give up its counters");
  return CMS_OK;
}

// The file is staged whole in device memory (through two pinned buffers), then
// merged (or subtracted) as a device image: the verify pass must see all of it before the
// first write, and a list row may straddle any staging boundary.
int merge_file(cms_handle* h, const char* path, Apply op) {
  File in;
  Image im;
  int rc = read_head_file(in, path, h, im);
  if (rc) return rc;
  const Header& hd = im.hd;
  DevBuf payload;
  if (payload.ensure((size_t)std::max<uint64_t>(hd.payload_bytes, 16)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(CMS_E_OOM, "%s: no device memory to stage the %.2f GB image",
                     op == Apply::kSub ? "cms_subtract_table" : "cms_merge_table", 1e-9 * (double)hd.payload_bytes);
  }
  const uint64_t nchunks = (hd.payload_bytes + kIoChunk - 1) / kIoChunk;
  if (nchunks > 0) {
    Staging st;
    if ((rc = st.init(std::min(kIoChunk, hd.payload_bytes), false))) return rc;
    const auto t_io = std::chrono::steady_clock::now();
    for (uint64_t i = 0; i < nchunks; ++i) {
      const int b = (int)(i & 1);
      const uint64_t o = i * kIoChunk, len = std::min(kIoChunk, hd.payload_bytes - o);
      if (i >= 2) CMS_HIP(hipEventSynchronize(st.ev_a[b]));  // pin[b] has left the host
      if (std::fread(st.pin[b], 1, (size_t)len, in.f) != len) return set_error(CMS_E_PARAM, "checkpoint %s: short read", path);
      CMS_HIP(hipMemcpyAsync(payload.as<uint8_t>() + o, st.pin[b], (size_t)len, hipMemcpyHostToDevice, h->side_stream));
      CMS_HIP(hipEventRecord(st.ev_a[b], h->side_stream));
    }
    CMS_HIP(hipStreamSynchronize(h->side_stream));
    add_host_time(h, "ckpt_io", t_io);
  }
  return apply_resident(h, op, im, payload.as<uint8_t>());
}

int merge_device(cms_handle* h, const void* d_buf, int64_t bytes, Apply op) {
  Image im;
  if (int rc = read_head_device(d_buf, bytes, h, im)) return rc;
  return apply_resident(h, op, im, static_cast<const uint8_t*>(d_buf) + im.hd.payload_off);
}

// ---- the table re-encoded at a width that divides its own, as an image ----
//
// Scan the rows as they fold (cms_fold.hip), give every folded row
// compact_form's form at shape (depth, wf) and its place in the payload on the
// host, pack.  The live table is only read.  cms_fold_table writes the image
// out; cms_compact_table, at wf == width where nothing folds, restores it in
// the table's place.
struct FoldPlan {
  Image im;  // header, IDs and directory of the folded image (its checksum after the pack)
  std::vector<uint8_t> tform;
  std::vector<uint64_t> dst;
  std::vector<DirEntry> was;  // the source rows' directory
};

int check_fold_width(cms_handle* h, int32_t wf) {
  if (wf < 1 || wf > h->p.width || h->p.width % wf != 0)
    return set_error(CMS_E_PARAM, "cms_fold_table: new_width %d is no divisor of the table's width %d", (int)wf,
                     (int)h->p.width);
  return CMS_OK;
}

int fold_plan(cms_handle* h, int32_t wf, FoldPlan& fp) {
  const int64_t n = h->n;
  const int depth = h->p.depth;
  Image old;  // the rows as they are: header, IDs, forms, place classes, bounds and masses (synchronises)
  int rc = plan_save(h, old);
  if (rc) return rc;
  // the tunables alone: compact_form rechecks the shape itself (wf % 32, 2 d wf <= 80 KiB, list_keys > 0), so at
  // wf == width they give the forms that forms_ok and lists_allowed() let the handle hold
  const bool forms = h->tune.forms;
  const int L = forms ? h->tune.list_keys : 0;
  const uint64_t list_mass_max =
      L > 0 && h->p.frac_bits == 0 ? (uint64_t)std::min(std::min(L, kListMaxKeys), kListMaxEntries / depth) : 0;
  std::vector<uint2> scan((size_t)n, make_uint2(0u, 0u));
  if (!h->empty) {  // (an empty handle's rows are all zero: its arrays are stale)
    DevBuf d_scan;
    CMS_HIP(d_scan.ensure(sizeof(uint2) * (size_t)n));
    if ((rc = fold_scan(h, wf, list_mass_max, d_scan.as<uint2>()))) return rc;
    CMS_HIP(hipMemcpyAsync(scan.data(), d_scan.ptr, sizeof(uint2) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
  }
  for (int64_t r = 0; r < n; ++r)
    if (scan[r].y & 2u)
      return set_error(CMS_E_OVERFLOW, "cms_fold_table: owner row %lld: a counter folded to width %d reaches 2^32; nothing is written",
                       (long long)r, (int)wf);
  Image& im = fp.im;
  im.hd = old.hd;
  im.hd.width = wf;
  im.ids = old.ids;
  im.dir.resize((size_t)n);
  fp.tform.resize((size_t)n);
  fp.dst.resize((size_t)n);
  std::vector<uint64_t> sums((size_t)depth);
  uint64_t at = 0;
  for (int64_t r = 0; r < n; ++r) {
    const uint64_t mass = old.dir[r].mass;
    const uint64_t* row_sums = nullptr;
    if (scan[r].y & 1u) {  // every sketch row sums to the mass
      std::fill(sums.begin(), sums.end(), mass);
      row_sums = sums.data();
    }
    uint64_t len = 0;
    const int form = compact_form(scan[r].x, mass, row_sums, depth, wf, h->p.frac_bits, L, forms, &len);
    DirEntry& e = im.dir[r];
    e.form = (uint8_t)form;
    e.cls = form >= kRowU1 && form <= kRowU16 ? (uint8_t)(form - kRowU1 + kCapU1) : 0;  // the form's own class
    e.rsv = 0;
    e.cbound = form == kRowHot ? 0u : scan[r].x;
    e.len = len;
    e.mass = mass;
    e.off = at;
    at += round16(len);
    fp.tform[r] = e.form;
    fp.dst[r] = e.off;
  }
  im.hd.payload_bytes = at;
  im.hd.file_bytes = im.hd.payload_off + at;
  im.hd.checksum = 0;
  if (const char* why = check_directory(im.hd, im.dir.data(), n))
    return set_error(CMS_E_STATE, "the directory of the rows re-formed at width %d is inconsistent (%s)", (int)wf, why);
  fp.was = std::move(old.dir);
  return CMS_OK;
}

// the folded rows into d_payload (payload_bytes of the plan, 16-byte aligned); the plan's header gets the checksum
int fold_payload(cms_handle* h, int32_t wf, FoldPlan& fp, uint8_t* d_payload) {
  const int64_t n = h->n;
  const uint64_t at = fp.im.hd.payload_bytes;
  if (at == 0) return CMS_OK;  // every row is zero
  DevBuf d_tform, d_dst, d_sum;
  CMS_HIP(d_tform.ensure((size_t)n));
  CMS_HIP(d_dst.ensure(sizeof(uint64_t) * (size_t)n));
  CMS_HIP(d_sum.ensure(2 * sizeof(unsigned long long)));
  CMS_HIP(hipMemcpyAsync(d_tform.ptr, fp.tform.data(), (size_t)n, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemcpyAsync(d_dst.ptr, fp.dst.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipMemsetAsync(d_sum.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
  if (int rc = fold_pack(h, wf, d_tform.as<uint8_t>(), d_dst.as<uint64_t>(), d_payload, at, d_sum.as<unsigned long long>()))
    return rc;
  unsigned long long sum = 0;
  CMS_HIP(hipMemcpyAsync(&sum, d_sum.ptr, sizeof(sum), hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  fp.im.hd.checksum = sum;
  return CMS_OK;
}

// ---- compact ----

// Every owner row re-stored in the form ckpt::compact_form gives its counters
// as they are now: the plan and the payload above at the table's own width.
// The scan, the rule, the re-formed payload beside the table and the loader's
// verify pass over it all leave the live rows alone: whatever can be refused
// is refused here, with the table as it was.  Then the arena is emptied and
// the payload restored as a load restores an image (restore_layout: no
// holes), and the handle's state -- finalized or not, its norms, its kept
// refresh lists -- is put back: none of it depends on how a row is stored.

// a step before the first change failed: its status (CMS_E_OOM for an
// allocation, as hip_fail reports it) under the call's own name
int compact_refused(int rc, int code = 0) {
  char was[384];
  std::snprintf(was, sizeof(was), "%s", cms_last_error());
  (void)hipGetLastError();  // (a refused allocation is not the next launch's error)
  return set_error(code ? code : rc, "cms_compact_table: %s; the table is unchanged", was);
}

int compact_table(cms_handle* h, int64_t* rows_changed) {
  const int64_t n = h->n;
  FoldPlan fp;
  int rc = fold_plan(h, h->p.width, fp);
  if (rc) return compact_refused(rc);
  Image& im = fp.im;
  int64_t changed = 0;
  for (int64_t r = 0; r < n; ++r) {
    // as the handle will hold the row: without the compact layout every narrow
    // row keeps a whole u16 slot, a row of zeros included
    uint8_t held_form = im.dir[r].form, held_cls = im.dir[r].cls;
    if (!h->compact && held_form != kRowHot) {
      held_cls = kCapU16;
      if (held_form == kRowZero) held_form = kRowU16;
    }
    changed += held_form != fp.was[r].form || held_cls != fp.was[r].cls;
  }
  const uint64_t at = im.hd.payload_bytes;
  DevBuf payload;
  if (payload.ensure((size_t)std::max<uint64_t>(at, 16)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(CMS_E_OOM, "cms_compact_table: no device memory for the re-formed rows; the table is unchanged");
  }
  if ((rc = fold_payload(h, h->p.width, fp, payload.as<uint8_t>()))) return compact_refused(rc);
  Segs sg;
  DevBuf d_out;
  // the loader's own pass over what the pack produced: checksum, pad bytes, every list entry.  A failure of the
  // pass itself keeps its status; a payload that fails it is this call's own fault, not the caller's argument
  if ((rc = verify_resident(h, im, payload.as<uint8_t>(), sg, d_out)))
    return compact_refused(rc, rc == CMS_E_PARAM ? CMS_E_STATE : 0);

  // ---- everything that can be refused has been: the old rows are given up ----
  const bool was_finalized = h->finalized, had_norms = h->norms_valid;
  unsigned long long res[2] = {0, 0};
  Expand ex;  // (stays empty: compact_form gives a handle only forms it holds)
  auto device_part = [&]() -> int {
    int r = restore_layout(h, im, ex);
    if (r) return r;
    build_segs(im, sg);
    if ((r = sg.upload(h))) return r;
    CMS_HIP(hipMemsetAsync(d_out.ptr, 0, 2 * sizeof(unsigned long long), h->stream));
    if ((r = unpack_range(h, sg, 0, at / 16, payload.as<uint8_t>(), d_out.as<unsigned long long>()))) return r;
    CMS_HIP(hipMemcpyAsync(res, d_out.ptr, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    CMS_HIP(hipStreamSynchronize(h->stream));
    return CMS_OK;
  };
  rc = device_part();
  if (rc || res[1] || res[0] != im.hd.checksum || !ex.rows.empty()) {
    (void)hipGetLastError();
    (void)leave_empty(h);
    return set_error(CMS_E_HIP, "cms_compact_table: the table was lost while its rows were laid out anew; the handle is empty, as after cms_reset");
  }
  h->finalized = was_finalized;
  h->norms_valid = had_norms;
  h->mfma_ready = false;  // the operand images are rebuilt when next asked for
  h->i8blk_ready = false;
  *rows_changed = changed;
  return CMS_OK;
}

// ---- fold: the image written out (cms_fold_table) ----

int fold_device(cms_handle* h, int32_t wf, void* d_buf, int64_t capacity, int64_t* bytes) {
  FoldPlan fp;
  int rc = fold_plan(h, wf, fp);
  if (rc) return rc;
  const Header& hd = fp.im.hd;
  *bytes = (int64_t)hd.file_bytes;
  if (!d_buf) return CMS_OK;  // (the size only)
  if (capacity < 0 || (uint64_t)capacity < hd.file_bytes)
    return set_error(CMS_E_PARAM, "folded device image needs %lld bytes, the buffer has %lld", (long long)hd.file_bytes,
                     (long long)capacity);
  if (reinterpret_cast<uintptr_t>(d_buf) & 15) return set_error(CMS_E_PARAM, "device image must be 16-byte aligned");
  uint8_t* base = static_cast<uint8_t*>(d_buf);
  if ((rc = fold_payload(h, wf, fp, base + hd.payload_off))) return rc;
  const std::vector<uint8_t> head = image_head(fp.im);
  CMS_HIP(hipMemcpyAsync(base, head.data(), head.size(), hipMemcpyHostToDevice, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

int fold_file(cms_handle* h, int32_t wf, const char* path) {
  FoldPlan fp;
  int rc = fold_plan(h, wf, fp);
  if (rc) return rc;
  const Header& hd = fp.im.hd;
  // the folded payload is packed whole beside the table (it is smaller than the table's stored bytes), then leaves
  // through the save path's pinned staging buffers
  DevBuf payload;
  if (payload.ensure((size_t)std::max<uint64_t>(hd.payload_bytes, 16)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(CMS_E_OOM, "cms_fold_table: no device memory for the folded rows; nothing is written");
  }
  if ((rc = fold_payload(h, wf, fp, payload.as<uint8_t>()))) return rc;
  return write_atomically(h, path, [&](FILE* f, bool& ok) -> int {
    const std::vector<uint8_t> head = image_head(fp.im);
    ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
    const uint64_t total = hd.payload_bytes, nchunks = (total + kIoChunk - 1) / kIoChunk;
    if (ok && nchunks > 0) {
      Staging st;
      if (int r = st.init(std::min(kIoChunk, total), false)) return r;
      auto span = [&](uint64_t i) { return std::min(total, (i + 1) * kIoChunk) - i * kIoChunk; };
      for (uint64_t i = 0; i <= nchunks && ok; ++i) {  // D2H of chunk i while the host writes chunk i - 1
        if (i < nchunks) {
          CMS_HIP(hipMemcpyAsync(st.pin[i & 1], payload.as<uint8_t>() + i * kIoChunk, (size_t)span(i), hipMemcpyDeviceToHost,
                                 h->stream));
          CMS_HIP(hipEventRecord(st.ev_a[i & 1], h->stream));
        }
        if (i >= 1) {
          CMS_HIP(hipEventSynchronize(st.ev_a[(i - 1) & 1]));
          ok = std::fwrite(st.pin[(i - 1) & 1], 1, (size_t)span(i - 1), f) == span(i - 1);
        }
      }
    }
    return CMS_OK;
  });
}

// what a fold accepts: what a save accepts, of u32 counters
int check_folds(cms_handle* h, int32_t wf) {
  if (int rc = check_saveable(h, "cms_fold_table")) return rc;
  if (h->f64)
    return set_error(CMS_E_STATE, "cms_fold_table: fp64 counters do not fold: a folded sum is not the sequential fp64 chain in ingest order, so the result would be no stream's table");
  return check_fold_width(h, wf);
}

}  // namespace
}  // namespace cms

using namespace cms;

extern "C" {

int cms_checkpoint_size(cms_handle* h, int64_t* bytes) {
  if (!h || !bytes) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;
  Guard g(h);
  if (int rc = check_saveable(h, "cms_checkpoint_size")) return rc;
  return save_device(h, nullptr, 0, bytes);
}

int cms_save_table(cms_handle* h, const char* path) {
  if (!h || !path) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;  // a pending device-ingest error: nothing is written
  Guard g(h);
  if (int rc = check_saveable(h, "cms_save_table")) return rc;
  return save_file(h, path);
}

int cms_save_table_device(cms_handle* h, void* d_buf, int64_t capacity, int64_t* bytes) {
  if (!h || !d_buf || !bytes) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;
  Guard g(h);
  if (int rc = check_saveable(h, "cms_save_table_device")) return rc;
  return save_device(h, d_buf, capacity, bytes);
}

int cms_load_table(cms_handle* h, const char* path) {
  if (!h || !path) return set_error(CMS_E_PARAM, "null argument");
  Guard g(h);
  return load_file(h, path);
}

int cms_load_table_device(cms_handle* h, const void* d_buf, int64_t bytes) {
  if (!h || !d_buf) return set_error(CMS_E_PARAM, "null argument");
  Guard g(h);
  return load_device(h, d_buf, bytes);
}

int cms_merge_table(cms_handle* h, const char* path) {
  if (!h || !path) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;  // a pending device-ingest error comes first: nothing is merged
  Guard g(h);
  if (int rc = check_receives_image(h, "cms_merge_table")) return rc;
  return merge_file(h, path, Apply::kAdd);
}

int cms_merge_table_device(cms_handle* h, const void* d_buf, int64_t bytes) {
  if (!h || !d_buf) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;
  Guard g(h);
  if (int rc = check_receives_image(h, "cms_merge_table_device")) return rc;
  return merge_device(h, d_buf, bytes, Apply::kAdd);
}

// (an fp64 subtraction is no inverse of the reference's rounded adds)
static int check_subtracts(cms_handle* h, const char* what) {
  if (int rc = check_receives_image(h, what)) return rc;
  if (h->f64)
    return set_error(CMS_E_STATE, "%s: fp64 counters do not subtract: (a + b) - b is not a in fp64, so the result would be no stream's table",
                     what);
  return CMS_OK;
}

int cms_subtract_table(cms_handle* h, const char* path) {
  if (!h || !path) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;  // a pending device-ingest error comes first: nothing is subtracted
  Guard g(h);
  if (int rc = check_subtracts(h, "cms_subtract_table")) return rc;
  return merge_file(h, path, Apply::kSub);
}

int cms_subtract_table_device(cms_handle* h, const void* d_buf, int64_t bytes) {
  if (!h || !d_buf) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;
  Guard g(h);
  if (int rc = check_subtracts(h, "cms_subtract_table_device")) return rc;
  return merge_device(h, d_buf, bytes, Apply::kSub);
}

int cms_compact_table(cms_handle* h, int64_t* rows_changed) {
  if (!h) return set_error(CMS_E_PARAM, "null handle");
  if (rows_changed) *rows_changed = 0;
  if (int rc = cms_synchronize(h)) return rc;  // a pending device-ingest error comes first: nothing is re-stored
  Guard g(h);
  if (h->per_owner)
    return set_error(CMS_E_STATE, "cms_compact_table: a per-owner-shape handle keeps the DataModel, not a table");
  if (h->comm || h->ext_comm || h->multi())
    return set_error(CMS_E_STATE, "cms_compact_table: the handle has a communicator (the ranks' copies would no longer be stored alike)");
  if (h->f64)
    return set_error(CMS_E_STATE, "cms_compact_table: fp64 counters are stored in one form: there is nothing to narrow");
  if (h->empty) return CMS_OK;  // every owner is on the zero row already
  int64_t changed = 0;
  const int rc = compact_table(h, &changed);
  if (rc == CMS_OK && rows_changed) *rows_changed = changed;
  return rc;
}

int cms_fold_size(cms_handle* h, int32_t new_width, int64_t* bytes) {
  if (!h || !bytes) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;  // a pending device-ingest error comes first
  Guard g(h);
  if (int rc = check_folds(h, new_width)) return rc;
  return fold_device(h, new_width, nullptr, 0, bytes);
}

int cms_fold_table(cms_handle* h, int32_t new_width, const char* path) {
  if (!h || !path) return set_error(CMS_E_PARAM, "null argument");
  if (int rc = cms_synchronize(h)) return rc;  // a pending device-ingest error comes first: nothing is written
  Guard g(h);
  if (int rc = check_folds(h, new_width)) return rc;
  return fold_file(h, new_width, path);
}

int cms_fold_table_device(cms_handle* h, int32_t new_width, void* d_buf, int64_t capacity, int64_t* bytes) {
  if (!h || !d_buf || !bytes) return set_error(CMS_E_PARAM, "null argument");
  *bytes = 0;
  if (int rc = cms_synchronize(h)) return rc;
  Guard g(h);
  if (int rc = check_folds(h, new_width)) return rc;
  return fold_device(h, new_width, d_buf, capacity, bytes);
}

int cms_checkpoint_info(const char* path, cms_params* out, int64_t* file_bytes) {
  if (!path || !out) return set_error(CMS_E_PARAM, "null argument");
  File in;
  Header hd;
  if (int rc = read_header_file(in, path, hd)) return rc;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(cms_params);
  out->depth = hd.depth;
  out->width = hd.width;
  out->counter_type = hd.counter_type;
  out->seed = hd.seed;
  out->num_owners = hd.num_owners;
  out->weighting = CMS_UNWEIGHTED;  // (an instance property, not the table's)
  out->device = -1;
  out->frac_bits = hd.frac_bits;
  out->flags = 0;
  if (file_bytes) *file_bytes = (int64_t)hd.file_bytes;
  return CMS_OK;
}

}  // extern "C"
