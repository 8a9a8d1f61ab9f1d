// cms_forms.h -- the storage forms of a narrow row, the classes of the places
// rows live in, and the per-row decisions of widen_rows (cms_table.hip).
//
// Everything here is a pure __host__ __device__ function: k_widen_mark and
// k_widen_rows call these and hold no second copy, and tests/test_forms_host.py
// enumerates them on the CPU (tests/cpp/forms_host_shim.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cms {

constexpr int32_t kFormU16 = -1, kFormU8 = -2, kFormU4 = -3, kFormU2 = -4, kFormU1 = -5, kFormList = -6;
constexpr uint32_t form_cap(int32_t form) {
  return form == kFormList ? 0u : form == kFormU1 ? 1u : form == kFormU2 ? 3u : form == kFormU4 ? 15u
       : form == kFormU8 ? 255u : 65535u;
}
__host__ __device__ constexpr int form_bits(int32_t f) {  // counter bits of a form (0: a list row)
  return f == kFormList ? 0 : f == kFormU1 ? 1 : f == kFormU2 ? 2 : f == kFormU4 ? 4 : f == kFormU8 ? 8 : 16;
}

constexpr int64_t kRowAlign = 64;  // u16 units (128 B: an L2 line, so no two rows share one) per arena allocation unit
__host__ __device__ constexpr int64_t slot_units(int64_t dw) { return (dw + kRowAlign - 1) / kRowAlign * kRowAlign; }
// off[row] bits 0-2 (the offset is a multiple of kRowAlign): the widest form
// the row's place holds -- a row is written in place only in a form no wider.
// kCapNone: a list row's place, or the shared zero row (offset 0).
constexpr int64_t kCapMask = 7;
enum : int { kCapNone = 0, kCapU1 = 1, kCapU2 = 2, kCapU4 = 3, kCapU8 = 4, kCapU16 = 5 };
__host__ __device__ constexpr int form_class(int32_t f) {
  return f == kFormU1 ? kCapU1 : f == kFormU2 ? kCapU2 : f == kFormU4 ? kCapU4 : f == kFormU8 ? kCapU8
       : f == kFormU16 ? kCapU16 : kCapNone;
}
// u16 units a form's row takes in the arena (rounded to kRowAlign)
__host__ __device__ constexpr int64_t class_units(int c, int64_t dw) {
  return c == kCapU16 ? slot_units(dw)
       : ((c == kCapU8 ? dw / 2 : c == kCapU4 ? dw / 4 : c == kCapU2 ? dw / 8 : c == kCapU1 ? dw / 16 : 0) +
          kRowAlign - 1) / kRowAlign * kRowAlign;
}
// the widest form a place of `units` u16 holds
__host__ __device__ constexpr int class_of_units(int64_t units, int64_t dw) {
  return units >= class_units(kCapU16, dw) ? kCapU16 : units >= class_units(kCapU8, dw) ? kCapU8
       : units >= class_units(kCapU4, dw) ? kCapU4 : units >= class_units(kCapU2, dw) ? kCapU2
       : units >= class_units(kCapU1, dw) && dw >= 16 ? kCapU1 : kCapNone;
}

// ---- widen_rows: what happens to one touched row ----
//
// zero_row: the owner has no counters of its own (off[r] == 0; its hidx reads
// kFormU16).  It holds nothing, so it counts as a list row of no entries in
// every decision below: any narrow form may be its target, it always moves,
// and it is rewritten by the list re-count -- which never reads the shared
// zero row and packs at any width.

// the smallest place a moved row takes (kCap class): a mover whose target
// form is narrower than u8 takes a u8 place, any other a whole slot.  With the
// rows' bounds from their tracked maxima most rows never pass u8: after the
// 1B-pair config-5 stream 78.7 GB in use against 102 GB with whole slots
// for every mover (scripts/stream_compact_probe.py)
#ifndef CMS_MOVE_CLASS
#define CMS_MOVE_CLASS 4
#endif

// Is a touched row (new bound nb) rewritten at all?  Its form must hold nb;
// an accumulate build (all_touched) rewrites every touched row, and a row on
// the zero row needs a place of its own before any add.
__host__ __device__ constexpr bool widen_needed(int32_t f, bool zero_row, uint64_t nb, bool all_touched) {
  return all_touched || zero_row || nb > (uint64_t)form_cap(f);
}

// The form a listed row is rewritten in: the narrowest form wider than its
// own whose capacity holds its new bound nb (u16 for an accumulate build) --
// a 2-bit row that one more pair lifts to 4 becomes a 4-bit row.  2-bit rows
// need w % 64 == 0 and 1-bit rows w % 128 == 0 (whole 32-bit words per sketch
// row at 16 counters per lane); forms exist only when w % 32 == 0.
__host__ __device__ constexpr int32_t widen_target(int32_t f, bool zero_row, uint32_t nb, int to_u16, int w) {
  const int sb = zero_row ? 0 : form_bits(f);
  if (to_u16 || (w & 31) != 0) return kFormU16;
  if (sb < 1 && nb <= 1u && (w & 127) == 0) return kFormU1;
  if (sb < 2 && nb <= 3u && (w & 63) == 0) return kFormU2;
  if (sb < 4 && nb <= 15u) return kFormU4;
  if (sb < 8 && nb <= 255u) return kFormU8;
  return kFormU16;
}

// A listed row is rewritten in place when its place (class cc) holds the
// target form, else it moves to a new place at the arena's end; a row on the
// zero row always moves.
__host__ __device__ constexpr bool widen_in_place(bool zero_row, int cc, int32_t tf) {
  return !zero_row && cc >= form_class(tf);
}
// The class of a mover's new place: CMS_MOVE_CLASS (a u8 place) for a target
// below u8, a whole slot for u8 and u16 -- places sized to each target form
// left a row moving once per widening (a 1B-pair stream then held 151 GB).
__host__ __device__ constexpr int widen_move_class(int32_t tf) {
  return form_class(tf) >= CMS_MOVE_CLASS ? kCapU16 : CMS_MOVE_CLASS;
}

// The rewrite's branch: list rows and zero-row owners are re-counted from
// their entries (none for the zero row), every other row is repacked densely.
__host__ __device__ constexpr bool widen_recount(int32_t f, bool zero_row) { return zero_row || f == kFormList; }

// Dense repack: counters [j, j + 16) (j % 16 == 0) of a row stored in form f
// at p8 (16-B aligned for u16 / u8 rows).
__host__ __device__ __forceinline__ void unpack16(int32_t f, const uint8_t* p8, int64_t j, uint32_t (&v)[16]) {
  if (f == kFormU16) {
    const uint4 x0 = *reinterpret_cast<const uint4*>(p8 + 2 * j);
    const uint4 x1 = *reinterpret_cast<const uint4*>(p8 + 2 * j + 16);
    const uint32_t wv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (wv[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
  } else if (f == kFormU8) {
    const uint4 x = *reinterpret_cast<const uint4*>(p8 + j);
    const uint32_t wv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (wv[q >> 2] >> ((q & 3) * 8)) & 255u;
  } else if (f == kFormU2) {
    const uint32_t x = *reinterpret_cast<const uint32_t*>(p8 + (j >> 2));
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (x >> (q * 2)) & 3u;
  } else if (f == kFormU1) {
    const uint32_t x = *reinterpret_cast<const uint16_t*>(p8 + (j >> 3));
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (x >> q) & 1u;
  } else {  // kFormU4
    const uint2 x = *reinterpret_cast<const uint2*>(p8 + (j >> 1));
    const uint32_t wv[2] = {x.x, x.y};
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (wv[q >> 3] >> ((q & 7) * 4)) & 15u;
  }
}

// 16 counters v[0..16) packed at 32 / C bits into C-counter words at w32[j / C ...]
template <int C>
__host__ __device__ __forceinline__ void pack16(const uint32_t (&v)[16], uint32_t* w32, int64_t j) {
#pragma unroll
  for (int q = 0; q < 16; q += C) {
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) word |= v[q + k] << (k * (32 / C));
    w32[(j + q) / C] = word;
  }
}
// Dense repack: the 16 counters at tb bits each, words [j tb / 32, (j + 16) tb / 32)
// of the row at w32.  A dense row's target is wider than its own form, so tb
// is 2, 4, 8 or 16; any other width writes nothing and returns false.
__host__ __device__ __forceinline__ bool pack16_bits(int tb, const uint32_t (&v)[16], uint32_t* w32, int64_t j) {
  switch (tb) {
    case 2: pack16<16>(v, w32, j); return true;
    case 4: pack16<8>(v, w32, j); return true;
    case 8: pack16<4>(v, w32, j); return true;
    case 16: pack16<2>(v, w32, j); return true;
    default: return false;
  }
}

// List re-count: output word q (< w tb / 32) of sketch row rr from the row's
// u8 counts c8[0..w), at tb bits per counter (any form's width).
__host__ __device__ __forceinline__ void pack_counts_word(int tb, const uint8_t* c8, uint32_t* w32, int64_t rr, int w,
                                                          int q) {
  const int cpw = 32 / tb;  // counters per output word
  uint32_t word = 0;
  for (int k = 0; k < cpw; ++k) word |= (uint32_t)c8[q * cpw + k] << (k * tb);
  w32[(rr * w) / cpw + q] = word;
}

}  // namespace cms
