// cms_set_bits.h -- what the host and the device share of the dense route of
// the set similarities (cms_set_bits.hip): the bit matrix's geometry and the
// expansion of its bits into the e2m1 operands of the fp4 MFMA.
//
// The bit matrix of a side: one row per list, one column per cross index, bit
// u of row a set iff list a holds cross index u.  A row is cut into K stages
// of kBitsStage cross indices (kBitsStageWords u32 words, bit u & 31 of word
// u >> 5); num is padded with zero bits to whole stages.  In memory the matrix
// is K-blocked: blocks of kBitsBlk rows, and inside a block every stage of its
// rows is one contiguous run ([stage][row][8 words], 4 KiB), so a stage of a
// workgroup's 128-row panel is a single run when its rows are consecutive.
// Rows past n inside the last block are zero.
//
// The counts.  A set bit becomes the e2m1 nibble 0x2 (1.0), a clear one 0x0,
// so every product is 0 or 1 and an f32 accumulator holds their sum exactly up
// to 2^24.  K is therefore cut into segments of at most kBitsSegMax cross
// indices (a whole number of stages); at a segment's end the accumulators are
// converted to u32, added to the running counts and cleared, and the result is
// the exact shared-entry count for any num below 2^31.
//
// Everything here is a pure __host__ __device__ function;
// tests/test_set_bits_host.py runs it on the CPU
// (tests/cpp/set_bits_host_shim.hip).
#pragma once
#include <stdint.h>

#include "cms_hash.h"

namespace cms {

constexpr int kBitsStage = 256;                    // cross indices of a row per K stage
constexpr int kBitsStageWords = kBitsStage / 32;   // ... as u32 words: 32 B of bits, 128 B of nibbles in LDS
constexpr int kBitsBlk = 128;                      // rows per block of the K-blocked matrix: one panel of a tile
constexpr int64_t kBitsSegMax = int64_t(1) << 24;  // cross indices per f32 segment
constexpr int64_t kBitsBudgetMbDefault = 16384;    // CMS_SET_BITS_MB

// Eight bits to eight e2m1 nibbles of one dword: nibble j is 0x2 (1.0) iff bit
// j of `byte` is set.
CMS_HD uint32_t bits_expand8(uint32_t byte) {
  uint32_t x = byte & 0xFFu;
  x = (x | (x << 12)) & 0x000F000Fu;
  x = (x | (x << 6)) & 0x03030303u;
  x = (x | (x << 3)) & 0x11111111u;
  return x << 1;
}

// K stages of a row over num cross indices (at least one: an empty face still has a stage of zeros)
CMS_HD int64_t bits_stages(int64_t num) { return num <= 0 ? 1 : (num + kBitsStage - 1) / kBitsStage; }
CMS_HD int64_t bits_padded_k(int64_t num) { return bits_stages(num) * kBitsStage; }
// stages per segment for a segment of `asked` cross indices (CMS_SET_BITS_KSEG; 0: the maximum): whole stages,
// at least one, at most kBitsSegMax cross indices
CMS_HD int64_t bits_seg_stages(int64_t asked) {
  if (asked <= 0 || asked >= kBitsSegMax) return kBitsSegMax / kBitsStage;
  return asked < kBitsStage ? 1 : asked / kBitsStage;
}
CMS_HD int64_t bits_segments(int64_t num, int64_t seg_stages) {
  return (bits_stages(num) + seg_stages - 1) / seg_stages;
}
// rows of the matrix: n padded to whole blocks
CMS_HD int64_t bits_padded_rows(int64_t n) { return (n + kBitsBlk - 1) / kBitsBlk * kBitsBlk; }
CMS_HD int64_t bits_matrix_bytes(int64_t n, int64_t num) { return bits_padded_rows(n) * (bits_padded_k(num) / 8); }
// the u32 word index of word w (cross indices [32 w, 32 w + 32)) of row `row`; stages: bits_stages(num)
CMS_HD int64_t bits_word_off(int64_t row, int64_t w, int64_t stages) {
  return (row / kBitsBlk) * (kBitsBlk * kBitsStageWords * stages) + (w / kBitsStageWords) * (kBitsBlk * kBitsStageWords) +
         (row % kBitsBlk) * kBitsStageWords + (w % kBitsStageWords);
}

}  // namespace cms
