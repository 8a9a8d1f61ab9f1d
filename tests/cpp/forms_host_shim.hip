// Host-side build of widen_rows' per-row decisions and its pack / unpack steps
// (mahout_amd/csrc/cms_forms.h) for the CPU test tests/test_forms_host.py.
// k_widen_mark and k_widen_rows (cms_table.hip) call the same functions.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../mahout_amd/csrc/cms_forms.h"

extern "C" {

int fh_const(int which) {
  const int v[] = {cms::kFormU16, cms::kFormU8, cms::kFormU4, cms::kFormU2, cms::kFormU1, cms::kFormList,
                   cms::kCapNone, cms::kCapU1,  cms::kCapU2,  cms::kCapU4,  cms::kCapU8,  cms::kCapU16,
                   (int)cms::kRowAlign};
  return v[which];
}
int fh_form_bits(int f) { return cms::form_bits(f); }
unsigned fh_form_cap(int f) { return cms::form_cap(f); }
int fh_form_class(int f) { return cms::form_class(f); }
long long fh_class_units(int c, long long dw) { return cms::class_units(c, dw); }
int fh_class_of_units(long long units, long long dw) { return cms::class_of_units(units, dw); }

int fh_widen_needed(int f, int zero_row, unsigned long long nb, int all_touched) {
  return cms::widen_needed(f, zero_row != 0, nb, all_touched != 0);
}
int fh_widen_target(int f, int zero_row, unsigned nb, int to_u16, int w) {
  return cms::widen_target(f, zero_row != 0, nb, to_u16, w);
}
int fh_widen_in_place(int zero_row, int cc, int tf) { return cms::widen_in_place(zero_row != 0, cc, tf); }
int fh_widen_move_class(int tf) { return cms::widen_move_class(tf); }
int fh_widen_recount(int f, int zero_row) { return cms::widen_recount(f, zero_row != 0); }

// One past the last byte k_widen_rows' rewrite stores for a whole [d][w] row
// (0: none), by running its stores -- the same lanes (dense: 16 counters at
// every j < dw) and the same output words (re-count: w tb / 32 per sketch
// row) -- over a buffer of sentinels; -1 when the dense pack refuses tb.
long long fh_rewrite_extent(int recount, int tb, int d, int w) {
  const long long dw = (long long)d * w;
  const size_t room = (size_t)(dw + 16) * 4 + 64;
  std::vector<uint32_t> buf(room / 4, 0xA5A5A5A5u);
  if (recount) {
    std::vector<uint8_t> c8((size_t)w + 32, 0);
    const int nw = w / (32 / tb);
    for (int rr = 0; (long long)rr * w < dw; ++rr)
      for (int q = 0; q < nw; ++q) cms::pack_counts_word(tb, c8.data(), buf.data(), rr, w, q);
  } else {
    const uint32_t v[16] = {};
    for (long long j = 0; j < dw; j += 16)
      if (!cms::pack16_bits(tb, v, buf.data(), j)) return -1;
  }
  const uint8_t* b = reinterpret_cast<const uint8_t*>(buf.data());
  for (long long i = (long long)room - 1; i >= 0; --i)
    if (b[i] != 0xA5) return i + 1;
  return 0;
}

// counters [0, 16 * lanes) of a dense row in form f (row: 16-B aligned)
void fh_unpack_row(int f, const uint8_t* row, long long lanes, uint32_t* out) {
  for (long long l = 0; l < lanes; ++l) {
    uint32_t v[16];
    cms::unpack16(f, row, l * 16, v);
    std::memcpy(out + l * 16, v, sizeof(v));
  }
}
// the 16 counters v of lane j / 16 packed at tb bits into row; 0: refused
int fh_pack16(int tb, const uint32_t* v16, uint8_t* row, long long j) {
  uint32_t v[16];
  std::memcpy(v, v16, sizeof(v));
  return cms::pack16_bits(tb, v, reinterpret_cast<uint32_t*>(row), j) ? 1 : 0;
}
// output word q of sketch row rr from its u8 counts (the list re-count)
void fh_pack_counts_word(int tb, const uint8_t* c8, uint8_t* row, long long rr, int w, int q) {
  cms::pack_counts_word(tb, c8, reinterpret_cast<uint32_t*>(row), rr, w, q);
}

}  // extern "C"
