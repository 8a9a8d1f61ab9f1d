// cms_checkpoint.cpp -- host-side validation of a checkpoint image
// (cms_checkpoint.h).  Host only: tests/test_checkpoint_host.py builds this
// file for the CPU (tests/cpp/checkpoint_host_shim.cpp).
//
// Every check here precedes every write of cms_load_table: the device only
// ever sees a directory whose forms, lengths and offsets are consistent with
// the handle's shape, so the scatter's addresses stay inside the rows' places.
#include "cms_checkpoint.h"

#include <cstring>

namespace cms {
namespace ckpt {

void layout_sections(Header* hd) {
  const uint64_t n = (uint64_t)hd->num_owners;
  hd->header_bytes = kHeaderBytes;
  hd->dir_entry_bytes = sizeof(DirEntry);
  hd->ids_off = kHeaderBytes;
  hd->ids_bytes = (hd->flags & kFlagOwnerIds) ? 8 * n : 0;
  hd->dir_off = round16(hd->ids_off + hd->ids_bytes);
  hd->dir_bytes = sizeof(DirEntry) * n;
  hd->payload_off = hd->dir_off + hd->dir_bytes;
}

const char* check_header(const Header& hd, uint64_t avail) {
  if (avail < kHeaderBytes) return "shorter than a checkpoint header";
  if (std::memcmp(hd.magic, kMagic, sizeof(kMagic)) != 0) return "not a checkpoint image (bad magic)";
  if (hd.version != kVersion) return "unknown checkpoint format version";
  if (hd.header_bytes != kHeaderBytes || hd.dir_entry_bytes != sizeof(DirEntry)) return "header or entry size";
  if (hd.counter_type != 0 && hd.counter_type != 1) return "unknown counter type";
  if (hd.depth < 1 || hd.depth > kMaxDepth) return "depth outside [1, 32]";
  if (hd.width < 1 || hd.width > (hd.counter_type == 1 ? (1 << 20) : (1 << 15))) return "width outside the counter type's range";
  if (hd.frac_bits < 0 || hd.frac_bits > 31) return "frac_bits outside [0, 31]";
  if (hd.num_owners < 1 || hd.num_owners > (int64_t(1) << 24)) return "num_owners outside [1, 2^24]";
  if (hd.pairs_ingested < 0) return "negative pairs_ingested";
  if (hd.flags & ~kFlagOwnerIds) return "unknown header flags";
  Header want = hd;
  layout_sections(&want);
  if (hd.ids_off != want.ids_off || hd.ids_bytes != want.ids_bytes || hd.dir_off != want.dir_off ||
      hd.dir_bytes != want.dir_bytes || hd.payload_off != want.payload_off)
    return "section offsets disagree with the shape";
  if (hd.payload_bytes % 16 != 0) return "payload length is not a multiple of 16";
  // (n <= 2^24 and d w <= 2^25: no sum here can wrap)
  if (hd.payload_bytes > (uint64_t(1) << 60)) return "payload length";
  if (hd.file_bytes != hd.payload_off + hd.payload_bytes) return "file length disagrees with the sections";
  if (avail < hd.file_bytes) return "shorter than its header claims";
  if (avail > hd.file_bytes) return "longer than its header claims";
  return nullptr;
}

const char* check_owner_ids(const int64_t* ids, int64_t n) {
  for (int64_t i = 1; i < n; ++i)
    if (ids[i] <= ids[i - 1]) return "owner IDs are not strictly ascending";
  return nullptr;
}

uint64_t dense_len(int form, int64_t dw) {
  switch (form) {
    case kRowU1: return (uint64_t)dw / 8;
    case kRowU2: return (uint64_t)dw / 4;
    case kRowU4: return (uint64_t)dw / 2;
    case kRowU8: return (uint64_t)dw;
    case kRowU16: return 2 * (uint64_t)dw;
    case kRowHot: return 4 * (uint64_t)dw;
    case kRowF64: return 8 * (uint64_t)dw;
    default: return 0;
  }
}

const char* check_directory(const Header& hd, const DirEntry* dir, int64_t n) {
  const int64_t d = hd.depth, w = hd.width, dw = d * w;
  const bool f64 = hd.counter_type == 1;
  const bool forms = !f64 && w % 32 == 0;                            // cms_handle::forms_ok
  const bool lists = forms && w % 8 == 0 && dw * 2 <= 80 * 1024;     // lists_allowed's shape part
  uint64_t at = 0;
  for (int64_t r = 0; r < n; ++r) {
    const DirEntry& e = dir[r];
    if (e.form >= kRowForms) return "unknown row form";
    if (e.rsv != 0) return "reserved directory bits set";
    if (e.cls > 5) return "unknown place class";
    uint64_t len = 0;
    int need_cls = 0;  // the narrowest class that holds the form
    switch (e.form) {
      case kRowZero:
        if (e.cls != 0) return "a zero row has no place";
        break;
      case kRowList: {
        if (!lists) return "a list row in a shape that has none";
        if (e.len < 2 || (e.len - 2) % (2 * (uint64_t)d) != 0) return "list row length disagrees with the depth";
        const uint64_t m = (e.len - 2) / (2 * (uint64_t)d);
        // (a list is stored only while it is smaller than the dense row: it fits a whole u16 slot)
        if (m > (uint64_t)kListMaxKeys || m * (uint64_t)d > (uint64_t)kListMaxEntries || e.len > 2 * (uint64_t)dw)
          return "list row too long";
        len = e.len;
        break;
      }
      case kRowU1:
        if (!forms || w % 128 != 0) return "a 1-bit row in a shape that has none";
        need_cls = 1;
        break;
      case kRowU2:
        if (!forms || w % 64 != 0) return "a 2-bit row in a shape that has none";
        need_cls = 2;
        break;
      case kRowU4:
        if (!forms) return "a 4-bit row in a shape that has none";
        need_cls = 3;
        break;
      case kRowU8:
        if (!forms) return "a u8 row in a shape that has none";
        need_cls = 4;
        break;
      case kRowU16:
        if (f64) return "a u16 row in an fp64 table";
        need_cls = 5;
        break;
      case kRowHot:
        if (f64) return "a u32 row in an fp64 table";
        if (e.cls != 0) return "a hot row has no arena place";
        break;
      case kRowF64:
        if (!f64) return "an fp64 row in a u32 table";
        if (e.cls != 0) return "an fp64 row has no arena place";
        break;
    }
    if (e.form >= kRowU1) {
      len = dense_len(e.form, dw);
      if (e.len != len) return "row length disagrees with its form and the shape";
    } else if (e.form == kRowZero && e.len != 0) {
      return "a zero row with stored bytes";
    }
    if (f64 && e.form != kRowF64 && e.form != kRowZero) return "a counter row in an fp64 table";
    if (e.cls < need_cls) return "place class narrower than the row's form";
    if (e.off % 16 != 0) return "payload offset not 16-byte aligned";
    if (e.off != at) return "payload offsets not ascending in row order";
    at += round16(len);
    if (at > hd.payload_bytes) return "a row past the end of the payload";
  }
  if (at != hd.payload_bytes) return "payload length disagrees with the directory";
  return nullptr;
}

// ---- cms_merge_table: every check here, like those above, precedes every
// write -- and the table it protects is populated, so a refusal must leave it
// bit for bit as it was ----

const char* check_merge_params(const Header& hd, const int64_t* live_a, const int64_t* live_b, const int64_t* live_ids,
                               const int64_t* image_ids) {
  // a sum of sketches under different hash functions is silently wrong
  for (int i = 0; i < hd.depth; ++i)
    if (hd.a[i] != live_a[i] || hd.b[i] != live_b[i]) return "the image was built with other hash parameters";
  if ((live_ids == nullptr) != (image_ids == nullptr))
    return live_ids ? "the handle has owner IDs, the image has none" : "the image has owner IDs, the handle has none";
  if (live_ids && std::memcmp(live_ids, image_ids, 8 * (size_t)hd.num_owners) != 0)
    return "the image's owner IDs differ from the handle's";
  return nullptr;
}

const char* check_merge_masses(const Header& hd, const DirEntry* dir, const uint64_t* live_mass, int64_t n) {
  if (hd.counter_type != 0) return nullptr;
  for (int64_t r = 0; r < n; ++r) {
    const uint64_t m = live_mass ? live_mass[r] : 0;
    // (either term alone past 2^32 also refuses: the sum below cannot wrap then)
    if (m >= (uint64_t(1) << 32) || dir[r].mass >= (uint64_t(1) << 32) || m + dir[r].mass >= (uint64_t(1) << 32))
      return "a row's total increment reached 2^32 (u32 counters)";
  }
  return nullptr;
}

const char* check_subtract_masses(const Header& hd, const DirEntry* dir, const uint64_t* live_mass, int64_t n) {
  if (hd.counter_type != 0) return "fp64 counters do not subtract";
  for (int64_t r = 0; r < n; ++r) {
    const uint64_t m = live_mass ? live_mass[r] : 0;
    if (m < dir[r].mass) return "a row's mass would fall below zero: the image is no part of this table's stream";
  }
  return nullptr;
}

uint64_t merge_increment(const DirEntry& e) {
  if (e.len == 0) return 0;
  uint64_t cap;
  switch (e.form) {
    case kRowList:
      if (e.len <= 2) return 0;  // (no entries)
      // every key may share a bucket: the loader bounds a list's length, not a bucket's count (a list a build
      // stored has counters below 2^8, and a cbound that says so)
      cap = (uint64_t)kListMaxKeys;
      break;
    case kRowU1: cap = 1; break;
    case kRowU2: cap = 3; break;
    case kRowU4: cap = 15; break;
    case kRowU8: cap = 255; break;
    // a u16 row in a whole slot takes its adds without a cbound update
    // (k_widen_mark skips it), so only its form and its mass bound it
    case kRowU16: return e.mass < 65535 ? e.mass : 65535;
    default: return e.mass;  // hot, fp64
  }
  if (e.cbound != 0 && e.cbound < cap) cap = e.cbound;
  return e.mass < cap ? e.mass : cap;
}

// ---- cms_compact_table: the one statement of the target form (the header's
// comment; mahout_amd.checkpoint.compact_form is its numpy twin) ----

int compact_form(uint32_t cmax, uint64_t mass, const uint64_t* row_sums, int depth, int width, int frac_bits,
                 int list_keys, bool forms, uint64_t* len) {
  const int64_t d = depth, w = width, dw = d * w;
  const bool narrow = forms && w % 32 == 0;
  int form;
  if (cmax == 0) {
    form = kRowZero;
  } else if (mass >= (uint64_t(1) << 16) || cmax >= (1u << 16)) {
    form = kRowHot;
  } else {
    form = narrow && w % 128 == 0 && cmax <= 1 ? kRowU1
         : narrow && w % 64 == 0 && cmax <= 3  ? kRowU2
         : narrow && cmax <= 15                ? kRowU4
         : narrow && cmax <= 255               ? kRowU8
                                               : kRowU16;
    const uint64_t m = mass;
    const uint64_t limit = (uint64_t)(list_keys < kListMaxKeys ? list_keys : kListMaxKeys);
    // (cmax <= 255: the in-place writers re-count a live list row's entries in u8 counters -- k_widen_rows -- as the
    // builder's own lists allow them to; a row with a fuller bucket stays dense)
    bool list = frac_bits == 0 && narrow && 2 * dw <= 80 * 1024 && list_keys > 0 && row_sums != nullptr && cmax <= 255;
    for (int i = 0; list && i < depth; ++i) list = row_sums[i] == m;
    if (list && m >= 1 && m <= limit && (uint64_t)d * m <= (uint64_t)kListMaxEntries &&
        2 + 2 * (uint64_t)d * m < dense_len(form, dw)) {
      if (len) *len = 2 + 2 * (uint64_t)d * m;
      return kRowList;
    }
  }
  if (len) *len = dense_len(form, dw);
  return form;
}

}  // namespace ckpt
}  // namespace cms
