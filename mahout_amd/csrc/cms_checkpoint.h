// cms_checkpoint.h -- the checkpoint image (format version 1; DESIGN.md 3
// "Checkpoint image") and its host-side validation.  Plain C++: no device
// code and no HIP types, so tests/cpp/checkpoint_host_shim.cpp builds it for
// the CPU.
//
// One image serves both sinks: a file is the image, a device image is the
// same bytes.  Little-endian throughout.
//
//   [0, 640)            Header
//   [640, 640 + 8 n)    owner IDs, i64 [n]      (only with kFlagOwnerIds)
//   dir_off (16-B al.)  row directory, DirEntry [n]
//   payload_off         payload: every row's stored bytes in row order, each
//                       row on a 16-byte boundary, pad bytes zero
#pragma once
#include <cstdint>

namespace cms {
namespace ckpt {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the image is little-endian and written from memory");

constexpr char kMagic[8] = {'M', 'C', 'M', 'S', 'C', 'K', 'P', 'T'};
constexpr uint32_t kVersion = 1;
constexpr uint32_t kHeaderBytes = 640;
constexpr int kMaxDepth = 32;  // CMS_MAX_DEPTH
constexpr uint32_t kFlagOwnerIds = 1u;

// stored form of one owner row
enum : uint8_t {
  kRowZero = 0,  // the owner has no counters of its own: no payload
  kRowList = 1,  // u16 m, then u16 [d][m] buckets: 2 + 2 d m bytes
  kRowU1 = 2,    // d w / 8 bytes
  kRowU2 = 3,    // d w / 4
  kRowU4 = 4,    // d w / 2
  kRowU8 = 5,    // d w
  kRowU16 = 6,   // 2 d w
  kRowHot = 7,   // u32 counters: 4 d w
  kRowF64 = 8,   // fp64 counters (CMS_COUNTER_F64 handles): 8 d w
  kRowForms = 9
};

struct Header {
  char magic[8];
  uint32_t version;       // kVersion
  uint32_t header_bytes;  // kHeaderBytes
  int32_t depth, width, counter_type, frac_bits;
  int64_t num_owners;
  int64_t pairs_ingested;
  int64_t seed;
  uint32_t flags;            // kFlagOwnerIds
  uint32_t dir_entry_bytes;  // sizeof(DirEntry)
  uint64_t ids_off, ids_bytes;
  uint64_t dir_off, dir_bytes;
  uint64_t payload_off, payload_bytes;
  uint64_t checksum;    // sum mod 2^64 of the payload as little-endian u64 words
  uint64_t file_bytes;  // payload_off + payload_bytes
  int64_t a[kMaxDepth];  // the hash parameters in use (rows >= depth: 0)
  int64_t b[kMaxDepth];
};
static_assert(sizeof(Header) == kHeaderBytes, "checkpoint header layout");

struct DirEntry {
  uint8_t form;    // kRow*
  uint8_t cls;     // place class: the low kCap* bits of off[r] (0 for zero, hot and fp64 rows)
  uint16_t rsv;    // 0
  uint32_t cbound; // bound of the row's counters (cms_owner_forms)
  uint64_t len;    // stored bytes
  uint64_t mass;   // row mass
  uint64_t off;    // byte offset in the payload (a multiple of 16)
};
static_assert(sizeof(DirEntry) == 32, "checkpoint directory entry layout");

constexpr uint64_t round16(uint64_t x) { return (x + 15) & ~uint64_t(15); }
constexpr int kListMaxKeys = 1024;     // the longest list a build stores (cms_build.hip kMidListKeys)
constexpr int kListMaxEntries = 8192;  // d m of a list row (k_widen_rows reads that many)

// Section offsets and sizes of an image of this shape (everything but
// payload_bytes, checksum and file_bytes).
void layout_sections(Header* hd);

// Each returns nullptr when the part is valid, else a message.  avail: bytes
// the file or device image really has.
const char* check_header(const Header& hd, uint64_t avail);
// strictly ascending, as cms_set_owner_ids requires
const char* check_owner_ids(const int64_t* ids, int64_t n);
// every entry's form, class and length against the shape; offsets ascending,
// 16-byte aligned and tiling [0, payload_bytes) exactly
const char* check_directory(const Header& hd, const DirEntry* dir, int64_t n);
// stored bytes of a dense form's row (0: zero rows, lists and unknown forms)
uint64_t dense_len(int form, int64_t dw);

// ---- merging an image into a live table (cms_merge_table) ----
// The image adds counter by counter only under the live table's hash
// functions and owner universe: a[i], b[i] for i < depth must equal the
// header's (rows >= depth are not in use), and the ID sections must agree --
// both absent (null), or both present and identical.  nullptr: compatible.
const char* check_merge_params(const Header& hd, const int64_t* live_a, const int64_t* live_b, const int64_t* live_ids,
                               const int64_t* image_ids);
// u32 counters: a row's mass plus the image's reaches 2^32 (the ingest's rule:
// old + inc >= 2^32).  nullptr: every row fits (always for fp64 counters).
const char* check_merge_masses(const Header& hd, const DirEntry* dir, const uint64_t* live_mass, int64_t n);
// the most the image's row can add to one counter of the live row: min(cbound,
// mass) for a form row (a list's counters are bounded the same way, and by
// kListMaxKeys: every key of a loaded list may share a bucket), the mass for a
// hot or fp64 row, 0 for a row that stores nothing
uint64_t merge_increment(const DirEntry& e);

// ---- subtracting an image from a live table (cms_subtract_table) ----
// u32 counters only.  No row's mass may fall below zero: live_mass[r] >=
// dir[r].mass for every r (live_mass null: an empty table, mass 0 everywhere,
// which accepts only an image whose masses are all 0).  The comparison is
// made on the 64-bit masses as they are: nothing is added, nothing wraps.
// nullptr: every row's mass stays at or above zero.  (The masses cannot show a
// single counter going below zero: that is the device's check.)
const char* check_subtract_masses(const Header& hd, const DirEntry* dir, const uint64_t* live_mass, int64_t n);

// ---- compacting a live table (cms_compact_table) ----
// The narrowest form (kRow*) that holds a u32 table's row as it is now, and
// *len = its stored bytes.  cmax: the row's largest counter; mass: its row
// mass; row_sums: the sums of its depth sketch rows (null: not known, which
// rules a list out).  forms: the handle stores 1- to 8-bit rows and lists
// where the shape has them (false: CMS_NO_FORMS); list_keys: the handle's list
// limit (0: it stores no lists).  In order:
//   1. cmax == 0: kRowZero -- the owner returns to the shared zero row;
//   2. mass >= 2^16 or cmax >= 2^16: kRowHot;
//   3. D = the narrowest of u1 (w % 128 == 0), u2 (w % 64 == 0), u4, u8
//      (w % 32 == 0 and forms) and u16 that holds cmax;
//   4. kRowList instead of D only when frac_bits == 0, the shape has lists
//      (forms, w % 32 == 0, 2 d w <= 80 KiB), every sketch row sums to the
//      mass m, 1 <= m <= min(list_keys, kListMaxKeys), d m <= kListMaxEntries,
//      2 + 2 d m is strictly less than D's stored bytes, and cmax <= 255: a
//      list never holds a bucket more than 255 times, as no built list does
//      (the writers re-count a list's entries in u8 counters).
int compact_form(uint32_t cmax, uint64_t mass, const uint64_t* row_sums, int depth, int width, int frac_bits,
                 int list_keys, bool forms, uint64_t* len);

}  // namespace ckpt
}  // namespace cms
