// Host build of the compaction's target-form rule and of the image validation
// (mahout_amd/csrc/cms_checkpoint.cpp) for tests/test_compact_host.py.
#include "../../mahout_amd/csrc/cms_checkpoint.h"

using namespace cms::ckpt;

extern "C" {

// the form (kRow*) of a row and *len = its stored bytes; row_sums may be NULL
int host_compact_form(uint32_t cmax, uint64_t mass, const uint64_t* row_sums, int depth, int width, int frac_bits,
                      int list_keys, int forms, uint64_t* len) {
  return compact_form(cmax, mass, row_sums, depth, width, frac_bits, list_keys, forms != 0, len);
}

const char* host_check_header(const void* hd, uint64_t avail) { return check_header(*static_cast<const Header*>(hd), avail); }

const char* host_check_owner_ids(const int64_t* ids, int64_t n) { return check_owner_ids(ids, n); }

const char* host_check_directory(const void* hd, const void* dir, int64_t n) {
  return check_directory(*static_cast<const Header*>(hd), static_cast<const DirEntry*>(dir), n);
}

}  // extern "C"
