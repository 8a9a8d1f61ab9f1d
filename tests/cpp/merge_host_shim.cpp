// Host build of the merge's header-level compatibility checks
// (mahout_amd/csrc/cms_checkpoint.cpp) for tests/test_merge_host.py: each
// check returns NULL when the image may be merged, else the reason it is
// refused.
#include "../../mahout_amd/csrc/cms_checkpoint.h"

using namespace cms::ckpt;

extern "C" {

// live_ids / image_ids: NULL for "no ID section"
const char* host_check_merge_params(const void* hd, const int64_t* live_a, const int64_t* live_b, const int64_t* live_ids,
                                    const int64_t* image_ids) {
  return check_merge_params(*static_cast<const Header*>(hd), live_a, live_b, live_ids, image_ids);
}

const char* host_check_merge_masses(const void* hd, const void* dir, const uint64_t* live_mass, int64_t n) {
  return check_merge_masses(*static_cast<const Header*>(hd), static_cast<const DirEntry*>(dir), live_mass, n);
}

uint64_t host_merge_increment(const void* entry) { return merge_increment(*static_cast<const DirEntry*>(entry)); }

}  // extern "C"
