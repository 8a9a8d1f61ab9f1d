// Host build of the subtraction's mass rule
// (mahout_amd/csrc/cms_checkpoint.cpp) for tests/test_subtract_host.py: NULL
// when no row's mass would fall below zero, else the reason the image is
// refused.
#include "../../mahout_amd/csrc/cms_checkpoint.h"

using namespace cms::ckpt;

extern "C" {

// live_mass: NULL for an empty handle
const char* host_check_subtract_masses(const void* hd, const void* dir, const uint64_t* live_mass, int64_t n) {
  return check_subtract_masses(*static_cast<const Header*>(hd), static_cast<const DirEntry*>(dir), live_mass, n);
}

}  // extern "C"
