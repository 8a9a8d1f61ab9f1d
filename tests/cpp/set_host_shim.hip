// Host-side build of what the set similarity kernels share with the host
// (mahout_amd/csrc/cms_set.h) for the CPU test tests/test_set_host.py.
// k_set_tile and k_set_pairs call the same functions.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_set.h"

extern "C" {

int64_t sh_intersection_size(const int64_t* xk, int64_t nx, const int64_t* yk, int64_t ny) {
  return cms::set_intersection_size(xk, nx, yk, ny);
}

double sh_finish(int measure, int64_t k, int64_t n1, int64_t n2, int64_t num, int owner_side) {
  switch (measure) {
    case cms::kSetCooccurrence: return cms::set_finish<cms::kSetCooccurrence>(k, n1, n2, num, owner_side);
    case cms::kSetTanimoto: return cms::set_finish<cms::kSetTanimoto>(k, n1, n2, num, owner_side);
    case cms::kSetCityBlock: return cms::set_finish<cms::kSetCityBlock>(k, n1, n2, num, owner_side);
    default: return cms::set_finish<cms::kSetLogLikelihood>(k, n1, n2, num, owner_side);
  }
}

int sh_tile_for(int asked) { return cms::set_tile_for(asked); }

}  // extern "C"
