// Host-side build of k_common_item_estimate's shape (mahout_amd/csrc/cms_common_item.h)
// and of the attach rules its fallbacks hang on (cms_exact.h) for the CPU test
// tests/test_common_item_host.py.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_common_item.h"

extern "C" {

int cih_cell_bytes(int measure, int kind) { return cms::common_item_cell_bytes(measure, kind); }
int cih_tile_default(int measure, int kind) { return cms::common_item_tile_default(measure, kind); }
int cih_tile_for(int measure, int kind, int asked) { return cms::common_item_tile_for(measure, kind, asked); }

// the attach's shift of the values, and whether a list of them is common-eligible under it
int cih_shift(const float* vals, int64_t n) { return cms::exact_shift_for(vals, n); }
int cih_eligible(const float* vals, int64_t n, int s) {
  uint64_t U;
  double sum2, root;
  cms::exact_owner_sums(vals, 0, n, s, U, sum2, root);
  return U < cms::kCommonEligible;
}

}  // extern "C"
