// Host-side build of what k_nb_estimate (mahout_amd/csrc/cms_neighbor.hip)
// shares with the host, for tests/test_neighbor_host.py: the two estimate
// structs of cms_ref.h fed one data point at a time, sequentially and as the
// kernel's fold feeds them -- the set bits of a chunk's mask in ascending order.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_neighbor.h"
#include "../../mahout_amd/csrc/cms_ref.h"

template <class Sum, class Add>
static Sum fold(const double* sims, int64_t m, int by_mask, Add add) {
  Sum e;
  if (!by_mask) {
    for (int64_t i = 0; i < m; ++i) add(e, i);
    return e;
  }
  constexpr int G = 16;  // chunks of G neighbours, every one holding the slot
  for (int64_t c = 0; c < m; c += G) {
    unsigned bits = m - c >= G ? 0xFFFFu : (1u << (m - c)) - 1u;
    for (; bits; bits &= bits - 1) add(e, c + __builtin_ctz(bits));
  }
  return e;
}

extern "C" {

float nb_generic(const double* sims, const float* prefs, int64_t m, int by_mask, int use_capper, float lo, float hi) {
  return fold<cms::ItemEstimate>(sims, m, by_mask, [&](cms::ItemEstimate& e, int64_t i) { e.add(sims + i, prefs + i, 1); })
      .finish(use_capper, lo, hi);
}

float nb_boolean(const double* sims, int64_t m, int by_mask) {
  return fold<cms::BoolUserEstimate>(sims, m, by_mask, [&](cms::BoolUserEstimate& e, int64_t i) { e.add(sims + i, 1); })
      .finish();
}

}  // extern "C"
