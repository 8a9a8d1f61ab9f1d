// Host build of the item-based recommender's host-side pieces for the CPU
// test tests/test_item_host.py: the candidate strategies of
// mahout_amd/csrc/cms_recommend.cpp (ItemCandidates: FastIDSet order over the
// transposed CSR) and item_estimate_one of mahout_amd/csrc/cms_ref.h, the
// function the kernel's estimate epilogue runs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../mahout_amd/csrc/cms_internal.h"
#include "../../mahout_amd/csrc/cms_ref.h"

extern "C" {

// candidates of the user at model row `row`; returns their count (out holds up to cap)
int64_t ih_candidates(int64_t n_users, const int64_t* pref_offsets, const int64_t* pref_items, int64_t row,
                      int strategy, int include_known, int64_t* out, int64_t cap) {
  cms::ItemCandidates model(n_users, pref_offsets, pref_items);
  std::vector<int64_t> c;
  model.candidates(pref_items + pref_offsets[row], pref_offsets[row + 1] - pref_offsets[row], strategy,
                   include_known != 0, c);
  for (size_t i = 0; i < c.size() && (int64_t)i < cap; ++i) out[i] = c[i];
  return (int64_t)c.size();
}

// getPreferencesForItem(item): the raters' model rows
int64_t ih_raters(int64_t n_users, const int64_t* pref_offsets, const int64_t* pref_items, int64_t item, int64_t* out,
                  int64_t cap) {
  cms::ItemCandidates model(n_users, pref_offsets, pref_items);
  std::vector<int64_t> r;
  model.raters(item, r);
  for (size_t i = 0; i < r.size() && (int64_t)i < cap; ++i) out[i] = r[i];
  return (int64_t)r.size();
}

float ih_item_estimate(const double* sims, const float* prefs, int64_t m, int use_capper, float lo, float hi) {
  return cms::item_estimate_one(sims, prefs, m, use_capper, lo, hi);
}

// the same preferences fed in pieces of `piece`, as the kernel's right tiles feed them
float ih_item_estimate_pieces(const double* sims, const float* prefs, int64_t m, int64_t piece, int use_capper,
                              float lo, float hi) {
  cms::ItemEstimate e;
  for (int64_t j = 0; j < m; j += piece) e.add(sims + j, prefs + j, m - j < piece ? m - j : piece);
  return e.finish(use_capper, lo, hi);
}

}  // extern "C"
