// Host-side build of what the exact estimate path shares with the host for the
// CPU test tests/test_exact_recommend_host.py: the plan of an estimate batch
// (mahout_amd/csrc/cms_exact_plan.h, what exact_estimate_batch uploads), the
// tile rule (cms_exact.h) and the estimate arithmetic as k_exact_estimate
// feeds it (ItemEstimate of cms_ref.h, one data point per add).
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_exact.h"
#include "../../mahout_amd/csrc/cms_exact_plan.h"
#include "../../mahout_amd/csrc/cms_ref.h"

extern "C" {

int er_tile_for(int asked) { return cms::exact_est_tile_for(asked); }

// The plan of n users' candidates over the model's nitems sorted unique keys.
// pos_slot [Q] is always written; slot_item (room for Q) and the tiles' three
// arrays (room for tile_cap) are; *slots and the return value are the counts
// (nothing past a capacity is written).
int64_t er_plan(const int64_t* ids, int64_t nitems, int64_t n, const int64_t* item_offsets, const int64_t* item_keys,
                int T, int64_t* pos_slot, int32_t* slot_item, int64_t* slots, int64_t* tile_user, int64_t* tile_lo,
                int32_t* tile_len, int64_t tile_cap) {
  cms::ExactEstPlan p;
  cms::exact_plan_estimates(std::vector<int64_t>(ids, ids + nitems), n, item_offsets, item_keys, T, p);
  for (size_t i = 0; i < p.pos_slot.size(); ++i) pos_slot[i] = p.pos_slot[i];
  for (size_t i = 0; i < p.slot_item.size(); ++i) slot_item[i] = p.slot_item[i];
  *slots = (int64_t)p.slot_item.size();
  for (size_t t = 0; t < p.tiles.size() && (int64_t)t < tile_cap; ++t) {
    tile_user[t] = p.tiles[t].user;
    tile_lo[t] = p.tiles[t].lo;
    tile_len[t] = p.tiles[t].len;
  }
  return (int64_t)p.tiles.size();
}

// One slot's estimate from its m data points in neighbourhood order
float er_estimate(const double* sims, const float* prefs, int64_t m, int use_capper, float lo, float hi) {
  cms::ItemEstimate e;
  for (int64_t i = 0; i < m; ++i) e.add(sims + i, prefs + i, 1);
  return e.finish(use_capper, lo, hi);
}

}  // extern "C"
