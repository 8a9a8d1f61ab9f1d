// Host-side build of what k_set_item_estimate shares with the host for the CPU
// test tests/test_set_item_host.py: the batch plan
// (mahout_amd/csrc/cms_set_item_plan.h) and the two estimates of
// mahout_amd/csrc/cms_ref.h, fed one data point per add as the kernel feeds them.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_ref.h"
#include "../../mahout_amd/csrc/cms_set_item_plan.h"

extern "C" {

// slot_item [Q], pos_slot [Q], tiles [Q][4] (user, lo, len, tile); counts[0] = slots, counts[1] = tiles
void sih_plan(const int64_t* ids, int64_t nids, int64_t n, const int64_t* cand_off, const int64_t* cand_keys, int T,
              int32_t* slot_item, int64_t* pos_slot, int64_t* tiles, int64_t* counts) {
  cms::SetItemPlan p;
  cms::set_item_plan(std::vector<int64_t>(ids, ids + nids), n, cand_off, cand_keys, T, p);
  std::copy(p.slot_item.begin(), p.slot_item.end(), slot_item);
  std::copy(p.pos_slot.begin(), p.pos_slot.end(), pos_slot);
  for (size_t t = 0; t < p.tiles.size(); ++t) {
    const cms::SetItemTile& x = p.tiles[t];
    const int64_t row[4] = {x.user, x.lo, x.len, x.tile};
    std::copy(row, row + 4, tiles + 4 * t);
  }
  counts[0] = (int64_t)p.slot_item.size();
  counts[1] = (int64_t)p.tiles.size();
}

float sih_estimate(int kind, const double* sims, const float* prefs, int64_t m, int use_capper, float lo, float hi) {
  cms::ItemEstimate w;
  cms::BoolItemEstimate b;
  for (int64_t i = 0; i < m; ++i) {
    if (kind == cms::kItemEstWeighted) w.add(sims + i, prefs + i, 1);
    else b.add(sims + i, 1);
  }
  return kind == cms::kItemEstWeighted ? w.finish(use_capper, lo, hi) : b.finish();
}

}  // extern "C"
