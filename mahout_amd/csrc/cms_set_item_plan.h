// cms_set_item_plan.h -- the host plan of one item-based estimate batch over
// the set similarities (cms_set_item.hip, k_set_item_estimate): which candidate
// of which user goes to which slot, and which (user, tile of T consecutive
// dense item indices) gets a workgroup.
//
// A user's candidate keys become the model's dense item indices, sorted and
// folded into slots exactly as exact_plan_estimates does it (pos_slot brings
// repeated, unsorted and unknown keys back in the caller's order; an unknown
// key takes no slot and reads NaN).  Unlike the exact estimate's tiles, which
// cut the slots, these tiles cut the item axis: tile t of a user covers the
// dense indices [t * T, (t + 1) * T), because the kernel counts into an LDS
// cell per item of the tile.  A user's slots ascend, so those that fall into
// one tile are a contiguous slot range; a tile without a slot is not emitted.
//
// The tile size and the LDS bytes per item of the two kinds are stated here
// for the host, the kernel and the CPU test alike.
//
// Host only; tests/test_set_item_host.py runs it through
// tests/cpp/set_item_host_shim.hip.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cms_exact_plan.h"

namespace cms {

// the values of CMS_ITEM_EST_* (mahout_cms.h)
enum SetItemKind : int32_t { kItemEstWeighted = 0, kItemEstBoolean = 1 };

// LDS per item of a tile: f64 total (weighted: and f64 preference), u32 cnt and
// an i32 (weighted: count; boolean: the found flag)
constexpr int set_item_cell_bytes(int kind) { return kind == kItemEstWeighted ? 24 : 16; }
// 64 KiB of boolean cells, 64,512 B of weighted ones: two workgroups per CU
constexpr int set_item_tile_default(int kind) { return kind == kItemEstWeighted ? 2688 : 4096; }
// CMS_SET_EST_TILE: any multiple of 64 up to the kind's default
inline int set_item_tile_for(int kind, int asked) {
  const int dflt = set_item_tile_default(kind);
  if (asked <= 0 || asked >= dflt) return dflt;
  return (asked + 63) / 64 * 64;
}

// slots [lo, lo + len) of the batch's slot array are user `user`'s candidates
// among the dense indices [tile * T, (tile + 1) * T)
struct SetItemTile {
  int64_t user;
  int64_t lo;
  int32_t len;
  int32_t tile;
};

struct SetItemPlan {
  std::vector<int32_t> slot_item;  // [S] dense item index, strictly ascending within a user
  std::vector<int64_t> pos_slot;   // [Q] candidate position -> slot; -1: the model lacks the key
  std::vector<SetItemTile> tiles;  // in (user, tile) order
};

template <class EachUser>
inline void set_item_plan(const std::vector<int64_t>& ids, int64_t n, const int64_t* cand_offsets,
                          const int64_t* cand_keys, int T, SetItemPlan& p, EachUser each_user) {
  ExactEstPlan e;  // the slots; its tiles (one per user: no cut) give every user's slot range
  exact_plan_estimates(ids, n, cand_offsets, cand_keys, INT32_MAX, e, each_user);
  p.slot_item.swap(e.slot_item);
  p.pos_slot.swap(e.pos_slot);
  p.tiles.clear();
  for (const ExactEstTile& u : e.tiles) {
    for (int64_t s = u.lo, hi = u.lo + u.len; s < hi;) {
      const int32_t tile = p.slot_item[(size_t)s] / T;
      int64_t t = s + 1;
      while (t < hi && p.slot_item[(size_t)t] / T == tile) ++t;
      p.tiles.push_back(SetItemTile{u.user, s, (int32_t)(t - s), tile});
      s = t;
    }
  }
}

// ... one user after another
inline void set_item_plan(const std::vector<int64_t>& ids, int64_t n, const int64_t* cand_offsets,
                          const int64_t* cand_keys, int T, SetItemPlan& p) {
  set_item_plan(ids, n, cand_offsets, cand_keys, T, p, [](int64_t users, auto f) {
    for (int64_t u = 0; u < users; ++u) f(u);
  });
}

// The preferred items' dense indices, in the caller's order.  Returns the
// position of the first key the model lacks, or -1 when it holds them all.
inline int64_t set_item_map_prefs(const std::vector<int64_t>& ids, int64_t m, const int64_t* pref_keys,
                                  std::vector<int32_t>& pref_idx) {
  pref_idx.resize((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const auto it = std::lower_bound(ids.begin(), ids.end(), pref_keys[i]);
    if (it == ids.end() || *it != pref_keys[i]) return i;
    pref_idx[(size_t)i] = (int32_t)(it - ids.begin());
  }
  return -1;
}

}  // namespace cms
