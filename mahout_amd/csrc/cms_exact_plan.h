// cms_exact_plan.h -- the host plan of one exact estimate batch
// (cms_exact.hip, k_exact_estimate): which candidate of which user goes to
// which slot of which workgroup.
//
// A user's candidate keys become the model's dense item indices (the position
// of the key among the attach's sorted unique keys).  A key the model does not
// hold has no data point with any neighbour: its estimate is NaN and it takes
// no slot.  The known candidates of a user are sorted by dense index and
// repeated ones folded, so a user's slots ascend strictly as a neighbour's
// item list does; pos_slot keeps, for every candidate position of the call,
// the slot whose estimate it receives, so repeated and unsorted keys come back
// in the caller's order.  A user's slots are cut into tiles of at most T: one
// workgroup each.
//
// Host only; tests/test_exact_recommend_host.py runs it through
// tests/cpp/exact_rec_host_shim.hip.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace cms {

// slots [lo, lo + len) of the batch's slot array belong to user `user`
struct ExactEstTile {
  int64_t user;
  int64_t lo;
  int32_t len;
  int32_t pad;
};

struct ExactEstPlan {
  std::vector<int32_t> slot_item;   // [S] dense item index, strictly ascending within a user
  std::vector<int64_t> pos_slot;    // [Q] candidate position -> slot; -1: the model lacks the key
  std::vector<ExactEstTile> tiles;  // in (user, slot) order
};

// ids: the model's item keys, sorted and unique.  User u's candidates are
// item_keys[item_offsets[u] .. item_offsets[u + 1]), u < n.  each_user(n, f)
// calls f(u) for every u < n, on as many threads as it likes: the users' key
// lookups and sorts are independent, the slots are numbered afterwards.
template <class EachUser>
inline void exact_plan_estimates(const std::vector<int64_t>& ids, int64_t n, const int64_t* item_offsets,
                                 const int64_t* item_keys, int T, ExactEstPlan& p, EachUser each_user) {
  p.slot_item.clear();
  p.tiles.clear();
  p.pos_slot.assign((size_t)item_offsets[n], -1);
  std::vector<std::vector<std::pair<int32_t, int64_t>>> per_user((size_t)n);  // (dense index, position), sorted
  each_user(n, [&](int64_t u) {
    auto& known = per_user[(size_t)u];
    for (int64_t i = item_offsets[u]; i < item_offsets[u + 1]; ++i) {
      const auto it = std::lower_bound(ids.begin(), ids.end(), item_keys[i]);
      if (it != ids.end() && *it == item_keys[i]) known.emplace_back((int32_t)(it - ids.begin()), i);
    }
    std::sort(known.begin(), known.end());
  });
  for (int64_t u = 0; u < n; ++u) {
    const auto& known = per_user[(size_t)u];
    const int64_t lo = (int64_t)p.slot_item.size();
    for (size_t k = 0; k < known.size(); ++k) {
      if (k == 0 || known[k].first != known[k - 1].first) p.slot_item.push_back(known[k].first);
      p.pos_slot[(size_t)known[k].second] = (int64_t)p.slot_item.size() - 1;
    }
    const int64_t hi = (int64_t)p.slot_item.size();
    for (int64_t t = lo; t < hi; t += T) p.tiles.push_back(ExactEstTile{u, t, (int32_t)std::min<int64_t>(T, hi - t), 0});
  }
}

// ... one user after another
inline void exact_plan_estimates(const std::vector<int64_t>& ids, int64_t n, const int64_t* item_offsets,
                                 const int64_t* item_keys, int T, ExactEstPlan& p) {
  exact_plan_estimates(ids, n, item_offsets, item_keys, T, p, [](int64_t users, auto f) {
    for (int64_t u = 0; u < users; ++u) f(u);
  });
}

}  // namespace cms
