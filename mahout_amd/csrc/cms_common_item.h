// cms_common_item.h -- the shape of k_common_item_estimate (cms_common_item.hip),
// stated once for the host, the kernel and the CPU test
// (tests/test_common_item_host.py through tests/cpp/common_item_host_shim.hip).
//
// LDS per item of a tile, as separate arrays in the order of the types'
// alignment: the measure's u64 wide sums (k_common_tile's: Euclidean the
// squared differences; uncentered S_xy, S_xx, S_yy; Pearson adds S_x, S_y), f64
// total, f64 preference (weighted only), u32 cnt and an i32 (weighted: count;
// boolean: the found flag).
#pragma once
#include "cms_common.h"

namespace cms {

// (kind: CMS_ITEM_EST_*, 0 weighted, 1 boolean -- SetItemKind of cms_set_item_plan.h)
CMS_HD constexpr int common_item_wide(int measure) {
  return measure == kCommonEuclidean ? 1 : measure == kCommonUncentered ? 3 : 5;
}
// weighted 32, 48, 64 B for Euclidean, uncentered, Pearson; boolean 24, 40, 56 B
CMS_HD constexpr int common_item_cell_bytes(int measure, int kind) { return 8 * common_item_wide(measure) + (kind == 0 ? 24 : 16); }
// Items per workgroup: the largest multiple of 64 whose cells fit 64 KiB, so two
// workgroups share a CU's 160 KiB (weighted 2048, 1344, 1024; boolean 2688,
// 1600, 1152).  CMS_COMMON_EST_TILE overrides it with any multiple of 64 up to
// the default.
CMS_HD constexpr int common_item_tile_default(int measure, int kind) {
  return 65536 / common_item_cell_bytes(measure, kind) / 64 * 64;
}
CMS_HD int common_item_tile_for(int measure, int kind, int asked) {
  const int dflt = common_item_tile_default(measure, kind);
  if (asked <= 0) return dflt;
  const int t = (asked + 63) / 64 * 64;
  return t > dflt ? dflt : t;
}

}  // namespace cms
