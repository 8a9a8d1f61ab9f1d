// cms_neighbor.h -- the shape of the user-based recommenders' estimate kernel
// over a chosen similarity (cms_neighbor.hip, k_nb_estimate<KIND>): the kinds,
// the chunk and tile of each kind, the LDS layout and the kernel's argument.
//
// The kind belongs to the recommender class, the similarity is any measure of
// the co-rated or the set family:
//   generic  GenericUserBasedRecommender.doEstimatePreference, sim == null
//            (:134-184): ItemEstimate of cms_ref.h, one data point per add;
//   boolean  GenericBooleanPrefUserBasedRecommender.doEstimatePreference
//            (:45-61): BoolUserEstimate of cms_ref.h.
//
// LDS of one workgroup, on the 16-byte dynamic base, every array aligned to
// its type (G and T are multiples of 2 and 64):
//   f64 sims[2][G], i64 lo[2][G], i64 hi[2][G]   the chunk's similarities and list
//                                                ranges, double-buffered   48 G bytes
//   i32 slot[T]                                  the tile's dense item indices
//   u32 mask[T]                                  bit g: chunk neighbour g holds the slot
//   f32 pref[G][T]                               generic only: that neighbour's value
// The sums live in registers: thread t owns the slots t, t + 256, ... and
// kNbSlotsPerThread<KIND> of them cover the kind's default tile.
//   generic  G = 16: 768 + 72 T bytes, T = 896: 65,280 bytes
//   boolean  G = 32: 1,536 + 8 T bytes, T = 4096: 34,304 bytes
// so two (generic) or four (boolean) workgroups share a CU's 160 KiB.
// CMS_NB_EST_TILE lowers T to any multiple of 64.
#pragma once
#include <stdint.h>

#include "cms_exact.h"
#include "cms_exact_plan.h"

namespace cms {

// the values of CMS_NB_* and CMS_FAMILY_* (mahout_cms.h)
enum NbKind : int32_t { kNbGeneric = 0, kNbBoolean = 1 };
enum NbFamily : int32_t { kFamilyCommon = 0, kFamilySet = 1 };

constexpr int kNbThreads = 256;  // four waves
CMS_HD constexpr int nb_chunk(int kind) { return kind == kNbGeneric ? 16 : 32; }  // G: at most 32, a mask word's bits
CMS_HD constexpr int nb_tile_default(int kind) { return kind == kNbGeneric ? 896 : 4096; }
CMS_HD constexpr int nb_slots_per_thread(int kind) { return (nb_tile_default(kind) + kNbThreads - 1) / kNbThreads; }
CMS_HD constexpr int nb_lds_bytes(int kind, int T) {
  return 48 * nb_chunk(kind) + (8 + (kind == kNbGeneric ? 4 * nb_chunk(kind) : 0)) * T;
}
static_assert(nb_lds_bytes(kNbGeneric, nb_tile_default(kNbGeneric)) <= 65536 &&
                  nb_lds_bytes(kNbBoolean, nb_tile_default(kNbBoolean)) <= 65536,
              "a workgroup's LDS stays at or under 64 KiB");
CMS_HD int nb_tile_for(int kind, int asked) {
  const int dflt = nb_tile_default(kind);
  if (asked <= 0) return dflt;
  const int t = (asked + 63) / 64 * 64;
  return t > dflt ? dflt : t;
}

// One batch: the users, their neighbourhoods with the similarities of the
// family's pair kernel, and the plan of cms_exact_plan.h.
struct NbEstArgs {
  const int64_t* urow;      // [n] the users' owner rows
  const int64_t* nb_off;    // [n + 1] user u's neighbours: nb_row / sims [nb_off[u], nb_off[u + 1])
  const int64_t* nb_row;    // the neighbours' owner rows, in the caller's order
  const double* sims;       // userSimilarity(user, neighbour) under the chosen measure
  const ExactEstTile* tiles;
  const int32_t* slot_item;  // [S]
  float* est;                // [S]
  int32_t T, use_capper;
  float lo, hi;
};

}  // namespace cms
