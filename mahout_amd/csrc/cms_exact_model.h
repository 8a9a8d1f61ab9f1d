// cms_exact_model.h -- the attached DataModel of a handle (exact_attach,
// cms_exact.hip), as the files that score over it see it: cms_exact.hip (the
// full-norm cosine), cms_common.hip (the co-rated similarities) and
// cms_set.hip (the set similarities), with the one view of a model's face
// (CommonSide) and the pair kernels' argument that the last two share.
#pragma once
#include <vector>

#include "cms_exact.h"
#include "cms_internal.h"
#include "cms_set_item_plan.h"

namespace cms {

struct ExactModel {
  int64_t n = 0, npairs = 0, nitems = 0;
  int shift = kExactNoShift;
  std::vector<uint8_t> h_seq;  // [n] 1: not integer-eligible
  std::vector<int64_t> ids;    // [nitems] getItemIDs(): the keys, sorted and unique (key -> dense item index)
  std::vector<int64_t> h_off, h_keys;  // the attached CSR's offsets and keys: the DataModel of the recommend call
  std::vector<float> h_vals;           // ... and its values, copied back from val by the first call that reads them (exact_host_vals)
  int64_t n_seq = 0;
  DevBuf off, item, val, unit;  // owner side: [n + 1] i64, [np] dense item (i32), float, unit (i32)
  DevBuf ioff, irow, iunit;     // item side: [nitems + 1] i64, [np] owner row ascending (i32), unit (i32)
  DevBuf U, root;               // [n] saturating sum of squared units (u64), Math.sqrt(sumX2) (f64)
  DevBuf seq_rows;              // [n_seq] the non-eligible rows (i64)
  DevBuf q1, q2, sel, out;      // a call's rows, selected queries and results
  DevBuf e_urow, e_nboff, e_slot, e_tiles, e_est;  // an estimate batch: users' rows, neighbour offsets, plan, estimates
  DevBuf i_poff, i_pidx, i_pval;  // an item-based estimate batch (cms_set_item.hip): preference offsets, dense items, values
  // the co-rated similarities (cms_common.hip): the floats in posting-list
  // order, the items' U over their posting lists, the item keys on the device
  // (the top-k's IDs on the key side), and per side the lists that are not
  // common-eligible (U >= 2^51): host flags and the device list
  DevBuf ival, iU, d_ids;       // [np] float, [nitems] u64, [nitems] i64
  std::vector<uint8_t> h_cseq[2];  // [n], [nitems]
  DevBuf cseq[2];                  // i64 indices, ascending
  int64_t n_cseq[2] = {0, 0};
  // the dense route of the set similarities (cms_set_bits.hip): per side (owner, key) the bit matrix, built by the
  // first call that needs it and gone with the model.  state 0: not tried, 1: built, -1: no room (budget or memory)
  DevBuf bits[2];
  int bits_state[2] = {0, 0};
};

// (the host array must stay alive until the stream is synchronised)
template <class T>
inline int upload(cms_handle* h, DevBuf& b, const T* v, size_t count) {
  CMS_HIP(b.ensure(sizeof(T) * count));
  if (count > 0) CMS_HIP(hipMemcpyAsync(b.ptr, v, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
  return CMS_OK;
}
template <class T>
inline int upload(cms_handle* h, DevBuf& b, const std::vector<T>& v) {
  return upload(h, b, v.data(), v.size());
}

// One face of the model: n lists of (cross index ascending, unit, float), and
// per cross index the lists that hold it (list index ascending, unit).
struct CommonSide {
  const int64_t* off;     // [n + 1]
  const int32_t* key;     // the lists' cross indices
  const int32_t* unit;
  const float* val;
  const int64_t* xoff;    // the cross lists
  const int32_t* xlist;
  const int32_t* xunit;
  const uint64_t* U;      // [n] saturating sum of squared units
  int64_t n;              // lists: the candidates, and the slab's columns
  int64_t num;            // normalizeWeightResult's num: the other face's count
  int32_t shift, weighted;
};

inline CommonSide common_side(const cms_handle* h, int32_t side) {
  const ExactModel& m = *h->exact;
  if (side == CMS_SIDE_OWNER)
    return CommonSide{m.off.as<int64_t>(),  m.item.as<int32_t>(), m.unit.as<int32_t>(),  m.val.as<float>(),
                      m.ioff.as<int64_t>(), m.irow.as<int32_t>(), m.iunit.as<int32_t>(), m.U.as<uint64_t>(),
                      m.n,                  m.nitems,             m.shift,               (int32_t)h->p.weighting};
  return CommonSide{m.ioff.as<int64_t>(), m.irow.as<int32_t>(), m.iunit.as<int32_t>(), m.ival.as<float>(),
                    m.off.as<int64_t>(),  m.item.as<int32_t>(), m.unit.as<int32_t>(),  m.iU.as<uint64_t>(),
                    m.nitems,             m.n,                  m.shift,               (int32_t)h->p.weighting};
}

// The pair kernels' argument (k_common_pairs, k_set_pairs).
// elementwise: out[t] = similarity(i1[t], i2[t]), t < n1.
// cross: query i (sel[i'] when sel is given, i' < n1) against column j < n2
// (list i2[j]; i2 null: list j) into out[i * ld + j], or, scattered, into
// out[i * ld + i2[j]] (the slab's column of that list).
struct CommonPairArgs {
  const int64_t* i1;
  const int64_t* i2;
  const int64_t* sel;
  int64_t n1, n2;
  int32_t cross, scatter;
  double* out;
  int64_t ld;
};

// Device arrays in, device results out, queued on the handle's stream under the timing scope `scope`: the launch
// inside common_pair_call (cms_common.hip) and set_pair_call (cms_set.hip), for a caller whose pairs and results
// stay on the device (cms_neighbor.hip).  measure and side are validated by the caller.
int common_pairs_device(cms_handle* h, int32_t measure, int32_t side, const CommonPairArgs& g, const char* scope);
int set_pairs_device(cms_handle* h, int32_t measure, int32_t side, const CommonPairArgs& g, const char* scope);

// The item-based estimate kernels' argument (k_set_item_estimate, k_common_item_estimate): one batch's preferences
// and the plan of cms_set_item_plan.h.
struct SetItemArgs {
  const int64_t* pref_off;   // [n + 1] user u's preferred items: pref_idx / pref_val [pref_off[u], pref_off[u + 1])
  const int32_t* pref_idx;   // dense item indices, in preference order
  const float* pref_val;     // (weighted only)
  const SetItemTile* tiles;
  const int32_t* slot_item;  // [S]
  float* est;                // [S]
  int32_t T, use_capper;
  float lo, hi;
};

// The host body of one item-based estimate batch (cms_set_item.hip), shaped as set_item_estimate_batch: `launch`
// runs the estimating kernel of (measure, kind) over the plan's ntiles tiles of T items on the handle's stream.
using ItemEstLaunch = int (*)(cms_handle* h, int32_t measure, int32_t kind, const CommonSide& v, const SetItemArgs& g,
                              int64_t ntiles);
int item_estimate_batch(cms_handle* h, ItemEstLaunch launch, int T, int32_t measure, int32_t kind, int64_t n,
                        const int64_t* pref_offsets, const int64_t* pref_keys, const float* pref_vals,
                        const int64_t* cand_offsets, const int64_t* cand_keys, int32_t use_capper, float cap_min,
                        float cap_max, float* out);

}  // namespace cms
