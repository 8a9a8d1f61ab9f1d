// Host-side build of the branch-free row hash (RowHash, mahout_amd/csrc/
// cms_hash.h) for the CPU test tests/test_hash_rows_host.py; k_build_slices
// and the streamed k_build_mid include the same header.
#include <hip/hip_runtime.h>
#include "../../mahout_amd/csrc/cms_hash.h"

namespace {

cms::HashParams params(const int64_t* a, const int64_t* b, int depth, int width) {
  cms::HashParams hp{};
  for (int i = 0; i < depth; ++i) {
    hp.ap[i] = cms::reduce_key(a[i]);
    hp.bp[i] = cms::reduce_key(b[i]);
  }
  hp.width = (uint32_t)width;
  hp.depth = depth;
  cms::hash_finish(hp);
  return hp;
}

// The kernels' use of the helper: all D rows at once, then -- one decision per
// key -- the rows again through bucket().  redo[i]: whether key i took it.
template <int D>
void rows(const cms::HashParams& hp, const int64_t* keys, int64_t n, int32_t* out, uint8_t* redo) {
  const cms::RowHash<D> rh(hp);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t kp = cms::reduce_key(keys[i]);
    uint32_t bk[D];
    const bool again = rh.rows(kp, bk);
    if (again)
      for (int r = 0; r < D; ++r) bk[r] = cms::bucket(hp, r, kp);
    for (int r = 0; r < D; ++r) out[i * D + r] = (int32_t)bk[r];
    if (redo) redo[i] = again ? 1 : 0;
  }
}

// The keys of [k0, k1) the helper sends to the redo, up to cap of them.
template <int D>
int64_t scan(const cms::HashParams& hp, int64_t k0, int64_t k1, int64_t* out, int64_t cap) {
  const cms::RowHash<D> rh(hp);
  int64_t n = 0;
  for (int64_t k = k0; k < k1 && n < cap; ++k) {
    uint32_t bk[D];
    if (rh.rows(cms::reduce_key(k), bk)) out[n++] = k;
  }
  return n;
}

}  // namespace

// depth 4 or 5, a power-of-two width up to 2^24 (hp.fastq); returns 0, or -1 for another shape
extern "C" int host_row_buckets(const int64_t* a, const int64_t* b, int depth, int width, const int64_t* keys,
                                int64_t n, int32_t* out, uint8_t* redo) {
  const cms::HashParams hp = params(a, b, depth, width);
  if (!hp.fastq || (depth != 4 && depth != 5)) return -1;
  if (depth == 4) rows<4>(hp, keys, n, out, redo);
  else rows<5>(hp, keys, n, out, redo);
  return 0;
}

extern "C" int64_t host_redo_keys(const int64_t* a, const int64_t* b, int depth, int width, int64_t k0, int64_t k1,
                                  int64_t* out, int64_t cap) {
  const cms::HashParams hp = params(a, b, depth, width);
  if (!hp.fastq || (depth != 4 && depth != 5)) return -1;
  return depth == 4 ? scan<4>(hp, k0, k1, out, cap) : scan<5>(hp, k0, k1, out, cap);
}
