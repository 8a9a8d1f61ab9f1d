// Host-side build of what the anonymous-profile kernels share with the host
// (mahout_amd/csrc/cms_anon.h) for the CPU test tests/test_anonymous_host.py:
// the batch validation, the sketch of one profile and the non-zero bucket
// list.  k_anon_sketch, k_anon_rows and the C entry points call the same
// functions.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_anon.h"

static cms::HashParams params(int depth, int width, int frac_bits, const int64_t* a, const int64_t* b) {
  cms::HashParams hp{};
  for (int i = 0; i < depth; ++i) {
    hp.ap[i] = cms::reduce_key(a[i]);
    hp.bp[i] = cms::reduce_key(b[i]);
  }
  hp.width = (uint32_t)width;
  hp.depth = depth;
  hp.frac_bits = frac_bits;
  cms::hash_finish(hp);
  return hp;
}

extern "C" {

// status of a batch (0 ok, 1 offsets, 5 value, 6 overflow: the ABI's codes)
int ah_validate(int64_t nq, const int64_t* offsets, const float* vals, int frac_bits) {
  return cms::anon_validate_batch(nq, offsets, vals, frac_bits);
}

// sk [depth][width] (zeroed by the caller) += the sketch of the profile (keys, vals or null)[0, m)
void ah_sketch(int depth, int width, int frac_bits, const int64_t* a, const int64_t* b, const int64_t* keys,
               const float* vals, int64_t m, uint32_t* sk) {
  const cms::HashParams hp = params(depth, width, frac_bits, a, b);
  cms::anon_sketch(hp, keys, vals, 0, m, sk);
}

// the non-zero buckets of one sketch row [width] -> buckets / counts; returns how many
uint32_t ah_nonzero(const uint32_t* row, int width, uint32_t* buckets, uint32_t* counts) {
  cms::AnonEntry* tmp = new cms::AnonEntry[width > 0 ? width : 1];
  const uint32_t n = cms::anon_nonzero(row, 0u, (uint32_t)width, tmp);
  for (uint32_t i = 0; i < n; ++i) {
    buckets[i] = tmp[i].bucket;
    counts[i] = tmp[i].count;
  }
  delete[] tmp;
  return n;
}

int ah_batch_size(int64_t width, int elem_bytes) { return cms::anon_batch_size(width, elem_bytes); }
int ah_elem_bytes(uint32_t max_counter) { return cms::anon_elem_bytes(max_counter); }
int ah_use_bucket_lists(int64_t batch_nnz, int64_t width) { return cms::anon_use_bucket_lists(batch_nnz, width) ? 1 : 0; }

}  // extern "C"
