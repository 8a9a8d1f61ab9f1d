// cms_anon.h -- what the host and the device share of the anonymous-profile
// queries (cms_anonymous.hip): the validation of a profile's values, the
// sketch of one profile, and the list of a sketch row's non-zero buckets.
//
// PlusAnonymousUserDataModel (T/impl/model/PlusAnonymousUserDataModel.java:74-137)
// serves a user the model does not hold; CosineCM sketches that user's
// preferences with exportProfile (CosineCM.java:41-58): update(key, value) per
// preference, in order, duplicate keys adding.  Everything here is a pure
// __host__ __device__ function, written as cms_ref.h is: the kernels call
// these and hold no second copy, and tests/test_anonymous_host.py runs them on
// the CPU against the oracle (tests/cpp/anonymous_host_shim.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#include "cms_hash.h"

namespace cms {

// status of a profile batch's validation (the ABI's codes, mahout_cms.h)
enum : int { kAnonOk = 0, kAnonParam = 1, kAnonValue = 5, kAnonOverflow = 6 };

// The increment of one preference value in counter units, as a host ingest
// takes it (load_inc, cms_device.h): val * 2^fb must be a non-negative
// integer below 2^32.  vals null: every value is 1.0.
CMS_HD bool anon_inc(const float* vals, int64_t i, int fb, uint32_t& inc) {
  if (vals == nullptr) {
    inc = 1u << fb;
    return true;
  }
  const float v = ldexpf(vals[i], fb);
  if (!(v >= 0.0f) || v != floorf(v) || v >= 4294967296.0f) {
    inc = 0u;
    return false;
  }
  inc = (uint32_t)v;
  return true;
}

// One profile, pairs [lo, hi): every value valid (kAnonValue otherwise) and the
// total mass in counter units below 2^32 (kAnonOverflow) -- no counter of the
// profile's sketch can then wrap.
CMS_HD int anon_validate_profile(const float* vals, int64_t lo, int64_t hi, int fb) {
  uint64_t mass = 0;
  for (int64_t i = lo; i < hi; ++i) {
    uint32_t inc;
    if (!anon_inc(vals, i, fb, inc)) return kAnonValue;
    mass += inc;  // < 2^32 after every step: no wrap of the u64
    if (mass >= (1ULL << 32)) return kAnonOverflow;
  }
  return kAnonOk;
}

// A batch of nq profiles in CSR form: offsets start at 0 and never decrease
// (kAnonParam), then every profile as above.  The first failure decides.
CMS_HD int anon_validate_batch(int64_t nq, const int64_t* offsets, const float* vals, int fb) {
  if (nq < 0 || (nq > 0 && offsets[0] != 0)) return kAnonParam;
  for (int64_t q = 0; q < nq; ++q)
    if (offsets[q + 1] < offsets[q]) return kAnonParam;
  for (int64_t q = 0; q < nq; ++q) {
    const int rc = anon_validate_profile(vals, offsets[q], offsets[q + 1], fb);
    if (rc != kAnonOk) return rc;
  }
  return kAnonOk;
}

// update(key, inc) of one validated pair: add(i, j, inc) for the bucket j of
// every sketch row i.  The kernel adds atomically, the host plainly.
template <class F>
CMS_HD void anon_update(const HashParams& hp, int64_t key, uint32_t inc, F&& add) {
  const uint64_t kp = reduce_key(key);
  for (int i = 0; i < hp.depth; ++i) add(i, bucket(hp, i, kp), inc);
}

// The sketch [d][w] of one validated profile (pairs [lo, hi)), added into sk
// (zeros before the first pair).
CMS_HD void anon_sketch(const HashParams& hp, const int64_t* keys, const float* vals, int64_t lo, int64_t hi,
                        uint32_t* sk) {
  for (int64_t t = lo; t < hi; ++t) {
    uint32_t inc;
    (void)anon_inc(vals, t, hp.frac_bits, inc);
    anon_update(hp, keys[t], inc, [&](int i, uint32_t j, uint32_t v) { sk[(int64_t)i * hp.width + j] += v; });
  }
}

// One non-zero bucket of a sketch row: its index and its counter.
struct AnonEntry {
  uint32_t bucket, count;
};

// The non-zero buckets of buckets [j0, j1) of one sketch row, ascending, at
// out[0 ..); returns how many.  The whole row is (0, w); the kernel's waves
// call it for the single bucket of a lane and place the entry by a ballot.
CMS_HD uint32_t anon_nonzero(const uint32_t* row, uint32_t j0, uint32_t j1, AnonEntry* out) {
  uint32_t n = 0;
  for (uint32_t j = j0; j < j1; ++j)
    if (row[j] != 0u) out[n++] = AnonEntry{j, row[j]};
  return n;
}

// ---- the similarity kernel's batch shape ----
// A workgroup keeps sketch row i of B profiles in LDS, bucket-major
// ([w][B] counters of elem_bytes each), within kAnonLds of the CU's 160 KiB:
// B is the largest power of two up to kAnonMaxB whose image fits, 0 when not
// even one profile's row does (such a width takes the bucket-list path only).
constexpr int64_t kAnonLds = 128 * 1024;
constexpr int kAnonMaxB = 8;  // 8 u64 partial dots per lane keep the kernel at 128 registers (16 waves per workgroup)
CMS_HD int anon_batch_size(int64_t w, int elem_bytes) {
  int b = kAnonMaxB;
  while (b > 0 && w * elem_bytes * b > kAnonLds) b >>= 1;
  return b;
}
// u16 elements hold a batch whose largest counter is below 2^16
CMS_HD int anon_elem_bytes(uint32_t max_counter) { return max_counter < 65536u ? 2 : 4; }

// Dense owner rows: read the owner's counters at the batch's non-zero buckets
// (instead of streaming the row against the LDS image) when the batch's
// bucket lists -- the sum over its profiles of the longest list of each --
// are at most an eighth of the row.
CMS_HD bool anon_use_bucket_lists(int64_t batch_nnz, int64_t w) { return batch_nnz * 8 <= w; }

}  // namespace cms
