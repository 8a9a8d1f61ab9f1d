// cms_retract.h -- what the host and the device share of the pair-by-pair
// retraction (cms_retract.hip): the validation of a batch's rows and values,
// and the step every run of one owner's pairs goes through for each sketch
// row -- sum the decrements per bucket, compare each sum with the live counter.
//
// The reference expresses a removed or changed preference in FileDataModel's
// update files (T/impl/model/file/FileDataModel.java:493-527) and rebuilds
// every sketch; here DoubleCountMinSketch.update(key, -val) is applied to the
// live counters instead, and only when the whole batch can be taken out:
// the comparison is on the SUM of a batch's decrements per counter -- two
// copies of a pair, or two keys that share a bucket of one sketch row, must
// fit the counter together.  Everything here is a pure __host__ __device__
// function, written as cms_anon.h is: the kernels call these and hold no
// second copy, and tests/test_retract_host.py runs them on the CPU
// (tests/cpp/retract_host_shim.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#include "cms_hash.h"

namespace cms {

// error bits of a batch's validation: the values of kFlagBadRow / kFlagBadValue
// (cms_internal.h), so the ingest's flag word reports them with the ingest's codes
enum : uint32_t { kRetractBadRow = 1u << 0, kRetractBadValue = 1u << 1 };

// An owner's pairs up to this many are one wave's run (k_retract_wave: a lane
// per pair, equal buckets combined across the lanes); longer runs take a
// workgroup and an LDS image of decrements (k_retract_image).
constexpr int kRetractWaveRun = 64;

// The decrement of one value in counter units, exactly as a host ingest takes
// an increment (load_inc, cms_device.h): val * 2^fb must be a non-negative
// integer below 2^32.  vals null: every value is 1.0.
CMS_HD bool retract_dec(const float* vals, int64_t i, int fb, uint32_t& dec) {
  if (vals == nullptr) {
    dec = 1u << fb;
    return true;
  }
  const float v = ldexpf(vals[i], fb);
  if (!(v >= 0.0f) || v != floorf(v) || v >= 4294967296.0f) {
    dec = 0u;
    return false;
  }
  dec = (uint32_t)v;
  return true;
}

// Pair i of a batch: its owner row inside [0, nrows) (rows null: not checked,
// the ID lookup has flagged unknown owners) and its value a valid decrement.
CMS_HD uint32_t retract_validate_pair(const int64_t* rows, const float* vals, int64_t i, int64_t nrows, int fb) {
  uint32_t f = 0;
  if (rows && (rows[i] < 0 || rows[i] >= nrows)) f |= kRetractBadRow;
  uint32_t dec;
  if (!retract_dec(vals, i, fb, dec)) f |= kRetractBadValue;
  return f;
}

// Member t of a run of cnt pairs of one owner, in one sketch row: sum = the
// decrements of every member whose bucket equals t's; returns whether t is the
// first member with that bucket (the leader, which alone compares or writes).
// bucket_at(s) / dec_at(s) read member s -- array reads on the host, wave
// shuffles on the device, where every lane of the wave calls this together
// (cnt is uniform) and both reads happen outside any divergent branch.
template <class BucketAt, class DecAt>
CMS_HD bool retract_combine(int t, uint32_t my_bucket, int cnt, BucketAt&& bucket_at, DecAt&& dec_at, uint64_t& sum) {
  bool leader = true;
  uint64_t s_sum = 0;
  for (int s = 0; s < cnt; ++s) {
    const uint32_t bs = bucket_at(s);
    const uint32_t ds = dec_at(s);
    if (bs == my_bucket) {
      s_sum += ds;
      if (s < t) leader = false;
    }
  }
  sum = s_sum;
  return leader;
}

// The rule itself: a counter gives up a summed decrement only when it holds it.
CMS_HD bool retract_under(uint64_t sum, uint32_t live) { return sum > (uint64_t)live; }

// One run against one sketch row on the host: the smallest offending bucket,
// or -1 when every summed decrement fits its counter.  get(bucket) is the live
// counter.  (The device runs the same two functions with a lane per member.)
template <class Get>
inline int64_t retract_check_run(const uint32_t* bucket, const uint32_t* dec, int cnt, Get&& get) {
  int64_t bad = -1;
  for (int t = 0; t < cnt; ++t) {
    uint64_t sum;
    const bool leader = retract_combine(
        t, bucket[t], cnt, [&](int s) { return bucket[s]; }, [&](int s) { return dec[s]; }, sum);
    if (leader && sum != 0 && retract_under(sum, get(bucket[t])) && (bad < 0 || (int64_t)bucket[t] < bad))
      bad = (int64_t)bucket[t];
  }
  return bad;
}

}  // namespace cms
