// Host-side build of what the retraction kernels share with the host
// (mahout_amd/csrc/cms_retract.h) for the CPU test tests/test_retract_host.py:
// the batch validation and the per-owner, per-sketch-row step "sum the
// decrements per bucket, compare each sum with the live counter".
// k_retract_validate, k_retract_wave and k_retract_image call the same
// functions.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_retract.h"

extern "C" {

// the ABI's code for a batch (0 ok, 1 a row outside [0, nrows), 5 a value no
// ingest takes; a bad row is reported first, as the ingest's flag word is read)
int rh_validate(const int64_t* rows, const float* vals, int64_t n, int64_t nrows, int frac_bits) {
  uint32_t f = 0;
  for (int64_t i = 0; i < n; ++i) f |= cms::retract_validate_pair(rows, vals, i, nrows, frac_bits);
  return (f & cms::kRetractBadRow) ? 1 : (f & cms::kRetractBadValue) ? 5 : 0;
}

// each value's decrement in counter units (ok[i] = 0 and dec[i] = 0 for a refused value)
void rh_dec(const float* vals, int64_t n, int frac_bits, uint32_t* dec, uint8_t* ok) {
  for (int64_t i = 0; i < n; ++i) ok[i] = cms::retract_dec(vals, i, frac_bits, dec[i]) ? 1 : 0;
}

// every member's summed decrement and whether it leads its bucket
void rh_combine(const uint32_t* bucket, const uint32_t* dec, int cnt, uint64_t* sum, uint8_t* leader) {
  for (int t = 0; t < cnt; ++t)
    leader[t] = cms::retract_combine(
                    t, bucket[t], cnt, [&](int s) { return bucket[s]; }, [&](int s) { return dec[s]; }, sum[t])
                    ? 1
                    : 0;
}

// one run against one sketch row's counters [w]: the smallest offending bucket, or -1
int64_t rh_check_run(const uint32_t* bucket, const uint32_t* dec, int cnt, const uint32_t* counters, int w) {
  return cms::retract_check_run(bucket, dec, cnt, [&](uint32_t b) { return (int)b < w ? counters[b] : 0u; });
}

int rh_wave_run(void) { return cms::kRetractWaveRun; }

}  // extern "C"
