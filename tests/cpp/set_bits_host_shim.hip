// Host-side build of what the dense set similarity kernels share with the host
// (mahout_amd/csrc/cms_set_bits.h) for the CPU test tests/test_set_bits_host.py.
// k_set_bits_pack and k_set_bits_mfma call the same functions.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_set_bits.h"

extern "C" {

uint32_t sb_expand8(uint32_t byte) { return cms::bits_expand8(byte); }
int64_t sb_stage() { return cms::kBitsStage; }
int64_t sb_padded_k(int64_t num) { return cms::bits_padded_k(num); }
int64_t sb_seg_stages(int64_t asked) { return cms::bits_seg_stages(asked); }
int64_t sb_segments(int64_t num, int64_t seg_stages) { return cms::bits_segments(num, seg_stages); }
int64_t sb_matrix_bytes(int64_t n, int64_t num) { return cms::bits_matrix_bytes(n, num); }
int64_t sb_word_off(int64_t row, int64_t w, int64_t stages) { return cms::bits_word_off(row, w, stages); }

}  // extern "C"
