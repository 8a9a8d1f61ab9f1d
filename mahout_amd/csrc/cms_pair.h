// cms_pair.h -- what the pair kernel (cms_query.hip) and the staged block
// kernel (cms_item.hip) share, so both form a row's quotient from one text.
#pragma once
#include <hip/hip_runtime.h>

#include "cms_internal.h"

namespace cms {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Reference-order sequential fp64 sums for one sketch row (inexact regime).
__device__ inline void seq_row_sums(const TableView& tv, int64_t ra, int64_t rb, int64_t c0, int w, double& A, double& B,
                                    double& AB) {
  A = 0.0;
  B = 0.0;
  AB = 0.0;
  for (int j = 0; j < w; ++j) {
    double xa = (double)tv.get(ra, c0 + j), xb = (double)tv.get(rb, c0 + j);
    A = __dadd_rn(A, __dmul_rn(xa, xa));
    B = __dadd_rn(B, __dmul_rn(xb, xb));
    AB = __dadd_rn(AB, __dmul_rn(xa, xb));
  }
}

}  // namespace cms
