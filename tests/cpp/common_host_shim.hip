// Host-side build of what the co-rated similarity kernels share with the host
// (mahout_amd/csrc/cms_common.h) for the CPU test tests/test_common_host.py.
// k_common_tile and k_common_pairs call the same functions.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_common.h"

static void put(const cms::CommonSums& s, double* out) {
  const double v[7] = {s.sumXY, s.sumX, s.sumY, s.sumX2, s.sumY2, s.sumD2, (double)s.count};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
}

extern "C" {

// sums[7]: sumXY, sumX, sumY, sumX2, sumY2, sumXYdiff2, count -- the sequential route's, what k_common_pairs forms
void ch_merge_join(const int64_t* xk, const float* xv, int64_t nx, const int64_t* yk, const float* yv, int64_t ny,
                   double* sums) {
  put(cms::common_merge_join(xk, xv, nx, yk, yv, ny), sums);
}

double ch_finish(int measure, const double* v, int64_t xlen, int64_t ylen, int64_t num, int weighted) {
  const int64_t n = (int64_t)v[6];
  switch (measure) {
    case cms::kCommonUncentered:
      return cms::common_finish<cms::kCommonUncentered>(v[0], v[1], v[2], v[3], v[4], v[5], n, xlen, ylen, num, weighted);
    case cms::kCommonPearson:
      return cms::common_finish<cms::kCommonPearson>(v[0], v[1], v[2], v[3], v[4], v[5], n, xlen, ylen, num, weighted);
    default:
      return cms::common_finish<cms::kCommonEuclidean>(v[0], v[1], v[2], v[3], v[4], v[5], n, xlen, ylen, num, weighted);
  }
}

// The integer route's sums: the cells of k_common_tile, filled in y's order from
// the last entry, as no order matters there.  Returns 1 when the pair is
// eligible (else sums is left alone); U[2] receives the lists' U.
int ch_cells(const int64_t* xk, const float* xv, int64_t nx, const int64_t* yk, const float* yv, int64_t ny, int s,
             uint64_t* U, double* sums) {
  double s2, root;
  cms::exact_owner_sums(xv, 0, nx, s, U[0], s2, root);
  cms::exact_owner_sums(yv, 0, ny, s, U[1], s2, root);
  if (s == cms::kExactNoShift || U[0] >= cms::kCommonEligible || U[1] >= cms::kCommonEligible) return 0;
  uint64_t sxy = 0, sx = 0, sy = 0, sxx = 0, syy = 0, d2 = 0;
  uint32_t count = 0;
  for (int64_t j = ny - 1; j >= 0; --j)
    for (int64_t i = 0; i < nx; ++i)
      if (xk[i] == yk[j]) {
        const int32_t xu = cms::exact_unit(xv[i], s), yu = cms::exact_unit(yv[j], s);
        sxy += cms::common_term_xy(xu, yu), sx += cms::common_term_lin(xu), sy += cms::common_term_lin(yu);
        sxx += cms::common_term_sq(xu), syy += cms::common_term_sq(yu), d2 += cms::common_term_d2(xu, yu);
        ++count;
      }
  put(cms::common_cells_to_sums(sxy, sx, sy, sxx, syy, d2, count, s), sums);
  return 1;
}

int ch_shift(const float* vals, int64_t n) { return cms::exact_shift_for(vals, n); }
int ch_tile_for(int measure, int asked) { return cms::common_tile_for(measure, asked); }

}  // extern "C"
