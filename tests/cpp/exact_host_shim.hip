// Host-side build of what the exact-cosine kernels share with the host
// (mahout_amd/csrc/cms_exact.h) for the CPU test tests/test_exact_host.py: the
// attach rules (shift, units, per-owner sums, CSR validation), the merge join
// and exact_finish.  k_exact_tile, k_exact_pairs and exact_attach call the
// same functions.
#include <hip/hip_runtime.h>

#include "../../mahout_amd/csrc/cms_exact.h"

extern "C" {

// the shift s of a value set (-1: none)
int eh_shift(const float* vals, int64_t n) { return cms::exact_shift_for(vals, n); }

int32_t eh_unit(float v, int s) { return cms::exact_unit(v, s); }

// one owner's U, sequential sumX2 and its square root; returns 1 when integer-eligible
int eh_owner(const float* vals, int64_t n, int s, uint64_t* U, double* sum2, double* root) {
  cms::exact_owner_sums(vals, 0, n, s, *U, *sum2, *root);
  return *U < cms::kExactEligible ? 1 : 0;
}

int eh_valid_csr(int64_t n, const int64_t* off, const int64_t* keys) { return cms::exact_valid_csr(n, off, keys) ? 1 : 0; }

double eh_merge_join(const int64_t* xi, const float* xv, int64_t nx, const int64_t* yi, const float* yv, int64_t ny) {
  return cms::exact_merge_join(xi, xv, nx, yi, yv, ny);
}

double eh_finish(double sumXY, double rootX, double rootY, int64_t xlen, int64_t ylen, int weighted) {
  return cms::exact_finish(sumXY, rootX, rootY, xlen, ylen, weighted);
}

// userSimilarity of two lists by the sequential route: what k_exact_pairs computes
double eh_similarity_seq(const int64_t* xi, const float* xv, int64_t nx, const int64_t* yi, const float* yv, int64_t ny,
                         int weighted) {
  uint64_t U;
  double s2, rx, ry;
  cms::exact_owner_sums(xv, 0, nx, cms::kExactNoShift, U, s2, rx);
  cms::exact_owner_sums(yv, 0, ny, cms::kExactNoShift, U, s2, ry);
  return cms::exact_finish(cms::exact_merge_join(xi, xv, nx, yi, yv, ny), rx, ry, nx, ny, weighted);
}

// ... by the integer route: the dot of the units in y's order, as no order matters
// there (k_exact_tile adds them in whatever order its lanes run); -1 in *ok
// when the pair is not eligible
double eh_similarity_int(const int64_t* xi, const float* xv, int64_t nx, const int64_t* yi, const float* yv, int64_t ny,
                         int s, int weighted, int* ok) {
  uint64_t Ux, Uy;
  double s2, rx, ry;
  cms::exact_owner_sums(xv, 0, nx, s, Ux, s2, rx);
  cms::exact_owner_sums(yv, 0, ny, s, Uy, s2, ry);
  *ok = (s != cms::kExactNoShift && Ux < cms::kExactEligible && Uy < cms::kExactEligible) ? 1 : -1;
  if (*ok < 0) return 0.0;
  unsigned long long dot = 0;
  for (int64_t j = ny - 1; j >= 0; --j)
    for (int64_t i = 0; i < nx; ++i)
      if (xi[i] == yi[j]) dot += (unsigned long long)((int64_t)cms::exact_unit(xv[i], s) * cms::exact_unit(yv[j], s));
  return cms::exact_finish(cms::exact_dot_to_sum((int64_t)dot, s), rx, ry, nx, ny, weighted);
}

int eh_tile_for(int asked) { return cms::exact_tile_for(asked); }

}  // extern "C"
