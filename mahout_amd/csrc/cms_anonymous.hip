// cms_anonymous.hip -- queries for profiles that are no row of the table.
//
// PlusAnonymousUserDataModel (T/impl/model/PlusAnonymousUserDataModel.java:74-137)
// lets recommender.recommend(TEMP_USER_ID, n) serve a user the model does not
// hold: CosineCM.userSimilarity sketches the temporary preferences with
// exportProfile (CosineCM.java:41-58) and compares that sketch with every
// owner's (:83-96).  Here a batch of such profiles is sketched on the device
// (k_anon_sketch, k_anon_rows) and compared with the stored rows by
// k_anon_cosine, which reads each owner's row once per batch of B profiles:
//
//   - a workgroup keeps sketch row i of the B profiles in LDS, bucket-major
//     ([w][B] u16 or u32 counters: one wide read serves all B profiles);
//   - a wave takes an owner.  A list row's dot with profile b is the sum of
//     the profile's counter at the owner's entries (update is linear, as
//     k_pair_cosine's list branch); a dense row is streamed against the image,
//     or read at the batch's non-zero buckets when those are few
//     (anon_use_bucket_lists);
//   - the B dots fold across the wave so that one lane ends with each
//     profile's sum, and that lane finishes the row's cosine: the integer dot
//     converted once over the product of the stored square roots, or -- a
//     norm at or above 2^53 on either side -- the reference's sequential fp64
//     sums (DoubleCountMinSketch.cosine :114-149), then the running Math.min
//     kept in the output slab and, after the last row, cosine_finish.
//
// The values are k_pair_cosine's for a twin owner holding the same stream,
// bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "cms_anon.h"
#include "cms_device.h"
#include "cms_internal.h"
#include "cms_ref.h"

namespace cms {

constexpr int kAnonThreads = 1024;  // 16 waves: four per SIMD, one workgroup per CU at the full LDS image

// ---- a. the profiles' sketches ----

// update(key, val) of every pair of profile c0 + blockIdx.x into its zeroed sketch
__global__ __launch_bounds__(256) void k_anon_sketch(HashParams hp, const int64_t* off, const int64_t* keys,
                                                     const float* vals, int64_t c0, uint32_t* qsk) {
  const int64_t q = blockIdx.x;
  uint32_t* sk = qsk + q * ((int64_t)hp.depth * hp.width);
  const int64_t hi = off[c0 + q + 1];
  for (int64_t t = off[c0 + q] + threadIdx.x; t < hi; t += blockDim.x) {
    uint32_t inc;
    if (!anon_inc(vals, t, hp.frac_bits, inc)) continue;  // (validated on the host)
    anon_update(hp, keys[t], inc, [&](int i, uint32_t j, uint32_t v) { atomicAdd(&sk[(int64_t)i * hp.width + j], v); });
  }
}

// One wave per (profile, sketch row): the sum of squares (saturating, as
// k_norms), Math.sqrt of it, the non-zero bucket list in ascending order and
// the profile's largest counter.
__global__ __launch_bounds__(256) void k_anon_rows(const uint32_t* qsk, int64_t cells, int d, int w, uint64_t* qnorm,
                                                   double* qnsq, uint32_t* qnnz, uint32_t* qmax, AnonEntry* qnz) {
  const int lane = threadIdx.x & 63;
  const int64_t cell = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (cell >= cells) return;
  const uint32_t* row = qsk + cell * w;
  AnonEntry* list = qnz + cell * w;
  uint64_t sq = 0;
  uint32_t vmax = 0, base = 0;
  for (int j0 = 0; j0 < w; j0 += 64) {
    const int j = j0 + lane;
    AnonEntry e{0u, 0u};
    const uint32_t have = j < w ? anon_nonzero(row, (uint32_t)j, (uint32_t)j + 1u, &e) : 0u;
    sq = sat_add(sq, (uint64_t)e.count * e.count);
    vmax = max(vmax, e.count);
    const uint64_t mask = __ballot(have != 0u);
    if (have) list[base + (uint32_t)__popcll(mask & ((1ULL << lane) - 1ULL))] = e;
    base += (uint32_t)__popcll(mask);
  }
  sq = wave_sum_u64_sat(sq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
  if (lane == 0) {
    qnorm[cell] = sq;
    qnsq[cell] = __dsqrt_rn((double)sq);
    qnnz[cell] = base;
    atomicMax(&qmax[cell / d], vmax);
  }
}

// ---- b. the similarity kernel ----

struct AnonArgs {
  TableView tv;
  const uint64_t* norm;  // the owners' [n][d] sums of squares and their square roots
  const double* nsqrt;
  const uint32_t* qsk;   // the chunk's sketches, norms, roots, bucket lists
  const uint64_t* qnorm;
  const double* qnsq;
  const uint32_t* qnnz;
  const AnonEntry* qnz;
  int64_t q0;            // first profile of the batch (index in the chunk)
  int32_t bact;          // profiles in the batch (<= B)
  int32_t d, w;
  const int64_t* rows;   // owner row of output column t (null: row t)
  int64_t ncols, nrows;
  double* out;           // [chunk profiles][ld]: the running min, then the similarity
  int64_t ld;
  int32_t weighted;
  int32_t lists;         // dense rows through the bucket lists (anon_use_bucket_lists)
};

// the B profiles' counters of one bucket: read in one piece
template <class ELT, int B>
struct alignas(sizeof(ELT) * B > 16 ? 16 : sizeof(ELT) * B) AnonVec {
  ELT v[B];
};

// Sums v[b] over the wave for every b at once: each step hands half of a
// lane's values to its partner, so log2(B) steps leave one value per lane and
// the remaining steps are a plain butterfly.  The total of profile
// b = lane >> (6 - log2 B) ends in v[0] of that lane.
template <int B>
__device__ __forceinline__ void wave_fold(uint64_t (&v)[B], int lane) {
  int o = 32;
#pragma unroll
  for (int half = B / 2; half >= 1; half >>= 1, o >>= 1) {
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      const uint64_t send = up ? v[k] : v[k + half];
      const uint64_t keep = up ? v[k + half] : v[k];
      v[k] = keep + __shfl_xor(send, o, 64);
    }
  }
  for (; o >= 1; o >>= 1) v[0] += __shfl_xor(v[0], o, 64);
}

template <int B>
struct Log2;
template <> struct Log2<1> { static constexpr int v = 0; };
template <> struct Log2<2> { static constexpr int v = 1; };
template <> struct Log2<4> { static constexpr int v = 2; };
template <> struct Log2<8> { static constexpr int v = 3; };
static_assert(kAnonMaxB == 8, "launch_anon_b instantiates B up to 8");

template <class ELT, int B>
__global__ __launch_bounds__(kAnonThreads) void k_anon_cosine(AnonArgs g) {
  extern __shared__ uint4 anon_lds[];
  using Vec = AnonVec<ELT, B>;
  const Vec* img = reinterpret_cast<const Vec*>(anon_lds);
  ELT* img_w = reinterpret_cast<ELT*>(anon_lds);
  constexpr int S = Log2<B>::v;
  const int lane = threadIdx.x & 63;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int myb = lane >> (6 - S);
  const bool writer = (lane & ((64 >> S) - 1)) == 0 && myb < g.bact;
  const int w = g.w, d = g.d;
  const int64_t qdw = (int64_t)d * w;

  for (int i = 0; i < d; ++i) {
    const int64_t c0 = (int64_t)i * w;
    // sketch row i of the batch's profiles -> LDS, bucket-major; lanes take b
    // fastest, so a wave reads whole 64-B runs of 64 / B buckets per profile
    __syncthreads();  // the last row's readers are done
    if ((w & 3) == 0) {
      for (int idx = threadIdx.x; idx < (w >> 2) * B; idx += blockDim.x) {
        const int b = idx & (B - 1), j4 = idx >> S;
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (b < g.bact) x = *reinterpret_cast<const uint4*>(g.qsk + (g.q0 + b) * qdw + c0 + 4 * j4);
        img_w[(4 * j4 + 0) * B + b] = (ELT)x.x;
        img_w[(4 * j4 + 1) * B + b] = (ELT)x.y;
        img_w[(4 * j4 + 2) * B + b] = (ELT)x.z;
        img_w[(4 * j4 + 3) * B + b] = (ELT)x.w;
      }
    } else {
      for (int idx = threadIdx.x; idx < w * B; idx += blockDim.x) {
        const int b = idx & (B - 1), j = idx >> S;
        img_w[idx] = b < g.bact ? (ELT)g.qsk[(g.q0 + b) * qdw + c0 + j] : (ELT)0;
      }
    }
    __syncthreads();

    for (int64_t t = wave; t < g.ncols; t += nwaves) {
      int64_t r = g.rows ? g.rows[t] : t;
      const bool valid = r >= 0 && r < g.nrows;
      if (!valid) r = 0;
      const uint64_t No = valid ? g.norm[r * d + i] : 0ULL;
      uint64_t acc[B];
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b] = 0;
      if (No != 0ULL && No < (1ULL << 53)) {  // else no integer dot is needed (den == 0, or the sequential sums)
        const int32_t form = g.tv.hidx[r];
        if (form == kFormList) {
          const uint32_t m = g.tv.list_m(r);
          const uint16_t* e = g.tv.list_row(r, i, m);
          for (uint32_t u = lane; u < m; u += 64) {
            const Vec y = img[e[u]];
#pragma unroll
            for (int b = 0; b < B; ++b) acc[b] += y.v[b];
          }
        } else if (g.lists) {
#pragma unroll 1
          for (int b = 0; b < g.bact; ++b) {
            const int64_t cell = (g.q0 + b) * d + i;
            const uint32_t nn = g.qnnz[cell];
            const AnonEntry* L = g.qnz + cell * w;
            uint64_t p = 0;
            for (uint32_t u = lane; u < nn; u += 64) {
              const AnonEntry en = L[u];
              p += (uint64_t)en.count * g.tv.get(r, c0 + en.bucket);
            }
#pragma unroll
            for (int k = 0; k < B; ++k)  // (acc stays in registers: no dynamic index)
              if (k == b) acc[k] = p;
          }
        } else if ((w & 3) == 0) {
          for (int j4 = lane; j4 < (w >> 2); j4 += 64) {
            const uint4 x = g.tv.get4(r, c0 + 4 * j4);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const Vec y = img[4 * j4 + k];
#pragma unroll
              for (int b = 0; b < B; ++b) acc[b] += (uint64_t)xs[k] * y.v[b];
            }
          }
        } else {
          for (int j = lane; j < w; j += 64) {
            const uint32_t x = g.tv.get(r, c0 + j);
            const Vec y = img[j];
#pragma unroll
            for (int b = 0; b < B; ++b) acc[b] += (uint64_t)x * y.v[b];
          }
        }
        wave_fold<B>(acc, lane);
      }
      if (writer) {
        const int64_t q = g.q0 + myb;
        double* o = g.out + q * g.ld + t;
        double minc = i == 0 ? DBL_MAX : *o;
        if (valid) {
          const uint64_t Nq = g.qnorm[q * d + i];
          double valueAB, den;
          if (Nq < (1ULL << 53) && No < (1ULL << 53)) {
            valueAB = (double)acc[0];
            den = __dmul_rn(g.qnsq[q * d + i], g.nsqrt[r * d + i]);
          } else {  // the reference's sums in j order (seq_row_sums, cms_query.hip)
            const uint32_t* qs = g.qsk + q * qdw + c0;
            double A = 0.0, Bn = 0.0;
            valueAB = 0.0;
            for (int j = 0; j < w; ++j) {
              const double xa = (double)qs[j], xb = (double)g.tv.get(r, c0 + j);
              A = __dadd_rn(A, __dmul_rn(xa, xa));
              Bn = __dadd_rn(Bn, __dmul_rn(xb, xb));
              valueAB = __dadd_rn(valueAB, __dmul_rn(xa, xb));
            }
            den = __dmul_rn(__dsqrt_rn(A), __dsqrt_rn(Bn));
          }
          if (den != 0.0) minc = java_min(minc, __ddiv_rn(valueAB, den));
        }
        *o = i == d - 1 ? cosine_finish(minc, g.weighted) : minc;
      }
    }
  }
}

// ---- host side ----

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int anon_upload(cms_handle* h, int64_t nq, const int64_t* offsets, const int64_t* keys, const float* vals,
                AnonBatch& ab) {
  const int64_t np = nq > 0 ? offsets[nq] : 0;
  const size_t o_off = 0, o_key = align_up(sizeof(int64_t) * (size_t)(nq + 1), 256);
  const size_t o_val = o_key + align_up(sizeof(int64_t) * (size_t)np, 256);
  CMS_HIP(h->an_in.ensure(o_val + align_up(sizeof(float) * (size_t)np, 256) + 256));
  char* base = h->an_in.as<char>();
  CMS_HIP(hipMemcpyAsync(base + o_off, offsets, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyHostToDevice, h->stream));
  if (np > 0) {
    CMS_HIP(hipMemcpyAsync(base + o_key, keys, sizeof(int64_t) * (size_t)np, hipMemcpyHostToDevice, h->stream));
    if (vals) CMS_HIP(hipMemcpyAsync(base + o_val, vals, sizeof(float) * (size_t)np, hipMemcpyHostToDevice, h->stream));
  }
  ab.nq = nq;
  ab.npairs = np;
  ab.d_off = reinterpret_cast<const int64_t*>(base + o_off);
  ab.d_keys = reinterpret_cast<const int64_t*>(base + o_key);
  ab.d_vals = vals ? reinterpret_cast<const float*>(base + o_val) : nullptr;
  return CMS_OK;
}

// A chunk's slab [qc][n] stays within slab_rows_for(n), and its sketches and
// bucket lists (12 B per counter and profile) within 1 GiB.
int64_t anon_chunk_rows(cms_handle* h) {
  const int64_t by_scratch = std::max<int64_t>(1, (int64_t(1) << 30) / (12 * std::max<int64_t>(1, h->dw)));
  return std::min<int64_t>(slab_rows_for(h->n), by_scratch);
}

// the chunk's per-(profile, row) arrays inside an_meta, for qc profiles
struct AnonMeta {
  uint64_t* norm;
  double* nsq;
  uint32_t* nnz;
  uint32_t* qmax;
};
static AnonMeta anon_meta(cms_handle* h, int64_t qc) {
  const int64_t cells = qc * h->p.depth;
  char* p = h->an_meta.as<char>();
  AnonMeta m;
  m.norm = reinterpret_cast<uint64_t*>(p);
  m.nsq = reinterpret_cast<double*>(p + 8 * cells);
  m.nnz = reinterpret_cast<uint32_t*>(p + 16 * cells);
  m.qmax = m.nnz + cells;
  return m;
}

int anon_build(cms_handle* h, AnonBatch& ab, int64_t c0, int64_t qc) {
  const int d = h->p.depth, w = h->p.width;
  const int64_t cells = qc * d;
  CMS_HIP(h->an_sk.ensure(sizeof(uint32_t) * (size_t)(qc * h->dw)));
  CMS_HIP(h->an_nz.ensure(sizeof(AnonEntry) * (size_t)(qc * h->dw)));
  CMS_HIP(h->an_meta.ensure((size_t)(20 * cells + 4 * qc)));
  const AnonMeta m = anon_meta(h, qc);
  {
    TimedScope ts(h, "anon_sketch");
    CMS_HIP(hipMemsetAsync(h->an_sk.ptr, 0, sizeof(uint32_t) * (size_t)(qc * h->dw), h->stream));
    CMS_HIP(hipMemsetAsync(m.qmax, 0, sizeof(uint32_t) * (size_t)qc, h->stream));
    hipLaunchKernelGGL(k_anon_sketch, dim3((unsigned)qc), dim3(256), 0, h->stream, h->hp, ab.d_off, ab.d_keys, ab.d_vals,
                       c0, h->an_sk.as<uint32_t>());
    CMS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_anon_rows, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, h->stream,
                       h->an_sk.as<uint32_t>(), cells, d, w, m.norm, m.nsq, m.nnz, m.qmax, h->an_nz.as<AnonEntry>());
    CMS_HIP(hipGetLastError());
  }
  // the batches' element width and dense-row rule are chosen on the host
  std::vector<uint32_t> nnz((size_t)cells);
  ab.qmax.assign((size_t)qc, 0u);
  CMS_HIP(hipMemcpyAsync(nnz.data(), m.nnz, sizeof(uint32_t) * (size_t)cells, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipMemcpyAsync(ab.qmax.data(), m.qmax, sizeof(uint32_t) * (size_t)qc, hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  ab.qnnz.assign((size_t)qc, 0u);
  for (int64_t q = 0; q < qc; ++q)
    for (int i = 0; i < d; ++i) ab.qnnz[q] = std::max(ab.qnnz[q], nnz[(size_t)(q * d + i)]);
  ab.c0 = c0;
  ab.qc = qc;
  return CMS_OK;
}

template <class ELT, int B>
static int launch_anon(cms_handle* h, const AnonArgs& g) {
  const size_t lds = std::max<size_t>(sizeof(ELT) * (size_t)B * (size_t)g.w, 16);
  static bool attr_set[64] = {};  // per instantiation and device
  const int dev = h->device & 63;
  if (!attr_set[dev]) {
    (void)hipFuncSetAttribute((const void*)k_anon_cosine<ELT, B>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kAnonLds);
    attr_set[dev] = true;
  }
  const int64_t per_cu = lds <= 64 * 1024 ? 2 : 1;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(h->num_cus * per_cu, (g.ncols + 15) / 16));
  hipLaunchKernelGGL((k_anon_cosine<ELT, B>), dim3((unsigned)grid), dim3(kAnonThreads), lds, h->stream, g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

template <class ELT>
static int launch_anon_b(cms_handle* h, int B, const AnonArgs& g) {
  switch (B) {
    case 8: return launch_anon<ELT, 8>(h, g);
    case 4: return launch_anon<ELT, 4>(h, g);
    case 2: return launch_anon<ELT, 2>(h, g);
    default: return launch_anon<ELT, 1>(h, g);
  }
}

int anon_cosines(cms_handle* h, const AnonBatch& ab, const int64_t* d_rows, int64_t ncols, double* d_out, int64_t ld) {
  if (ab.qc <= 0 || ncols <= 0) return CMS_OK;
  const int w = h->p.width;
  const AnonMeta m = anon_meta(h, ab.qc);
  AnonArgs g{};
  g.tv = h->tview();
  g.norm = h->d_norm;
  g.nsqrt = h->d_norm_sqrt;
  g.qsk = h->an_sk.as<uint32_t>();
  g.qnorm = m.norm;
  g.qnsq = m.nsq;
  g.qnnz = m.nnz;
  g.qnz = h->an_nz.as<AnonEntry>();
  g.d = h->p.depth;
  g.w = w;
  g.rows = d_rows;
  g.ncols = ncols;
  g.nrows = h->n;
  g.out = d_out;
  g.ld = ld;
  g.weighted = (int)h->p.weighting;
  TimedScope ts(h, "anon_cosine");
  for (int64_t q = 0; q < ab.qc;) {
    // u16 elements unless one of the batch's profiles holds a counter past them
    int elem = 2, B = anon_batch_size(w, 2);
    int64_t bact = std::min<int64_t>(B, ab.qc - q);
    uint32_t mx = 0;
    for (int64_t b = 0; b < bact; ++b) mx = std::max(mx, ab.qmax[(size_t)(q + b)]);
    if (B == 0 || anon_elem_bytes(mx) == 4) {
      elem = 4;
      B = anon_batch_size(w, 4);
      bact = std::min<int64_t>(B, ab.qc - q);
    }
    if (B <= 0) return set_error(CMS_E_PARAM, "width %d is beyond the LDS image of one profile's sketch row", w);
    int64_t nnz = 0;
    for (int64_t b = 0; b < bact; ++b) nnz += ab.qnnz[(size_t)(q + b)];
    g.q0 = q;
    g.bact = (int32_t)bact;
    g.lists = anon_use_bucket_lists(nnz, w) ? 1 : 0;
    const int rc = elem == 2 ? launch_anon_b<uint16_t>(h, B, g) : launch_anon_b<uint32_t>(h, B, g);
    if (rc) return rc;
    q += bact;
  }
  return CMS_OK;
}

}  // namespace cms
