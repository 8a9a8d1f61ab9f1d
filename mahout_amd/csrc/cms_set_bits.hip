// cms_set_bits.hip -- the dense route of the set similarities (cms_set.h): the
// shared-entry counts of many lists against many lists as a 0/1 GEMM on the
// fp4 matrix units, over a bit matrix of the attached model's side
// (cms_set_bits.h states its layout and why the counts are exact).  It serves
// the all-lists job (set_bits_top_k_all) and the dense block query
// (set_bits_block); the per-query calls keep the posting-list walk of
// cms_set.hip.  The sketch table is neither read nor written.
//
//   - k_set_bits_pack: one wave per list.  The list's cross indices ascend and
//     are distinct, so the entries of one u32 word sit in neighbouring lanes: a
//     segmented OR over at most 32 lanes (five shuffle steps) forms the word in
//     the run's first lane, which stores it whole.  Only the first and the last
//     run of a 64-entry batch can continue in the neighbouring batch; those two
//     go out with an atomic OR into the zeroed matrix.
//   - k_set_bits_mfma<MEASURE>: a workgroup of 256 threads per 128 x 128 tile
//     of (query lists x candidate lists); wave (wr, wc) owns 64 x 64 as 2 x 2
//     fragments of v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1 operands.  Tile
//     rows come through index arrays (list index per row, null: base + row),
//     so one kernel serves the all-lists job, its query chunks and the block
//     query over arbitrary IDs; rows past the end load zero bits and store
//     nothing.  A K stage is 256 cross indices: thread t loads 16 B of bits of
//     row t / 2 of each panel (half t % 2 of the row's 32 B), expands every
//     byte to a dword of nibbles (bits_expand8) once, on the way into LDS, and
//     writes four 16-B chunks per panel under the XOR swizzle of lds_off_bk.
//     The next stage's two loads are issued before the barrier and stay in
//     flight through the current stage's sixteen MFMAs; LDS holds two stages
//     (2 x 32 KiB), one barrier per stage.  At a segment's end (at most 2^24
//     cross indices) the f32 accumulators are converted to u32, added to the
//     running counts in registers and cleared.  The epilogue parks the tile's
//     counts in the LDS the stages used and walks it row by row, column per
//     thread: set_finish<MEASURE> with the lengths from off, as k_set_tile
//     takes them, and plain coalesced f64 stores.
//   - the top-k is launch_top_k on the slab, as set_top_k calls it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "cms_exact_model.h"
#include "cms_mfma.h"
#include "cms_set.h"
#include "cms_set_bits.h"

namespace cms {

constexpr int kBitsThreads = 256;  // 4 waves: 2 x 2 of 64 x 64
constexpr int kBitsTile = 128;     // rows and columns of a workgroup's tile
constexpr int kBitsPanelBytes = kBitsTile * (kBitsStage / 2);  // one panel's stage in LDS: 128 rows x 128 B of nibbles
constexpr int kBitsStageBytes = 2 * kBitsPanelBytes;           // both panels: 32 KiB
constexpr int kBitsPackThreads = 256;
constexpr int64_t kBitsRowsMax = 65535 * (int64_t)kBitsTile;   // tile rows of one launch (grid.y)
static_assert(kBitsTile == kBitsBlk, "a tile's panel is one block of the matrix when its rows are consecutive");
static_assert(2 * kBitsStageBytes == kBitsTile * kBitsTile * 4, "the count tile reuses the two stages exactly");

// ---- the pack kernel ----
__global__ __launch_bounds__(kBitsPackThreads) void k_set_bits_pack(const int64_t* off, const int32_t* key, int64_t n,
                                                                    int64_t stages, uint32_t* bits) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (kBitsPackThreads >> 6);
  for (int64_t a = (blockIdx.x * (int64_t)kBitsPackThreads + threadIdx.x) >> 6; a < n; a += nwaves) {
    const int64_t lo = off[a], hi = off[a + 1];
    for (int64_t p0 = lo; p0 < hi; p0 += 64) {  // (uniform over the wave)
      const bool live = p0 + lane < hi;
      const int32_t u = live ? key[p0 + lane] : 0;
      const int32_t w = live ? (u >> 5) : -1;  // dead lanes: a word of their own, never stored
      uint32_t v = live ? 1u << (u & 31) : 0u;
#pragma unroll
      for (int d = 1; d < 32; d <<= 1) {  // the OR of the run's lanes from this one on
        const int32_t wd = __shfl_down(w, d);
        const uint32_t vd = __shfl_down(v, d);
        if (lane + d < 64 && wd == w) v |= vd;
      }
      const int32_t wp = __shfl_up(w, 1);
      const int32_t wfirst = __shfl(w, 0);
      const int32_t wlast = __shfl(w, (int)min((int64_t)63, hi - p0 - 1));
      if (live && (lane == 0 || wp != w)) {
        uint32_t* dst = bits + bits_word_off(a, w, stages);
        const bool shared = (w == wfirst && p0 > lo) || (w == wlast && p0 + 64 < hi);
        if (shared) atomicOr(dst, v);
        else *dst = v;
      }
    }
  }
}

// ---- the count kernel ----
struct BitsArgs {
  const uint32_t* bits;
  int64_t stages;        // K stages of a row
  int64_t seg_stages;    // stages per f32 segment
  const int64_t* ia;     // tile row r < na: list ia[r] (null: a0 + r)
  const int64_t* ib;     // tile column c < nb: list ib[c] (null: b0 + c)
  int64_t a0, na, b0, nb;
  const int64_t* off;    // the side's list offsets: the lengths
  int64_t num;
  int32_t owner_side;
  double* out;           // out[r * ld + c]
  int64_t ld;
};

// 16 B of a row's bits as four 16-B chunks of nibbles: chunk ch0 + c is word c
__device__ __forceinline__ void bits_put(unsigned char* panel, int row, int ch0, const uint4& x) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int c = 0; c < 4; ++c)
    *reinterpret_cast<uint4*>(panel + lds_off_bk<128>(row, ch0 + c)) =
        make_uint4(bits_expand8(w[c]), bits_expand8(w[c] >> 8), bits_expand8(w[c] >> 16), bits_expand8(w[c] >> 24));
}

template <int MEASURE>
__global__ __launch_bounds__(kBitsThreads) void k_set_bits_mfma(BitsArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kBitsStageBytes];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, wr = wid >> 1, wc = wid & 1;
  const int64_t row0 = (int64_t)blockIdx.y * kBitsTile, col0 = (int64_t)blockIdx.x * kBitsTile;
  // this thread's part of a stage fill: row t / 2 of both panels, words 4 (t % 2) .. + 3
  const int frow = t >> 1, fch = (t & 1) * 4;
  const bool va = row0 + frow < g.na, vb = col0 + frow < g.nb;
  const int64_t la = !va ? 0 : g.ia ? g.ia[row0 + frow] : g.a0 + row0 + frow;
  const int64_t lb = !vb ? 0 : g.ib ? g.ib[col0 + frow] : g.b0 + col0 + frow;
  const uint4* pa = reinterpret_cast<const uint4*>(g.bits + bits_word_off(la, fch, g.stages));
  const uint4* pb = reinterpret_cast<const uint4*>(g.bits + bits_word_off(lb, fch, g.stages));
  constexpr int64_t kStep = kBitsBlk * kBitsStageWords / 4;  // uint4s from one stage of a block to the next
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  f32x16 acc[2][2];
  uint32_t cnt[2][2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        acc[i][j][e] = 0.0f;
        cnt[i][j][e] = 0u;
      }

  uint4 xa = va ? pa[0] : zero, xb = vb ? pb[0] : zero;
  int64_t left = g.seg_stages;
  for (int64_t s = 0; s < g.stages; ++s) {
    // stage s goes into the buffer that iteration s - 2 read: every wave has passed the barrier of s - 1 since
    unsigned char* A = lds + (s & 1) * kBitsStageBytes;
    unsigned char* B = A + kBitsPanelBytes;
    bits_put(A, frow, fch, xa);
    bits_put(B, frow, fch, xb);
    if (s + 1 < g.stages) {  // in flight through this stage's MFMAs
      xa = va ? pa[(s + 1) * kStep] : zero;
      xb = vb ? pb[(s + 1) * kStep] : zero;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kBitsStage / 64; ++ks) {
      const int ch = 2 * ks + (lane >> 5);
      i8x16 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fa[i] = *reinterpret_cast<const i8x16*>(A + lds_off_bk<128>(wr * 64 + i * 32 + (lane & 31), ch));
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const i8x16*>(B + lds_off_bk<128>(wc * 64 + j * 32 + (lane & 31), ch));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_step<1>(fa[i], fb[j], acc[i][j]);
    }
    if (--left == 0 || s + 1 == g.stages) {  // the segment's end: exact integers at most 2^24
      left = g.seg_stages;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            cnt[i][j][e] += (uint32_t)acc[i][j][e];
            acc[i][j][e] = 0.0f;
          }
    }
  }

  // ---- the epilogue: the tile's counts through LDS, then a column per thread ----
  __syncthreads();  // the last stage has been read
  uint32_t* tile = reinterpret_cast<uint32_t*>(lds);  // [128][128]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        const int c = wc * 64 + j * 32 + (lane & 31);
        tile[r * kBitsTile + c] = cnt[i][j][e];
      }
  __syncthreads();
  const int c = t & (kBitsTile - 1);
  if (col0 + c >= g.nb) return;
  const int64_t lc = g.ib ? g.ib[col0 + c] : g.b0 + col0 + c;
  const int64_t n2 = g.off[lc + 1] - g.off[lc];
  const int rows = (int)min((int64_t)kBitsTile, g.na - row0);
#pragma unroll 1
  for (int r = t / kBitsTile; r < rows; r += kBitsThreads / kBitsTile) {
    const int64_t lr = g.ia ? g.ia[row0 + r] : g.a0 + row0 + r;
    const int64_t n1 = g.off[lr + 1] - g.off[lr];
    g.out[(row0 + r) * g.ld + col0 + c] =
        set_finish<MEASURE>((int64_t)tile[r * kBitsTile + c], n1, n2, g.num, g.owner_side);
  }
}

// ---- host side ----

// The side's bit matrix, built by the first call that needs it; *bits stays null when the budget
// (CMS_SET_BITS_MB) or the device's memory has no room for it, and the caller answers through cms_set.hip.
static int set_bits_matrix(cms_handle* h, int32_t side, const CommonSide& v, const uint32_t** bits) {
  ExactModel& m = *h->exact;
  const int s = side == CMS_SIDE_OWNER ? 0 : 1;
  *bits = nullptr;
  if (m.bits_state[s] == 0) {
    m.bits_state[s] = -1;
    const int64_t bytes = bits_matrix_bytes(v.n, v.num);
    if (h->tune.set_bits_mb <= 0 || bytes > h->tune.set_bits_mb * (int64_t(1) << 20)) return CMS_OK;
    if (m.bits[s].ensure((size_t)bytes) != hipSuccess) {
      (void)hipGetLastError();  // no room: not an error of the call
      return CMS_OK;
    }
    TimedScope ts(h, "set_bits_pack");
    CMS_HIP(hipMemsetAsync(m.bits[s].ptr, 0, (size_t)bytes, h->stream));
    const int64_t grid = std::min<int64_t>((v.n + 3) / 4, (int64_t)h->num_cus * 8);
    hipLaunchKernelGGL(k_set_bits_pack, dim3((unsigned)grid), dim3(kBitsPackThreads), 0, h->stream, v.off, v.key, v.n,
                       bits_stages(v.num), m.bits[s].as<uint32_t>());
    CMS_HIP(hipGetLastError());
    m.bits_state[s] = 1;
  }
  if (m.bits_state[s] == 1) *bits = m.bits[s].as<uint32_t>();
  return CMS_OK;
}

template <int MEASURE>
static int launch_set_bits_as(cms_handle* h, const BitsArgs& g) {
  TimedScope ts(h, "set_bits_mfma");
  const dim3 grid((unsigned)((g.nb + kBitsTile - 1) / kBitsTile), (unsigned)((g.na + kBitsTile - 1) / kBitsTile));
  hipLaunchKernelGGL(k_set_bits_mfma<MEASURE>, grid, dim3(kBitsThreads), 0, h->stream, g);
  CMS_HIP(hipGetLastError());
  return CMS_OK;
}

static int launch_set_bits(cms_handle* h, int32_t measure, const BitsArgs& g) {
  switch (measure) {
    case kSetCooccurrence: return launch_set_bits_as<kSetCooccurrence>(h, g);
    case kSetTanimoto: return launch_set_bits_as<kSetTanimoto>(h, g);
    case kSetCityBlock: return launch_set_bits_as<kSetCityBlock>(h, g);
    default: return launch_set_bits_as<kSetLogLikelihood>(h, g);
  }
}

static BitsArgs bits_args(cms_handle* h, const CommonSide& v, int32_t side, const uint32_t* bits) {
  BitsArgs g{};
  g.bits = bits;
  g.stages = bits_stages(v.num);
  g.seg_stages = bits_seg_stages(h->tune.set_bits_kseg);
  g.off = v.off;
  g.num = v.num;
  g.owner_side = side == CMS_SIDE_OWNER;
  return g;
}

int64_t set_side_lists(const cms_handle* h, int32_t side) { return common_side(h, side).n; }

int set_bits_top_k_all(cms_handle* h, int32_t measure, int32_t side, int32_t k, int64_t* d_ids, double* d_scores,
                       int32_t* d_counts) {
  ExactModel& m = *h->exact;
  const CommonSide v = common_side(h, side);
  const int64_t n = v.n;
  if (n == 0) return CMS_OK;
  const uint32_t* bits;
  int rc;
  if ((rc = set_bits_matrix(h, side, v, &bits))) return rc;
  if (!bits) {  // no matrix: the posting-list walk over every list, in its own chunks
    std::vector<int64_t> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), int64_t(0));
    return set_top_k(h, measure, side, idx.data(), n, k, d_ids, d_scores, d_counts);
  }
  const int64_t chunk = std::min<int64_t>({slab_rows_for(n), kBitsRowsMax, n});
  CMS_HIP(h->ws_slab.ensure(sizeof(double) * (size_t)(chunk * n)));
  double* slab = h->ws_slab.as<double>();
  const int64_t* col_ids = side == CMS_SIDE_OWNER ? h->d_owner_ids : m.d_ids.as<int64_t>();
  BitsArgs g = bits_args(h, v, side, bits);
  g.nb = n;
  g.out = slab;
  g.ld = n;
  for (int64_t q0 = 0; q0 < n; q0 += chunk) {
    const int64_t qc = std::min(chunk, n - q0);
    g.a0 = q0;
    g.na = qc;
    if ((rc = launch_set_bits(h, measure, g))) return rc;
    std::vector<TopQuery> qs((size_t)qc);
    for (int64_t q = 0; q < qc; ++q) qs[(size_t)q] = TopQuery{q, q0 + q, q0 + q};
    // (launch_top_k synchronises the stream: qs may go)
    if ((rc = launch_top_k(h, slab, qs, k, nullptr, d_ids, d_scores, d_counts, n, col_ids))) return rc;
  }
  return CMS_OK;
}

int set_bits_block(cms_handle* h, int32_t measure, int32_t side, const int64_t* i1, int64_t n1, const int64_t* i2,
                   int64_t n2, double* out) {
  ExactModel& m = *h->exact;
  if (n1 <= 0 || n2 <= 0) return CMS_OK;
  const CommonSide v = common_side(h, side);
  const uint32_t* bits;
  int rc;
  if ((rc = set_bits_matrix(h, side, v, &bits))) return rc;
  if (!bits) return set_pair_call(h, measure, side, i1, n1, i2, n2, true, out);  // k_set_pairs, cross
  if ((rc = upload(h, m.q1, i1, (size_t)n1)) || (rc = upload(h, m.q2, i2, (size_t)n2))) return rc;
  CMS_HIP(m.out.ensure(sizeof(double) * (size_t)(n1 * n2)));
  BitsArgs g = bits_args(h, v, side, bits);
  g.ib = m.q2.as<int64_t>();
  g.nb = n2;
  g.ld = n2;
  for (int64_t r0 = 0; r0 < n1; r0 += kBitsRowsMax) {
    g.ia = m.q1.as<int64_t>() + r0;
    g.na = std::min(kBitsRowsMax, n1 - r0);
    g.out = m.out.as<double>() + r0 * n2;
    if ((rc = launch_set_bits(h, measure, g))) return rc;
  }
  CMS_HIP(hipMemcpyAsync(out, m.out.ptr, sizeof(double) * (size_t)(n1 * n2), hipMemcpyDeviceToHost, h->stream));
  CMS_HIP(hipStreamSynchronize(h->stream));
  return CMS_OK;
}

}  // namespace cms
