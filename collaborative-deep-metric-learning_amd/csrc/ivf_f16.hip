// fp16 lists of the IVF index and the exact fp32 re-rank (include/cdml_ivf_f16.h).  The index of
// csrc/ivf.hip keeps its lists as fp32 rows and scans them on v_mfma_f32_32x32x2_f32; this file holds the two launches of
// the compressed form:
//
//   k_ivf_scan_f16  k_ivf_scan's grouped (ragged) score product with fp16 operands on v_mfma_f32_32x32x16_f16: the same work
//                   item (list, 128-slot tile, 128-row tile), the same slot / offset tables and score buffer, the same
//                   clamped loads and guarded stores, plain 64-bit addressing.  2 x 2 waves of 64 x 64, K-tiles of 32
//                   halves through LDS (rows 80 B apart: the 16-B fragment reads of a 16-lane group fall on 16 different
//                   16-B slots of the 256-B bank row), the next K-tile's global loads under this tile's MFMAs.
//   k_ivf_refine    one wave per query: the direct form d = sum_j (q_j - x_j)^2 in fp32 of the first r candidates of the
//                   merge's list against fp32 catalogue rows gathered by id, then the bitonic keeper over the r keys (d, id).
// The list-keeping device functions are one more copy of knn.hip's (csrc/ivf.hip and csrc/knn.hip keep their instructions).
#include "common.h"
#include "../../include/cdml_ivf_f16.h"

namespace cdml {
namespace {

constexpr int kListCap = CDML_KNN_LIST;   // entries per query list (k <= r <= kListCap)
constexpr int kRowsPerBlock = 4;          // one wave per query
constexpr int kNoId = 0x7fffffff;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- the grouped score product, fp16 operands --------------------------------------------------------------------------
constexpr int kTile = 128;                // slots x rows per work item (knn.IVF_TILE)
constexpr int kBK = 32;                   // K-tile depth in halves: 64 B of a row, two MFMA k-steps of 16
constexpr int kLdS = kBK + 8;             // LDS row stride in halves: 80 B = five 16-B slots, odd, so rows r and r' of one
//                                           ds_read_b128 lane group (16 rows, distinct mod 16) never share a slot

__global__ void __launch_bounds__(256)
k_ivf_scan_f16(const _Float16 *__restrict__ Q, int64_t ldq, int n_queries, const int32_t *__restrict__ slot_query,
               const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off,
               const _Float16 *__restrict__ rows, int64_t ldr, const int32_t *__restrict__ list_start, int Dp,
               const int4 *__restrict__ tiles, float *__restrict__ scores) {
  __shared__ __attribute__((aligned(16))) _Float16 sA[kTile * kLdS];
  __shared__ __attribute__((aligned(16))) _Float16 sB[kTile * kLdS];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;

  const int4 tl = tiles[blockIdx.x];
  const int c = tl.x, i0 = tl.y, j0 = tl.z;
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const int r0 = list_start[c], len = list_start[c + 1] - r0;
  if (i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len) return;    // block-uniform, before any barrier
  const int ld_c = (len + 3) & ~3;

  // loader: thread t moves chunk t & 3 (16 B = 8 halves) of tile rows (t >> 2) + 64 j; a row past the end is the last valid one
  const int chunk = t & 3, lrow = t >> 2;
  const _Float16 *pa[2], *pb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ra = min(i0 + lrow + 64 * j, nq_c - 1);
    const int q = min(max(slot_query[s0 + ra], 0), n_queries - 1);
    pa[j] = Q + (int64_t)q * ldq + 8 * chunk;
    const int rb = min(j0 + lrow + 64 * j, len - 1);
    pb[j] = rows + (int64_t)(r0 + rb) * ldr + 8 * chunk;
  }
  f16x8 ga[2], gb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    ga[j] = *reinterpret_cast<const f16x8 *>(pa[j]);
    gb[j] = *reinterpret_cast<const f16x8 *>(pb[j]);
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int n_ktiles = Dp / kBK;
  for (int kt = 0; kt < n_ktiles; ++kt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<f16x8 *>(sA + (lrow + 64 * j) * kLdS + 8 * chunk) = ga[j];
      *reinterpret_cast<f16x8 *>(sB + (lrow + 64 * j) * kLdS + 8 * chunk) = gb[j];
    }
    __syncthreads();
    if (kt + 1 < n_ktiles) {                   // the next K-tile's rows travel under this one's MFMAs
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ga[j] = *reinterpret_cast<const f16x8 *>(pa[j] + (kt + 1) * kBK);
        gb[j] = *reinterpret_cast<const f16x8 *>(pb[j] + (kt + 1) * kBK);
      }
    }
    // k-step ks = 16 k values; a lane's fragment is A[row lane & 31][k = 16 ks + 8 (lane >> 5) + j], j < 8, and B alike
#pragma unroll
    for (int ks = 0; ks < kBK / 16; ++ks) {
      f16x8 fa[2], fb[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        fa[mi] = *reinterpret_cast<const f16x8 *>(sA + (wm * 64 + mi * 32 + l31) * kLdS + 16 * ks + 8 * h);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        fb[ni] = *reinterpret_cast<const f16x8 *>(sB + (wn * 64 + ni * 32 + l31) * kLdS + 16 * ks + 8 * h);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();                           // the stage is free again
  }

  // C/D layout: column = lane & 31 (a list row), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (a slot)
  float *blk = scores + slot_off[s0];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int j = j0 + wn * 64 + ni * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i < nq_c && j < len) blk[(int64_t)i * ld_c + j] = acc[mi][ni][r];
      }
    }
}

// ---- the list keeper (csrc/knn.hip's, over kListCap keys) ------------------------------------------------------------------
__device__ __forceinline__ bool key_less(float d1, int i1, float d2, int i2) {
  return d1 < d2 || (d1 == d2 && i1 < i2);
}

// In-place bitonic sort of the wave's kListCap (d, id) keys in LDS, ascending.  All 64 lanes of ONE wave take part; LDS
// operations of a wave retire in order, so the only fence needed between passes is against compiler reordering.
__device__ __forceinline__ void sort_buffer(float *kd, int *ki, int lane) {
#pragma unroll 1
  for (int size = 2; size <= kListCap; size <<= 1) {
#pragma unroll 1
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int t = 0; t < kListCap / 128; ++t) {
        const int p = lane + 64 * t;
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int j = i + stride;
        const bool up = (i & size) == 0;
        const float di = kd[i], dj = kd[j];
        const int ii = ki[i], ij = ki[j];
        if (key_less(dj, ij, di, ii) == up) {
          kd[i] = dj; ki[i] = ij;
          kd[j] = di; ki[j] = ii;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- the exact re-rank -------------------------------------------------------------------------------------------------
constexpr int kCandStep = 4;              // candidates in flight per wave: their row loads are issued together

__global__ void __launch_bounds__(256)
k_ivf_refine(const float *__restrict__ Q, int64_t ldq, int nq, const float *__restrict__ base, int64_t ldb, int64_t n_rows,
             int Dp, const int32_t *__restrict__ cand, int r, float *__restrict__ best_d, int *__restrict__ best_i) {
  __shared__ float s_d[kRowsPerBlock][kListCap];
  __shared__ int s_i[kRowsPerBlock][kListCap];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerBlock + w;
  if (row >= nq) return;                       // whole wave leaves; no block barrier below
  float *kd = s_d[w];
  int *ki = s_i[w];
  const float inf = __builtin_inff();
#pragma unroll
  for (int t = 0; t < kListCap / 64; ++t) {
    kd[lane + 64 * t] = inf;
    ki[lane + 64 * t] = kNoId;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  const float *q = Q + (int64_t)row * ldq;
  const int32_t *cr = cand + (int64_t)row * kListCap;
  for (int c0 = 0; c0 < r; c0 += kCandStep) {  // wave-uniform
    int id[kCandStep];
    const float *x[kCandStep];
    float acc[kCandStep];
#pragma unroll
    for (int u = 0; u < kCandStep; ++u) {
      const int v = c0 + u < r ? cr[c0 + u] : kNoId;           // wave-uniform
      id[u] = (v >= 0 && (int64_t)v < n_rows) ? v : kNoId;     // no candidate (or no such row): row 0 is read and dropped
      x[u] = base + (id[u] == kNoId ? (int64_t)0 : (int64_t)id[u] * ldb);
      acc[u] = 0.f;
    }
    for (int j = lane; j < Dp; j += 64) {      // lane l: coordinates l, l + 64, ... in ascending order
      const float qj = q[j];
#pragma unroll
      for (int u = 0; u < kCandStep; ++u) {
        const float e = qj - x[u][j];
        acc[u] = __builtin_fmaf(e, e, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kCandStep; ++u) {
      float d = acc[u];
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) d += __shfl_xor(d, m, 64);   // the fixed butterfly: every lane ends with the same bits
      if (id[u] != kNoId && d == d && lane == 0) {             // a NaN distance passes no compare: it is no candidate
        kd[c0 + u] = d;
        ki[c0 + u] = id[u];
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  sort_buffer(kd, ki, lane);
  float *bd = best_d + (int64_t)row * kListCap;
  int *bi = best_i + (int64_t)row * kListCap;
#pragma unroll
  for (int t = 0; t < kListCap / 64; ++t) {
    const int p = lane + 64 * t;
    bd[p] = kd[p];
    bi[p] = ki[p];
  }
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_ivf_scan_f16(const uint16_t *Q, int64_t ldq, int n_queries, const int32_t *slot_query,
                                 const int32_t *slot_start, const int64_t *slot_off, const uint16_t *rows, int64_t ldr,
                                 const int32_t *list_start, int Dp, const int32_t *tiles, int n_tiles, float *scores,
                                 cdml_stream_t stream) {
  CDML_REQUIRE(Q && slot_query && slot_start && slot_off && rows && list_start && tiles && scores, CDML_E_BADARG,
               "ivf_scan_f16: null pointer");
  CDML_REQUIRE(n_queries > 0 && n_tiles > 0 && Dp > 0, CDML_E_BADARG, "ivf_scan_f16: bad size");
  CDML_REQUIRE(Dp % 32 == 0, CDML_E_UNSUPPORTED, "ivf_scan_f16: Dp must be a multiple of 32, got %d", Dp);
  CDML_REQUIRE(!(ldq & 7) && !(ldr & 7) && ldq >= Dp && ldr >= Dp && aligned16(Q) && aligned16(rows) && aligned16(tiles) &&
                   aligned16(scores),
               CDML_E_ALIGN, "ivf_scan_f16: strides multiples of 8 halves and >= Dp, bases 16-B aligned");
  hipLaunchKernelGGL(k_ivf_scan_f16, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const _Float16 *>(Q),
                     ldq, n_queries, slot_query, slot_start, slot_off, reinterpret_cast<const _Float16 *>(rows), ldr,
                     list_start, Dp, reinterpret_cast<const int4 *>(tiles), scores);
  return check_launch("ivf_scan_f16");
}

extern "C" int cdml_ivf_refine(const float *Q, int64_t ldq, int nq, const float *base, int64_t ldb, int64_t n_rows, int Dp,
                               const int32_t *cand, int r, int k, float *best_d, int32_t *best_i, cdml_stream_t stream) {
  CDML_REQUIRE(Q && base && cand && best_d && best_i, CDML_E_BADARG, "ivf_refine: null pointer");
  CDML_REQUIRE(nq > 0 && n_rows > 0 && Dp > 0 && ldq >= Dp && ldb >= Dp, CDML_E_BADARG,
               "ivf_refine: bad size (nq, n_rows and Dp positive, ldq and ldb >= Dp)");
  CDML_REQUIRE(k >= 1 && k <= r && r <= kListCap, CDML_E_UNSUPPORTED, "ivf_refine: 1 <= k <= r <= %d required, got k = %d, r = %d",
               kListCap, k, r);
  hipLaunchKernelGGL(k_ivf_refine, dim3((nq + kRowsPerBlock - 1) / kRowsPerBlock), dim3(256), 0, (hipStream_t)stream, Q, ldq, nq,
                     base, ldb, n_rows, Dp, cand, r, best_d, best_i);
  return check_launch("ivf_refine");
}
