// The threshold-filter scan of the IVF index (include/cdml_ivf_filter.h): the grouped score product
// of csrc/ivf.hip / csrc/ivf_f16.hip with no score buffer.  Every query of the chunk already has a keep-th best distance tau
// from its seed lists (the buffered launches); a tile of this scan writes none of its 128 x 128 products and appends the few
// elements with d <= tau[query] to the query's candidate list (atomic slot counter, integer atomics only), which
// cdml_knn_merge_list (csrc/knn.hip) folds into the query's sorted list.
//
//   k_ivf_filter_f32  k_ivf_scan's tile loop to the letter (work item = tiles[blockIdx.x], clamped loads, 2 x 2 waves of
//                     64 x 64, K-tiles of 32 through LDS, the same MFMA order on v_mfma_f32_32x32x2_f32): the bits of a
//                     (query, row) product are those of the buffered scan.
//   k_ivf_filter_f16  k_ivf_scan_f16's tile loop to the letter on v_mfma_f32_32x32x16_f16.
// Both end in one epilogue (filter_epilogue): d exactly as k_ivf_merge forms it, (q_sq + r_sq) - 2 s clamped at 0 by a compare
// that keeps a NaN (2 s is exact, so contracting the subtraction into an FMA changes no bit).  The tile's 128 slots' (query,
// q_sq, tau) are staged in LDS once by the first two waves -- in arrays of their own, written before the K loop, whose
// barriers publish them: no extra barrier, and the operand stage is not re-typed -- a slot past the list's block gets tau = -1,
// which no clamped distance passes.  A lane loads r_sq / ids of its column once per 32-column block.
#include "common.h"
#include "../../include/cdml_ivf_filter.h"

namespace cdml {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kTile = 128;                // slots x rows per work item (knn.IVF_TILE)
constexpr int kBK = 32;                   // K-tile depth, both forms

struct FilterArgs {
  const float *q_sq, *tau;                // per query of the chunk
  int32_t *cnt;                           // per query of the chunk: candidates appended so far (dropped ones included)
  const float *r_sq;                      // per listed row
  const int32_t *ids;                     // per listed row
  uint2 *cand;                            // [n_queries][cap] (bits of d, id)
  int cap;
};

// thread t < 128 stages slot i0 + t of the list's block; the K loop's barriers publish the three arrays
__device__ __forceinline__ void stage_slots(int t, int i0, int nq_c, int s0, int n_queries, const int32_t *__restrict__ slot_query,
                                            const FilterArgs &f, int *sQ, float *sQs, float *sTau) {
  if (t < kTile) {
    const bool in = i0 + t < nq_c;
    const int q = min(max(slot_query[s0 + min(i0 + t, nq_c - 1)], 0), n_queries - 1);
    sQ[t] = q;
    sQs[t] = f.q_sq[q];
    sTau[t] = in ? f.tau[q] : -1.f;       // d >= 0 or NaN: a slot past the block's end appends nothing
  }
}

// C/D layout: column = lane & 31 (a list row), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (a slot)
__device__ __forceinline__ void filter_epilogue(const f32x16 (&acc)[2][2], int wm, int wn, int l31, int h, int r0, int j0, int len,
                                                const FilterArgs &f, const int *sQ, const float *sQs, const float *sTau) {
  float rs[2];
  int id[2];
  bool col_in[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int j = j0 + wn * 64 + ni * 32 + l31;
    col_in[ni] = j < len;
    const int row = r0 + min(j, len - 1);                    // clamped as the loads are: a valid listed row
    rs[ni] = f.r_sq[row];
    id[ni] = f.ids[row];
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int ib = wm * 64 + mi * 32 + 4 * h;                // tile-local slot of register 0
#pragma unroll
    for (int g = 0; g < 4; ++g) {                            // registers 4 g .. 4 g + 3 = slots ib + 8 g .. + 3
      const f32x4 qs = *reinterpret_cast<const f32x4 *>(sQs + ib + 8 * g);
      const f32x4 tau = *reinterpret_cast<const f32x4 *>(sTau + ib + 8 * g);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dr = (qs[e] + rs[ni]) - 2.f * acc[mi][ni][4 * g + e];
          const float d = dr < 0.f ? 0.f : dr;               // the clamp keeps a NaN; NaN never passes
          if (d <= tau[e] && col_in[ni]) {                   // rare
            const int q = sQ[ib + 8 * g + e];
            const int pos = atomicAdd(f.cnt + q, 1);
            if ((unsigned)pos < (unsigned)f.cap) f.cand[(int64_t)q * f.cap + pos] = make_uint2(__float_as_uint(d), (uint32_t)id[ni]);
          }
        }
    }
  }
}

// ---- fp32 lists: k_ivf_scan's tile loop -------------------------------------------------------------------------------
constexpr int kLdS32 = kBK + 4;           // LDS row stride in floats: 16-B aligned rows, 144 B apart

__global__ void __launch_bounds__(256)
k_ivf_filter_f32(const float *__restrict__ Q, int64_t ldq, int n_queries, const int32_t *__restrict__ slot_query,
                 const int32_t *__restrict__ slot_start, const float *__restrict__ rows, int64_t ldr,
                 const int32_t *__restrict__ list_start, int Dp, const int4 *__restrict__ tiles, FilterArgs f) {
  __shared__ __attribute__((aligned(16))) float sA[kTile * kLdS32];
  __shared__ __attribute__((aligned(16))) float sB[kTile * kLdS32];
  __shared__ __attribute__((aligned(16))) float sQs[kTile];
  __shared__ __attribute__((aligned(16))) float sTau[kTile];
  __shared__ int sQ[kTile];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;

  const int4 tl = tiles[blockIdx.x];
  const int c = tl.x, i0 = tl.y, j0 = tl.z;
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const int r0 = list_start[c], len = list_start[c + 1] - r0;
  if (i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len) return;    // block-uniform, before any barrier

  // loader: thread t moves chunk t & 7 (16 B) of tile rows (t >> 3) + 32 j; a row past the end is the last valid one
  const int chunk = t & 7, lrow = t >> 3;
  const float *pa[4], *pb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ra = min(i0 + lrow + 32 * j, nq_c - 1);
    const int q = min(max(slot_query[s0 + ra], 0), n_queries - 1);
    pa[j] = Q + (int64_t)q * ldq + 4 * chunk;
    const int rb = min(j0 + lrow + 32 * j, len - 1);
    pb[j] = rows + (int64_t)(r0 + rb) * ldr + 4 * chunk;
  }
  f32x4 ga[4], gb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ga[j] = *reinterpret_cast<const f32x4 *>(pa[j]);
    gb[j] = *reinterpret_cast<const f32x4 *>(pb[j]);
  }
  stage_slots(t, i0, nq_c, s0, n_queries, slot_query, f, sQ, sQs, sTau);

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
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<f32x4 *>(sA + (lrow + 32 * j) * kLdS32 + 4 * chunk) = ga[j];
      *reinterpret_cast<f32x4 *>(sB + (lrow + 32 * j) * kLdS32 + 4 * chunk) = gb[j];
    }
    __syncthreads();
    if (kt + 1 < n_ktiles) {                   // the next K-tile's rows travel under this one's MFMAs
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ga[j] = *reinterpret_cast<const f32x4 *>(pa[j] + (kt + 1) * kBK);
        gb[j] = *reinterpret_cast<const f32x4 *>(pb[j] + (kt + 1) * kBK);
      }
    }
    // k-group grp = 8 k values; lane half h owns 4 of them: MFMA u multiplies k = 8 grp + u and 8 grp + 4 + u
#pragma unroll
    for (int grp = 0; grp < kBK / 8; ++grp) {
      f32x4 fa[2], fb[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        fa[mi] = *reinterpret_cast<const f32x4 *>(sA + (wm * 64 + mi * 32 + l31) * kLdS32 + 8 * grp + 4 * h);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        fb[ni] = *reinterpret_cast<const f32x4 *>(sB + (wn * 64 + ni * 32 + l31) * kLdS32 + 8 * grp + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][u], fb[ni][u], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();                           // the stage is free again
  }
  filter_epilogue(acc, wm, wn, l31, h, r0, j0, len, f, sQ, sQs, sTau);
}

// ---- fp16 lists: k_ivf_scan_f16's tile loop -----------------------------------------------------------------------------
constexpr int kLdS16 = kBK + 8;           // LDS row stride in halves: 80 B = five 16-B slots (csrc/ivf_f16.hip)

// (four waves per SIMD, as k_ivf_scan_f16 runs: without the bound the epilogue's registers take the kernel to 82 + 64 and three)
__global__ void __launch_bounds__(256, 4)
k_ivf_filter_f16(const _Float16 *__restrict__ Q, int64_t ldq, int n_queries, const int32_t *__restrict__ slot_query,
                 const int32_t *__restrict__ slot_start, const _Float16 *__restrict__ rows, int64_t ldr,
                 const int32_t *__restrict__ list_start, int Dp, const int4 *__restrict__ tiles, FilterArgs f) {
  __shared__ __attribute__((aligned(16))) _Float16 sA[kTile * kLdS16];
  __shared__ __attribute__((aligned(16))) _Float16 sB[kTile * kLdS16];
  __shared__ __attribute__((aligned(16))) float sQs[kTile];
  __shared__ __attribute__((aligned(16))) float sTau[kTile];
  __shared__ int sQ[kTile];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;

  const int4 tl = tiles[blockIdx.x];
  const int c = tl.x, i0 = tl.y, j0 = tl.z;
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const int r0 = list_start[c], len = list_start[c + 1] - r0;
  if (i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len) return;    // block-uniform, before any barrier

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
  stage_slots(t, i0, nq_c, s0, n_queries, slot_query, f, sQ, sQs, sTau);

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
      *reinterpret_cast<f16x8 *>(sA + (lrow + 64 * j) * kLdS16 + 8 * chunk) = ga[j];
      *reinterpret_cast<f16x8 *>(sB + (lrow + 64 * j) * kLdS16 + 8 * chunk) = gb[j];
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
        fa[mi] = *reinterpret_cast<const f16x8 *>(sA + (wm * 64 + mi * 32 + l31) * kLdS16 + 16 * ks + 8 * h);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        fb[ni] = *reinterpret_cast<const f16x8 *>(sB + (wn * 64 + ni * 32 + l31) * kLdS16 + 16 * ks + 8 * h);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();                           // the stage is free again
  }
  filter_epilogue(acc, wm, wn, l31, h, r0, j0, len, f, sQ, sQs, sTau);
}

// the argument checks of both launches; `name` is the launch's own
int check_filter_args(const char *name, const void *Q, int64_t ldq, int n_queries, const void *slot_query, const void *slot_start,
                      const void *q_sq, const void *tau, const void *cnt, const void *rows, int64_t ldr, const void *list_start,
                      const void *r_sq, const void *ids, int Dp, const void *tiles, int n_tiles, const void *cand, int cap,
                      int stride_unit) {
  CDML_REQUIRE(Q && slot_query && slot_start && q_sq && tau && cnt && rows && list_start && r_sq && ids && tiles && cand,
               CDML_E_BADARG, "%s: null pointer", name);
  CDML_REQUIRE(n_queries > 0 && n_tiles > 0 && Dp > 0, CDML_E_BADARG, "%s: bad size", name);
  CDML_REQUIRE(Dp % 32 == 0, CDML_E_UNSUPPORTED, "%s: Dp must be a multiple of 32, got %d", name, Dp);
  CDML_REQUIRE(cap > 0 && !(cap & (cap - 1)), CDML_E_UNSUPPORTED, "%s: cap must be a positive power of two, got %d", name, cap);
  CDML_REQUIRE(!(ldq % stride_unit) && !(ldr % stride_unit) && ldq >= Dp && ldr >= Dp && aligned16(Q) && aligned16(rows) &&
                   aligned16(tiles) && (reinterpret_cast<uintptr_t>(cand) & 7) == 0,
               CDML_E_ALIGN, "%s: strides multiples of %d and >= Dp, Q, rows and tiles 16-B aligned, cand 8-B aligned", name,
               stride_unit);
  return CDML_OK;
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_ivf_filter_f32(const float *Q, int64_t ldq, int n_queries, const int32_t *slot_query,
                                   const int32_t *slot_start, const float *q_sq, const float *tau, int32_t *cnt,
                                   const float *rows, int64_t ldr, const int32_t *list_start, const float *r_sq,
                                   const int32_t *ids, int Dp, const int32_t *tiles, int n_tiles, void *cand, int cap,
                                   cdml_stream_t stream) {
  const int rc = check_filter_args("ivf_filter_f32", Q, ldq, n_queries, slot_query, slot_start, q_sq, tau, cnt, rows, ldr,
                                   list_start, r_sq, ids, Dp, tiles, n_tiles, cand, cap, 4);
  if (rc != CDML_OK) return rc;
  const FilterArgs f{q_sq, tau, cnt, r_sq, ids, reinterpret_cast<uint2 *>(cand), cap};
  hipLaunchKernelGGL(k_ivf_filter_f32, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, Q, ldq, n_queries, slot_query, slot_start,
                     rows, ldr, list_start, Dp, reinterpret_cast<const int4 *>(tiles), f);
  return check_launch("ivf_filter_f32");
}

extern "C" int cdml_ivf_filter_f16(const uint16_t *Q, int64_t ldq, int n_queries, const int32_t *slot_query,
                                   const int32_t *slot_start, const float *q_sq, const float *tau, int32_t *cnt,
                                   const uint16_t *rows, int64_t ldr, const int32_t *list_start, const float *r_sq,
                                   const int32_t *ids, int Dp, const int32_t *tiles, int n_tiles, void *cand, int cap,
                                   cdml_stream_t stream) {
  const int rc = check_filter_args("ivf_filter_f16", Q, ldq, n_queries, slot_query, slot_start, q_sq, tau, cnt, rows, ldr,
                                   list_start, r_sq, ids, Dp, tiles, n_tiles, cand, cap, 8);
  if (rc != CDML_OK) return rc;
  const FilterArgs f{q_sq, tau, cnt, r_sq, ids, reinterpret_cast<uint2 *>(cand), cap};
  hipLaunchKernelGGL(k_ivf_filter_f16, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const _Float16 *>(Q),
                     ldq, n_queries, slot_query, slot_start, reinterpret_cast<const _Float16 *>(rows), ldr, list_start, Dp,
                     reinterpret_cast<const int4 *>(tiles), f);
  return check_launch("ivf_filter_f16");
}
