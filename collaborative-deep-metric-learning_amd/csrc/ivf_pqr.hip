// Residual product-quantised lists of the IVF index (include/cdml_ivf_pqr.h): the codes describe the
// row minus its list's centroid.  The codebooks are shared by all lists, so the lookup table stays per query
// (cdml_pq_lut, csrc/ivf_pq.hip) and the centroid's share of a score is one scalar per (query, probed list) slot.
// The scan and the any-dsub encoder are the residual instances of the plain form's bodies (csrc/pq_common.h).
//
//   k_pqr_encode     k_pq_encode's launch (one block per (256 rows, subspace), the 256 codewords in LDS, a lane's sub-vector
//                    in registers) with the centroid's sub-vector subtracted as the row's is loaded: the residual matrix is
//                    never in memory.  A lane whose assign is outside [0, nlist) reads no centroid and writes codes 0,
//                    dist +inf.  k_pqr_encode_any (pq_encode_any_body<true>) for a dsub outside {1, 2, 4, 8, 16, 32}.
//   k_ivf_slot_dots  one wave per slot: b(q, c) = <q, C[c]> over Dp columns, lane-strided fmaf chains and a fixed xor fold
//                    (the order is in the header).  grid = (nlist, Y): a list's 4 Y waves take its slots round robin, four
//                    slots of a wave in flight at a time.
//   k_ivf_scan_pqr   pq_scan_body<M8, true>: k_ivf_scan_pq's work item with the accumulator of a slot starting from its base
//                    -- one block-uniform load per slot and tile, one add per (slot, row).
#include <algorithm>

#include "pq_common.h"
#include "../../include/cdml_ivf_pqr.h"

namespace cdml {
namespace {

constexpr int kCw = CDML_PQ_CODEWORDS;

// ---- encode --------------------------------------------------------------------------------------------------------
template <int DS>
__global__ void __launch_bounds__(256)
k_pqr_encode(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cen, int64_t ldcen, int nlist,
             const int64_t *__restrict__ assign, const float *__restrict__ cb, uint8_t *__restrict__ codes, int64_t ldc,
             float *__restrict__ dist, int64_t ldd) {
  __shared__ __attribute__((aligned(16))) float sC[kCw * DS];
  const int t = threadIdx.x, m = blockIdx.y;
  const float *cbm = cb + (int64_t)m * kCw * DS;
#pragma unroll
  for (int i = 0; i < DS; ++i) sC[t + 256 * i] = cbm[t + 256 * i];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + t;
  if (r >= n) return;                          // after the only barrier
  const int64_t a = assign[r];
  float best = __builtin_inff();
  int code = 0;
  if (a >= 0 && a < nlist) {
    float ev[DS];
    const float *xr = x + r * ldx + (int64_t)m * DS;
    const float *cr = cen + a * ldcen + (int64_t)m * DS;
#pragma unroll
    for (int j = 0; j < DS; ++j) ev[j] = xr[j] - cr[j];
    // (nearest_codeword's walk, written out: the helper gives this kernel other machine code than it had -- DESIGN.md 9f.7)
#pragma unroll 4
    for (int c = 0; c < kCw; ++c) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < DS; ++j) {
        const float diff = ev[j] - sC[c * DS + j];
        d = __builtin_fmaf(diff, diff, d);
      }
      if (d < best) { best = d; code = c; }    // ties keep the lower c; a NaN passes nothing
    }
  }
  codes[r * ldc + m] = (uint8_t)code;
  if (dist) dist[r * ldd + m] = best;
}

__global__ void __launch_bounds__(256)
k_pqr_encode_any(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cen, int64_t ldcen, int nlist,
                 const int64_t *__restrict__ assign, const float *__restrict__ cb, int dsub, uint8_t *__restrict__ codes,
                 int64_t ldc, float *__restrict__ dist, int64_t ldd) {
  pq_encode_any_body<true>(x, ldx, n, cen, ldcen, nlist, assign, cb, dsub, codes, ldc, dist, ldd);
}

// ---- the slot scalars ----------------------------------------------------------------------------------------------
constexpr int kDotThreads = 256;              // four waves a block
constexpr int kDotSlots = 4;                  // slots a wave has in flight: their loads are independent
constexpr int kDotYMax = 16;                  // at most 16 blocks (64 waves) a list

// grid = (nlist, Y): the 4 Y waves of a list take its slots round robin, kDotSlots at a time.  Which wave computes a slot
// changes nothing of its bits: the order of the sum is the lane-strided one of the header for every slot.
__global__ void __launch_bounds__(kDotThreads)
k_ivf_slot_dots(const float *__restrict__ Q, int64_t ldq, int n_queries, const float *__restrict__ cen, int64_t ldcen, int Dp,
                const int32_t *__restrict__ slot_query, const int32_t *__restrict__ slot_start, float *__restrict__ slot_base) {
  const int c = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.y * (kDotThreads / 64) + (threadIdx.x >> 6));   // scalar: slot loads are s_loads
  const int stride = gridDim.y * (kDotThreads / 64);
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const float *cr = cen + (int64_t)c * ldcen;
  for (int i = wave; i < nq_c; i += kDotSlots * stride) {            // wave-uniform; no barrier in this kernel
    const float *qr[kDotSlots];
    float p[kDotSlots];
#pragma unroll
    for (int u = 0; u < kDotSlots; ++u) {
      const int iu = i + u * stride;                                 // a slot past the list's end reads slot i again, stores nothing
      const int q = min(max(slot_query[s0 + (iu < nq_c ? iu : i)], 0), n_queries - 1);
      qr[u] = Q + (int64_t)q * ldq;
      p[u] = 0.f;
    }
    for (int j = lane; j < Dp; j += 64) {
      const float cv = cr[j];
#pragma unroll
      for (int u = 0; u < kDotSlots; ++u) p[u] = __builtin_fmaf(qr[u][j], cv, p[u]);
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1)
#pragma unroll
      for (int u = 0; u < kDotSlots; ++u) p[u] = p[u] + __shfl_xor(p[u], w, 64);
#pragma unroll
    for (int u = 0; u < kDotSlots; ++u) {
      const int iu = i + u * stride;
      if (lane == 0 && iu < nq_c) slot_base[s0 + iu] = p[u];
    }
  }
}

template <int M8>
__global__ void __launch_bounds__(kScanThreads)
k_ivf_scan_pqr(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
               const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off, const float *__restrict__ slot_base,
               const uint8_t *__restrict__ codes, int64_t ldc, const int32_t *__restrict__ list_start,
               const int4 *__restrict__ tiles, float *__restrict__ scores) {
  pq_scan_body<M8, true>(lut, n_queries, slot_query, slot_start, slot_off, slot_base, codes, ldc, list_start, tiles, scores);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_pqr_encode(const float *x, int64_t ldx, int64_t n, const float *centroids, int64_t ldcen, int nlist,
                               const int64_t *assign, const float *codebooks, int M, int dsub, uint8_t *codes, int64_t ldc,
                               float *dist, int64_t ldd, cdml_stream_t stream) {
  if (int rc = check_pq_encode_args(
          "pqr_encode", x && centroids && assign && codebooks && codes, n, nlist, M, dsub,
          ldx >= (int64_t)M * dsub && ldcen >= (int64_t)M * dsub && ldc >= M && (!dist || ldd >= M),
          "ldx >= M dsub, ldcen >= M dsub, ldc >= M and ldd >= M"))
    return rc;
  const dim3 grid((unsigned)((n + 255) / 256), M);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dsub(
      dsub,
      [&](auto ds) {
        hipLaunchKernelGGL(k_pqr_encode<decltype(ds)::value>, grid, dim3(256), 0, st, x, ldx, n, centroids, ldcen, nlist, assign,
                           codebooks, codes, ldc, dist, ldd);
      },
      [&] {
        hipLaunchKernelGGL(k_pqr_encode_any, grid, dim3(256), 0, st, x, ldx, n, centroids, ldcen, nlist, assign, codebooks, dsub,
                           codes, ldc, dist, ldd);
      });
  return check_launch("pqr_encode");
}

extern "C" int cdml_ivf_slot_dots(const float *Q, int64_t ldq, int n_queries, const float *centroids, int64_t ldcen, int Dp,
                                  const int32_t *slot_query, const int32_t *slot_start, int nlist, float *slot_base,
                                  cdml_stream_t stream) {
  CDML_REQUIRE(Q && centroids && slot_query && slot_start && slot_base, CDML_E_BADARG, "ivf_slot_dots: null pointer");
  CDML_REQUIRE(n_queries > 0 && Dp >= 1, CDML_E_BADARG, "ivf_slot_dots: bad size");
  CDML_REQUIRE(nlist >= 1, CDML_E_BADARG, "ivf_slot_dots: nlist must be >= 1, got %d", nlist);
  CDML_REQUIRE(ldq >= Dp && ldcen >= Dp, CDML_E_BADARG, "ivf_slot_dots: ldq >= Dp and ldcen >= Dp (Dp = %d)", Dp);
  // blocks a list: enough waves for the slots a list gets when every query probes it once, between 1 and kDotYMax
  const int y = (int)std::min<int64_t>(kDotYMax, std::max<int64_t>(1, ((int64_t)n_queries + nlist - 1) / nlist));
  hipLaunchKernelGGL(k_ivf_slot_dots, dim3(nlist, y), dim3(kDotThreads), 0, (hipStream_t)stream, Q, ldq, n_queries,
                     centroids, ldcen, Dp, slot_query, slot_start, slot_base);
  return check_launch("ivf_slot_dots");
}

extern "C" int cdml_ivf_scan_pqr(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                                 const int64_t *slot_off, const float *slot_base, const uint8_t *codes, int64_t ldc,
                                 const int32_t *list_start, int M, const int32_t *tiles, int n_tiles, float *scores,
                                 cdml_stream_t stream) {
  if (int rc = check_pq_scan_args(
          "ivf_scan_pqr", lut && slot_query && slot_start && slot_off && slot_base && codes && list_start && tiles && scores, lut,
          n_queries, codes, ldc, M, tiles, n_tiles, scores))
    return rc;
  const int4 *tl = reinterpret_cast<const int4 *>(tiles);
  hipStream_t st = (hipStream_t)stream;
  dispatch_m8(M, [&](auto m8) {
    hipLaunchKernelGGL(k_ivf_scan_pqr<decltype(m8)::value>, dim3(n_tiles), dim3(kScanThreads), 0, st, lut, n_queries, slot_query,
                       slot_start, slot_off, slot_base, codes, ldc, list_start, tl, scores);
  });
  return check_launch("ivf_scan_pqr");
}
