// Product-quantised lists of the IVF index (include/cdml_ivf_pq.h): M bytes per listed row instead
// of the row.  Plain (non-residual) PQ: one set of codebooks [M][256][dsub] for the catalogue, one lookup table per query.
// What the residual and the 4-bit form share with this one is in csrc/pq_common.h (DESIGN.md section 9f.7 says which kernel
// uses what, and why the others keep their own text).
//
//   k_pq_encode      one block per (256 rows, subspace): the subspace's 256 codewords in LDS, a lane owns one row's
//                    sub-vector in registers and walks the codewords in order (nearest_codeword) -- every lane reads the same
//                    LDS address (a broadcast, conflict-free).  dsub is a template parameter for {1, 2, 4, 8, 16, 32};
//                    k_pq_encode_any (pq_encode_any_body<false>) reads both operands from memory for any other dsub (the
//                    same sums in the same order).
//   k_pq_lut         LUT[q][m][c] = <q_m, cb[m][c]>: one block per (64 queries, subspace), thread c keeps codeword c in
//                    registers (the same dsub set; k_pq_lut_any = pq_lut_any_body<256> otherwise), the query's sub-vector is
//                    block-uniform.  The launch is bound by its nq x M KiB of stores.
//   k_ivf_scan_pq    pq_scan_body<M8, false>: the ADC scan, sums in ascending m from the first term.
#include "pq_common.h"

namespace cdml {
namespace {

constexpr int kCw = CDML_PQ_CODEWORDS;

template <int DS>
__global__ void __launch_bounds__(256)
k_pq_encode(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cb, uint8_t *__restrict__ codes,
            int64_t ldc, float *__restrict__ dist, int64_t ldd) {
  __shared__ __attribute__((aligned(16))) float sC[kCw * DS];
  const int t = threadIdx.x, m = blockIdx.y;
  const float *cbm = cb + (int64_t)m * kCw * DS;
#pragma unroll
  for (int i = 0; i < DS; ++i) sC[t + 256 * i] = cbm[t + 256 * i];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + t;
  if (r >= n) return;                          // after the only barrier
  float xv[DS];
  const float *xr = x + r * ldx + (int64_t)m * DS;
#pragma unroll
  for (int j = 0; j < DS; ++j) xv[j] = xr[j];
  const Nearest nn = nearest_codeword<kCw, DS>(xv, sC);
  codes[r * ldc + m] = (uint8_t)nn.code;
  if (dist) dist[r * ldd + m] = nn.dist;
}

__global__ void __launch_bounds__(256)
k_pq_encode_any(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cb, int dsub,
                uint8_t *__restrict__ codes, int64_t ldc, float *__restrict__ dist, int64_t ldd) {
  pq_encode_any_body<false>(x, ldx, n, nullptr, 0, 0, nullptr, cb, dsub, codes, ldc, dist, ldd);
}

template <int DS>
__global__ void __launch_bounds__(256)
k_pq_lut(const float *__restrict__ Q, int64_t ldq, int nq, const float *__restrict__ cb, int M, float *__restrict__ lut) {
  const int c = threadIdx.x, m = blockIdx.y;
  const float *src = cb + ((int64_t)m * kCw + c) * DS;
  float cw[DS];
#pragma unroll
  for (int j = 0; j < DS; ++j) cw[j] = src[j];
  const int q1 = min(nq, ((int)blockIdx.x + 1) * kLutQ);
  for (int q = blockIdx.x * kLutQ; q < q1; ++q) {
    const float *qm = Q + (int64_t)q * ldq + (int64_t)m * DS;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < DS; ++j) acc = __builtin_fmaf(qm[j], cw[j], acc);
    lut[((int64_t)q * M + m) * kCw + c] = acc;
  }
}

__global__ void __launch_bounds__(256)
k_pq_lut_any(const float *__restrict__ Q, int64_t ldq, int nq, const float *__restrict__ cb, int M, int dsub,
         float *__restrict__ lut) {
  pq_lut_any_body<kCw, int>(Q, ldq, nq, cb, M, dsub, lut);
}

template <int M8>
__global__ void __launch_bounds__(kScanThreads)
k_ivf_scan_pq(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
              const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off, const uint8_t *__restrict__ codes,
              int64_t ldc, const int32_t *__restrict__ list_start, const int4 *__restrict__ tiles, float *__restrict__ scores) {
  pq_scan_body<M8, false>(lut, n_queries, slot_query, slot_start, slot_off, nullptr, codes, ldc, list_start, tiles, scores);
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_pq_encode(const float *x, int64_t ldx, int64_t n, const float *codebooks, int M, int dsub, uint8_t *codes,
                              int64_t ldc, float *dist, int64_t ldd, cdml_stream_t stream) {
  if (int rc = check_pq_encode_args("pq_encode", x && codebooks && codes, n, 1, M, dsub,
                                    ldx >= (int64_t)M * dsub && ldc >= M && (!dist || ldd >= M),
                                    "ldx >= M dsub, ldc >= M and ldd >= M"))
    return rc;
  const dim3 grid((unsigned)((n + 255) / 256), M);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dsub(
      dsub,
      [&](auto ds) {
        hipLaunchKernelGGL(k_pq_encode<decltype(ds)::value>, grid, dim3(256), 0, st, x, ldx, n, codebooks, codes, ldc, dist, ldd);
      },
      [&] { hipLaunchKernelGGL(k_pq_encode_any, grid, dim3(256), 0, st, x, ldx, n, codebooks, dsub, codes, ldc, dist, ldd); });
  return check_launch("pq_encode");
}

extern "C" int cdml_pq_lut(const float *Q, int64_t ldq, int nq, const float *codebooks, int M, int dsub, float *lut,
                           cdml_stream_t stream) {
  CDML_REQUIRE(Q && codebooks && lut, CDML_E_BADARG, "pq_lut: null pointer");
  CDML_REQUIRE(nq > 0, CDML_E_BADARG, "pq_lut: nq must be positive");
  CDML_REQUIRE_PQ_M("pq_lut", M);
  CDML_REQUIRE(dsub >= 1, CDML_E_BADARG, "pq_lut: dsub must be >= 1, got %d", dsub);
  CDML_REQUIRE(ldq >= (int64_t)M * dsub, CDML_E_BADARG, "pq_lut: ldq >= M dsub (M = %d, dsub = %d)", M, dsub);
  CDML_REQUIRE(aligned16(lut), CDML_E_ALIGN, "pq_lut: lut must be 16-B aligned");
  const dim3 grid((nq + kLutQ - 1) / kLutQ, M);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dsub(
      dsub,
      [&](auto ds) { hipLaunchKernelGGL(k_pq_lut<decltype(ds)::value>, grid, dim3(256), 0, st, Q, ldq, nq, codebooks, M, lut); },
      [&] { hipLaunchKernelGGL(k_pq_lut_any, grid, dim3(256), 0, st, Q, ldq, nq, codebooks, M, dsub, lut); });
  return check_launch("pq_lut");
}

extern "C" int cdml_ivf_pq_tile(int M, int *slots, int *rows) {
  CDML_REQUIRE(slots && rows, CDML_E_BADARG, "ivf_pq_tile: null pointer");
  CDML_REQUIRE_PQ_M("ivf_pq_tile", M);
  *slots = kLutKiB / M;
  *rows = kTileRows;
  return CDML_OK;
}

extern "C" int cdml_ivf_scan_pq(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                                const int64_t *slot_off, const uint8_t *codes, int64_t ldc, const int32_t *list_start, int M,
                                const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream) {
  if (int rc = check_pq_scan_args("ivf_scan_pq", lut && slot_query && slot_start && slot_off && codes && list_start && tiles && scores,
                                  lut, n_queries, codes, ldc, M, tiles, n_tiles, scores))
    return rc;
  const int4 *tl = reinterpret_cast<const int4 *>(tiles);
  hipStream_t st = (hipStream_t)stream;
  dispatch_m8(M, [&](auto m8) {
    hipLaunchKernelGGL(k_ivf_scan_pq<decltype(m8)::value>, dim3(n_tiles), dim3(kScanThreads), 0, st, lut, n_queries, slot_query,
                       slot_start, slot_off, codes, ldc, list_start, tl, scores);
  });
  return check_launch("ivf_scan_pq");
}
