// Product-quantised lists of the IVF index (include/cdml_ivf_pq.h): M bytes per listed row instead
// of the row.  Plain (non-residual) PQ: one set of codebooks [M][256][dsub] for the catalogue, one lookup table per query.
//
//   k_pq_encode      one block per (256 rows, subspace): the subspace's 256 codewords in LDS, a lane owns one row's
//                    sub-vector in registers and walks the codewords in order -- every lane reads the same LDS address (a
//                    broadcast, conflict-free).  dsub is a template parameter for {1, 2, 4, 8, 16, 32}; k_pq_encode_any
//                    reads both operands from memory for any other dsub (the same sums in the same order).
//   k_pq_lut         LUT[q][m][c] = <q_m, cb[m][c]>: one block per (64 queries, subspace), thread c keeps codeword c in
//                    registers (the same dsub set; k_pq_lut_any otherwise), the query's sub-vector is block-uniform.  The
//                    launch is bound by its nq x M KiB of stores.
//   k_ivf_scan_pq    the ADC scan.  Work item = (list, S-slot tile, R-row tile) from the tile table.  A block of 512 lanes
//                    keeps the M code bytes of its two rows per lane in registers (8-byte loads), stages the S = 64 / M
//                    lookup tables of its slots in LDS (M KiB each, 64 KiB a block: two blocks a CU), and per slot and row
//                    does M ds_read_b32 gathers and M - 1 adds in ascending m.  The gather address is 256 m + code: the
//                    bank is code mod 32, random; nothing is done about it (DESIGN.md section 9f.3 says why).
// The slot / offset tables and the store rules are k_ivf_scan's (csrc/ivf.hip).
#include "common.h"
#include "../../include/cdml_ivf_pq.h"

namespace cdml {
namespace {

constexpr int kCw = CDML_PQ_CODEWORDS;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- encode --------------------------------------------------------------------------------------------------------
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
  float best = __builtin_inff();
  int code = 0;
#pragma unroll 4
  for (int c = 0; c < kCw; ++c) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < DS; ++j) {
      const float diff = xv[j] - sC[c * DS + j];
      d = __builtin_fmaf(diff, diff, d);
    }
    if (d < best) { best = d; code = c; }      // ties keep the lower c; a NaN passes nothing
  }
  codes[r * ldc + m] = (uint8_t)code;
  if (dist) dist[r * ldd + m] = best;
}

__global__ void __launch_bounds__(256)
k_pq_encode_any(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cb, int dsub,
                uint8_t *__restrict__ codes, int64_t ldc, float *__restrict__ dist, int64_t ldd) {
  const int m = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float *cbm = cb + (int64_t)m * kCw * dsub;   // block-uniform addresses: scalar loads
  const float *xr = x + r * ldx + (int64_t)m * dsub;
  float best = __builtin_inff();
  int code = 0;
  for (int c = 0; c < kCw; ++c) {
    float d = 0.f;
    for (int j = 0; j < dsub; ++j) {
      const float diff = xr[j] - cbm[(int64_t)c * dsub + j];
      d = __builtin_fmaf(diff, diff, d);
    }
    if (d < best) { best = d; code = c; }
  }
  codes[r * ldc + m] = (uint8_t)code;
  if (dist) dist[r * ldd + m] = best;
}

// ---- lookup tables -------------------------------------------------------------------------------------------------
constexpr int kLutQ = 64;                     // queries per block

// thread c keeps its codeword in registers; a query's sub-vector is block-uniform (scalar loads)
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
  const int c = threadIdx.x, m = blockIdx.y;
  const float *cw = cb + ((int64_t)m * kCw + c) * dsub;
  const int q1 = min(nq, ((int)blockIdx.x + 1) * kLutQ);
  for (int q = blockIdx.x * kLutQ; q < q1; ++q) {
    const float *qm = Q + (int64_t)q * ldq + (int64_t)m * dsub;    // block-uniform
    float acc = 0.f;
    for (int j = 0; j < dsub; ++j) acc = __builtin_fmaf(qm[j], cw[j], acc);
    lut[((int64_t)q * M + m) * kCw + c] = acc;
  }
}

// ---- the ADC scan ----------------------------------------------------------------------------------------------------
constexpr int kScanThreads = 512;
constexpr int kRowsPerLane = 2;
constexpr int kTileRows = kScanThreads * kRowsPerLane;        // R = 1024
constexpr int kLutKiB = 64;                   // LDS of a block's lookup tables: S(M) = kLutKiB / M slots

template <int M8>
__global__ void __launch_bounds__(kScanThreads)
k_ivf_scan_pq(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
              const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off, const uint8_t *__restrict__ codes,
              int64_t ldc, const int32_t *__restrict__ list_start, const int4 *__restrict__ tiles, float *__restrict__ scores) {
  constexpr int M = 8 * M8, S = kLutKiB / M, W = M / 4;
  __shared__ __attribute__((aligned(16))) float sL[S * M * kCw];
  const int t = threadIdx.x;

  const int4 tl = tiles[blockIdx.x];
  const int c = tl.x, i0 = tl.y, j0 = tl.z;
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const int r0 = list_start[c], len = list_start[c + 1] - r0;
  if (i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len) return;    // block-uniform, before any barrier
  const int ld_c = (len + 3) & ~3;
  const int ns = min(S, nq_c - i0);

  // the lane's rows j0 + t and j0 + t + 512: their codes stay in registers across the tile's slots
  uint32_t cw[kRowsPerLane][W];
#pragma unroll
  for (int u = 0; u < kRowsPerLane; ++u) {
    const int j = j0 + t + kScanThreads * u;
    if (j < len) {
      const uint2 *p = reinterpret_cast<const uint2 *>(codes + (int64_t)(r0 + j) * ldc);
#pragma unroll
      for (int g = 0; g < M8; ++g) {
        const uint2 v = p[g];
        cw[u][2 * g] = v.x;
        cw[u][2 * g + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int g = 0; g < W; ++g) cw[u][g] = 0u;
    }
  }

  // the slots' lookup tables: M * 256 floats each, M * 64 16-byte pieces over 512 lanes = M8 pieces a lane
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s < ns) {
      const int q = min(max(slot_query[s0 + i0 + s], 0), n_queries - 1);
      const f32x4 *src = reinterpret_cast<const f32x4 *>(lut + (int64_t)q * (M * kCw));
      f32x4 *dst = reinterpret_cast<f32x4 *>(sL + s * (M * kCw));
#pragma unroll
      for (int g = 0; g < M8; ++g) dst[t + kScanThreads * g] = src[t + kScanThreads * g];
    }
  }
  __syncthreads();

  float *blk = scores + slot_off[s0];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s < ns) {                                // block-uniform
      const float *L = sL + s * (M * kCw);
      float acc[kRowsPerLane];
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int u = 0; u < kRowsPerLane; ++u) {
          const uint32_t code = (cw[u][m >> 2] >> (8 * (m & 3))) & 255u;
          const float v = L[m * kCw + code];
          acc[u] = m == 0 ? v : acc[u] + v;    // ascending m, from the first term
        }
#pragma unroll
      for (int u = 0; u < kRowsPerLane; ++u) {
        const int j = j0 + t + kScanThreads * u;
        if (j < len) blk[(int64_t)(i0 + s) * ld_c + j] = acc[u];
      }
    }
  }
}

bool pq_m_ok(int M) { return M >= CDML_PQ_M_MIN && M <= CDML_PQ_M_MAX && M % 8 == 0; }

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_pq_encode(const float *x, int64_t ldx, int64_t n, const float *codebooks, int M, int dsub, uint8_t *codes,
                              int64_t ldc, float *dist, int64_t ldd, cdml_stream_t stream) {
  CDML_REQUIRE(x && codebooks && codes, CDML_E_BADARG, "pq_encode: null pointer");
  CDML_REQUIRE(n > 0, CDML_E_BADARG, "pq_encode: n must be positive");
  CDML_REQUIRE(pq_m_ok(M), CDML_E_BADARG, "pq_encode: M must be a multiple of 8 in [%d, %d], got %d", CDML_PQ_M_MIN,
               CDML_PQ_M_MAX, M);
  CDML_REQUIRE(dsub >= 1, CDML_E_BADARG, "pq_encode: dsub must be >= 1, got %d", dsub);
  CDML_REQUIRE(ldx >= (int64_t)M * dsub && ldc >= M && (!dist || ldd >= M), CDML_E_BADARG,
               "pq_encode: ldx >= M dsub, ldc >= M and ldd >= M (M = %d, dsub = %d)", M, dsub);
  CDML_REQUIRE((n + 255) / 256 <= 0x7fffffff, CDML_E_UNSUPPORTED, "pq_encode: too many rows");
  const dim3 grid((unsigned)((n + 255) / 256), M);
  hipStream_t st = (hipStream_t)stream;
#define CDML_PQ_ENC(DS)                                                                                                \
  case DS:                                                                                                             \
    hipLaunchKernelGGL(k_pq_encode<DS>, grid, dim3(256), 0, st, x, ldx, n, codebooks, codes, ldc, dist, ldd);          \
    break;
  switch (dsub) {
    CDML_PQ_ENC(1)
    CDML_PQ_ENC(2)
    CDML_PQ_ENC(4)
    CDML_PQ_ENC(8)
    CDML_PQ_ENC(16)
    CDML_PQ_ENC(32)
    default:
      hipLaunchKernelGGL(k_pq_encode_any, grid, dim3(256), 0, st, x, ldx, n, codebooks, dsub, codes, ldc, dist, ldd);
  }
#undef CDML_PQ_ENC
  return check_launch("pq_encode");
}

extern "C" int cdml_pq_lut(const float *Q, int64_t ldq, int nq, const float *codebooks, int M, int dsub, float *lut,
                           cdml_stream_t stream) {
  CDML_REQUIRE(Q && codebooks && lut, CDML_E_BADARG, "pq_lut: null pointer");
  CDML_REQUIRE(nq > 0, CDML_E_BADARG, "pq_lut: nq must be positive");
  CDML_REQUIRE(pq_m_ok(M), CDML_E_BADARG, "pq_lut: M must be a multiple of 8 in [%d, %d], got %d", CDML_PQ_M_MIN, CDML_PQ_M_MAX,
               M);
  CDML_REQUIRE(dsub >= 1, CDML_E_BADARG, "pq_lut: dsub must be >= 1, got %d", dsub);
  CDML_REQUIRE(ldq >= (int64_t)M * dsub, CDML_E_BADARG, "pq_lut: ldq >= M dsub (M = %d, dsub = %d)", M, dsub);
  CDML_REQUIRE(aligned16(lut), CDML_E_ALIGN, "pq_lut: lut must be 16-B aligned");
  const dim3 grid((nq + kLutQ - 1) / kLutQ, M);
  hipStream_t st = (hipStream_t)stream;
#define CDML_PQ_LUT(DS)                                                                                                \
  case DS:                                                                                                             \
    hipLaunchKernelGGL(k_pq_lut<DS>, grid, dim3(256), 0, st, Q, ldq, nq, codebooks, M, lut);                           \
    break;
  switch (dsub) {
    CDML_PQ_LUT(1)
    CDML_PQ_LUT(2)
    CDML_PQ_LUT(4)
    CDML_PQ_LUT(8)
    CDML_PQ_LUT(16)
    CDML_PQ_LUT(32)
    default:
      hipLaunchKernelGGL(k_pq_lut_any, grid, dim3(256), 0, st, Q, ldq, nq, codebooks, M, dsub, lut);
  }
#undef CDML_PQ_LUT
  return check_launch("pq_lut");
}

extern "C" int cdml_ivf_pq_tile(int M, int *slots, int *rows) {
  CDML_REQUIRE(slots && rows, CDML_E_BADARG, "ivf_pq_tile: null pointer");
  CDML_REQUIRE(pq_m_ok(M), CDML_E_BADARG, "ivf_pq_tile: M must be a multiple of 8 in [%d, %d], got %d", CDML_PQ_M_MIN,
               CDML_PQ_M_MAX, M);
  *slots = kLutKiB / M;
  *rows = kTileRows;
  return CDML_OK;
}

extern "C" int cdml_ivf_scan_pq(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                                const int64_t *slot_off, const uint8_t *codes, int64_t ldc, const int32_t *list_start, int M,
                                const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream) {
  CDML_REQUIRE(lut && slot_query && slot_start && slot_off && codes && list_start && tiles && scores, CDML_E_BADARG,
               "ivf_scan_pq: null pointer");
  CDML_REQUIRE(n_queries > 0 && n_tiles > 0, CDML_E_BADARG, "ivf_scan_pq: bad size");
  CDML_REQUIRE(pq_m_ok(M), CDML_E_BADARG, "ivf_scan_pq: M must be a multiple of 8 in [%d, %d], got %d", CDML_PQ_M_MIN,
               CDML_PQ_M_MAX, M);
  CDML_REQUIRE(ldc >= M, CDML_E_BADARG, "ivf_scan_pq: ldc >= M (got %lld, M = %d)", (long long)ldc, M);
  CDML_REQUIRE(aligned16(lut) && aligned16(scores) && aligned16(tiles) && !(ldc & 7) &&
                   !(reinterpret_cast<uintptr_t>(codes) & 7),
               CDML_E_ALIGN, "ivf_scan_pq: lut, scores and tiles 16-B aligned, codes 8-B aligned, ldc a multiple of 8");
  const int4 *tl = reinterpret_cast<const int4 *>(tiles);
  hipStream_t st = (hipStream_t)stream;
#define CDML_PQ_SCAN(M8)                                                                                               \
  case M8:                                                                                                             \
    hipLaunchKernelGGL(k_ivf_scan_pq<M8>, dim3(n_tiles), dim3(kScanThreads), 0, st, lut, n_queries, slot_query,        \
                       slot_start, slot_off, codes, ldc, list_start, tl, scores);                                      \
    break;
  switch (M / 8) {
    CDML_PQ_SCAN(1)
    CDML_PQ_SCAN(2)
    CDML_PQ_SCAN(3)
    CDML_PQ_SCAN(4)
    CDML_PQ_SCAN(5)
    CDML_PQ_SCAN(6)
    CDML_PQ_SCAN(7)
    CDML_PQ_SCAN(8)
  }
#undef CDML_PQ_SCAN
  return check_launch("ivf_scan_pq");
}
