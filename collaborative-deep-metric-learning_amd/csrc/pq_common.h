// What the three product-quantised forms of the IVF index share (csrc/ivf_pq.hip, ivf_pqr.hip, ivf_pq4.hip; DESIGN.md section
// 9f.7): the nearest-codeword walk of the encoders, the any-dsub encoder and lookup-table bodies, the 8-bit ADC scan (tile
// decode, the lane's code registers, the sums with or without a base), and on the host the argument checks and the two
// template dispatches.  Internal: each translation unit instantiates what it launches; the __global__ kernels and the C ABI
// stay in the .hip files.  A kernel is built from these pieces only where tools/isa_ab.py or a timing showed that it loses
// nothing by it; section 9f.7 lists the ones that keep their own text.
#pragma once
#include <type_traits>

#include "common.h"
#include "../../include/cdml_ivf_pq.h"

namespace cdml {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- encode --------------------------------------------------------------------------------------------------------
struct Nearest {
  float dist;
  int code;
};

// The lowest of NCW codewords of DS floats (cw[c * DS + j]; in LDS every lane reads the same address: a broadcast) nearest to
// the sub-vector v, which is in registers.  Ascending c, one fmaf chain over j per codeword.
// (c is declared ahead of best and code on purpose: the order of the three decides the order of the loop's selects, and
// with this one k_pq_encode and k_pq4_encode keep the machine code they had before the walk was a function.)
template <int NCW, int DS>
__device__ __forceinline__ Nearest nearest_codeword(const float *v, const float *cw) {
  int c = 0;
  float best = __builtin_inff();
  int code = 0;
#pragma unroll 4
  for (; c < NCW; ++c) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < DS; ++j) {
      const float diff = v[j] - cw[c * DS + j];
      d = __builtin_fmaf(diff, diff, d);
    }
    if (d < best) { best = d; code = c; }        // ties keep the lower c; a NaN passes nothing
  }
  return {best, code};
}

// Its twin for any dsub, both operands in memory (cw block-uniform: scalar loads), the same sums in the same order.  With
// kResidual the sub-vector is xr - cr, formed as it is read.
template <int NCW, bool kResidual>
__device__ __forceinline__ Nearest nearest_codeword_any(const float *xr, const float *cr, const float *cw, int dsub) {
  int c = 0;
  float best = __builtin_inff();
  int code = 0;
  for (; c < NCW; ++c) {
    float d = 0.f;
    for (int j = 0; j < dsub; ++j) {
      float diff;
      if constexpr (kResidual) diff = (xr[j] - cr[j]) - cw[(int64_t)c * dsub + j];
      else diff = xr[j] - cw[(int64_t)c * dsub + j];
      d = __builtin_fmaf(diff, diff, d);
    }
    if (d < best) { best = d; code = c; }
  }
  return {best, code};
}

// The 8-bit encoders for any dsub, one lane per (row, subspace m = blockIdx.y).  kResidual: a lane whose assign is outside
// [0, nlist) reads no centroid and writes codes 0, dist +inf.
template <bool kResidual>
__device__ __forceinline__ void pq_encode_any_body(const float *__restrict__ x, int64_t ldx, int64_t n,
                                                   const float *__restrict__ cen, int64_t ldcen, int nlist,
                                                   const int64_t *__restrict__ assign, const float *__restrict__ cb, int dsub,
                                                   uint8_t *__restrict__ codes, int64_t ldc, float *__restrict__ dist,
                                                   int64_t ldd) {
  constexpr int kCw = CDML_PQ_CODEWORDS;
  const int m = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int64_t a = 0;
  if constexpr (kResidual) a = assign[r];
  Nearest nn = {__builtin_inff(), 0};
  if (!kResidual || (a >= 0 && a < nlist)) {
    const float *cbm = cb + (int64_t)m * kCw * dsub;   // block-uniform addresses: scalar loads
    const float *xr = x + r * ldx + (int64_t)m * dsub;
    const float *cr = kResidual ? cen + a * ldcen + (int64_t)m * dsub : nullptr;
    nn = nearest_codeword_any<kCw, kResidual>(xr, cr, cbm, dsub);
  }
  codes[r * ldc + m] = (uint8_t)nn.code;
  if (dist) dist[r * ldd + m] = nn.dist;
}

// ---- lookup tables -------------------------------------------------------------------------------------------------
constexpr int kLutQ = 64;                     // queries per block

// LUT[q][sub][c] = <q_sub, cb[sub][c]> for any dsub and subspaces of CW codewords (256, or 16 for the 4-bit form): one block
// per (64 queries, 256 / CW subspaces), thread t takes codeword blockIdx.y * 256 + t of the codebooks (it stays in memory) and
// the block stores 256 consecutive floats per query; ``subspaces`` is the table's count of them.  For CW = 256 the thread's
// share of the subspace index is the constant 0, not t / 256: the query's sub-vector stays block-uniform (scalar loads).
// Y is the type blockIdx.y is held in (int: sign-extended into the addresses, as k_pq_lut_any always did; unsigned:
// zero-extended, as k_pq4_lut_any did) -- one scalar instruction apart, kept so that both kernels' machine code is unchanged.
template <int CW, class Y>
__device__ __forceinline__ void pq_lut_any_body(const float *__restrict__ Q, int64_t ldq, int nq, const float *__restrict__ cb,
                                                int subspaces, int dsub, float *__restrict__ lut) {
  constexpr int kSub = 256 / CW;
  const int t = threadIdx.x;
  const Y y = blockIdx.y;
  const int m = y * kSub + (CW == 256 ? 0 : t / CW);
  const float *cw = cb + ((int64_t)y * 256 + t) * dsub;
  const int q1 = min(nq, ((int)blockIdx.x + 1) * kLutQ);
  for (int q = blockIdx.x * kLutQ; q < q1; ++q) {
    const float *qm = Q + (int64_t)q * ldq + (int64_t)m * dsub;
    float acc = 0.f;
    for (int j = 0; j < dsub; ++j) acc = __builtin_fmaf(qm[j], cw[j], acc);
    lut[((int64_t)q * subspaces + y * kSub) * CW + t] = acc;
  }
}

// ---- the scans' work item ------------------------------------------------------------------------------------------------
constexpr int kScanThreads = 512;
constexpr int kRowsPerLane = 2;
constexpr int kTileRows = kScanThreads * kRowsPerLane;        // R = 1024

// (list, S-slot tile, R-row tile) of the tile table.  The slot / offset tables and the store rules are k_ivf_scan's
// (csrc/ivf.hip).
struct ScanTile {
  int i0, s0, nq_c;                           // slots: the tile's first within the list, the list's first, the list's count
  int j0, r0, len;                            // rows: the same three
  bool valid;                                 // block-uniform: a block returns on !valid before any barrier
  __device__ __forceinline__ ScanTile(const int4 *__restrict__ tiles, const int32_t *__restrict__ slot_start,
                                      const int32_t *__restrict__ list_start) {
    const int4 tl = tiles[blockIdx.x];
    const int c = tl.x;
    i0 = tl.y, j0 = tl.z;
    s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
    r0 = list_start[c], len = list_start[c + 1] - r0;
    valid = !(i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len);
  }
  __device__ __forceinline__ int ld_c() const { return (len + 3) & ~3; }   // row stride of the list's block of scores
};

// The 8 M8 code bytes of row j of the list that starts at r0 (zeros past the list's end), 8-byte loads.  A lane calls it for its
// rows j0 + t and j0 + t + 512 and keeps the words in registers across the tile's slots.
template <int M8>
__device__ __forceinline__ void load_row_codes(const uint8_t *__restrict__ codes, int64_t ldc, int r0, int j, int len,
                                               uint32_t (&cw)[2 * M8]) {
  if (j < len) {
    const uint2 *p = reinterpret_cast<const uint2 *>(codes + (int64_t)(r0 + j) * ldc);
#pragma unroll
    for (int g = 0; g < M8; ++g) {
      const uint2 v = p[g];
      cw[2 * g] = v.x;
      cw[2 * g + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int g = 0; g < 2 * M8; ++g) cw[g] = 0u;
  }
}

// ---- the 8-bit ADC scan ----------------------------------------------------------------------------------------------
constexpr int kLutKiB = 64;                   // LDS of a block's lookup tables: S(M) = kLutKiB / M slots

// A block of 512 lanes stages the S = 64 / M lookup tables of its slots in LDS (M KiB each, 64 KiB a block: two blocks a CU),
// and per slot and row does M ds_read_b32 gathers and the adds in ascending m -- from the first term, or with kBase from
// slot_base[slot] (block-uniform: a scalar load).  The order of the additions is the contract of the two headers.  The gather
// address is 256 m + code: the bank is code mod 32, random; nothing is done about it (DESIGN.md section 9f.3 says why).
//
// What becomes of a slot's sums is the body's last step.  The buffered scans store them (Out = ScoreStore: the text below, as
// it always stood -- handing that store to a functor too moved instructions of k_ivf_scan_pq / _pqr).
// Any other Out (the filter's append, csrc/ivf_range.hip) takes no slot_off / scores (null) and is called instead:
// out.begin(tile, t) once, behind the barrier that publishes the tables, then out.slot(tile, s, t, acc) per slot with the lane's
// two sums (rows tile.j0 + t and + 512; a row past the list's end has the sums of code 0: the step masks it).
struct ScoreStore {};

template <int M8, bool kBase, class Out = ScoreStore>
__device__ __forceinline__ void pq_scan_body(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
                                             const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off,
                                             const float *__restrict__ slot_base, const uint8_t *__restrict__ codes, int64_t ldc,
                                             const int32_t *__restrict__ list_start, const int4 *__restrict__ tiles,
                                             float *__restrict__ scores, Out out = Out()) {
  constexpr bool kStore = std::is_same<Out, ScoreStore>::value;
  constexpr int kCw = CDML_PQ_CODEWORDS;
  constexpr int M = 8 * M8, S = kLutKiB / M, W = M / 4;
  __shared__ __attribute__((aligned(16))) float sL[S * M * kCw];
  const int t = threadIdx.x;

  const ScanTile tile(tiles, slot_start, list_start);
  if (!tile.valid) return;
  const int i0 = tile.i0, j0 = tile.j0, s0 = tile.s0, len = tile.len, ld_c = tile.ld_c();
  const int ns = min(S, tile.nq_c - i0);

  uint32_t cw[kRowsPerLane][W];
#pragma unroll
  for (int u = 0; u < kRowsPerLane; ++u) load_row_codes<M8>(codes, ldc, tile.r0, j0 + t + kScanThreads * u, len, cw[u]);

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

  float *blk = nullptr;
  if constexpr (kStore) blk = scores + slot_off[s0];
  else out.begin(tile, t);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s < ns) {                                // block-uniform
      const float *L = sL + s * (M * kCw);
      float acc[kRowsPerLane];
      if constexpr (kBase) {
        const float base = slot_base[s0 + i0 + s];
#pragma unroll
        for (int u = 0; u < kRowsPerLane; ++u) acc[u] = base;
      }
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int u = 0; u < kRowsPerLane; ++u) {
          const uint32_t code = (cw[u][m >> 2] >> (8 * (m & 3))) & 255u;
          const float v = L[m * kCw + code];
          acc[u] = !kBase && m == 0 ? v : acc[u] + v;
        }
      if constexpr (kStore) {
#pragma unroll
        for (int u = 0; u < kRowsPerLane; ++u) {
          const int j = j0 + t + kScanThreads * u;
          if (j < len) blk[(int64_t)(i0 + s) * ld_c + j] = acc[u];
        }
      } else {
        out.slot(tile, s, t, acc);
      }
    }
  }
}

// ---- host: argument checks and template dispatch --------------------------------------------------------------------
inline bool pq_m_ok(int M) { return M >= CDML_PQ_M_MIN && M <= CDML_PQ_M_MAX && M % 8 == 0; }

#define CDML_REQUIRE_PQ_M(name, M)                                                                                      \
  CDML_REQUIRE(pq_m_ok(M), CDML_E_BADARG, "%s: M must be a multiple of 8 in [%d, %d], got %d", name, CDML_PQ_M_MIN,    \
               CDML_PQ_M_MAX, M)

// The checks of a scan entry point ``name``; ``pointers``: every pointer argument of that entry point is non-null.
inline int check_pq_scan_args(const char *name, bool pointers, const float *lut, int n_queries, const uint8_t *codes, int64_t ldc,
                              int M, const int32_t *tiles, int n_tiles, const float *scores) {
  CDML_REQUIRE(pointers, CDML_E_BADARG, "%s: null pointer", name);
  CDML_REQUIRE(n_queries > 0 && n_tiles > 0, CDML_E_BADARG, "%s: bad size", name);
  CDML_REQUIRE_PQ_M(name, M);
  CDML_REQUIRE(ldc >= M, CDML_E_BADARG, "%s: ldc >= M (got %lld, M = %d)", name, (long long)ldc, M);
  CDML_REQUIRE(aligned16(lut) && aligned16(scores) && aligned16(tiles) && !(ldc & 7) &&
                   !(reinterpret_cast<uintptr_t>(codes) & 7),
               CDML_E_ALIGN, "%s: lut, scores and tiles 16-B aligned, codes 8-B aligned, ldc a multiple of 8", name);
  return CDML_OK;
}

// The checks of an encoder ``name``; ``pointers`` as above; nlist: 1 for an encoder that takes no lists; ``ld_ok`` / ``ld_text``: the
// entry point's condition on its leading dimensions and its wording.
inline int check_pq_encode_args(const char *name, bool pointers, int64_t n, int nlist, int M, int dsub, bool ld_ok,
                                const char *ld_text) {
  CDML_REQUIRE(pointers, CDML_E_BADARG, "%s: null pointer", name);
  CDML_REQUIRE(n > 0, CDML_E_BADARG, "%s: n must be positive", name);
  CDML_REQUIRE(nlist >= 1, CDML_E_BADARG, "%s: nlist must be >= 1, got %d", name, nlist);
  CDML_REQUIRE_PQ_M(name, M);
  CDML_REQUIRE(dsub >= 1, CDML_E_BADARG, "%s: dsub must be >= 1, got %d", name, dsub);
  CDML_REQUIRE(ld_ok, CDML_E_BADARG, "%s: %s (M = %d, dsub = %d)", name, ld_text, M, dsub);
  CDML_REQUIRE((n + 255) / 256 <= 0x7fffffff, CDML_E_UNSUPPORTED, "%s: too many rows", name);
  return CDML_OK;
}

template <int N>
using int_c = std::integral_constant<int, N>;

// f(int_c<dsub>) for a dsub the kernels are instantiated for, any() for every other
template <class F, class Any>
inline void dispatch_dsub(int dsub, F &&f, Any &&any) {
  switch (dsub) {
    case 1: f(int_c<1>()); break;
    case 2: f(int_c<2>()); break;
    case 4: f(int_c<4>()); break;
    case 8: f(int_c<8>()); break;
    case 16: f(int_c<16>()); break;
    case 32: f(int_c<32>()); break;
    default: any();
  }
}

// f(int_c<M / 8>) for an M that pq_m_ok
template <class F>
inline void dispatch_m8(int M, F &&f) {
  switch (M / 8) {
    case 1: f(int_c<1>()); break;
    case 2: f(int_c<2>()); break;
    case 3: f(int_c<3>()); break;
    case 4: f(int_c<4>()); break;
    case 5: f(int_c<5>()); break;
    case 6: f(int_c<6>()); break;
    case 7: f(int_c<7>()); break;
    case 8: f(int_c<8>()); break;
  }
}

}  // namespace cdml
