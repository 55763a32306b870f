// 4-bit product-quantised lists of the IVF index (include/cdml_ivf_pq4.h): M bytes per listed row as
// for 8 bits, but Ms = 2 M subspaces of 16 codewords, two codes a byte (the even subspace in the low nibble).  A query's
// lookup table is Ms x 16 floats = 128 M bytes, an eighth of the 8-bit one.
//
// The encoders' codeword walk, the any-dsub lookup-table body, the argument checks and the dispatches are those of the 8-bit
// forms (csrc/pq_common.h); k_pq4_lut and the scan keep their own text (DESIGN.md section 9f.7 says why).
//
//   k_pq4_encode     one block per (256 rows, byte): the 32 codewords of the byte's two subspaces in LDS, a lane owns its
//                    row's two sub-vectors in registers, walks each subspace's 16 codewords in order and stores the WHOLE byte
//                    once.  dsub is a template parameter for {1, 2, 4, 8, 16, 32}; k_pq4_encode_any reads both operands from
//                    memory for any other dsub (the same sums in the same order).
//   k_pq4_lut        LUT[q][m][c] = <q_m, cb[m][c]>: one block per (64 queries, 16 subspaces), thread (m', c) keeps its
//                    codeword in registers; a block stores 256 consecutive floats per query.  k_pq4_lut_any is
//                    pq_lut_any_body<16> for a dsub outside the set.
//   k_ivf_scan_pq4   the scan.  Work item = (list, S-slot tile, R-row tile) from the tile table, 512 lanes.  A lane keeps the
//                    M code bytes of its two rows in M / 4 registers each (8-byte loads) across the tile's slots; the S =
//                    min(16, 512 / M) lookup tables of the slots are staged into LDS with 16-byte accesses (128 M bytes
//                    each, at most 64 KiB a block: two blocks a CU).  Per slot, row and byte: two ds_read_b32 gathers, the
//                    pair add, the running add.  A nibble's byte offset is (word >> (4 k - 2)) & 0x3C, formed once for a
//                    group of 8 (S = 16) or S slots; the slot in the group and the subspace's 64 m bytes are the read's
//                    immediate offset, the group's table base is or-ed in (tables are 64-byte multiples).
//                    A subspace's 16 entries are 16 consecutive dwords: the distinct addresses of a 32-lane group sit in
//                    distinct banks, equal ones broadcast -- no bank conflict by construction.
#include "pq_common.h"
#include "../../include/cdml_ivf_pq4.h"

namespace cdml {
namespace {

constexpr int kCw4 = CDML_PQ4_CODEWORDS;

// ---- encode --------------------------------------------------------------------------------------------------------
template <int DS>
__global__ void __launch_bounds__(256)
k_pq4_encode(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cb, uint8_t *__restrict__ codes,
             int64_t ldc, float *__restrict__ dist, int64_t ldd) {
  constexpr int kPair = 2 * kCw4 * DS;         // the floats of the byte's two subspaces, contiguous in the codebooks
  __shared__ __attribute__((aligned(16))) float sC[kPair];
  const int t = threadIdx.x, b = blockIdx.y;
  const float *cbb = cb + (int64_t)b * kPair;
#pragma unroll
  for (int i = 0; i < (kPair + 255) / 256; ++i)
    if (t + 256 * i < kPair) sC[t + 256 * i] = cbb[t + 256 * i];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + t;
  if (r >= n) return;                          // after the only barrier
  float xv[2 * DS];
  const float *xr = x + r * ldx + (int64_t)b * (2 * DS);
#pragma unroll
  for (int j = 0; j < 2 * DS; ++j) xv[j] = xr[j];
  uint32_t byte = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {                // h = 0: subspace 2 b, the low nibble
    const Nearest nn = nearest_codeword<kCw4, DS>(xv + h * DS, sC + h * kCw4 * DS);
    byte |= (uint32_t)nn.code << (4 * h);
    if (dist) dist[r * ldd + 2 * b + h] = nn.dist;
  }
  codes[r * ldc + b] = (uint8_t)byte;          // the whole byte, once
}

__global__ void __launch_bounds__(256)
k_pq4_encode_any(const float *__restrict__ x, int64_t ldx, int64_t n, const float *__restrict__ cb, int dsub,
                 uint8_t *__restrict__ codes, int64_t ldc, float *__restrict__ dist, int64_t ldd) {
  const int b = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  uint32_t byte = 0;
  for (int h = 0; h < 2; ++h) {
    const int m = 2 * b + h;
    const Nearest nn = nearest_codeword_any<kCw4, false>(x + r * ldx + (int64_t)m * dsub, nullptr,
                                                         cb + (int64_t)m * kCw4 * dsub, dsub);
    byte |= (uint32_t)nn.code << (4 * h);
    if (dist) dist[r * ldd + m] = nn.dist;
  }
  codes[r * ldc + b] = (uint8_t)byte;
}

// ---- lookup tables -------------------------------------------------------------------------------------------------
constexpr int kLutSub = 256 / kCw4;           // subspaces per block: thread t is (subspace t / 16, codeword t % 16)

template <int DS>
__global__ void __launch_bounds__(256)
k_pq4_lut(const float *__restrict__ Q, int64_t ldq, int nq, const float *__restrict__ cb, int Ms, float *__restrict__ lut) {
  const int t = threadIdx.x, m = blockIdx.y * kLutSub + (t >> 4);
  const float *src = cb + ((int64_t)blockIdx.y * 256 + t) * DS;       // codeword (m, t % 16)
  float cw[DS];
#pragma unroll
  for (int j = 0; j < DS; ++j) cw[j] = src[j];
  const int q1 = min(nq, ((int)blockIdx.x + 1) * kLutQ);
  for (int q = blockIdx.x * kLutQ; q < q1; ++q) {
    const float *qm = Q + (int64_t)q * ldq + (int64_t)m * DS;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < DS; ++j) acc = __builtin_fmaf(qm[j], cw[j], acc);
    lut[((int64_t)q * Ms + blockIdx.y * kLutSub) * kCw4 + t] = acc;   // = lut[q][m][t % 16]
  }
}

__global__ void __launch_bounds__(256)
k_pq4_lut_any(const float *__restrict__ Q, int64_t ldq, int nq, const float *__restrict__ cb, int Ms, int dsub,
              float *__restrict__ lut) {
  pq_lut_any_body<kCw4, unsigned>(Q, ldq, nq, cb, Ms, dsub, lut);
}

// ---- the scan --------------------------------------------------------------------------------------------------------
constexpr int kMaxSlots = 16;
constexpr int kLutBytes = 65536;              // LDS of a block's lookup tables, 128 M bytes each

constexpr int scan_slots(int M) { return kLutBytes / (128 * M) < kMaxSlots ? kLutBytes / (128 * M) : kMaxSlots; }

constexpr int scan_group(int S) { return S <= 12 ? S : 8; }    // slots whose sums run side by side (16 = two groups of 8)

// One row against SG consecutive slots, bytes outermost: a nibble's LDS byte offset ((word >> (4 k - 2)) & 0x3C, with the first
// slot's table base -- a multiple of 64 -- or-ed in) is formed once per byte and serves all SG slots; the slot within the
// group and the subspace are the read's immediate offset (s * 128 M + 64 m < 65536).  acc[s] sums the pairs in ascending b
// from the first pair, whatever SG is.  Called for rows and slots inside the list only: every sum is stored, so loads, adds
// and stores share one region of control flow (a guard around the stores alone lets the adds sink below all the loads,
// which then spill).
template <int M, int SG>
__device__ __forceinline__ void scan_row_slots(const float *sL, uint32_t (&cw)[M / 4], int s_first,
                                               float *__restrict__ out, int ld_c) {
  constexpr int kTableBytes = 2 * M * kCw4 * 4;
  // (an empty statement that "rewrites" each code word in place: without it the 2 M shifted-and-masked offsets are hoisted
  // out of the slot loops as loop invariants -- 2 M live registers, one block a CU or a spill -- to save two instructions
  // per nibble and group.  It emits no instruction.  After a compiler upgrade re-read the "VGPRs:" remark of k_ivf_scan_pq4:
  // __graft_entry__.VGPR_CEILINGS refuses a build in which an instance exceeds 128.)
#pragma unroll
  for (int g = 0; g < M / 4; ++g) asm volatile("" : "+v"(cw[g]));
  const char *base = reinterpret_cast<const char *>(sL);
  const uint32_t sb = (uint32_t)s_first * kTableBytes;
  float acc[SG];
#pragma unroll
  for (int b = 0; b < M; ++b) {
    const uint32_t w = cw[b >> 2];
    const int k = 2 * (b & 3);                   // the low nibble's index in its word
    const uint32_t lo = ((k == 0 ? w << 2 : w >> (4 * k - 2)) & 0x3Cu) | sb;
    const uint32_t hi = ((w >> (4 * k + 2)) & 0x3Cu) | sb;
#pragma unroll
    for (int s = 0; s < SG; ++s) {
      const float p = *reinterpret_cast<const float *>(base + lo + (s * kTableBytes + (2 * b) * 64)) +
                      *reinterpret_cast<const float *>(base + hi + (s * kTableBytes + (2 * b + 1) * 64));   // the pair first
      acc[s] = b == 0 ? p : acc[s] + p;          // ascending b, from the first pair
    }
    // (a byte at a time: 2 SG gathers in flight.  Left alone, the scheduler issues a small M's 2 M SG gathers ahead of every
    // add and spills)
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int s = 0; s < SG; ++s) out[(int64_t)(s_first + s) * ld_c] = acc[s];
}

template <int M8>
__global__ void __launch_bounds__(kScanThreads)
k_ivf_scan_pq4(const float *__restrict__ lut, int n_queries, const int32_t *__restrict__ slot_query,
               const int32_t *__restrict__ slot_start, const int64_t *__restrict__ slot_off, const uint8_t *__restrict__ codes,
               int64_t ldc, const int32_t *__restrict__ list_start, const int4 *__restrict__ tiles, float *__restrict__ scores) {
  constexpr int M = 8 * M8, S = scan_slots(M), W = M / 4;
  constexpr int kTable = 2 * M * kCw4;         // floats of one query's table (128 M bytes)
  constexpr int kPieces = kTable / 4;          // its 16-byte pieces: 64 M8
  __shared__ __attribute__((aligned(64))) float sL[S * kTable];
  const int t = threadIdx.x;

  const int4 tl = tiles[blockIdx.x];
  const int c = tl.x, i0 = tl.y, j0 = tl.z;
  const int s0 = slot_start[c], nq_c = slot_start[c + 1] - s0;
  const int r0 = list_start[c], len = list_start[c + 1] - r0;
  if (i0 < 0 || j0 < 0 || i0 >= nq_c || j0 >= len) return;    // block-uniform, before any barrier
  const int ld_c = (len + 3) & ~3;
  const int ns = min(S, nq_c - i0);

  // the lane's rows j0 + t and j0 + t + 512: their codes stay in registers across the tile's slots
  // (this prologue is pq_common.h's ScanTile and load_row_codes written out: through them this kernel, which is steered to
  // its register count, gets other machine code than it had -- DESIGN.md section 9f.7)
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

  // the slots' lookup tables, one flat walk over the ns * kPieces 16-byte pieces (a table is smaller than a pass of the block
  // for M < 64)
#pragma unroll
  for (int g = 0; g < (S * kPieces + kScanThreads - 1) / kScanThreads; ++g) {
    const int idx = t + kScanThreads * g;
    const int s = idx / kPieces, piece = idx - s * kPieces;
    if (s < ns) {
      const int q = min(max(slot_query[s0 + i0 + s], 0), n_queries - 1);
      reinterpret_cast<f32x4 *>(sL)[idx] = reinterpret_cast<const f32x4 *>(lut + (int64_t)q * kTable)[piece];
    }
  }
  __syncthreads();

  float *blk = scores + slot_off[s0] + (int64_t)i0 * ld_c;
  constexpr int SG = scan_group(S);
#pragma unroll
  for (int u = 0; u < kRowsPerLane; ++u) {
    const int j = j0 + t + kScanThreads * u;
    if (j < len) {
      int s = 0;                                 // block-uniform trip counts under the lane's row guard
#pragma unroll 1
      for (; s + SG <= ns; s += SG) scan_row_slots<M, SG>(sL, cw[u], s, blk + j, ld_c);
#pragma unroll 1
      for (; s < ns; ++s) scan_row_slots<M, 1>(sL, cw[u], s, blk + j, ld_c);
    }
  }
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_pq4_encode(const float *x, int64_t ldx, int64_t n, const float *codebooks, int M, int dsub, uint8_t *codes,
                               int64_t ldc, float *dist, int64_t ldd, cdml_stream_t stream) {
  if (int rc = check_pq_encode_args("pq4_encode", x && codebooks && codes, n, 1, M, dsub,
                                    ldx >= (int64_t)2 * M * dsub && ldc >= M && (!dist || ldd >= 2 * M),
                                    "ldx >= 2 M dsub, ldc >= M and ldd >= 2 M"))
    return rc;
  const dim3 grid((unsigned)((n + 255) / 256), M);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dsub(
      dsub,
      [&](auto ds) {
        hipLaunchKernelGGL(k_pq4_encode<decltype(ds)::value>, grid, dim3(256), 0, st, x, ldx, n, codebooks, codes, ldc, dist, ldd);
      },
      [&] { hipLaunchKernelGGL(k_pq4_encode_any, grid, dim3(256), 0, st, x, ldx, n, codebooks, dsub, codes, ldc, dist, ldd); });
  return check_launch("pq4_encode");
}

extern "C" int cdml_pq4_lut(const float *Q, int64_t ldq, int nq, const float *codebooks, int M, int dsub, float *lut,
                            cdml_stream_t stream) {
  CDML_REQUIRE(Q && codebooks && lut, CDML_E_BADARG, "pq4_lut: null pointer");
  CDML_REQUIRE(nq > 0, CDML_E_BADARG, "pq4_lut: nq must be positive");
  CDML_REQUIRE_PQ_M("pq4_lut", M);
  CDML_REQUIRE(dsub >= 1, CDML_E_BADARG, "pq4_lut: dsub must be >= 1, got %d", dsub);
  CDML_REQUIRE(ldq >= (int64_t)2 * M * dsub, CDML_E_BADARG, "pq4_lut: ldq >= 2 M dsub (M = %d, dsub = %d)", M, dsub);
  CDML_REQUIRE(aligned16(lut), CDML_E_ALIGN, "pq4_lut: lut must be 16-B aligned");
  const int Ms = 2 * M;                                   // a multiple of 16: Ms / kLutSub blocks of 16 subspaces
  const dim3 grid((nq + kLutQ - 1) / kLutQ, Ms / kLutSub);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dsub(
      dsub,
      [&](auto ds) { hipLaunchKernelGGL(k_pq4_lut<decltype(ds)::value>, grid, dim3(256), 0, st, Q, ldq, nq, codebooks, Ms, lut); },
      [&] { hipLaunchKernelGGL(k_pq4_lut_any, grid, dim3(256), 0, st, Q, ldq, nq, codebooks, Ms, dsub, lut); });
  return check_launch("pq4_lut");
}

extern "C" int cdml_ivf_pq4_tile(int M, int *slots, int *rows) {
  CDML_REQUIRE(slots && rows, CDML_E_BADARG, "ivf_pq4_tile: null pointer");
  CDML_REQUIRE_PQ_M("ivf_pq4_tile", M);
  *slots = scan_slots(M);
  *rows = kTileRows;
  return CDML_OK;
}

extern "C" int cdml_ivf_scan_pq4(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                                 const int64_t *slot_off, const uint8_t *codes, int64_t ldc, const int32_t *list_start, int M,
                                 const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream) {
  if (int rc = check_pq_scan_args("ivf_scan_pq4", lut && slot_query && slot_start && slot_off && codes && list_start && tiles && scores,
                                  lut, n_queries, codes, ldc, M, tiles, n_tiles, scores))
    return rc;
  const int4 *tl = reinterpret_cast<const int4 *>(tiles);
  hipStream_t st = (hipStream_t)stream;
  dispatch_m8(M, [&](auto m8) {
    hipLaunchKernelGGL(k_ivf_scan_pq4<decltype(m8)::value>, dim3(n_tiles), dim3(kScanThreads), 0, st, lut, n_queries, slot_query,
                       slot_start, slot_off, codes, ldc, list_start, tl, scores);
  });
  return check_launch("ivf_scan_pq4");
}
