// The N-pair loss on the config-4 precision (fp16 catalogue, bf16 MFMA; include/cdml_npair_bf16.h; build-defined): the
// element-wise launches around the bf16 GEMMs that csrc/gemm_bf16.hip already has.  The chain is
//   e (fp32 unit rows) -> k_npair_operands_bf16 -> S = A [P; Mem]^T (cdml_gemm_bf16_nt, epilogue 3: fp32) -> the statistics
//   launches of csrc/npair.hip as they are -> W in ONE bf16 plane (the kWBf16 format of k_npair_w / k_npair_mem_w there)
//   -> dA = W [P; Mem] (cdml_gemm_bf16_nt against the transposed image), dP = W^T A (cdml_gemm_bf16_tn) -> the ring push
// where the plane path (precision f32x3) writes and reads three planes of every operand and runs six plane products per
// product.  Two launches live here, both enqueue-only, no atomics, nothing summed:
//   k_npair_operands_bf16   the three operand images of a batch instead of three casts: A and P (row images) and PT, the
//                           positives transposed -- each e row is read once (fp32, a 256-B run per wave), A and P are
//                           stored one bf16 per lane (a 128-B run per wave) and PT goes through a 64 x 64 LDS tile so that
//                           its stores are 128-B runs along contiguous addresses too (k_mixed_split's and
//                           k_npair_mem_push's pattern)
//   k_npair_mem_push_bf16   k_npair_mem_push with one-plane slot images
// Every bf16 is the round-to-nearest-even of its fp32 value (the conversion of cdml_cast_f32_bf16 and tensor.to(bfloat16)).
#include "common.h"
#include "../../include/cdml_npair_bf16.h"

namespace cdml {
namespace {

constexpr int kObThreads = 256;
constexpr int kObTile = 64;
constexpr int kObStep = kObThreads / kObTile;      // tile rows per pass

// block (x, y): columns 64 x .. + 63 of pairs 64 y .. + 63.  e[2 i] = a_i, e[2 i + 1] = p_i
__global__ void __launch_bounds__(kObThreads)
k_npair_operands_bf16(const float *__restrict__ e, int64_t lde, int B, int D, __bf16 *__restrict__ A, int64_t lda,
                      __bf16 *__restrict__ P, int64_t ldp, __bf16 *__restrict__ PT, int64_t ldt) {
  __shared__ float tile[kObTile][kObTile + 1];
  const int c0 = blockIdx.x * kObTile, r0 = blockIdx.y * kObTile;
  const int lane = threadIdx.x % kObTile, sub = threadIdx.x / kObTile;
  for (int r = sub; r < kObTile; r += kObStep) {
    const int gr = r0 + r, gc = c0 + lane;
    if (gr >= B || gc >= D) continue;
    const float *src = e + 2 * (int64_t)gr * lde + gc;
    const float a = src[0], p = src[lde];
    A[(int64_t)gr * lda + gc] = (__bf16)a;
    P[(int64_t)gr * ldp + gc] = (__bf16)p;
    tile[r][lane] = p;
  }
  __syncthreads();
  for (int c = sub; c < kObTile; c += kObStep) {
    const int gr = r0 + lane, gc = c0 + c;
    if (gr >= B || gc >= D) continue;              // (the same pairs and columns as above: every entry read was written)
    PT[(int64_t)gc * ldt + gr] = (__bf16)tile[lane][c];
  }
}

// The ring push of step t = step_imm + *step_dev (when t >= start): slots s .. s + B - 1, s = ((t - start) mod (M / B)) B,
// take the B positives P[r] (fp32 rows, D columns) and their ids ids[2 r + 1], and the slots' operand images
// R[s + r][c] = T[c][s + r] = bf16(P[r][c]); block (x, y): columns 64 x .. of positives 64 y ..
__global__ void __launch_bounds__(kObThreads)
k_npair_mem_push_bf16(const float *__restrict__ P, int64_t ldp, const int32_t *__restrict__ ids, int B, int D,
                      uint64_t step_imm, const uint64_t *__restrict__ step_dev, int64_t start, int M, float *__restrict__ mem,
                      int64_t ldm, int32_t *__restrict__ mem_id, __bf16 *__restrict__ R, int64_t ldr, __bf16 *__restrict__ T,
                      int64_t ldt) {
  __shared__ float tile[kObTile][kObTile + 1];
  const uint64_t t = step_imm + (step_dev ? *step_dev : 0);
  if (t < (uint64_t)start) return;                 // (the whole grid takes the same branch: no barrier is skipped by some)
  const int64_t s = (int64_t)((t - (uint64_t)start) % (uint64_t)(M / B)) * B;
  const int c0 = blockIdx.x * kObTile, r0 = blockIdx.y * kObTile;
  const int lane = threadIdx.x % kObTile, sub = threadIdx.x / kObTile;
  if (blockIdx.x == 0 && threadIdx.x < kObTile && r0 + (int)threadIdx.x < B)
    mem_id[s + r0 + threadIdx.x] = ids[2 * (r0 + threadIdx.x) + 1];
  for (int r = sub; r < kObTile; r += kObStep) {
    const int gr = r0 + r, gc = c0 + lane;
    if (gr >= B || gc >= D) continue;
    const float v = P[(int64_t)gr * ldp + gc];
    mem[(s + gr) * ldm + gc] = v;
    R[(s + gr) * ldr + gc] = (__bf16)v;
    tile[r][lane] = v;
  }
  __syncthreads();
  for (int c = sub; c < kObTile; c += kObStep) {
    const int gr = r0 + lane, gc = c0 + c;
    if (gr >= B || gc >= D) continue;
    T[(int64_t)gc * ldt + s + gr] = (__bf16)tile[lane][c];
  }
}

}  // namespace
}  // namespace cdml

using namespace cdml;

extern "C" int cdml_npair_operands_bf16(const float *e, int64_t lde, int B, int D, uint16_t *A, int64_t lda, uint16_t *P,
                                        int64_t ldp, uint16_t *PT, int64_t ldt, cdml_stream_t stream) {
  CDML_REQUIRE(e && A && P && PT, CDML_E_BADARG, "npair_operands_bf16: null pointer");
  CDML_REQUIRE(B >= 1 && D >= 1, CDML_E_BADARG, "npair_operands_bf16: needs B >= 1 and D >= 1 (got B %d, D %d)", B, D);
  CDML_REQUIRE(lde >= D && (lde & 3) == 0 && lda >= D && (lda & 7) == 0 && ldp >= D && (ldp & 7) == 0 && ldt >= B &&
                   (ldt & 7) == 0,
               CDML_E_BADARG,
               "npair_operands_bf16: needs lde >= D (%d), a multiple of 4; lda and ldp >= D, multiples of 8; ldt >= B (%d), a "
               "multiple of 8 (got lde %lld, lda %lld, ldp %lld, ldt %lld)", D, B, (long long)lde, (long long)lda,
               (long long)ldp, (long long)ldt);
  CDML_REQUIRE(aligned16(e) && aligned16(A) && aligned16(P) && aligned16(PT), CDML_E_BADARG,
               "npair_operands_bf16: e, A, P and PT need 16-B aligned bases (the images are GEMM operands)");
  const dim3 grid((unsigned)((D + kObTile - 1) / kObTile), (unsigned)((B + kObTile - 1) / kObTile));
  hipLaunchKernelGGL(k_npair_operands_bf16, grid, dim3(kObThreads), 0, (hipStream_t)stream, e, lde, B, D,
                     reinterpret_cast<__bf16 *>(A), lda, reinterpret_cast<__bf16 *>(P), ldp, reinterpret_cast<__bf16 *>(PT), ldt);
  return check_launch("npair_operands_bf16");
}

extern "C" int cdml_npair_memory_push_bf16(const float *P, int64_t ldp, const int32_t *ids, int B, int D, uint64_t step,
                                           const uint64_t *step_dev, int64_t start, int M, float *mem, int64_t ldm,
                                           int32_t *mem_id, uint16_t *R, int64_t ldr, uint16_t *T, int64_t ldt,
                                           cdml_stream_t stream) {
  CDML_REQUIRE(P && ids && mem && mem_id && R && T, CDML_E_BADARG, "npair_memory_push_bf16: null pointer");
  CDML_REQUIRE(B >= 1 && D >= 1 && M >= B && M % B == 0, CDML_E_BADARG,
               "npair_memory_push_bf16: needs B >= 1, D >= 1 and M a multiple of B (got B %d, D %d, M %d)", B, D, M);
  CDML_REQUIRE(ldp >= D && ldm >= D && ldr >= D && ldt >= M && start >= 0, CDML_E_BADARG,
               "npair_memory_push_bf16: ldp, ldm and ldr must be >= D (%d), ldt >= M (%d) and start >= 0 (got ldp %lld, ldm "
               "%lld, ldr %lld, ldt %lld, start %lld)", D, M, (long long)ldp, (long long)ldm, (long long)ldr, (long long)ldt,
               (long long)start);
  const dim3 grid((unsigned)((D + kObTile - 1) / kObTile), (unsigned)((B + kObTile - 1) / kObTile));
  hipLaunchKernelGGL(k_npair_mem_push_bf16, grid, dim3(kObThreads), 0, (hipStream_t)stream, P, ldp, ids, B, D, step, step_dev,
                     start, M, mem, ldm, mem_id, reinterpret_cast<__bf16 *>(R), ldr, reinterpret_cast<__bf16 *>(T), ldt);
  return check_launch("npair_memory_push_bf16");
}
