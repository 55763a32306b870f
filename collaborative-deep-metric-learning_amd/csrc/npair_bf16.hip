// The N-pair loss on the config-4 precision (fp16 catalogue, bf16 MFMA; include/cdml_npair_bf16.h; build-defined): the
// element-wise launches around the bf16 GEMMs that csrc/gemm_bf16.hip already has.  The chain is
//   e (fp32 unit rows) -> k_npair_operands_bf16 -> S = A [P; Mem]^T (cdml_gemm_bf16_nt, epilogue 3: fp32) -> the statistics
//   launches of csrc/npair.hip as they are -> W in ONE bf16 plane (the kWBf16 format of k_npair_w / k_npair_mem_w there)
//   -> dA = W [P; Mem] (cdml_gemm_bf16_nt against the transposed image), dP = W^T A (cdml_gemm_bf16_tn) -> the ring push
// where the plane path (precision f32x3) writes and reads three planes of every operand and runs six plane products per
// product.  One launch lives here, enqueue-only, no atomics, nothing summed:
//   k_npair_operands_bf16   the three operand images of a batch instead of three casts: A and P (row images) and PT, the
//                           positives transposed -- each e row is read once (fp32, a 256-B run per wave), A and P are
//                           stored one bf16 per lane (a 128-B run per wave) and PT goes through a 64 x 64 LDS tile so that
//                           its stores are 128-B runs along contiguous addresses too (k_mixed_split's and
//                           k_npair_mem_push's pattern)
// (the ring push with one-plane slot images, cdml_npair_memory_push_bf16, is k_npair_mem_push<kWBf16> of csrc/npair.hip)
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
