/* cdml_npair_bf16.h -- C ABI of the N-pair loss on the config-4 precision (fp16 catalogue, bf16 MFMA; build-defined, the
 * reference has only the triplet hinge): csrc/npair_bf16.hip and the one-plane forms of csrc/npair.hip's gradient-weight
 * kernels, of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on
 * `stream`, status ints, cdml_last_error()); the loss, its masks and the logQ / memory arguments are those of
 * cdml_npair_stats / cdml_npair_grad_f32 and their _memory_ / _logq_ forms there.
 *
 * The chain on this precision: the embedded rows e (fp32) -> their bf16 images -> S = A [P; Mem]^T by cdml_gemm_bf16_nt
 * (epilogue 3: S stays fp32) -> cdml_npair_stats / _memory_stats / _logq_stats as they are -> W as ONE bf16 plane ->
 * dA = W [P; Mem] by cdml_gemm_bf16_nt against the transposed image, dP = W^T A by cdml_gemm_bf16_tn -> the ring push.
 * bf16 buffers are passed as uint16_t*; every rounding is round-to-nearest-even (what tensor.to(bfloat16) does).
 *
 * cdml_npair_operands_bf16: the three operand images of a batch in one launch.  e fp32 [2B][lde], row 2i = a_i, row
 *   2i+1 = p_i, D columns.  A[i][c] = bf16(a_i[c]) (bf16 [B][lda]), P[i][c] = bf16(p_i[c]) (bf16 [B][ldp]) and the
 *   transposed PT[c][i] = P[i][c] (bf16 [D][ldt]: the k-contiguous operand of dA = W P; through a 64 x 64 LDS tile, so
 *   that both images are stored along contiguous addresses).  Only rows < B / columns < D of A and P and rows < D /
 *   columns < B of PT are written: a caller's zeroed padding stays zero.  The images are GEMM operands: e, A, P, PT 16-B
 *   aligned, lde a multiple of 4 and >= D, lda / ldp multiples of 8 and >= D, ldt a multiple of 8 and >= B.
 * cdml_npair_grad_bf16 / cdml_npair_logq_grad_bf16: W[i][j] bf16 [B][ldw] = the round-to-nearest-even of EXACTLY the fp32
 *   value cdml_npair_grad_f32 / cdml_npair_logq_grad_f32 write for the same S, lse, ids (and bias); entries no rule counts
 *   are exactly 0; only columns < B are written.  W 8-B aligned, ldw >= B and a multiple of 4.
 * cdml_npair_memory_grad_bf16 / cdml_npair_memory_logq_grad_bf16: the memory block W[i][mem_col + k], k < M, likewise
 *   the rounded value of cdml_npair_memory_grad_f32 / _logq_grad_f32; ldw >= mem_col + M.
 * cdml_npair_memory_push_bf16: cdml_npair_memory_push (the same step / start convention: slots s .. s + B - 1, s =
 *   ((t - start) mod (M / B)) B, of step t = step + *step_dev, nothing before `start`, M a multiple of B so a push never
 *   wraps) that also writes the slots' one-plane operand images R[(s + r) ldr + c] = T[c ldt + s + r] = bf16(P[r][c])
 *   beside the fp32 ring rows mem and their ids mem_id.  ldp, ldm, ldr >= D, ldt >= M.
 * Enqueue-only, no atomics, fixed summation orders: bit-reproducible.  Bad arguments (null pointers, B < 1, t <= 0 or not
 * finite, short or misaligned leading dimensions, an M that is no multiple of B for the push) return CDML_E_BADARG before
 * any HIP call. */
#ifndef CDML_NPAIR_BF16_H_
#define CDML_NPAIR_BF16_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_npair_operands_bf16(const float *e, int64_t lde, int B, int D, uint16_t *A, int64_t lda, uint16_t *P, int64_t ldp,
                             uint16_t *PT, int64_t ldt, cdml_stream_t stream);
int cdml_npair_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, float temperature, int symmetric,
                         const float *lse, uint16_t *W, int64_t ldw, cdml_stream_t stream);
int cdml_npair_logq_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, const float *bias, float temperature,
                              int symmetric, const float *lse, uint16_t *W, int64_t ldw, cdml_stream_t stream);
int cdml_npair_memory_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                const int32_t *mem_id, int M, float temperature, int symmetric, const float *lse,
                                uint16_t *W, int64_t ldw, cdml_stream_t stream);
int cdml_npair_memory_logq_grad_bf16(const float *S, int64_t lds, const int32_t *ids, int B, int64_t mem_col,
                                     const int32_t *mem_id, const float *mem_bias, int M, float temperature, int symmetric,
                                     const float *lse, uint16_t *W, int64_t ldw, cdml_stream_t stream);
int cdml_npair_memory_push_bf16(const float *P, int64_t ldp, const int32_t *ids, int B, int D, uint64_t step,
                                const uint64_t *step_dev, int64_t start, int M, float *mem, int64_t ldm, int32_t *mem_id,
                                uint16_t *R, int64_t ldr, uint16_t *T, int64_t ldt, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_NPAIR_BF16_H_ */
