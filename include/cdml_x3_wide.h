/* cdml_x3_wide.h -- C ABI of the first layer's weight gradient with its data-gradient operand k8-interleaved (csrc/
 * gemm_bf16x3.hip, csrc/gemm_bf16_256.hip of libcdml_hip.so).  The conventions are cdml.h's (device pointers, caller-owned
 * buffers, enqueue-only on `stream`, status ints, cdml_last_error()).
 *
 * cdml_gemm_bf16x3_tn_kb: C[M][N] (fp32) = sum_k A[k][m] B[k][n], six plane products, like cdml_gemm_bf16x3_tn with ONLY B
 * k8-interleaved:
 *   A  row-major bf16 planes [K][lda], plane p at columns p * plane_a (a column window is a moved base, as there);
 *   B  bf16 [3 planes][K / 8][nb][8 rows] (what epilogue 12 of cdml_gemm_bf16x3_nt and cdml_interleave8_bf16x3 write), the
 *      product takes columns [b_col0, b_col0 + N) of every row group.
 * A wave's tile of the k-strided kernel is 128 x 64, so the row operand A supplies two thirds of the fragment reads; this
 * entry's kernel tiles its waves 64 x 128 instead, so that the interleaved operand B does -- each of its fragments one aligned
 * 16-B LDS read instead of two transposed ones.  Same LDS images, DMA schedule, plane-product order and K partition as the
 * row-major form: C and colsum[n] = sum_k B[k][n] (nullable) are bit-identical to cdml_gemm_bf16x3_tn's.  M, N % 256 == 0,
 * K % 128 == 0; the split rule, slab sum and workspace of the row-major form (cdml_gemm_bf16x3_workspace(1, M, N, K, 6)). */
#ifndef CDML_X3_WIDE_H
#define CDML_X3_WIDE_H
#include "cdml.h"
#ifdef __cplusplus
extern "C" {
#endif
int cdml_gemm_bf16x3_tn_kb(const uint16_t *A, int64_t lda, int64_t plane_a, const uint16_t *B, int nb, int b_col0,
                           int M, int N, int K, float *C, int64_t ldc, float *colsum, void *workspace,
                           size_t workspace_bytes, cdml_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
