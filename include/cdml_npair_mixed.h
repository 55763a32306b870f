/* cdml_npair_mixed.h -- C ABI of the N-pair loss with mixed negative sampling (Yang et al., WWW 2020 companion;
 * build-defined, the reference has only the triplet hinge): csrc/npair_mixed.hip of libcdml_hip.so.  The conventions are
 * cdml.h's (device pointers, caller-owned buffers, enqueue-only on `stream`, status ints, cdml_last_error()).
 *
 * A batch of B triplets in the uniform sampler's own layout: ids int32 [3B] with ids[3i] = id(a_i), ids[3i+1] = id(p_i),
 * ids[3i+2] = id(n_i) (cdml_sample_uniform's idx; NULL = every row a video of its own), embedded rows e[3i], e[3i+1],
 * e[3i+2].  The softmax of anchor i runs over the column set [P | N | Mem]: S fp32 [B][lds] = A [P; N; Mem]^T with the
 * in-batch block at columns 0 .. B-1, the uniform block at neg_col .. neg_col + B - 1 and (M > 0) the memory block at
 * mem_col .. mem_col + M - 1; t = temperature.
 *   in-batch block   column j counts for row i when j == i or id(p_j) is neither id(a_i) nor id(p_i); the column term
 *                    (symmetric) over this block only: row i counts for column j when i == j or id(a_i) is neither
 *                    id(a_j) nor id(p_j) -- cdml_npair_stats' rules
 *   uniform block    column j counts for row i when id(n_j) is neither id(a_i) nor id(p_i) (no special diagonal: the
 *                    sampler guarantees it for j == i)
 *   memory block     slot k counts when mem_id[k] >= 0 is neither id(a_i) nor id(p_i) -- cdml_npair_memory_stats' rule
 *   lse_i = log( sum_j m_ij exp(S_ij / t - lq(p_j)) + sum_j cn_ij exp(U_ij / t - lq_u) + sum_k cm_ik exp(Sm_ik / t - lq(mem_k)) )
 * The sampling-bias correction (logQ): bias fp32 [2B] laid out as cdml_logq_*_gather writes it for the [2B] ids (a_i, p_i)
 * -- bias[2i] = lq(a_i), bias[2i+1] = lq(p_i) --, mem_bias [M], and lq_u, ONE scalar for the whole uniform block (a
 * uniform draw has one probability; a non-uniform proposal takes one value per negative through the _nb entry points of
 * cdml_negweights.h).  bias == NULL: the uncorrected loss (lq_u and mem_bias are not read).
 *
 * cdml_npair_mixed_stats: lse[i] as above, symmetric != 0 also lse[B + j] = the in-batch column's (lse float [2B]);
 *   stats[0] = mean_i (lse_i - (S_ii / t - lq(p_i))) or the mean of that and the column term; [1] = mean 2 - 2 S_ii;
 *   [2] = mean 2 - 2 S over the counted negatives of all three blocks, [3] = their fraction of B (B - 1) + B B + B M.
 *   workspace: cdml_npair_mixed_workspace(B, M) bytes, 16-B aligned.
 * cdml_npair_mixed_grad_x3 / _f32: ONE launch writes the gradient weights of all blocks -- in-batch as
 *   cdml_npair_grad_* with this lse, W[i][neg_col + j] = cn_ij exp(U_ij / t - lq_u - lse_i) / (B t) and
 *   W[i][mem_col + k] = cm_ik exp(Sm_ik / t - lq(mem_k) - lse_i) / (B t), both halved with symmetric; entries a rule
 *   does not count are exactly 0; columns between the blocks are not written.  _x3: three exact bf16 planes
 *   W[i][p * plane + c] (cdml_split_f32_bf16x3's split; 8-B aligned, plane >= the column span, ldw >= 2 plane + span);
 *   _f32: fp32 W[B][ldw] (16-B aligned, ldw >= span).  span = mem_col + M, or neg_col + B without a memory.
 *   dA = W [P; N; Mem] is one product over the span; dP = W_p^T A; dN = W_n^T A (the uniform negatives get a gradient,
 *   the memory none).
 * cdml_npair_mixed_split_x3: the bf16 plane images of the embedded rows straight from e's stride-3 rows (e fp32
 *   [3B][lde], D columns) -- A3[i][p * plane_a + c] = plane p of a_i[c]; the row image R3[i][..] = p_i, R3[neg_row + i][..]
 *   = n_i (plane stride plane_r); the transposed image T3[c][p * plane_t + i] = p_i[c], T3[c][p * plane_t + neg_row + i] =
 *   n_i[c].  Only rows < B (of each block) and columns < D are written.
 * Every size that is vectorised is a multiple of 4: B, M, D, neg_col, mem_col, neg_row, every leading dimension and
 * plane stride; S, ids, mem_id, bias, mem_bias, lse, e 16-B aligned.  neg_col >= B, mem_col >= neg_col + B.
 * Enqueue-only, no atomics, fixed summation orders: bit-reproducible.  Bad arguments (null pointers, sizes that are not
 * positive multiples of 4, t <= 0 or not finite, lq_u not finite, short or misaligned leading dimensions, a short
 * workspace) return CDML_E_BADARG before any HIP call. */
#ifndef CDML_NPAIR_MIXED_H_
#define CDML_NPAIR_MIXED_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t cdml_npair_mixed_workspace(int B, int M);
int cdml_npair_mixed_stats(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                           const int32_t *mem_id, int M, const float *bias, float lq_u, const float *mem_bias,
                           float temperature, int symmetric, float *lse, float *stats, void *workspace,
                           size_t workspace_bytes, cdml_stream_t stream);
int cdml_npair_mixed_grad_x3(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                             const int32_t *mem_id, int M, const float *bias, float lq_u, const float *mem_bias,
                             float temperature, int symmetric, const float *lse, uint16_t *W, int64_t ldw, int64_t plane,
                             cdml_stream_t stream);
int cdml_npair_mixed_grad_f32(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                              const int32_t *mem_id, int M, const float *bias, float lq_u, const float *mem_bias,
                              float temperature, int symmetric, const float *lse, float *W, int64_t ldw,
                              cdml_stream_t stream);
int cdml_npair_mixed_split_x3(const float *e, int64_t lde, int B, int D, uint16_t *A3, int64_t lda, int64_t plane_a,
                              uint16_t *R3, int64_t ldr, int64_t plane_r, uint16_t *T3, int64_t ldt, int64_t plane_t,
                              int64_t neg_row, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_NPAIR_MIXED_H_ */
