/* cdml_npair_dp.h -- C ABI of the data-parallel multi-class N-pair loss (one softmax over every rank's positives;
 * build-defined, the reference has only the triplet hinge): csrc/npair_dp.hip of libcdml_hip.so.  The conventions are
 * cdml.h's (device pointers, caller-owned buffers, enqueue-only on `stream`, status ints, cdml_last_error()).
 *
 * W ranks of B pairs each, G = W B global pairs; this rank's local pair i is the global pair col0 + i (col0 = rank B).
 * The loss is cdml_npair_stats' on the G global pairs; a rank computes its B rows of it.
 *   ids_all   int32 [2G], laid out like cdml_npair_stats' ids over the GLOBAL batch: ids_all[2j] = id(a_j), ids_all[2j+1] =
 *             id(p_j) (every rank's sampler slice, gathered; NULL = every row a video of its own).  The column rule of
 *             column j reads id(a_j) too, so both ids of a pair travel.
 *   S         fp32 [B][lds], S[i][j] = <a_(col0+i), p_j> for j < G: this rank's anchors against every rank's positives;
 *             the diagonal of local row i sits at column col0 + i.  t = temperature.
 *   row term     column j counts for local row i when j == col0 + i or id(p_j) is neither id(a_(col0+i)) nor id(p_(col0+i))
 *   column term  local row i counts for column j when col0 + i == j or id(a_(col0+i)) is neither id(a_j) nor id(p_j)
 *
 * cdml_npair_dp_local_stats: lse_row[i] = log sum_j m_ij exp(S_ij / t) over all G columns (float [B]); the row's loss /
 *   stat partials into the workspace (read back by cdml_npair_dp_stats: the SAME workspace goes to both); symmetric != 0:
 *   colpart float [G][2] = the (max, sum of exp(. - max)) of column j's counted logits over this rank's B rows -- a
 *   column without a counted local row is (-inf, 0).  symmetric == 0: colpart is not written (may be NULL).
 *   workspace: cdml_npair_dp_workspace(B, G) bytes, 16-B aligned.
 * cdml_npair_dp_col_fold: lse_col[j] = log sum over every rank's counted rows, from the gathered partials colpart_all float
 *   [world][G][2]: the ranks are folded in the order 0 .. world - 1 (the same bits on every rank); a (-inf, 0) partial
 *   folds without a NaN, a column nobody counted gives -inf.  No relation between G and world is assumed here.
 * cdml_npair_dp_stats: stats[0] = mean_i (lse_row_i - S_ii / t), or with symmetric the mean of that and of the column term
 *   of the B columns this rank owns, mean_i (lse_col[col0 + i] - S_ii / t) -- this rank's share: the mean over the ranks
 *   is the loss of the global batch; [1] = mean 2 - 2 S_ii; [2] = mean 2 - 2 S over the local rows' counted negatives, [3]
 *   = their fraction of B (G - 1).
 * cdml_npair_dp_grad_x3 / _f32: the gradient weights of this rank's rows, W[i][j] = (m_ij exp(S_ij / t - lse_row_i) - d) /
 *   (B t), with symmetric the mean of that and (m'_ij exp(S_ij / t - lse_col_j) - d) / (B t), d = 1 at j == col0 + i -- the
 *   LOCAL-mean scale: averaging the ranks' parameter gradients gives the global mean's.  Entries neither rule counts are
 *   exactly 0.  _x3: three exact bf16 planes W[i][p * plane + j] (cdml_split_f32_bf16x3's split; 8-B aligned, plane >= G,
 *   ldw >= 2 plane + G); _f32: fp32 W[B][ldw] (16-B aligned, ldw >= G).  dA = W P_all; W^T A is this rank's partial
 *   gradient of ALL G positives, whose row blocks go back to their owners.
 * cdml_npair_dp_pos_fold: de[(2i + 1) ldde + c] = recv[0][i][c] + recv[1][i][c] + ... + recv[world - 1][i][c] (fp32, in that
 *   order) for i < B, c < D: the owners' sum of the partial positive gradients, recv float [world][B][ldr].  Rows 2i of de
 *   and columns >= D are not written.
 * Every size that is vectorised is a multiple of 4: G, D, col0, every leading dimension and plane stride; S, ids_all,
 * lse_row, lse_col, colpart, colpart_all, recv, de 16-B aligned.  0 <= col0, col0 + B <= G.
 * Enqueue-only, no atomics, fixed summation orders: bit-reproducible.  Bad arguments (null pointers, sizes out of range,
 * t <= 0 or not finite, short or misaligned leading dimensions, a short workspace) return CDML_E_BADARG before any HIP
 * call. */
#ifndef CDML_NPAIR_DP_H_
#define CDML_NPAIR_DP_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t cdml_npair_dp_workspace(int B, int G);
int cdml_npair_dp_local_stats(const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0, float temperature,
                              int symmetric, float *lse_row, float *colpart, void *workspace, size_t workspace_bytes,
                              cdml_stream_t stream);
int cdml_npair_dp_col_fold(const float *colpart_all, int world, int G, float *lse_col, cdml_stream_t stream);
int cdml_npair_dp_stats(const float *S, int64_t lds, int B, int G, int col0, float temperature, int symmetric,
                        const float *lse_col, float *stats, const void *workspace, size_t workspace_bytes,
                        cdml_stream_t stream);
int cdml_npair_dp_grad_x3(const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0, float temperature,
                          int symmetric, const float *lse_row, const float *lse_col, uint16_t *W, int64_t ldw, int64_t plane,
                          cdml_stream_t stream);
int cdml_npair_dp_grad_f32(const float *S, int64_t lds, const int32_t *ids_all, int B, int G, int col0, float temperature,
                           int symmetric, const float *lse_row, const float *lse_col, float *W, int64_t ldw,
                           cdml_stream_t stream);
int cdml_npair_dp_pos_fold(const float *recv, int64_t ldr, int world, int B, int D, float *de, int64_t ldde,
                           cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_NPAIR_DP_H_ */
