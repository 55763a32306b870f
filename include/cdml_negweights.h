/* cdml_negweights.h -- C ABI of the popularity-weighted negatives: a triplet's negative drawn from a proposal distribution
 * over the catalogue given as integer tables (unigram^0.75 of word2vec, Mikolov et al. 2013, and its mixtures with uniform;
 * build-defined, the reference draws uniformly only) -- sampler mode 3 of csrc/sampler_gather.hip -- and the per-negative
 * logQ correction of the mixed N-pair softmax that goes with it (the importance-sampled softmax of Bengio & Senecal 2008):
 * csrc/npair_mixed.hip, csrc/negweights.hip of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned
 * buffers, enqueue-only on `stream`, status ints, cdml_last_error()).
 *
 * The tables (cdml_amd/negweights.py builds them).  Row v of the catalogue owns quanta[v] of the 2^32 values of a 32-bit
 * word, sum quanta = 2^32 exactly, quanta[v] = 0 exactly for the rows of weight 0:
 *   start   uint32 bits in int32 [n_live]: the exclusive prefix sum of quanta; n_live = 1 + the last row with quanta > 0
 *           (rows at or after n_live own nothing; their prefix, 2^32, does not fit)
 *   coarse  int32 [2^bits + 1], bits in [8, 24]: coarse[b] = owner(b << (32 - bits)), coarse[2^bits] = n_live - 1
 *   owner(r) = the largest v < n_live with start[v] <= r; that row has quanta > 0, row v owns exactly quanta[v] words, and
 *           owner(r) lies in [coarse[r >> (32 - bits)], coarse[(r >> (32 - bits)) + 1]]
 *
 * The draw.  Inputs: the uniform sampler's arguments (cdml_sample_uniform) and the tables.  For the triplet at `slot` of
 * `step` with pair ids (a, p) = pairs[(step * batch_global + slot) mod n_pairs]:
 *
 *   H = WordStream(seed, step, slot, purpose = 3)            (purposes 0 = uniform negative, 1 = in-batch shift and 2 = listed
 *                                                             negative keep their meaning; the stream is oracle/sampler.py's)
 *   while not H.exhausted():                                 (64 words)
 *       r = H.next();  v = owner(r)                          (one coarse[] load, then a binary search in start[lo..hi])
 *       if v != a and v != p: return v                       kind = 1
 *   return the uniform negative of (seed, step, slot, a, p, n_rows)       kind = 0; cdml_sample_uniform's draw, unchanged
 *
 * A pure function of the tables and the counter; the search bounds are clamped into [0, n_live), so a malformed table
 * cannot index outside `start` (coarse is read at r >> (32 - bits) and the entry after it: it must hold 2^bits + 1 entries).
 * The probability of row v under this draw is quanta[v] / 2^32 up to the redraws on {a, p}.
 *
 * cdml_sample_weighted: ids only, the twin of cdml_sample_listed -- idx_out int32 [3 * batch] = a, p, n per triplet;
 *   kind_out (or NULL) int32 [batch]: 1 when the negative came from the weighted draw, 0 from the fall-back.
 * cdml_sample_gather_weighted / _x3 / _f16: the fused sampler + gather + input l2-normalise in sampler mode 3 -- every
 *   argument after the tables, every layout and stride rule, the oob_flag (a PAIR id outside the catalogue; the triplet is
 *   still drawn) and kind_out [n_steps][batch] as cdml_sample_gather_listed / _x3 / _f16 (cdml_hardneg.h).  The
 *   two-fp16-plane output (cdml_sample_gather_h2) has no weighted form.
 * Bad arguments return CDML_E_BADARG (or the fused launch's own status) before any HIP call: a null table, n_live outside
 * [3, n_rows], bits outside [8, 24], kind_step_stride < batch with n_steps > 1, and whatever the un-weighted twin refuses.
 *
 * The per-negative bias of the mixed N-pair loss (cdml_npair_mixed.h).  cdml_npair_mixed_stats_nb / _grad_x3_nb /
 * _grad_f32_nb are cdml_npair_mixed_stats / _grad_x3 / _grad_f32 with `const float *neg_bias` in place of the scalar lq_u:
 * fp32 [B], 16-B aligned, one entry per column of the uniform block, whose logit becomes U_ij / t - neg_bias[j]; the masks,
 * the in-batch block, the memory block and the column term are unchanged.  neg_bias is required when bias != NULL and not
 * read otherwise.  With neg_bias[j] = c for every j the results are those of the scalar entry points at lq_u = c.
 * cdml_negw_bias: neg_bias[j] = lq[ids3[3j + 2]] + offset for j < B (lq fp32 [n_rows], ids3 the sampler's [3B] layout);
 *   an id outside [0, n_rows) gives 0. */
#ifndef CDML_NEGWEIGHTS_H_
#define CDML_NEGWEIGHTS_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_sample_weighted(const int32_t *pairs, int64_t n_pairs, int64_t n_rows, uint64_t seed, uint64_t step,
                         const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global, const int32_t *start,
                         int64_t n_live, const int32_t *coarse, int bits, int32_t *idx_out, int32_t *kind_out,
                         cdml_stream_t stream);
int cdml_sample_gather_weighted(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step, const uint64_t *step_dev,
                                int batch, int64_t slot0, int64_t batch_global, const float *table, int64_t n_rows,
                                int64_t row_stride, int F, const int32_t *start, int64_t n_live, const int32_t *coarse,
                                int bits, int32_t *idx_out, int32_t *kind_out, float *x_out, int64_t out_stride, int n_steps,
                                int64_t x_step_stride, int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag,
                                cdml_stream_t stream);
int cdml_sample_gather_weighted_x3(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                   const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                   const float *table, int64_t n_rows, int64_t row_stride, int F, const int32_t *start,
                                   int64_t n_live, const int32_t *coarse, int bits, int32_t *idx_out, int32_t *kind_out,
                                   uint16_t *x_out_planes, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                   int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag, uint16_t *x_ki,
                                   int64_t ki_step_stride, cdml_stream_t stream);
int cdml_sample_gather_weighted_f16(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                    const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                    const uint16_t *table, int64_t n_rows, int64_t row_stride, int F, const int32_t *start,
                                    int64_t n_live, const int32_t *coarse, int bits, int32_t *idx_out, int32_t *kind_out,
                                    uint16_t *x_out_bf16, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                    int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream);

int cdml_npair_mixed_stats_nb(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                              const int32_t *mem_id, int M, const float *bias, const float *neg_bias, const float *mem_bias,
                              float temperature, int symmetric, float *lse, float *stats, void *workspace,
                              size_t workspace_bytes, cdml_stream_t stream);
int cdml_npair_mixed_grad_x3_nb(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                                const int32_t *mem_id, int M, const float *bias, const float *neg_bias, const float *mem_bias,
                                float temperature, int symmetric, const float *lse, uint16_t *W, int64_t ldw, int64_t plane,
                                cdml_stream_t stream);
int cdml_npair_mixed_grad_f32_nb(const float *S, int64_t lds, const int32_t *ids, int B, int64_t neg_col, int64_t mem_col,
                                 const int32_t *mem_id, int M, const float *bias, const float *neg_bias, const float *mem_bias,
                                 float temperature, int symmetric, const float *lse, float *W, int64_t ldw,
                                 cdml_stream_t stream);
int cdml_negw_bias(const float *lq, int64_t n_rows, const int32_t *ids3, int B, float offset, float *neg_bias,
                   cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_NEGWEIGHTS_H_ */
