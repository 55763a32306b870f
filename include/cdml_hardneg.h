/* cdml_hardneg.h -- C ABI of the listed ("hard") negatives: a triplet's negative drawn from a per-video candidate list
 * (the anchor's current nearest neighbours in the catalogue, mined with the exact kNN and refreshed as the model moves:
 * ANCE, Xiong et al. 2020; build-defined, the reference draws uniformly only): sampler mode 2 of csrc/sampler_gather.hip
 * of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on `stream`,
 * status ints, cdml_last_error()).
 *
 * The draw.  Inputs: the uniform sampler's arguments (pairs, n_pairs, n_rows, seed, step + *step_dev, batch, slot0,
 * batch_global: cdml_sample_uniform), `lists` int32 [n_rows][ldl] with L valid columns per row and -1 for an empty entry,
 * and hard_thresh = round(hard_fraction * 2^32), a uint64 in [0, 2^32].  For the triplet at `slot` of `step` with pair
 * ids (a, p) = pairs[(step * batch_global + slot) mod n_pairs]:
 *
 *   H  = WordStream(seed, step, slot, purpose = 2)          (purposes 0 = uniform negative and 1 = in-batch shift keep
 *                                                             their meaning; the stream is oracle/sampler.py's)
 *   w0 = H.next();  hard = (uint64) w0 < hard_thresh
 *   if hard and 0 <= a < n_rows:
 *       j_t = H.bounded(L) for t = 0..3                     (all four drawn before any list entry is read, so the four
 *                                                             list loads do not depend on one another)
 *       for t = 0..3 in order:
 *           c = lists[a * ldl + j_t]                        (skipped when the stream ran out: j_t < 0)
 *           if 0 <= c < n_rows and c != a and c != p: return c            kind = 1
 *   return the uniform negative of (seed, step, slot, a, p, n_rows)       kind = 0; cdml_sample_uniform's draw, unchanged
 *
 * So with hard_thresh = 0, with every list empty, or with an anchor outside the catalogue, the ids are bit-identical to
 * the uniform sampler's; a list entry that is empty, outside the catalogue, a or p is passed over; duplicates in a list
 * only weight the draw.  `lists` must hold n_rows rows: row a is read for every anchor 0 <= a < n_rows.
 *
 * cdml_sample_listed: ids only, the twin of cdml_sample_uniform -- idx_out int32 [3 * batch] = a, p, n per triplet;
 *   kind_out (or NULL) int32 [batch]: 1 when the negative came from the list, 0 otherwise.
 * cdml_sample_gather_listed / _x3 / _f16: the fused sampler + gather + input l2-normalise of cdml_sample_gather /
 *   cdml_sample_gather_x3 (x_ki == NULL) and _x3k (x_ki != NULL) / cdml_sample_gather_f16 in sampler mode 2: three rows per
 *   triplet, every layout rule, stride rule and the oob_flag (a PAIR id outside the catalogue) as there; kind_out (or
 *   NULL) int32 [n_steps][batch], steps kind_step_stride >= batch elements apart, written with plain stores by the lane
 *   that writes the negative's id.  The two-fp16-plane output (cdml_sample_gather_h2) has no listed form.
 * Bad arguments return CDML_E_BADARG (or the fused launch's own status) before any HIP call: lists NULL, L outside
 * [1, 1024], ldl < L, hard_thresh > 2^32, kind_step_stride < batch with n_steps > 1, and whatever the un-listed entry
 * point refuses.  Bit-reproducible: counter-based, no atomics but the oob flag's. */
#ifndef CDML_HARDNEG_H_
#define CDML_HARDNEG_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_sample_listed(const int32_t *pairs, int64_t n_pairs, int64_t n_rows, uint64_t seed, uint64_t step,
                       const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global, const int32_t *lists,
                       int64_t ldl, int L, uint64_t hard_thresh, int32_t *idx_out, int32_t *kind_out, cdml_stream_t stream);
int cdml_sample_gather_listed(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step, const uint64_t *step_dev,
                              int batch, int64_t slot0, int64_t batch_global, const float *table, int64_t n_rows,
                              int64_t row_stride, int F, const int32_t *lists, int64_t ldl, int L, uint64_t hard_thresh,
                              int32_t *idx_out, int32_t *kind_out, float *x_out, int64_t out_stride, int n_steps,
                              int64_t x_step_stride, int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag,
                              cdml_stream_t stream);
int cdml_sample_gather_listed_x3(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                 const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                 const float *table, int64_t n_rows, int64_t row_stride, int F, const int32_t *lists,
                                 int64_t ldl, int L, uint64_t hard_thresh, int32_t *idx_out, int32_t *kind_out,
                                 uint16_t *x_out_planes, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                 int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag, uint16_t *x_ki,
                                 int64_t ki_step_stride, cdml_stream_t stream);
int cdml_sample_gather_listed_f16(const int32_t *pairs, int64_t n_pairs, uint64_t seed, uint64_t step,
                                  const uint64_t *step_dev, int batch, int64_t slot0, int64_t batch_global,
                                  const uint16_t *table, int64_t n_rows, int64_t row_stride, int F, const int32_t *lists,
                                  int64_t ldl, int L, uint64_t hard_thresh, int32_t *idx_out, int32_t *kind_out,
                                  uint16_t *x_out_bf16, int64_t out_stride, int n_steps, int64_t x_step_stride,
                                  int64_t idx_step_stride, int64_t kind_step_stride, int32_t *oob_flag, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_HARDNEG_H_ */
