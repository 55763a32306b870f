/* cdml_ivf_f16.h -- C ABI of the fp16 lists of the IVF index and of its exact fp32 re-rank (build-defined, as the index
 * itself: cdml_ivf.h): csrc/ivf_f16.hip of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned
 * buffers, enqueue-only on `stream`, status ints, cdml_last_error()); the slot / tile / offset tables, the ragged score
 * buffer and cdml_ivf_merge are cdml_ivf.h's, unchanged.
 *
 * THE INDEX with storage "f16" keeps rows = the fp16 image (round to nearest even) of the prepared catalogue rows, cluster-
 * major, and r_sq = the fp32 squared norms OF THE ROUNDED VALUES; a row whose image has a non-finite coordinate is in no
 * list.  k-means, assign, centroids and the probes are those of the fp32 index.  A chunk's queries are rounded the same way
 * and q_sq comes from the rounded values; a query whose image is non-finite probes nothing.
 *
 * SEARCH without re-rank = EXACTLY the k best listed rows of the probed lists under the key (d~, id),
 *       d~ = (|q~|^2 + |x~|^2) - 2 s~, clamped as cdml_ivf_merge clamps, s~ = the fp32-accumulated inner product of the fp16
 *       images on v_mfma_f32_32x32x16_f16: a chain over k in an order that is a function of Dp alone, so the bits of
 *       s~(query, row) do not depend on the tile, the slot or the chunk it lands in.
 * SEARCH with re-rank r (k <= r <= CDML_KNN_LIST): the merge keeps r entries; cdml_ivf_refine re-scores them against fp32
 *       rows gathered by id and returns the k best under (d, id), d the fp32 distance of the fp32 rows.
 *
 * cdml_ivf_scan_f16: cdml_ivf_scan_f32 with fp16 operands.  Q fp16 [n_queries][ldq], rows fp16 [n_listed][ldr] (16-bit
 *   words; ldq, ldr in halves, multiples of 8, >= Dp); Dp a multiple of 32; Q, rows, tiles, scores 16-B aligned.  tiles,
 *   slot_query, slot_start, slot_off, list_start and scores as there: a tile is 128 slots x 128 rows, a slot or row past its
 *   list's end loads a clamped valid row and stores nothing, the pad floats [len, ld_c) of a score row are never written,
 *   all addressing is 64-bit.
 * cdml_ivf_refine: one wave per query q < nq.  Q fp32 [nq][ldq]; base fp32 [n_rows][ldb] (ldq, ldb >= Dp); cand int32
 *   [nq][CDML_KNN_LIST] = cdml_ivf_merge's best_i as it is (0x7fffffff = no candidate; an id outside [0, n_rows) counts as
 *   none).  For each of the first r candidates, d = sum_j (q_j - x_j)^2 over j < Dp in fp32: lane l of 64 adds its
 *   coordinates l, l + 64, ... in ascending order (fused multiply-add), then a fixed xor-butterfly (32, 16, ..., 1) adds the
 *   lanes; no expansion into norms, no clamp: d is a function of (q, x, Dp) alone.  A NaN d passes no compare and is no
 *   candidate.  The r keys (d, id) are sorted and the query's WHOLE list best_d / best_i [nq][CDML_KNN_LIST] is written:
 *   the valid keys ascending, then +inf / 0x7fffffff.  cand and best_i are different buffers.
 * Bad arguments (a null pointer, a non-positive size, Dp not a multiple of 32, strides not multiples of 8 halves or < Dp,
 * misaligned bases, 1 <= k <= r <= CDML_KNN_LIST violated) return a negative status before any HIP call. */
#ifndef CDML_IVF_F16_H_
#define CDML_IVF_F16_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_ivf_scan_f16(const uint16_t *Q, int64_t ldq, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                      const int64_t *slot_off, const uint16_t *rows, int64_t ldr, const int32_t *list_start, int Dp,
                      const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream);
int cdml_ivf_refine(const float *Q, int64_t ldq, int nq, const float *base, int64_t ldb, int64_t n_rows, int Dp,
                    const int32_t *cand, int r, int k, float *best_d, int32_t *best_i, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_F16_H_ */
