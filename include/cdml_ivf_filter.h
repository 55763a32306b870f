/* cdml_ivf_filter.h -- C ABI of the threshold-filter scan of the IVF index (build-defined, as the index itself: cdml_ivf.h,
 * cdml_ivf_f16.h): csrc/ivf_filter.hip of libcdml_hip.so; DESIGN.md section 9f.2.  The conventions are cdml.h's (device
 * pointers, caller-owned buffers, enqueue-only on `stream`, status ints, cdml_last_error()); the slot and tile tables are
 * cdml_ivf.h's, unchanged.
 *
 * SEARCH with scan = "filter" (knn.IVFIndex.search), per query chunk and with keep = the re-rank width r, or k without one:
 *   1. seed     the first s columns of the probe table through the buffered launches (cdml_ivf_scan_f32 | _f16, then
 *               cdml_ivf_merge with k = keep): every query's sorted list, and tau[q] = its keep-th distance (+inf where
 *               fewer than keep rows were seeded);
 *   2. filter   the other columns through ONE launch of this header over cdml_ivf.h's tile table: the same grouped product,
 *               no score written; every (query q, listed row x) element with d <= tau[q] is appended to q's candidate list;
 *   3. merge    cdml_knn_merge_list (cdml.h) folds the candidates into the seeded lists;
 *   4. a query whose count exceeded cap lost candidates: the caller searches it again through the buffered launches.
 * THE CONTRACT: the first keep entries of every query's list are those of the buffered search (cdml_ivf_merge over all nprobe
 * columns), bit for bit, for either storage, any keep, chunking, query order, cap and s.  The seed and the filter columns are
 * disjoint lists, so no row appears twice; every row of a non-seed list that belongs to the keep best has d <= tau; the
 * products carry the buffered scan's bits (below).  Entries behind keep are NOT promised: cdml_knn_merge_list filters against
 * the keep-th key.
 *
 * cdml_ivf_filter_f32 / cdml_ivf_filter_f16: Q, ldq, n_queries, slot_query, slot_start, rows, ldr, list_start, Dp, tiles and
 *   n_tiles as cdml_ivf_scan_f32 / cdml_ivf_scan_f16 take them (a tile is 128 slots x 128 rows; a slot or row past its list's
 *   end loads a clamped valid row; 64-bit addressing) and the SAME tile loop: the bits of a (query, row) product s are those
 *   of the buffered scan.  In place of slot_off and scores:
 *     q_sq, tau fp32 [n_queries], cnt int32 [n_queries]   per query of the chunk;
 *     r_sq fp32 [n_listed], ids int32 [n_listed]          per listed row, in list order;
 *     cand [n_queries][cap] pairs of 32-bit words, cap a power of two.
 *   Per element: d = (q_sq[q] + r_sq[row]) - 2 s, then d = 0 where d < 0 (a compare that keeps a NaN) -- cdml_ivf_merge's
 *   arithmetic to the letter; 2 s is exact, so contracting the subtraction into a fused multiply-add changes no bit.  Where
 *   d <= tau[q] (a NaN d or tau passes no compare): pos = atomic cnt[q] += 1 (integer atomics only); when pos < cap,
 *   cand[q * cap + pos] = (the bits of d, ids[row]).  cnt counts the dropped ones too: cnt[q] > cap says that q lost
 *   candidates.  A slot or row past its list's end appends nothing; nothing else is written: no score, no slot of cand from
 *   min(cnt[q], cap) on.  The ORDER of a query's candidates depends on the schedule; their SET does not.
 * Bad arguments (a null pointer, a non-positive size, Dp not a multiple of 32, cap not a positive power of two, strides not
 * multiples of 4 floats | 8 halves or < Dp, Q, rows or tiles not 16-B aligned, cand not 8-B aligned) return a negative status
 * before any HIP call. */
#ifndef CDML_IVF_FILTER_H_
#define CDML_IVF_FILTER_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_ivf_filter_f32(const float *Q, int64_t ldq, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                        const float *q_sq, const float *tau, int32_t *cnt, const float *rows, int64_t ldr,
                        const int32_t *list_start, const float *r_sq, const int32_t *ids, int Dp, const int32_t *tiles,
                        int n_tiles, void *cand, int cap, cdml_stream_t stream);
int cdml_ivf_filter_f16(const uint16_t *Q, int64_t ldq, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                        const float *q_sq, const float *tau, int32_t *cnt, const uint16_t *rows, int64_t ldr,
                        const int32_t *list_start, const float *r_sq, const int32_t *ids, int Dp, const int32_t *tiles,
                        int n_tiles, void *cand, int cap, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_FILTER_H_ */
