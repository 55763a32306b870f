/* cdml_ivf_range.h -- C ABI of the filter scan over product-quantised lists of the IVF index, the launch behind
 * knn.IVFIndex.range_search on storage "pq": csrc/ivf_range.hip of libcdml_hip.so; DESIGN.md section 9f.8.  The conventions
 * are cdml.h's; the lookup tables, the tile (cdml_ivf_pq_tile) and the constants are cdml_ivf_pq.h's, the slot scalars
 * cdml_ivf_pqr.h's, the slot and tile tables cdml_ivf.h's, the candidate lists cdml_ivf_filter.h's -- all unchanged.
 *
 * RANGE SEARCH (knn.IVFIndex.range_search), per query chunk: the tables of the chunk's probe rows, the lookup tables (and the
 * slot scalars of a residual index), ONE filter launch with tau[q] = the query's radius into cnt / cand, one host read of cnt.
 * fp32 and fp16 lists take cdml_ivf_filter_f32 / _f16 for that launch; 8-bit product-quantised lists take this header's.
 * The 4-bit form (cdml_ivf_pq4.h) has no filter launch.
 *
 * cdml_ivf_filter_pq / cdml_ivf_filter_pqr: lut, n_queries, slot_query, slot_start, [slot_base,] codes, ldc, list_start, M,
 *   tiles and n_tiles as cdml_ivf_scan_pq / cdml_ivf_scan_pqr take them, the SAME work item (cdml_ivf_pq_tile(M): S = 64 / M
 *   slots x 1024 rows, the S lookup tables in 64 KiB of LDS, two rows per lane with their code words in registers) and the same
 *   sums: s = ((LUT[q][0][code_0] + LUT[q][1][code_1]) + ...) over ascending m, from slot_base[slot] in the residual form: the
 *   bits of a (query, row) sum are those of the buffered scan.  In place of slot_off and scores, cdml_ivf_filter.h's set:
 *     q_sq, tau fp32 [n_queries], cnt int32 [n_queries]   per query of the chunk;
 *     r_sq fp32 [n_listed], ids int32 [n_listed]          per listed row, in list order;
 *     cand [n_queries][cap] pairs of 32-bit words, cap a positive power of two.
 *   Per (slot, row) with q = slot_query[slot]: d = (q_sq[q] + r_sq[row]) - 2 s, then d = 0 where d < 0 (a compare that keeps
 *   a NaN) -- cdml_ivf_merge's arithmetic to the letter.  Where d <= tau[q] (a NaN d or tau passes no compare):
 *   pos = atomic cnt[q] += 1 (integer atomics only); when pos < cap, cand[q * cap + pos] = (the bits of d, ids[row]).  cnt
 *   counts the dropped ones too, so one launch tells how many slots a query needs.  A row past its list's end appends nothing,
 *   and neither does a slot whose slot_query is outside [0, n_queries) (its lookup table is loaded from a clamped query, as
 *   the scan loads it).  Nothing else is written: no score, no slot of cand from min(cnt[q], cap) on.  The ORDER of a query's
 *   candidates depends on the schedule; their SET and cnt do not.
 * Bad arguments (a null pointer, a non-positive size, M not a multiple of 8 in [8, 64], ldc < M or not a multiple of 8,
 * misaligned lut / tiles (16 B) / codes / cand (8 B), cap not a positive power of two) return a negative status with a
 * cdml_last_error() text before any HIP call. */
#ifndef CDML_IVF_RANGE_H_
#define CDML_IVF_RANGE_H_

#include "cdml_ivf_pqr.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_ivf_filter_pq(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                       const float *q_sq, const float *tau, int32_t *cnt, const uint8_t *codes, int64_t ldc,
                       const int32_t *list_start, const float *r_sq, const int32_t *ids, int M, const int32_t *tiles,
                       int n_tiles, void *cand, int cap, cdml_stream_t stream);
int cdml_ivf_filter_pqr(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                        const float *slot_base, const float *q_sq, const float *tau, int32_t *cnt, const uint8_t *codes,
                        int64_t ldc, const int32_t *list_start, const float *r_sq, const int32_t *ids, int M,
                        const int32_t *tiles, int n_tiles, void *cand, int cap, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_RANGE_H_ */
