/* cdml_ivf_pq.h -- C ABI of the product-quantised lists of the IVF index (build-defined, as the index itself: cdml_ivf.h):
 * csrc/ivf_pq.hip of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on
 * `stream`, status ints, cdml_last_error()); the slot / offset tables, the ragged score buffer, cdml_ivf_merge and
 * cdml_ivf_refine are cdml_ivf.h's and cdml_ivf_f16.h's, unchanged.
 *
 * THE INDEX with storage "pq" and parameter M (a multiple of 8 in [CDML_PQ_M_MIN, CDML_PQ_M_MAX] that divides Dp) works on
 * the prepared rows X fp32 [n][Dp] as the other storages do.  dsub = Dp / M; subspace m is columns [m dsub, (m + 1) dsub);
 * the zero pad columns are ordinary columns.  k-means, assign, centroids and the probes are those of the fp32 index; a row
 * with a non-finite coordinate is in no list.  This is plain (non-residual) PQ: one set of codebooks for the whole
 * catalogue, one lookup table per query.
 *   codebooks fp32 [M][256][dsub], contiguous.
 *   codes uint8 [n_listed][M], cluster-major: code[r][m] = the LOWEST c attaining the minimum of
 *       d(c) = sum_j (x[m dsub + j] - codebooks[m][c][j])^2, in fp32 over ascending j as acc = fmaf(diff, diff, acc) from 0
 *       (the direct form, as in cdml_ivf_refine); c runs upwards from 0 against best = +inf under `d < best`, so a d that
 *       passes no compare (NaN, +inf) leaves code 0.  A function of (x, codebooks) alone.
 *   The decoded row x^ is the concatenation of its codewords; r_sq = |x^|^2 (cdml_row_sqnorm of the decoded rows).
 *   LUT[q][m][c] = sum_j q[m dsub + j] codebooks[m][c][j], fp32, ascending j, acc = fmaf(q_j, cb_j, acc) from 0.
 *   s~(q, row) = ((LUT[q][0][code_0] + LUT[q][1][code_1]) + LUT[q][2][code_2]) + ...: plain fp32 adds over ascending m,
 *       starting from the first term.  The bits of s~(query, row) are a function of (q, codebooks, the row's codes) alone:
 *       they do not depend on the tile, the slot, the chunk or the order of the queries.
 * SEARCH without re-rank = EXACTLY the k best listed rows of the probed lists under the key (d~, id),
 *       d~ = (|q|^2 + |x^|^2) - 2 s~, clamped as cdml_ivf_merge clamps; |q|^2 is the fp32 norm of the unrounded query.
 * SEARCH with re-rank r (k <= r <= CDML_KNN_LIST): the merge keeps r entries and cdml_ivf_refine re-scores them against the
 *       fp32 rows, so (D, I) are fp32 distances of fp32 rows again.
 *
 * cdml_pq_encode: x fp32 [n][ldx] (ldx >= M dsub), rows in any order; codes uint8 [n][ldc] (ldc >= M): exactly the M bytes
 *   [0, M) of every row are written, the bytes [M, ldc) never; dist fp32 [n][ldd] (ldd >= M) or null: dist[r][m] = the
 *   attained minimum (+inf where no d passed a compare), not written when null.  One block per (256 rows, subspace): the
 *   subspace's 256 codewords in LDS, a lane owns one row's sub-vector (in registers for dsub in {1, 2, 4, 8, 16, 32}; any
 *   other dsub takes a launch that reads both operands from memory, the same sums in the same order).
 * cdml_pq_lut: Q fp32 [nq][ldq] (ldq >= M dsub); lut fp32 [nq][M][256], 16-B aligned: exactly nq M 256 floats are written.
 * cdml_ivf_pq_tile: the scan's tile for M: *slots = S(M) = 64 / M (integer division: the lookup tables of a block's slots
 *   fill at most 64 KiB of LDS, M KiB each), *rows = R = 1024.  Host arithmetic; no HIP call.
 * cdml_ivf_scan_pq: the table-lookup (asymmetric distance) scan.  slot_query, slot_start, slot_off, list_start and scores
 *   are cdml_ivf_scan_f32's: S_c[i][j] = s~(slot_query[slot_start[c] + i], row list_start[c] + j).  tiles int32
 *   [n_tiles][4] = (list c, first slot of the tile RELATIVE to slot_start[c], first row RELATIVE to list_start[c], 0); a
 *   tile is S(M) slots x R rows.  A slot or row past its list's end stores nothing (a row past the end is not loaded
 *   either); the pad floats [len, ld_c) of a score row are never written; all addressing is 64-bit; a slot_query outside
 *   [0, n_queries) is clamped into it.  lut fp32 [n_queries][M][256] as cdml_pq_lut writes it; codes uint8 [n_listed][ldc]
 *   read with 8-byte loads: ldc a multiple of 8, >= M, codes 8-B aligned; lut, tiles and scores 16-B aligned.
 * Bad arguments (a null pointer other than dist, a non-positive size, M not a multiple of 8 in [8, 64], dsub < 1, ldc < M,
 * ldx / ldq / ldd too short, misaligned lut / scores / tiles / codes) return a negative status before any HIP call. */
#ifndef CDML_IVF_PQ_H_
#define CDML_IVF_PQ_H_

#include "cdml.h"

#define CDML_PQ_M_MIN 8
#define CDML_PQ_M_MAX 64
#define CDML_PQ_CODEWORDS 256

#ifdef __cplusplus
extern "C" {
#endif

int cdml_pq_encode(const float *x, int64_t ldx, int64_t n, const float *codebooks, int M, int dsub, uint8_t *codes, int64_t ldc,
                   float *dist, int64_t ldd, cdml_stream_t stream);
int cdml_pq_lut(const float *Q, int64_t ldq, int nq, const float *codebooks, int M, int dsub, float *lut, cdml_stream_t stream);
int cdml_ivf_pq_tile(int M, int *slots, int *rows);
int cdml_ivf_scan_pq(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                     const int64_t *slot_off, const uint8_t *codes, int64_t ldc, const int32_t *list_start, int M,
                     const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_PQ_H_ */
