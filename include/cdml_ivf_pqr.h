/* cdml_ivf_pqr.h -- C ABI of the RESIDUAL product-quantised lists of the IVF index (pq_residual=True on storage "pq"):
 * csrc/ivf_pqr.hip of libcdml_hip.so.  The conventions are cdml.h's; the plain pq index, its codebook layout, its lookup
 * tables (cdml_pq_lut), its tile (cdml_ivf_pq_tile) and its constants are cdml_ivf_pq.h's, unchanged; the slot / offset
 * tables, the ragged score buffer, cdml_ivf_merge and cdml_ivf_refine are cdml_ivf.h's and cdml_ivf_f16.h's, unchanged.
 *
 * THE INDEX.  k-means, assign, centroids, probes, the coarse search, ids, list_start, M, dsub = Dp / M and the subspace
 * columns are the plain pq index's.  C fp32 [nlist][Dp] is the padded centroid matrix; pad columns are ordinary columns.
 *   residual of a listed row x with a = assign: e_j = x_j - C[a][j], ONE fp32 subtract per column.
 *   codebooks fp32 [M][256][dsub], contiguous: one set for all lists, trained on residuals.
 *   codes uint8 [n_listed][M]: code[r][m] = the LOWEST c attaining the minimum of
 *       d(c) = sum_j (e[m dsub + j] - codebooks[m][c][j])^2, in fp32 over ascending j as acc = fmaf(diff, diff, acc) from 0;
 *       c runs upwards from 0 against best = +inf under `d < best` (cdml_pq_encode's arithmetic and tie rule on e).  A row
 *       whose assign is outside [0, nlist) reads no centroid and gets codes 0 and dist +inf.
 *   The decoded row: x^_j = C[a][j] + codebooks[m][code_m][j - m dsub], ONE fp32 add; r_sq = |x^|^2 (cdml_row_sqnorm of the
 *       decoded rows).
 *   The slot scalar b(q, c) = the fp32 inner product of the prepared query q and centroid c over Dp columns, in an order that
 *       is a function of Dp alone: for l in [0, 64): p_l = 0, then over j = l, l + 64, l + 128, ... < Dp ascending
 *       p_l = fmaf(q_j, C[c][j], p_l); then for w = 32, 16, 8, 4, 2, 1 in this order, all l at once: p_l = p_l + p_(l xor w);
 *       b = p_0 (all 64 are the same bits: fp32 addition commutes).  A function of (q, c) alone: it does not depend on the
 *       slot, the chunk or the order of the queries.
 *   s~(q, row) = (((b(q, c_a) + LUT[q][0][code_0]) + LUT[q][1][code_1]) + ...): plain fp32 adds over ascending m, starting
 *       from b.  LUT is cdml_pq_lut's on the residual codebooks.  The bits are a function of (q, the row's centroid, the
 *       codebooks, the row's codes) alone: not of the tile, the slot, the chunk or the order of the queries.
 * SEARCH without re-rank = EXACTLY the k best listed rows of the probed lists under the key (d~, id),
 *       d~ = (|q|^2 + |x^|^2) - 2 s~ as cdml_ivf_merge forms and clamps it.  With re-rank r the merge's r candidates go
 *       through cdml_ivf_refine as for the plain index.
 *
 * cdml_pqr_encode: the fused residual encoder; the residual matrix is never materialised.  x fp32 [n][ldx] (ldx >= M dsub),
 *   rows in any order; centroids fp32 [nlist][ldcen] (ldcen >= M dsub); assign int64 [n]; codes uint8 [n][ldc] (ldc >= M):
 *   exactly the bytes [0, M) of every row are written; dist fp32 [n][ldd] (ldd >= M) or null: the attained minima (+inf where
 *   no d passed a compare or assign is outside [0, nlist)).  cdml_pq_encode's launch shape: one block per (256 rows,
 *   subspace), the 256 codewords in LDS, a lane's residual sub-vector in registers (the centroid's sub-vector is subtracted
 *   as the row's is loaded) for dsub in {1, 2, 4, 8, 16, 32}; any other dsub takes a launch that reads the operands from
 *   memory, the same sums in the same order.
 * cdml_ivf_slot_dots: slot_base[slot_start[c] + i] = b(slot_query[slot_start[c] + i], c) for every list c in [0, nlist) and
 *   every i in [0, slot_start[c + 1] - slot_start[c]): exactly n_slots = slot_start[nlist] floats are written.  Q fp32
 *   [n_queries][ldq] (ldq >= Dp), centroids fp32 [nlist][ldcen] (ldcen >= Dp); a slot_query outside [0, n_queries) is clamped
 *   into it, as the scan clamps it.  One wave per slot.
 * cdml_ivf_scan_pqr: cdml_ivf_scan_pq with the accumulator starting from slot_base[slot]: S_c[i][j] = s~(slot_query[
 *   slot_start[c] + i], row list_start[c] + j).  The tile is cdml_ivf_pq_tile(M)'s (S(M) = 64 / M slots x R = 1024 rows, 64 KiB
 *   of tables a block, two rows per lane); tiles, the stores (a slot or row past its list's end stores nothing, a row past
 *   the end is not loaded, the pad floats [len, ld_c) are never written), the 64-bit addressing, the clamp of slot_query and
 *   the alignment rules (ldc a multiple of 8, >= M; codes 8-B aligned; lut, tiles and scores 16-B aligned) are
 *   cdml_ivf_scan_pq's.  slot_base fp32 [n_slots] as cdml_ivf_slot_dots writes it.
 * Bad arguments (a null pointer other than dist, a non-positive size, nlist < 1, M not a multiple of 8 in [8, 64], dsub < 1,
 * Dp < 1, ldc < M, ldx / ldcen / ldq / ldd too short, misaligned lut / scores / tiles / codes) return a negative status with a
 * cdml_last_error() text before any HIP call. */
#ifndef CDML_IVF_PQR_H_
#define CDML_IVF_PQR_H_

#include "cdml_ivf_pq.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_pqr_encode(const float *x, int64_t ldx, int64_t n, const float *centroids, int64_t ldcen, int nlist,
                    const int64_t *assign, const float *codebooks, int M, int dsub, uint8_t *codes, int64_t ldc, float *dist,
                    int64_t ldd, cdml_stream_t stream);
int cdml_ivf_slot_dots(const float *Q, int64_t ldq, int n_queries, const float *centroids, int64_t ldcen, int Dp,
                       const int32_t *slot_query, const int32_t *slot_start, int nlist, float *slot_base,
                       cdml_stream_t stream);
int cdml_ivf_scan_pqr(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                      const int64_t *slot_off, const float *slot_base, const uint8_t *codes, int64_t ldc,
                      const int32_t *list_start, int M, const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_PQR_H_ */
