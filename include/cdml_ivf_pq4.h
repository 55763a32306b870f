/* cdml_ivf_pq4.h -- C ABI of the 4-bit product-quantised lists of the IVF index (build-defined, as the index itself:
 * cdml_ivf.h): csrc/ivf_pq4.hip of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned buffers,
 * enqueue-only on `stream`, status ints, cdml_last_error()); the slot / offset tables, the ragged score buffer, cdml_ivf_merge
 * and cdml_ivf_refine are cdml_ivf.h's and cdml_ivf_f16.h's, unchanged; the 8-bit form is cdml_ivf_pq.h's, unchanged.
 *
 * THE INDEX with storage "pq", pq_bits = 4 and parameter M (the BYTES per listed row, as for 8 bits: a multiple of 8 in
 * [CDML_PQ_M_MIN, CDML_PQ_M_MAX]) has Ms = 2 M subspaces of CDML_PQ4_CODEWORDS = 16 codewords; 2 M must divide Dp, dsub =
 * Dp / Ms >= 1; subspace m is columns [m dsub, (m + 1) dsub); the zero pad columns are ordinary columns.  k-means, assign,
 * centroids and the probes are those of the fp32 index; a row with a non-finite coordinate is in no list.  Plain
 * (non-residual) PQ: one set of codebooks for the whole catalogue, one lookup table per query.
 *   codebooks fp32 [Ms][16][dsub], contiguous.
 *   codes uint8 [n_listed][M], cluster-major, standing where the 8-bit codes stand: byte b of a row = code(2b) |
 *       code(2b + 1) << 4 (the EVEN subspace in the low nibble); code(m) = the LOWEST c in [0, 16) attaining the minimum of
 *       d(c) = sum_j (x[m dsub + j] - codebooks[m][c][j])^2, in fp32 over ascending j as acc = fmaf(diff, diff, acc) from 0;
 *       c runs upwards from 0 against best = +inf under `d < best`, so a d that passes no compare (NaN, +inf) leaves code 0
 *       (cdml_pq_encode's rule, word for word).  A function of (x, codebooks) alone.
 *   The decoded row x^ is the concatenation of its Ms codewords; r_sq = |x^|^2 (cdml_row_sqnorm of the decoded rows).
 *   LUT[q][m][c] = sum_j q[m dsub + j] codebooks[m][c][j], fp32, ascending j, acc = fmaf(q_j, cb_j, acc) from 0; fp32
 *       [nq][Ms][16].
 *   s~(q, row) = ((p_0 + p_1) + p_2) + ... + p_{M-1}: plain fp32 adds over ascending b, starting from p_0, where
 *       p_b = LUT[q][2b][low nibble of byte b] + LUT[q][2b + 1][high nibble of byte b] -- THE PAIR IS ADDED FIRST (a scan may
 *       gather from the 16-entry tables or from 256-entry pair tables it expands in LDS: the bits are the same).  The bits
 *       of s~(query, row) are a function of (q, codebooks, the row's codes) alone: they do not depend on the tile, the slot,
 *       the chunk or the order of the queries.
 * SEARCH without re-rank = EXACTLY the k best listed rows of the probed lists under the key (d~, id),
 *       d~ = (|q|^2 + |x^|^2) - 2 s~, clamped as cdml_ivf_merge clamps.  SEARCH with re-rank r: cdml_ivf_refine, unchanged.
 *
 * cdml_pq4_encode: x fp32 [n][ldx] (ldx >= 2 M dsub), rows in any order; codes uint8 [n][ldc] (ldc >= M): exactly the M
 *   bytes [0, M) of every row are written, the bytes [M, ldc) never; dist fp32 [n][ldd] (ldd >= 2 M) or null: dist[r][m] =
 *   the attained minimum of subspace m (+inf where no d passed a compare), not written when null.  One block per (256 rows,
 *   byte): the 32 codewords of the byte's two subspaces in LDS, ONE thread produces the whole byte (both nibbles) of its
 *   row -- no read-modify-write of the codes, no byte atomics (sub-vectors in registers for dsub in {1, 2, 4, 8, 16, 32}; any
 *   other dsub takes a launch that reads both operands from memory, the same sums in the same order).
 * cdml_pq4_lut: Q fp32 [nq][ldq] (ldq >= 2 M dsub); lut fp32 [nq][2 M][16], 16-B aligned: exactly nq 2 M 16 floats are
 *   written.
 * cdml_ivf_pq4_tile: the scan's tile for M: *slots = S(M) = min(16, 512 / M) (integer division: the lookup tables of a
 *   block's slots, 128 M bytes each, fill at most 64 KiB of LDS), *rows = R = 1024.  Host arithmetic; no HIP call.
 * cdml_ivf_scan_pq4: the table-lookup scan; the argument list and the guarantees of cdml_ivf_scan_pq.  S_c[i][j] =
 *   s~(slot_query[slot_start[c] + i], row list_start[c] + j).  tiles int32 [n_tiles][4] = (list c, first slot of the tile
 *   RELATIVE to slot_start[c], first row RELATIVE to list_start[c], 0); a tile is S(M) slots x R rows.  A slot or row past
 *   its list's end stores nothing (a row past the end is not loaded either); the pad floats [len, ld_c) of a score row are
 *   never written; all addressing is 64-bit; a slot_query outside [0, n_queries) is clamped into it.  lut fp32
 *   [n_queries][2 M][16] as cdml_pq4_lut writes it; codes uint8 [n_listed][ldc] read with 8-byte loads: ldc a multiple of
 *   8, >= M, codes 8-B aligned; lut, tiles and scores 16-B aligned.
 * Bad arguments (a null pointer other than dist, a non-positive size, M not a multiple of 8 in [8, 64], dsub < 1, ldc < M,
 * ldx / ldq / ldd too short, misaligned lut / scores / tiles / codes) return a negative status before any HIP call. */
#ifndef CDML_IVF_PQ4_H_
#define CDML_IVF_PQ4_H_

#include "cdml.h"
#include "cdml_ivf_pq.h"

#define CDML_PQ4_CODEWORDS 16

#ifdef __cplusplus
extern "C" {
#endif

int cdml_pq4_encode(const float *x, int64_t ldx, int64_t n, const float *codebooks, int M, int dsub, uint8_t *codes, int64_t ldc,
                    float *dist, int64_t ldd, cdml_stream_t stream);
int cdml_pq4_lut(const float *Q, int64_t ldq, int nq, const float *codebooks, int M, int dsub, float *lut, cdml_stream_t stream);
int cdml_ivf_pq4_tile(int M, int *slots, int *rows);
int cdml_ivf_scan_pq4(const float *lut, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                      const int64_t *slot_off, const uint8_t *codes, int64_t ldc, const int32_t *list_start, int M,
                      const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_PQ4_H_ */
