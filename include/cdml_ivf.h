/* cdml_ivf.h -- C ABI of the inverted-file (IVF-Flat) index of the kNN: k-means lists and a probed exact scan
 * (build-defined; the reference's faiss_knn.calc_knn builds an approximate HNSW index, knn.knn_search is brute force):
 * csrc/ivf.hip of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on
 * `stream`, status ints, cdml_last_error()).
 *
 * THE INDEX over catalogue rows x_r (l2-normalised first when the index says so):
 *   centroids c_j, fp32, j < nlist, and one list per centroid.  A finite row is in exactly one list, the list assign[r];
 *   a row with a non-finite coordinate is in no list (assign[r] = -1) and is nobody's neighbour.  The lists are stored
 *   cluster-major: ids int32 [n_listed] sorted by (assign, id); list_start int32 [nlist + 1]; rows fp32 [n_listed][Dp]
 *   (D zero-padded to Dp, a multiple of 32) and r_sq [n_listed] = |row|^2 (cdml_row_sqnorm) in that order.
 *
 * BUILD = Lloyd's k-means, deterministic.  The initial centroids are the rows init_rows: the sorted first nlist ids of a
 * seeded CPU permutation of the finite rows; the training rows are the first train_rows ids of the same permutation
 * (default min(n, 256 nlist)).  An iteration assigns every training row to its nearest centroid with the exact search
 * (knn_search(centroids, rows, 1): squared L2, ties to the lower centroid id, a non-finite row -1) and replaces every
 * non-empty list's centroid by the list's mean (cdml_ivf_centroid_sums); an empty list keeps its centroid.  After the
 * last iteration ALL rows are assigned once more to the final centroids and no update follows, so assign and centroids
 * belong together.  Centroids are plain means, not re-normalised.  objective[t] (float64) = the sum of the assigned
 * distances of iteration t.
 *
 * SEARCH(queries, k, nprobe), 1 <= k <= CDML_KNN_LIST, 1 <= nprobe <= min(nlist, CDML_KNN_LIST):
 *   probe[q][:] = the ids of the nprobe nearest centroids (the exact search again; queries normalised once before);
 *   the result is EXACTLY the k best listed rows of the probed lists under the key (d, id), with
 *       d = (|q|^2 + |x|^2) - 2 s, clamped at 0 by a compare that keeps a NaN (cdml_knn_merge's arithmetic to the letter),
 *       s = the fp32 inner product on v_mfma_f32_32x32x2_f32: a chain of fused multiply-adds over k in an order that is a
 *           function of k alone, so the bits of s(query, row) do not depend on the tile, the slot or the chunk it lands in.
 *   D fp32 ascending, I the catalogue ids; +inf / 0x7fffffff where fewer than k rows were probed; a non-finite query passes
 *   no compare and gets those throughout; a probe id of -1 contributes nothing.  Given (centroids, assign) the output is a
 *   function of the inputs: ties by id, no atomics on floats, bit-identical from run to run and across chunkings.
 *
 * The three launches.  A SLOT is one (query, probed list) pair.  Slots are sorted by list, so the slots
 * [slot_start[c], slot_start[c+1]) of list c form a dense score block S_c [nq_c][ld_c], ld_c = len(c) rounded up to 4:
 * slot s of list c owns the ld_c floats at scores + slot_off[s] (int64; slot_off[s + 1] = slot_off[s] + ld_c inside a list),
 *       S_c[i][j] = < Q[slot_query[slot_start[c] + i]], rows[list_start[c] + j] >.
 *
 * cdml_ivf_centroid_sums: x fp32 [n][ldx]; order int32 [n_listed] = row ids sorted by (list, id); list_start int32
 *   [nlist + 1]; centroids fp32 [nlist][ldc].  Columns [0, D) of list c become the mean of its L = list_start[c+1] -
 *   list_start[c] rows when L > 0 and are NOT written when L == 0.  One block per (list, 64-column slab); wave w of four
 *   adds rows w, w + 4, ... in order, the four partials fold as ((p0 + p1) + p2) + p3, then one division by L: the order is
 *   fixed by L alone.  No atomics.
 * cdml_ivf_scan_f32: the grouped product.  tiles int32 [n_tiles][4] = (list c, first slot of the tile RELATIVE to
 *   slot_start[c], first row of the tile RELATIVE to list_start[c], 0); a tile is 128 slots x 128 rows; tiles of one list
 *   are neighbours in the table.  A slot or row past its list's end loads a clamped valid row and stores nothing; the pad
 *   floats [len, ld_c) of a score row are never written.  All addressing is 64-bit (no buffer descriptors).
 *   Q fp32 [n_queries][ldq] (a slot_query outside [0, n_queries) is clamped into it); Dp a multiple of 32; ldq, ldr
 *   multiples of 4, >= Dp; Q, rows, tiles, scores 16-B aligned.
 * cdml_ivf_merge: one wave per query q < nq: over j < nprobe with c = probe[q * nprobe + j] >= 0 and s = slot_of[q * nprobe
 *   + j], the score row scores + slot_off[s] of len(c) columns, column t being catalogue id ids[list_start[c] + t] with
 *   |x|^2 = r_sq[list_start[c] + t]; keeps the best under (d, id) as cdml_knn_merge does and writes the query's WHOLE list
 *   best_d / best_i [nq][CDML_KNN_LIST], sorted, empty entries +inf / 0x7fffffff (as there, the first k entries are the k
 *   best; what lies behind them is sorted and otherwise unspecified).  scores 16-B aligned, every slot_off a multiple of 4.
 * Bad arguments (a null pointer, a non-positive size, D > ldx or ldc, Dp not a multiple of 32, strides not multiples of 4,
 * misaligned bases, k or nprobe outside [1, CDML_KNN_LIST]) return a negative status before any HIP call. */
#ifndef CDML_IVF_H_
#define CDML_IVF_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_ivf_centroid_sums(const float *x, int64_t ldx, const int32_t *order, const int32_t *list_start, int nlist, int D,
                           float *centroids, int64_t ldc, cdml_stream_t stream);
int cdml_ivf_scan_f32(const float *Q, int64_t ldq, int n_queries, const int32_t *slot_query, const int32_t *slot_start,
                      const int64_t *slot_off, const float *rows, int64_t ldr, const int32_t *list_start, int Dp,
                      const int32_t *tiles, int n_tiles, float *scores, cdml_stream_t stream);
int cdml_ivf_merge(const float *scores, const int64_t *slot_off, const int32_t *slot_of, const int32_t *probe, int nq,
                   int nprobe, const int32_t *list_start, const int32_t *ids, const float *r_sq, const float *q_sq, int k,
                   float *best_d, int32_t *best_i, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_H_ */
