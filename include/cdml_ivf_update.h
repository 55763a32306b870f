/* cdml_ivf_update.h -- C ABI of the in-place updates of the IVF index (build-defined, as the index itself: cdml_ivf.h):
 * csrc/ivf_update.hip of libcdml_hip.so.  The conventions are cdml.h's (device pointers, caller-owned buffers, enqueue-only on
 * `stream`, status ints, cdml_last_error()).  Nothing a search reads changes its meaning: the lists stay cluster-major, ids
 * ascend inside a list, list_start is the exclusive scan of the lengths (cdml_ivf.h).
 *
 * THE LISTS of an index are three parallel arrays over the listed positions: a payload of `row_bytes` bytes a row (fp32 rows,
 * fp16 rows or PQ codes: opaque bytes here), ids int32 and r_sq fp32.  An update writes NEW arrays from the old ones and from a
 * chunk of added rows; list c of the new arrays = its kept old rows in their old order, then its added rows in chunk order
 * (an added id exceeds every listed id, so this IS the order by (list, id)).
 *
 * cdml_ivf_lists_move: one launch writes the new payload, ids and r_sq.  Output-driven: for every destination position o in
 *   [0, n_new), with c the list of o (new_start[c] <= o < new_start[c + 1]), off = o - new_start[c] and kept_c =
 *   kept_start[c + 1] - kept_start[c]:
 *     off <  kept_c: the source is old position p = kept_start[c] + off, mapped through old_pos[p] when old_pos is not null
 *                    (old_pos null = the identity: the pure append): payload row, old_ids[p], old_r_sq[p];
 *     off >= kept_c: the source is chunk row j = add_order[add_start[c] + off - kept_c]: payload row j of the chunk, the id
 *                    id0 + j, add_r_sq[j].
 *   kept_start, add_start, new_start int32 [nlist + 1] (exclusive scans; new_start = kept_start + add_start element-wise);
 *   old_pos int32 [n_kept] or null; add_order int32 [n_add] (chunk rows sorted stably by list: a chunk row in no list is in no
 *   add_order); n_kept = kept_start[nlist] and n_add = add_start[nlist] as the caller knows them; n_old / n_chunk = the rows
 *   of the old arrays / of the chunk.  Strides (old_ld, add_ld, new_ld) are in BYTES, >= row_bytes, multiples of 8; row_bytes
 *   is a positive multiple of 8; the three payload bases are 16-B aligned.  Copies go in 16-byte pieces where row_bytes and
 *   the three strides are multiples of 16, in 8-byte pieces otherwise.  Exactly the bytes [0, row_bytes) of the rows [0, n_new)
 *   of the new payload, new_ids[0, n_new) and new_r_sq[0, n_new) are written, each once (no atomics); the stride gaps and
 *   everything past n_new never.  All addressing is 64-bit.  The old arrays may be null when n_old = 0, the chunk's when
 *   n_chunk = 0; a source index outside its array (tables that contradict the sizes) is clamped into it, and a source array
 *   with no row gives zero bytes, id -1 and r_sq 0: no load leaves the given arrays.  The new arrays overlap no input.
 * cdml_ivf_locate: one thread per query id q in [0, nq): c = assign[q_ids[q]]; pos[q] = the position p in
 *   [list_start[c], list_start[c + 1]) with ids[p] == q_ids[q] (a binary search: ids ascend inside a list), or -1 where the id
 *   is outside [0, n_rows), c is outside [0, nlist) or the list does not hold the id.  q_ids int64 [nq], assign int64
 *   [n_rows], ids int32 [n_listed] (may be null when n_listed = 0), list_start int32 [nlist + 1] (clamped into [0,
 *   n_listed]), pos int32 [nq]: exactly nq entries are written.
 * Bad arguments (a null pointer that is not allowed to be null, a non-positive n_new / nq / nlist / n_rows, a negative count,
 * a size above 2^31 - 1, n_kept + n_add != n_new, n_kept > n_old with old_pos null, row_bytes not a positive multiple of 8, a
 * stride below row_bytes or not a multiple of 8, a payload base that is not 16-B aligned) return a negative status before any
 * HIP call. */
#ifndef CDML_IVF_UPDATE_H_
#define CDML_IVF_UPDATE_H_

#include "cdml.h"

#ifdef __cplusplus
extern "C" {
#endif

int cdml_ivf_lists_move(const void *old_rows, int64_t old_ld, const int32_t *old_ids, const float *old_r_sq, int64_t n_old,
                        const int32_t *old_pos, int64_t n_kept, const void *add_rows, int64_t add_ld, const float *add_r_sq,
                        int64_t n_chunk, const int32_t *add_order, int64_t n_add, int32_t id0, const int32_t *kept_start,
                        const int32_t *add_start, const int32_t *new_start, int nlist, int64_t row_bytes, void *new_rows,
                        int64_t new_ld, int32_t *new_ids, float *new_r_sq, int64_t n_new, cdml_stream_t stream);
int cdml_ivf_locate(const int64_t *q_ids, int64_t nq, const int64_t *assign, int64_t n_rows, const int32_t *ids, int64_t n_listed,
                    const int32_t *list_start, int nlist, int32_t *pos, cdml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CDML_IVF_UPDATE_H_ */
