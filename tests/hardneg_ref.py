"""Host models of the hard-negative feature (plain module, no pytest configuration).

``listed_negative`` is the draw of include/cdml_hardneg.h, written on the device stream's specification in
oracle/sampler.py (``_Stream``, ``_bounded``, ``uniform_negative``: imported, not restated); ``mine_lists`` is a brute-force
float64 numpy version of cdml_amd.hardneg.mine_lists."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.sampler import _Stream, _bounded, pair_index, uniform_negative  # noqa: E402

PURPOSE_LISTED_NEG = 2


def hard_threshold(hard_fraction):
    return int(round(float(hard_fraction) * 2.0 ** 32))


def listed_negative(seed, step, slot, a, p, n_rows, lists, L, hard_thresh):
    """(negative id, kind) of one triplet; lists: int array [n_rows, >= L] (only columns < L are read)."""
    st = _Stream(seed, step, slot, PURPOSE_LISTED_NEG)
    w0 = st.next()
    if w0 < hard_thresh and 0 <= a < n_rows:
        js = [_bounded(st, L) for _ in range(4)]             # all four before any list entry is read
        for j in js:
            if j is None:
                continue
            c = int(lists[a][j])
            if 0 <= c < n_rows and c != a and c != p:
                return c, 1
    return uniform_negative(seed, step, slot, a, p, n_rows), 0


def listed_triplets(pairs, n_rows, seed, step, batch, lists, L, hard_fraction, slot0=0, batch_global=None):
    """Spec of the listed sampler -> (int32 [batch, 3], int32 [batch] kinds)."""
    pairs = np.asarray(pairs)
    bg = batch if batch_global is None else batch_global
    th = hard_threshold(hard_fraction)
    out = np.empty((batch, 3), dtype=np.int32)
    kind = np.empty(batch, dtype=np.int32)
    for i in range(batch):
        slot = slot0 + i
        a, p = (int(v) for v in pairs[pair_index(step, slot, bg, len(pairs))])
        n, kind[i] = listed_negative(seed, step, slot, a, p, n_rows, lists, L, th)
        out[i] = (a, p, n)
    return out, kind


def list_width(k):
    return (k + 3) // 4 * 4


def neighbours(emb, w):
    """fp64 brute force: (ids [n, w], squared distances [n, w]) of the w nearest rows of the l2-normalised ``emb`` to each
    of its rows, the row itself included, ordered by (distance, id)."""
    x = np.asarray(emb, dtype=np.float64)
    x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
    d = np.maximum(2.0 - 2.0 * (x @ x.T), 0.0)
    n = len(x)
    ids = np.empty((n, w), dtype=np.int64)
    for i in range(n):
        ids[i] = np.lexsort((np.arange(n), d[i]))[:w]
    return ids, np.take_along_axis(d, ids, 1)


def filter_row(i, ids, k, skip_top, partners):
    """the list of row i from its k + skip_top + 1 nearest ids (nearest first)"""
    ids = [int(c) for c in ids]
    if i in ids:
        ids.remove(i)
    else:
        ids = ids[:-1]
    ids = [c for c in ids[skip_top:] if c >= 0 and (i, c) not in partners]
    return ids + [-1] * (list_width(k) - len(ids))


def partner_set(pairs):
    s = set()
    if pairs is not None:
        for a, b in np.asarray(pairs).reshape(-1, 2):
            s.add((int(a), int(b)))
            s.add((int(b), int(a)))
    return s


def mine_lists(emb, k, skip_top=0, pairs=None):
    """int32 [n, list_width(k)]: the brute-force lists."""
    ids, _ = neighbours(emb, min(k + skip_top + 1, len(emb)))
    if ids.shape[1] < k + skip_top + 1:
        ids = np.concatenate([ids, np.full((len(ids), k + skip_top + 1 - ids.shape[1]), -1, dtype=np.int64)], 1)
    partners = partner_set(pairs)
    return np.asarray([filter_row(i, ids[i], k, skip_top, partners) for i in range(len(ids))], dtype=np.int32)
