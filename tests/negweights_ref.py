"""Host model of the weighted negative draw (plain module, no pytest configuration).

``weighted_negative`` is the draw of include/cdml_negweights.h, written on the device stream's specification in
oracle/sampler.py (``_Stream``, ``uniform_negative``: imported, not restated).  ``owner`` is the DEFINITION -- the largest
v < n_live with start[v] <= r, by a search over all of ``start`` -- so it does not depend on the coarse table the kernels
bracket their search with.  The weight tables the host and the GPU tests share are built here too."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.sampler import _Stream, pair_index, uniform_negative  # noqa: E402

PURPOSE_WEIGHTED_NEG = 3
TOTAL = 1 << 32


def start_of(quanta):
    """(start int64 [n_live], n_live) of integer quanta that sum to 2^32"""
    q = np.asarray(quanta, dtype=np.int64)
    assert int(q.sum()) == TOTAL
    n_live = int(np.flatnonzero(q)[-1]) + 1
    return (np.cumsum(q) - q)[:n_live], n_live


def as_start(start_i32):
    """the uint32 bits of an int32 start table as int64"""
    return np.asarray(start_i32).astype(np.int32).view(np.uint32).astype(np.int64)


def owner(start, r):
    """start: int64 [n_live] (ascending, start[0] = 0); r: int or integer array of 32-bit words"""
    return np.searchsorted(start, np.asarray(r, dtype=np.int64), side="right") - 1


def weighted_negative(seed, step, slot, a, p, n_rows, start):
    """(negative id, kind) of one triplet"""
    st = _Stream(seed, step, slot, PURPOSE_WEIGHTED_NEG)
    while not st.exhausted():
        v = int(owner(start, st.next()))
        if v != a and v != p:
            return v, 1
    return uniform_negative(seed, step, slot, a, p, n_rows), 0


def weighted_triplets(pairs, n_rows, seed, step, batch, start, slot0=0, batch_global=None):
    """Spec of the weighted sampler -> (int32 [batch, 3], int32 [batch] kinds)."""
    pairs = np.asarray(pairs)
    bg = batch if batch_global is None else batch_global
    out = np.empty((batch, 3), dtype=np.int32)
    kind = np.empty(batch, dtype=np.int32)
    for i in range(batch):
        slot = slot0 + i
        a, p = (int(v) for v in pairs[pair_index(step, slot, bg, len(pairs))])
        n, kind[i] = weighted_negative(seed, step, slot, a, p, n_rows, start)
        out[i] = (a, p, n)
    return out, kind


def ideal_quanta(w):
    """float64 [n]: 1 + w / sum(w) * (2^32 - |P|) for the positive entries, 0 for the others"""
    w = np.asarray(w, dtype=np.float64)
    pos = w > 0
    out = np.zeros(len(w))
    out[pos] = 1.0 + w[pos] / w[pos].sum() * float(TOTAL - int(pos.sum()))
    return out


# ---- the weight tables of the tests ----
def equal_weights(n):
    return np.ones(n)


def zipf_weights(n, seed, power=0.75):
    """unigram^power of Zipf counts, the popular rows scattered over the ids"""
    rng = np.random.default_rng(seed)
    counts = 1e6 / (1.0 + rng.permutation(n))
    return counts ** power


def half_zero_weights(n, seed):
    """leading and trailing rows of weight 0 and half of all entries 0"""
    rng = np.random.default_rng(seed)
    w = rng.random(n) + 0.05
    edge = max(1, n // 50)
    w[:edge] = 0
    w[-edge:] = 0
    inner = np.arange(edge, n - edge)
    w[rng.choice(inner, size=max(0, n // 2 - 2 * edge), replace=False)] = 0
    return w


def two_row_weights(n, a, p, third):
    """all mass on rows a and p; the third positive row a table needs gets the one quantum every positive row has"""
    w = np.zeros(n)
    w[a] = w[p] = 1.0
    w[third] = 1e-30
    return w
