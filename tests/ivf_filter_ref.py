"""Host model of the threshold-filter search of the IVF index (include/cdml_ivf_filter.h; cdml_amd.knn.IVFIndex.search(scan=
"filter")), on top of tests/ivf_ref.py: the seed lists and their threshold tau, the candidate sets behind tau, and the search
= seed list + candidates -> the keep best.  Distances are ivf_ref's: int64 on exact grids (empty = xs.INF_I) or float64
(empty = +inf; a NaN passes no compare), UNCLAMPED on entry.  Every rule has a switch that turns it into the single mutation
tests/test_ivf_filter_host.py must see: the compare ``d <= tau`` (``strict``: ``<`` loses a tie at tau), tau taken from the
keep-th entry (``tau_rank``: from the k-th under a re-rank), the seed columns masked out of the filter pass (``mask_seed``
off: a seed row comes twice).

Plain module, no pytest configuration; numpy on the CPU only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_ref as ref  # noqa: E402


def split_probe(probe, s):
    """(seed, rest): the probe table with the columns from ``s`` on / the first ``s`` columns set to -1"""
    p = np.asarray(probe, np.int64)
    seed, rest = p.copy(), p.copy()
    seed[:, s:] = -1
    rest[:, :s] = -1
    return seed, rest


def seed_tau(d, assign, nlist, probe, s, keep, bad_queries=(), tau_rank=None):
    """(Ds [nq, keep], Is [nq, keep], tau [nq]): the keep best (max(d, 0), id) over the first ``s`` probed lists of every
    query, and tau = the keep-th distance (``tau_rank``-th where given) -- the empty value (+inf) where fewer rows were seeded"""
    seed, _ = split_probe(probe, s)
    Ds, Is = ref.search(d, assign, nlist, seed, keep, bad_queries=bad_queries)
    return Ds, Is, Ds[:, (keep if tau_rank is None else tau_rank) - 1].copy()


def candidates(d, assign, nlist, probe, s, tau, bad_queries=(), strict=False, mask_seed=True):
    """Per query the list of (max(d, 0), id) over the rows of its probed lists behind the seed columns with d <= tau[q] (a
    NaN d passes no compare); sorted by (d, id).  ``mask_seed`` off: over ALL its probed lists."""
    d = np.asarray(d)
    integer = d.dtype.kind == "i"
    _, rest = split_probe(probe, s)
    table = rest if mask_seed else np.asarray(probe, np.int64)
    mem = {}
    out = []
    for q in range(d.shape[0]):
        got = []
        if q not in bad_queries:
            for c in table[q]:
                if c < 0:
                    continue
                if c not in mem:
                    mem[c] = ref.members(assign, nlist, int(c))
                m = mem[c]
                v = d[q, m]
                if not integer:
                    m, v = m[~np.isnan(v)], v[~np.isnan(v)]
                v = np.maximum(v, 0)
                sel = (v < tau[q]) if strict else (v <= tau[q])
                got += list(zip(v[sel].tolist(), m[sel].tolist()))
        out.append(sorted(got))
    return out


def search(d, assign, nlist, probe, s, keep, bad_queries=(), tau_rank=None, strict=False, mask_seed=True, parts=False):
    """(D [nq, keep], I int64 [nq, keep]): the keep best keys (d, id) of seed list + candidates, as a MULTISET (a row that
    comes twice is kept twice: what a merge of two lists does).  ``parts``: (D, I, tau, candidates) instead."""
    d = np.asarray(d)
    inf = xs.INF_I if d.dtype.kind == "i" else np.inf
    Ds, Is, tau = seed_tau(d, assign, nlist, probe, s, keep, bad_queries, tau_rank)
    cands = candidates(d, assign, nlist, probe, s, tau, bad_queries, strict, mask_seed)
    D = np.full((d.shape[0], keep), inf, dtype=d.dtype)
    I = np.full((d.shape[0], keep), -1, dtype=np.int64)
    for q in range(d.shape[0]):
        keys = [(Ds[q, t], int(Is[q, t])) for t in range(keep) if Is[q, t] >= 0] + cands[q]
        keys.sort()
        for t, (v, i) in enumerate(keys[:keep]):
            D[q, t], I[q, t] = v, i
    return (D, I, tau, cands) if parts else (D, I)


def default_seed_probes(keep, nprobe, nlist, n_listed):
    """min(nprobe, max(1, ceil(4 keep nlist / n_listed)))"""
    return min(nprobe, max(1, -(-4 * keep * nlist // n_listed)))


def default_filter_cap(keep):
    """the smallest power of two >= 4 keep, at least 64"""
    cap = 64
    while cap < 4 * keep:
        cap *= 2
    return cap


def chunk_costs(probe, list_len, s, cap):
    """int64 [nq]: a query's floats under scan="filter" = the padded lengths of its SEED lists + 2 cap"""
    seed, _ = split_probe(probe, s)
    ld = (np.asarray(list_len, np.int64) + 3) // 4 * 4
    return np.where(seed >= 0, ld[np.maximum(seed, 0)], 0).sum(1) + 2 * cap
