"""Host models of the IVF index (include/cdml_ivf.h; cdml_amd.knn.IVFIndex): lists from an assignment, probes, the search
restricted to the probed lists (int64 on exact grids, fp64 otherwise), column means, and a numpy Lloyd loop started from
given ``init_rows``.  Every rule of the search model has a switch that turns it into the single mutation
tests/test_ivf_host.py must see: ties by id, the clamp at 0, a -1 probe, unlisted rows, empty lists.

The grid case (``grid_case``) is built on tests/exact_select.py's integer grid: every norm, inner product and distance an
integer multiple of one power-of-two unit far below 2^24, so any summation order gives the same fp32 bits and the
comparison is ``torch.equal``; ``assert_select_exact_safe`` is recorded for the case.

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402


# ---- lists -------------------------------------------------------------------------------------------------------------
def lists_from_assign(assign, nlist):
    """(ids int64 [n_listed] sorted by (assign, id), list_start int64 [nlist + 1]); assign < 0 = unlisted"""
    a = np.asarray(assign, np.int64)
    listed = np.nonzero(a >= 0)[0]
    ids = listed[np.lexsort((listed, a[listed]))]
    start = np.zeros(nlist + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(a[listed], minlength=nlist)[:nlist])
    return ids, start


def members(assign, nlist, c, list_unlisted=False, empty_borrows=False):
    """row ids of list c, ascending.  Mutations: ``list_unlisted`` = an unlisted row (assign -1) counts as a member of the
    LAST list (what indexing with -1 does); ``empty_borrows`` = an empty list hands out the next non-empty list's rows (what
    a search by offset instead of by (start, length) does)."""
    a = np.asarray(assign, np.int64)
    if list_unlisted:
        a = np.where(a < 0, nlist - 1, a)
    m = np.nonzero(a == c)[0]
    if empty_borrows and len(m) == 0:
        for c2 in range(c + 1, nlist):
            m = np.nonzero(a == c2)[0]
            if len(m):
                break
    return m


# ---- probes --------------------------------------------------------------------------------------------------------------
def probes(dc, nprobe, bad_queries=()):
    """int64 [nq, nprobe]: per query the nprobe centroids of smallest distance ``dc`` [nq, nlist] (int64 or float64), ties
    to the lower id; -1 throughout for a query of ``bad_queries`` (non-finite); a NaN distance (a non-finite centroid) is
    nobody's nearest: -1 where fewer than nprobe centroids are left"""
    dc = np.asarray(dc)
    ids = np.arange(dc.shape[1])
    P = np.full((dc.shape[0], nprobe), -1, dtype=np.int64)
    for q in range(dc.shape[0]):
        if q in bad_queries:
            continue
        ok = ids if dc.dtype.kind == "i" else ids[~np.isnan(dc[q])]
        o = ok[np.lexsort((ok, dc[q, ok]))[:nprobe]]
        P[q, :len(o)] = o
    return P


# ---- the search restricted to the probed lists -------------------------------------------------------------------------------
def search(d, assign, nlist, probe, k, bad_queries=(), clamp=True, tie_larger=False, minus_one_is_last=False,
           list_unlisted=False, empty_borrows=False):
    """(D [nq, k], I int64 [nq, k]): per query the k best (max(d, 0), id) over the members of its probed lists.  ``d`` [nq, n]
    UNCLAMPED distances: int64 (exact grids; empty = xs.INF_I) or float64 (empty = +inf; a NaN passes no compare).  A probe
    of -1 contributes nothing; a query of ``bad_queries`` gets nothing.  The switches are the mutations (module docstring);
    ``minus_one_is_last`` = a -1 probe scans the LAST list."""
    d = np.asarray(d)
    integer = d.dtype.kind == "i"
    inf = xs.INF_I if integer else np.inf
    nq = d.shape[0]
    D = np.full((nq, k), inf, dtype=d.dtype)
    I = np.full((nq, k), -1, dtype=np.int64)
    mem = {}
    for q in range(nq):
        if q in bad_queries:
            continue
        cand = []
        for c in np.asarray(probe[q], np.int64):
            if c < 0:
                if not minus_one_is_last:
                    continue
                c = nlist - 1
            if c not in mem:
                mem[c] = members(assign, nlist, int(c), list_unlisted, empty_borrows)
            cand.append(mem[c])
        if not cand:
            continue
        cand = np.unique(np.concatenate(cand)).astype(np.int64)
        dq = d[q, cand]
        if not integer:
            keep = ~np.isnan(dq)
            cand, dq = cand[keep], dq[keep]
        if clamp:
            dq = np.maximum(dq, 0)
        o = np.lexsort((-cand if tie_larger else cand, dq))[:k]
        D[q, :len(o)] = dq[o]
        I[q, :len(o)] = cand[o]
    return D, I


def fp64_dist(q, b, l2_norm=True):
    """float64 [nq, n] unclamped squared distances as oracle/knn.py forms them (rows through float32 first)"""
    b = np.asarray(b, np.float32).astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64)
    if l2_norm:
        b = b / np.maximum(np.linalg.norm(b, axis=1, keepdims=True), 1e-6)
        q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-6)
    return (q * q).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * q @ b.T


# ---- k-means ---------------------------------------------------------------------------------------------------------------
def column_means(x, assign, nlist, keep=None):
    """float64 [nlist, D]: every non-empty list's mean; an empty list keeps ``keep[c]`` (NaN without ``keep``)"""
    x = np.asarray(x, np.float64)
    out = np.full((nlist, x.shape[1]), np.nan) if keep is None else np.array(keep, np.float64)
    a = np.asarray(assign, np.int64)
    for c in range(nlist):
        m = a == c
        if m.any():
            out[c] = x[m].mean(0)
    return out


def nearest(x, C):
    """(assign int64 [n], d float64 [n]): the nearest centroid of every row, ties to the lower id"""
    d = (x * x).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * x @ C.T
    a = d.argmin(1)
    return a, np.maximum(d[np.arange(len(x)), a], 0.0)


def lloyd(x, init_rows, iters):
    """Lloyd's k-means in float64 from the centroids x[init_rows]: ``iters`` times (assign, update; an empty list keeps its
    centroid), then one final assignment.  Returns (centroids, assign, objective [iters])."""
    x = np.asarray(x, np.float64)
    C = x[np.asarray(init_rows, np.int64)].copy()
    obj = []
    for _ in range(iters):
        a, d = nearest(x, C)
        obj.append(d.sum())
        C = column_means(x, a, len(C), keep=C)
    a, _ = nearest(x, C)
    return C, a, np.asarray(obj)


def recall(I, Iref):
    """the mean share of a query's reference neighbours (ids >= 0) found in its row of I"""
    hit = tot = 0
    for a, b in zip(np.asarray(I), np.asarray(Iref)):
        b = b[b >= 0]
        hit += len(np.intersect1d(a[a >= 0], b))
        tot += len(b)
    return hit / max(tot, 1)


# ---- the grid case -----------------------------------------------------------------------------------------------------------
GRID_LENS = (0, 1, 127, 128, 129, 300, 5, 130, 64, 116)       # list lengths: empty, one row, around the 128-row tile, three tiles
GRID_NLIST = len(GRID_LENS)
GRID_N = sum(GRID_LENS) + 1                                   # + one NaN row (unlisted)
GRID_NQ, GRID_NPROBE = 300, 3
GRID_Q127, GRID_Q140 = 2, 5                                   # list 2 is probed by exactly 127 queries, list 5 by 140
GRID_FEW = 298                                                # this query probes lists 0, 1, 6: six rows for k = 128
GRID_NAN_QUERY = 299
GRID_KS = (51, 128)
GRID_DIMS = (48, 256)
GRID_LOW = (7, 333, 901)                                      # rows whose |x|^2 the clamp case lowers: raw distances go negative


def grid_case(D):
    """About 1 000 grid rows (x PIPE_UNIT) in ten lists of a host-chosen assignment (ids scattered over the lists), one NaN
    row; duplicates of one row planted in two different lists, below and above the ids they tie with; centroid j = one
    large coordinate j, so that a query's probes are the three largest of its first ten coordinates: 300 queries, list 2
    probed by exactly 127 of them, list 5 by 140, the empty list 0 by several, one query whose lists hold six rows, one
    NaN query.  ``probe_hand``: the same table with some finite queries' probes set to -1; ``r_low``: |x|^2 lowered for three
    rows (the kernels only read it), so that raw distances go negative and the clamp decides."""
    def make():
        rng = xg.case_rng("ivfgrid", GRID_N, GRID_NQ, D)
        n, nlist = GRID_N, GRID_NLIST
        nan_row = 500
        assign = np.repeat(np.arange(nlist), GRID_LENS)
        rng.shuffle(assign)
        assign = np.insert(assign, nan_row, -1)
        xi = xs.grid_rows(n, D, rng)
        # one row and its duplicates: ids below and above, in the source's own list and in another one
        src = int(np.nonzero(assign == 5)[0][40])
        same = np.nonzero(assign == 5)[0]
        other = np.nonzero(assign == 7)[0]
        dups = [int(same[same < src][0]), int(same[same > src][-1]), int(other[other < src][0]), int(other[other > src][-1])]
        xs.plant(xi, [(src, dups)])
        ci = np.zeros((nlist, D), dtype=np.int64)
        ci[np.arange(nlist), np.arange(nlist)] = xs.GRID
        # queries: coordinates [0, nlist) pick the probes (4, 3, 2 on the probed lists, <= 1 elsewhere), the rest is random
        qi = xs.grid_rows(GRID_NQ, D, rng)
        want_probe = np.zeros((GRID_NQ, GRID_NPROBE), dtype=np.int64)
        rest = [c for c in range(nlist) if c not in (GRID_Q127, GRID_Q140)]
        for q in range(GRID_NQ):
            if q < 140:
                p = [GRID_Q140] + list(rng.choice(rest, size=2, replace=False))
            elif q < 267:
                p = [GRID_Q127] + list(rng.choice(rest, size=2, replace=False))
            else:
                p = list(rng.choice(rest, size=3, replace=False))
            if q == GRID_FEW:
                p = [0, 1, 6]
            rng.shuffle(p)
            qi[q, :nlist] = rng.randint(-xs.GRID, 2, size=nlist)
            qi[q, p] = [4, 3, 2]
            want_probe[q] = p
        qi[:6] = xi[[src, dups[0], dups[3], 0, 1, n - 1]]      # catalogue rows as queries (d = 0 where their list is probed) ...
        for q in range(6):                                     # ... with the probe coordinates put back
            qi[q, :nlist] = rng.randint(-xs.GRID, 2, size=nlist)
            qi[q, want_probe[q]] = [4, 3, 2]
        u = xs.PIPE_UNIT
        x, q, c = xi * u, qi * u, ci * u
        unit = u * u
        safe = xs.assert_select_exact_safe((q * q).sum(1), (x * x).sum(1), unit, [q], [x], xg.PAIRS1)
        safe_c = xs.assert_select_exact_safe((q * q).sum(1), (c * c).sum(1), unit, [q], [c], xg.PAIRS1)
        d = xs.grid_dist(qi, xi)
        dc = xs.grid_dist(qi, ci)
        probe = probes(dc, GRID_NPROBE, bad_queries=(GRID_NAN_QUERY,))
        ok = np.arange(GRID_NQ) != GRID_NAN_QUERY
        assert np.array_equal(probe[ok], want_probe[ok])
        assert (probe == GRID_Q127).sum() == 127 and (probe == GRID_Q140).sum() >= 129 and (probe == 0).sum() >= 3
        probe_hand = probe.copy()
        probe_hand[10:40, 1] = -1                              # finite queries with a -1 probe
        probe_hand[20:30, 0] = -1
        probe_hand[25] = -1
        # lowered norms: |x|^2 - 2 |q|^2-ish so that the raw distance to most queries is negative; stays a multiple of the unit
        low = np.zeros(n, dtype=np.int64)
        low[list(GRID_LOW)] = -int((xi * xi).sum(1).max()) * 3
        assert all(assign[r] >= 0 for r in GRID_LOW)
        r_low = ((xi * xi).sum(1) + low) * unit
        safe_low = xs.assert_select_exact_safe((q * q).sum(1), r_low, unit, [q], [x], xg.PAIRS1)
        xf, qf = x.astype(np.float32), q.astype(np.float32)
        xf[nan_row, 3] = np.nan
        qf[GRID_NAN_QUERY, 1] = np.nan
        return dict(name="ivf grid D=%d" % D, D=D, n=n, nlist=nlist, assign=assign, x=xf, q=qf, c=c.astype(np.float32), xi=xi,
                    qi=qi, unit=unit, safe=max(safe, safe_c, safe_low), d=d, d_low=d + low[None, :], r_low=r_low.astype(np.float32),
                    probe=probe, probe_hand=probe_hand, nan_row=nan_row, src=src, dups=dups, bad_queries=(GRID_NAN_QUERY,))
    return xs.cached(("ivfgrid", D), make)


def grid_want(c, k, probe=None, low=False, **rule):
    """(D float32 tensor [nq, k], I int64 tensor [nq, k]) of the grid case from the int64 model"""
    Dm, Im = search(c["d_low"] if low else c["d"], c["assign"], c["nlist"], c["probe"] if probe is None else probe, k,
                    bad_queries=c["bad_queries"], **rule)
    return xs.from_units(Dm, c["unit"]), torch.from_numpy(Im)
