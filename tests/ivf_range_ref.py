"""Host model of the range search of the IVF index (cdml_amd.knn.IVFIndex.range_search; include/cdml_ivf_range.h) on top of
tests/ivf_ref.py: for a matrix of UNCLAMPED distances (int64 on exact grids, float64 otherwise), an assignment, a probe table
and a radius per query, every listed row of the query's probed lists with max(d, 0) <= radius, sorted by (d, id).  The rules
have switches that turn them into the single mutations tests/test_ivf_range_host.py must see: ``strict`` (`<` instead of `<=`:
a tie at the radius is lost) and ``list_unlisted`` (an unlisted row counts as a member of the last list).  Also the model of
``knn.range_compact``, the radii the GPU tests use, and integer PQ cases for the scan's tile edges (plain and residual).

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_pqr_ref as pqr  # noqa: E402
import ivf_ref as ref  # noqa: E402


def members_of(assign, nlist, probe_row, list_unlisted=False):
    """int64 ids, ascending and distinct: the rows of the lists of one probe row (-1 = no list)"""
    rows = [ref.members(assign, nlist, int(c), list_unlisted) for c in np.asarray(probe_row, np.int64) if c >= 0]
    return np.unique(np.concatenate(rows + [np.zeros(0, np.int64)])).astype(np.int64)


def range_search(d, assign, nlist, probe, radius, bad_queries=(), strict=False, list_unlisted=False):
    """(lims int64 [nq + 1], D [total] in d's type, I int64 [total]): per query the (max(d, 0), id) of the members of its probed
    lists with max(d, 0) <= radius[q], sorted by (d, id).  ``radius``: a scalar or [nq], in d's units (a NaN or a negative one
    passes nothing; +inf passes every row whose d is no NaN).  A query of ``bad_queries`` gets nothing."""
    d = np.asarray(d)
    nq = d.shape[0]
    rad = np.broadcast_to(np.asarray(radius, dtype=np.float64), (nq,))
    lims = np.zeros(nq + 1, dtype=np.int64)
    Ds, Is = [], []
    for q in range(nq):
        cand = np.zeros(0, np.int64) if q in bad_queries else members_of(assign, nlist, probe[q], list_unlisted)
        dq = d[q, cand]
        if d.dtype.kind != "i":
            ok = ~np.isnan(dq)
            cand, dq = cand[ok], dq[ok]
        dq = np.maximum(dq, 0)
        with np.errstate(invalid="ignore"):
            ok = dq < rad[q] if strict else dq <= rad[q]
        cand, dq = cand[ok], dq[ok]
        o = np.lexsort((cand, dq))
        Ds.append(dq[o])
        Is.append(cand[o])
        lims[q + 1] = lims[q] + len(o)
    D = np.concatenate(Ds + [np.zeros(0, d.dtype)])
    return lims, D, np.concatenate(Is + [np.zeros(0, np.int64)]).astype(np.int64)


def kth_radius(d, assign, nlist, probe, k, bad_queries=()):
    """float64 [nq]: the query's k-th model distance (a tie AT the radius for the range search); +inf where it has fewer
    than k rows, -1 for a query of ``bad_queries``"""
    Dk, _ = ref.search(d, assign, nlist, probe, k, bad_queries=bad_queries)
    r = Dk[:, k - 1].astype(np.float64)
    r[Dk[:, k - 1] == (xs.INF_I if np.asarray(d).dtype.kind == "i" else np.inf)] = np.inf
    r[list(bad_queries)] = -1.0
    return r


def gap_radius(d, assign, nlist, probe, rank, bad_queries=()):
    """float64 [nq]: halfway between two DISTINCT consecutive model distances of the query, the first such pair at or behind
    ``rank`` (else the last before it; -1 where the query has no two distinct distances)"""
    d = np.asarray(d)
    out = np.full(d.shape[0], -1.0)
    for q in range(d.shape[0]):
        if q in bad_queries:
            continue
        dq = d[q, members_of(assign, nlist, probe[q])]
        ds = np.unique(np.maximum(dq[~np.isnan(dq)] if d.dtype.kind != "i" else dq, 0)).astype(np.float64)
        if len(ds) > 1:
            i = min(rank, len(ds) - 2)
            out[q] = 0.5 * (ds[i] + ds[i + 1])
    return out


def as_tensors(res, unit=None):
    """the model's (lims, D, I) as the tensors ``range_search`` returns: int64 units -> exact float32 with ``unit``"""
    lims, D, I = res
    Dt = xs.from_units(D, unit) if unit is not None else torch.from_numpy(np.asarray(D, np.float32))
    return torch.from_numpy(lims), Dt.reshape(-1), torch.from_numpy(I)


def compact(cand, cnt, cap):
    """the model of ``knn.range_compact`` on numpy: cand int32 [m, cap, 2], cnt [m]"""
    cand = np.asarray(cand, np.int32).reshape(len(cnt), cap, 2)
    lims = np.zeros(len(cnt) + 1, dtype=np.int64)
    Ds, Is = [], []
    for q, c in enumerate(np.asarray(cnt, np.int64)):
        m = int(min(max(c, 0), cap))
        dq = cand[q, :m, 0].copy().view(np.float32)
        iq = cand[q, :m, 1].astype(np.int64)
        o = np.lexsort((iq, dq))
        Ds.append(dq[o])
        Is.append(iq[o])
        lims[q + 1] = lims[q] + m
    return lims, np.concatenate(Ds + [np.zeros(0, np.float32)]), np.concatenate(Is + [np.zeros(0, np.int64)])


# ---- integer PQ cases for the scan's tile edges ------------------------------------------------------------------------------------
def tile_case(M, D, S, R, residual, tag="ivfrange-tiles"):
    """tests/test_gpu_ivf_pq.py's test_tile_edges construction: list lengths 0, 1, R - 1, R, R + 1, 2 R + 5; list 5 probed by
    S + 2 queries (S + 1 without the first), list 4 by S, list 3 by S - 1; -1 probes; integer rows and distinct grid codewords
    (residual: on small integer centroids).  Returns a dict with the float operands, the int64 distances of the DECODED rows
    ``d`` and ``unit``; ``assert_select_exact_safe`` < 2^24 is asserted here."""
    rng = xg.case_rng(tag, M, int(residual))
    dsub = D // M
    lens = (0, 1, R - 1, R, R + 1, 2 * R + 5)
    nlist, n = len(lens), sum(lens)
    groups = [(5, S + 1), (4, S), (3, S - 1), (2, 3), (1, 2), (0, 2)]
    probe = [[1, 5]] + [[a, -1] for a, cnt in groups for _ in range(cnt)]
    probe[-1] = [0, 2]
    probe = np.asarray(probe, dtype=np.int64)
    nq = len(probe)
    assign = np.repeat(np.arange(nlist), lens)
    rng.shuffle(assign)
    xi = xs.grid_rows(n, D, rng)
    ci = rng.randint(-2, 3, size=(nlist, D)).astype(np.int64) if residual else np.zeros((nlist, D), dtype=np.int64)
    cbi = np.stack([pq._distinct_codewords(rng, dsub, dsub)[0] for _ in range(M)])
    if residual:
        codes, _ = pqr.encode(xi, ci, assign, cbi)
        xh = pqr.decode(codes, ci, assign, cbi)
    else:
        codes, _ = pq.encode(xi, cbi)
        xh = pq.decode(codes, cbi)
    qi = xs.grid_rows(nq, D, rng)
    u = xs.PIPE_UNIT
    q, xd = qi * u, xh * u
    assert xs.assert_select_exact_safe((q * q).sum(1), (xd * xd).sum(1), u * u, [q], [xd], xg.PAIRS1) < 2.0 ** 24
    assert float(np.abs(pqr.slot_dot(qi, ci)).max() + np.abs(pq.lut(qi, cbi)).max(2).sum(1).max()) < 2.0 ** 24
    cnt = np.bincount(probe[probe >= 0], minlength=nlist)
    assert cnt[4] == S and cnt[3] == S - 1 and cnt[5] == S + 2
    return dict(M=M, D=D, lens=lens, nlist=nlist, n=n, nq=nq, assign=assign, probe=probe, codes=codes, residual=bool(residual),
                x=(xi * u).astype(np.float32), q=q.astype(np.float32), c=(ci * u).astype(np.float32),
                cb=(cbi * u).astype(np.float32), d=xs.grid_dist(qi, xh), unit=u * u)
