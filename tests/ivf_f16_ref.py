"""Host models of the fp16 lists of the IVF index and of its exact re-rank (include/cdml_ivf_f16.h; cdml_amd.knn.IVFIndex
with storage="f16"):

* ``quantise`` = numpy's ``astype(float16)`` (round to nearest even, overflow to inf): the image the index stores;
* the scan model = tests/ivf_ref.py's ``search`` on the distances of the ROUNDED values, over an assignment in which a
  row with a non-finite image is unlisted (``listed_assign``) and with the queries whose image is non-finite as
  ``bad_queries`` (``lost_queries``);
* the re-rank model ``refine``: the direct form sum (q - x)^2 in float64 (int64 on exact grids) over a GIVEN candidate
  table, key (d, id).  Every rule has a switch that turns it into the single mutation tests/test_ivf_f16_host.py must see:
  ties by id, a 0x7fffffff candidate, ``r`` cutting the list, the direct form against the clamped expansion.

Plain module, no pytest configuration; numpy on the CPU only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_ref as ref  # noqa: E402

NO_ID = xs.NO_ID
E_UNIT = 2.0 ** -8 + 2.0 ** -20        # |d~ - d| of unit rows under fp16 rounding (``rounding_bound``)


def quantise(x):
    """float32 -> float16, round to nearest even; |x| >= 65520 -> inf"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def listed_assign(assign, x):
    """``assign`` with -1 for every row of x (float32, as prepared) whose fp16 image has a non-finite coordinate"""
    a = np.array(assign, dtype=np.int64)
    a[~np.isfinite(quantise(x)).all(1)] = -1
    return a


def lost_queries(q):
    """the queries whose fp16 image has a non-finite coordinate (NaN queries included): they get -1 / +inf throughout"""
    return tuple(np.nonzero(~np.isfinite(quantise(q)).all(1))[0].tolist())


def rounded_dist(q, x):
    """float64 [nq, n] unclamped squared distances (|q~|^2 + |x~|^2) - 2 <q~, x~> of the fp16 images of prepared rows (no
    normalisation here: the index rounds what it prepared)"""
    with np.errstate(invalid="ignore", over="ignore"):
        qh, xh = quantise(q).astype(np.float64), quantise(x).astype(np.float64)
        return (qh * qh).sum(1)[:, None] + (xh * xh).sum(1)[None, :] - 2.0 * qh @ xh.T


def scan_search(q, x, assign, nlist, probe, k, **rule):
    """the f16 index at refine = 0: ``ivf_ref.search`` on the rounded values"""
    return ref.search(rounded_dist(q, x), listed_assign(assign, x), nlist, probe, k, bad_queries=lost_queries(q), **rule)


def refine(q, x, cand, r, k, tie_larger=False, sentinel_is_row=False, r_is_whole_list=False, expanded=False):
    """(D [nq, k], I int64 [nq, k]): per query the k best (d, id) among the first ``r`` entries of its row of ``cand`` (int
    [nq, LIST], NO_ID = no candidate), d = sum_j (q_j - x_j)^2 over the rows x[id]: int64 for integer q, x (empty = xs.INF_I),
    float64 otherwise (empty = +inf; a NaN d is no candidate).  No norms, no clamp.  The switches are the mutations:
    ``tie_larger`` = equal distances go to the larger id; ``sentinel_is_row`` = NO_ID gathers the last row (a clamped
    index); ``r_is_whole_list`` = all LIST entries are re-scored; ``expanded`` = d = max((|q|^2 + |x|^2) - 2 <q, x>, 0) in
    float32, the merge's form."""
    q, x, cand = np.asarray(q), np.asarray(x), np.asarray(cand, np.int64)
    integer = q.dtype.kind == "i" and x.dtype.kind == "i"
    if not integer:
        q, x = q.astype(np.float64), x.astype(np.float64)
    inf = xs.INF_I if integer else np.inf
    nq, n = q.shape[0], x.shape[0]
    D = np.full((nq, k), inf, dtype=np.int64 if integer else np.float64)
    I = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        c = cand[i] if r_is_whole_list else cand[i, :r]
        if sentinel_is_row:
            c = np.minimum(c, n - 1)
        c = c[(c >= 0) & (c < n)]
        if not len(c):
            continue
        if expanded:
            q32, x32 = q[i].astype(np.float32), x[c].astype(np.float32)
            d = np.maximum(((q32 * q32).sum() + (x32 * x32).sum(1)) - np.float32(2.0) * (x32 @ q32), np.float32(0.0))
            d = d.astype(np.int64) if integer else d.astype(np.float64)
        else:
            e = q[i][None, :] - x[c]
            d = (e * e).sum(1)
        if not integer:
            keep = ~np.isnan(d)
            c, d = c[keep], d[keep]
        o = np.lexsort((-c if tie_larger else c, d))[:k]
        D[i, :len(o)] = d[o]
        I[i, :len(o)] = c[o]
    return D, I


def direct_dist(q, x):
    """float64 [nq, n]: sum_j (q_j - x_j)^2, the direct form"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    return ((q[:, None, :] - x[None, :, :]) ** 2).sum(2)


def rounding_bound():
    """E with |d~ - d| <= E for unit rows q, x and their fp16 images: every coordinate moves by at most 2^-11 |v| (round to
    nearest, 11 significant bits), so |q~ - q| <= 2^-11, |x~ - x| <= 2^-11 and | |q~ - x~| - |q - x| | <= 2^-10 = e; with
    |q - x| <= 2, |d~ - d| = | |q~ - x~| - |q - x| | (|q~ - x~| + |q - x|) <= e (4 + e) = 2^-8 + 2^-20.  (A coordinate below
    2^-14 has a subnormal image and moves by at most 2^-25 instead: at most sqrt(D) 2^-25 more on each norm, under 2^-19 on d at
    D = 32 -- inside the 4 tol that ``recoverable`` adds for the device's own arithmetic.)"""
    e = 2.0 ** -10
    assert e * (4 + e) == E_UNIT
    return E_UNIT


def recovery_fixture(seed=3, clusters=64, per=16, D=32, noise=0.02, nq=256):
    """The clustered catalogue of the recovery test: ``clusters`` x ``per`` rows around Gaussian centres, l2-normalised in
    float64 and stored as float32 (the index takes them as they are, l2_norm=False); the queries are catalogue rows.
    Returns (x float32 [n, D], q float32 [nq, D])."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(clusters, D)
    x = np.repeat(centres, per, axis=0) + noise * rng.randn(clusters * per, D)
    x = x[rng.permutation(len(x))]
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = x[rng.choice(len(x), size=nq, replace=False)].copy()
    return x, q


def recoverable(d_true, probe, assign, nlist, k, r, tol):
    """bool [nq]: the queries for which the r candidates of the rounded distances must hold the whole true top k: the
    (r + 1)-th true distance among the rows of the probed lists exceeds the k-th by more than 2 E + 4 tol (fewer than r + 1
    probed rows: every probed row is a candidate)."""
    out = np.zeros(d_true.shape[0], dtype=bool)
    for i in range(d_true.shape[0]):
        m = np.concatenate([ref.members(assign, nlist, int(c)) for c in probe[i] if c >= 0] or [np.zeros(0, np.int64)])
        ds = np.sort(d_true[i, np.unique(m)])
        if len(ds) <= r:
            out[i] = True
        else:
            out[i] = ds[r] - ds[k - 1] > 2 * rounding_bound() + 4 * tol
    return out
