"""Exact-arithmetic operands and integer oracles for the kernels that CHOOSE instead of sum: the kNN list kernels
(k_knn_merge, k_knn_merge_list in csrc/knn.hip), the kNN filter, the rank count and the semi-hard miner (the epilogues
BE_KNN_X3, BE_RANK_X3, BE_MINE_X3 of csrc/gemm_bf16_256.hip, each also built for fp16) and the unfused k_semihard_select
(csrc/loss.hip).

A test against fp64 on Gaussian data has to allow a band around every compare, and inside that band live the rules this
code spends most of its lines on: ties by id or by column, ``<`` against ``<=``, the clamp at 0, self / partner
exclusion, padding rows, ``n_valid`` cutting a 4-vector, the fallback merged across strips.  The operands built here make
every norm, inner product and distance an integer multiple of one power-of-two unit, far below 2^24 units, so any
summation order, with or without fma contraction, gives the same fp32 bits; the expectation is an int64 computation and
every comparison is ``torch.equal``, ties included.

* grid rows: integers in [-4, 4] times a power of two: one bf16 / fp16 plane holds them, the dropped plane products are 0;
* three-/two-plane operands (tests/exact_gemm.py ``plane_operand``) for the entries that take planes and norms as
  separate arguments: the score is ``expected(Ap, Bp, PAIRS6 | PAIRS_H2)``, |q|^2, |b|^2 and tau integers of the case's
  own choosing (the kernels only read them) -- this pins the pair list and the (row, column) of every accumulator element
  inside the three epilogues;
* duplicates planted on purpose, below and above the ids they tie with, straddling tile boundaries;
* ``assert_select_exact_safe``: the condition under which zero tolerance is legitimate, computed; every case builder calls
  it and records the result under "safe" -- a test runs no case without it;
* oracles in int64 (distance units): ``knn_int``, ``filter_int``, ``rank_int``, ``semihard_int``, ``merge_model``; every
  rule they implement has a switch that turns it into the single mutation tests/test_exact_select_host.py must see.

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import footprint as fp  # noqa: E402

INF_I = np.iinfo(np.int64).max        # "+inf" of the integer oracles
NO_ID = 0x7FFFFFFF                    # the id of an empty list slot (csrc/knn.hip)
LIST = 128                            # CDML_KNN_LIST: entries per query list (tests assert ops.knn_list_capacity() == LIST)
GRID = 4                              # grid rows: integers in [-GRID, GRID]
_CASES = {}


def cached(key, make):
    """one case per key: the host tests check exactly the objects the GPU tests launch"""
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ---- units -------------------------------------------------------------------------------------------------------------
def to_units(x, unit):
    """float64 values -> int64 multiples of ``unit``, asserting that nothing is rounded (+inf -> INF_I)"""
    x = np.asarray(x, dtype=np.float64)
    r = x / unit
    fin = np.isfinite(r)
    assert np.array_equal(r[fin], np.rint(r[fin])), "a value is no multiple of the unit"
    assert not np.isnan(r).any() and not (r == -np.inf).any()
    out = np.full(r.shape, INF_I, dtype=np.int64)
    out[fin] = np.rint(r[fin]).astype(np.int64)
    return out


def from_units(d, unit):
    """int64 units -> float32 tensor, asserting exactness (INF_I -> +inf)"""
    d = np.asarray(d, dtype=np.int64)
    v = np.where(d == INF_I, np.inf, d.astype(np.float64) * unit)
    w = v.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), v), "the expected distance is not an fp32 number"
    return torch.from_numpy(w)


def assert_select_exact_safe(q_sq, b_sq, unit, Ap=None, Bp=None, pairs=None, scale=1.0, score=None):
    """Zero tolerance is legitimate for d = (|q|^2 + |b|^2) - 2 scale <q, b>:

    * every |q|^2, |b|^2 and 2 scale <q, b> is an integer multiple of the power of two ``unit`` -- for a product given as
      planes (``Ap``, ``Bp``, ``pairs``) every single term 2 scale a b is (exact_gemm.assert_exact_safe on the unit of the
      accumulator, unit / (2 scale)), for a score given directly (``score``) the score itself;
    * for every (query, row) the sum of the absolute values of all product terms stays below 2^24 accumulator units, and
      |q|^2 + |b|^2 + 2 scale sum |a| |b| below 2^24 ``unit``: every partial sum, in any order, contracted into fmas or not,
      is an integer number of units below 2^24 -- exact in fp32.

    Returns the largest such sum in units."""
    ue = np.log2(unit)
    assert ue == np.floor(ue), "unit must be a power of two"
    q_sq, b_sq = np.asarray(q_sq, np.float64), np.asarray(b_sq, np.float64)
    for v in (q_sq, b_sq):
        assert np.isfinite(v).all() and xg._granule_exp(v) >= ue, "a squared norm is no multiple of the unit"
    if score is None:
        acc_unit = unit / (2.0 * scale)
        xg.assert_exact_safe(Ap, Bp, pairs, acc_unit)
        tot = None
        for p, q in pairs:
            t = np.abs(Ap[p]) @ np.abs(Bp[q]).T
            tot = t if tot is None else tot + t
    else:
        tot = np.abs(np.asarray(score, np.float64))
        assert xg._granule_exp(2.0 * scale * tot) >= ue, "a score is no multiple of half the unit"
    worst = float((np.abs(q_sq)[:, None] + np.abs(b_sq)[None, :] + 2.0 * scale * tot).max()) / unit
    assert worst < 2.0 ** 24, "the absolute sums reach %g units of 2^%d: not below 2^24" % (worst, ue)
    return worst


def assert_h2_exact(x, scale):
    """x * scale (the fp16 split's input, knn._planes_h2 / the miner's prep) is an fp16 number inside its range: the high
    plane holds it, the low plane is zero"""
    v = np.asarray(x, np.float64) * scale
    h = torch.from_numpy(v).to(torch.float16).double().numpy()
    assert np.isfinite(h).all() and np.array_equal(h, v), "the grid is not exact in fp16 at scale %g" % scale


def h2_scale_of(x):
    """the scale knn._planes_h2 picks for a tensor: pow2_for(max |x|, 2^13) (restated: a power of two putting the maximum
    in (2^12, 2^13])"""
    amax = float(np.abs(np.asarray(x, np.float64)).max())
    return 2.0 ** max(-30, min(40, int(np.floor(np.log2(2.0 ** 13 / amax)))))


# ---- distances in units -------------------------------------------------------------------------------------------------
def _keep(n, drop_k):
    keep = np.ones(n, dtype=bool)
    if drop_k is not None:
        keep[drop_k[0]:drop_k[1]] = False
    return keep


def grid_dist(qi, bi, drop_k=None):
    """int64 [nq][nb]: |q|^2 + |b|^2 - 2 <q, b> of integer grid rows (units of unit^2), unclamped.  ``drop_k`` = (lo, hi):
    the product without those k (a dropped K tile; the norms are separate inputs of the kernels and stay)"""
    qi, bi = np.asarray(qi, np.int64), np.asarray(bi, np.int64)
    keep = _keep(qi.shape[1], drop_k)
    return (qi * qi).sum(1)[:, None] + (bi * bi).sum(1)[None, :] - 2 * (qi[:, keep] @ bi[:, keep].T)


def plane_dist(Ap, Bp, pairs, q_sq, b_sq, unit, scale=1.0, drop_k=None):
    """int64 [nq][nb] units: (q_sq + b_sq) - 2 scale sum_pairs A_p B_q^T, unclamped (float64 holds every value exactly)"""
    keep = _keep(Ap[0].shape[1], drop_k)
    s = xg.expected([a[:, keep] for a in Ap], [b[:, keep] for b in Bp], pairs)
    return to_units(np.asarray(q_sq, np.float64)[:, None] + np.asarray(b_sq, np.float64)[None, :] - 2.0 * scale * s, unit)


def permute_tile(d, kind, tile=256):
    """the ways a register-layout index can be wrong: rows r <-> r ^ 1 or columns c <-> c ^ 1 | c ^ 4 | c ^ 16 swapped
    inside a tile (a partner outside the matrix: unchanged)"""
    d = np.asarray(d)
    axis, bit = {"r^1": (0, 1), "c^1": (1, 1), "c^4": (1, 4), "c^16": (1, 16)}[kind]
    n = d.shape[axis]
    idx = np.arange(n) ^ bit
    idx = np.where(idx < n, idx, np.arange(n))
    assert (idx // tile == np.arange(n) // tile).all()
    return d[idx] if axis == 0 else d[:, idx]


TILE_PERMUTATIONS = ("r^1", "c^1", "c^4", "c^16")


# ---- oracles (int64; every switch is one mutation of the rule) -----------------------------------------------------------
def knn_from_dist(d, ids, k, n_valid=None, clamp=True, tie_larger=False):
    """(D int64 [nq][k], I int64 [nq][k]): per query the k smallest (max(d, 0), id) over ids < n_valid, by lexsort; where
    fewer than k valid rows exist the tail is INF_I / -1"""
    d, ids = np.asarray(d, np.int64), np.asarray(ids, np.int64)
    if clamp:
        d = np.maximum(d, 0)
    sel = np.nonzero(ids < (INF_I if n_valid is None else n_valid))[0]
    D = np.full((d.shape[0], k), INF_I, dtype=np.int64)
    I = np.full((d.shape[0], k), -1, dtype=np.int64)
    key = -ids[sel] if tie_larger else ids[sel]
    for r in range(d.shape[0]):
        o = sel[np.lexsort((key, d[r, sel]))[:k]]
        D[r, :len(o)] = d[r, o]
        I[r, :len(o)] = ids[o]
    return D, I


def knn_int(qi, bi, k, n_valid=None, **rule):
    """the exact kNN of integer grid rows: ordered by (max(d, 0), id)"""
    return knn_from_dist(grid_dist(qi, bi), np.arange(len(bi)), k, n_valid, **rule)


def filter_int(d, ids, tau, n_valid, strict=False, clamp=True):
    """per query the SET {(d, id): max(d, 0) <= tau, id < n_valid} as an int64 array [m][2] sorted by (d, id)"""
    d, ids = np.asarray(d, np.int64), np.asarray(ids, np.int64)
    if clamp:
        d = np.maximum(d, 0)
    out = []
    for r in range(d.shape[0]):
        ok = (ids < n_valid) & ((d[r] < tau[r]) if strict else (d[r] <= tau[r]))
        c = np.stack([d[r, ok], ids[ok]], axis=1)
        out.append(c[np.lexsort((c[:, 1], c[:, 0]))])
    return out


def rank_int(d, self_id, pos_id, n_valid, clamp=True, tie="smaller", exclude_self=True, exclude_partner=True):
    """(tau int64 [nq], count int64 [nq]) over the whole catalogue (column j = id j): the full rule of
    Evaluation.ranks / the comment block of BE_RANK_X3 -- tau = max(d(i, p_i), 0); count = #{j < n_valid, j != a_i, p_i:
    d < tau or (d == tau and j < p_i)} on clamped distances.  ``tie``: "smaller" (the rule), "larger" (id > partner),
    "none" (d < tau only), "all" (d <= tau)."""
    d = np.asarray(d, np.int64)
    if clamp:
        d = np.maximum(d, 0)
    nq, n = d.shape
    j = np.arange(n)
    tau = d[np.arange(nq), pos_id]
    cnt = np.zeros(nq, dtype=np.int64)
    for i in range(nq):
        ok = j < n_valid
        if exclude_self:
            ok &= j != self_id[i]
        if exclude_partner:
            ok &= j != pos_id[i]
        eq = d[i] == tau[i]
        ahead = d[i] < tau[i]
        if tie == "smaller":
            ahead |= eq & (j < pos_id[i])
        elif tie == "larger":
            ahead |= eq & (j > pos_id[i])
        elif tie == "all":
            ahead |= eq
        cnt[i] = int((ok & ahead).sum())
    return tau, cnt


def semihard_from_dist(dist, rows, ge=False, tie_larger=False, skip_cols=None):
    """neg_row int32 [B] by oracle.tower.semihard_select's rule on an integer distance matrix [B][2B] (NOT clamped: the
    rule has no clamp): eligible = other videos than the anchor's and the positive's; the closest eligible row with
    d > d_p (``ge``: >=), first index on a tie (``tie_larger``: last); none: the farthest eligible row, first index; none
    eligible: -1.  ``skip_cols`` = (lo, hi): those columns ignored (a strip the merge lost)."""
    dist, rows = np.asarray(dist, np.int64), np.asarray(rows)
    B = dist.shape[0]
    d_p = dist[np.arange(B), 2 * np.arange(B) + 1]
    elig = (rows[None, :] != rows[0::2, None]) & (rows[None, :] != rows[1::2, None])
    if skip_cols is not None:
        elig[:, skip_cols[0]:skip_cols[1]] = False
    outside = elig & ((dist >= d_p[:, None]) if ge else (dist > d_p[:, None]))
    neg = np.full(B, -1, dtype=np.int32)
    pick = (lambda m: len(m) - 1 - int(np.argmax(m[::-1]))) if tie_larger else (lambda m: int(np.argmax(m)))
    for i in range(B):
        if outside[i].any():
            v = np.where(outside[i], dist[i], INF_I)
            neg[i] = pick(v == v.min())
        elif elig[i].any():
            v = np.where(elig[i], dist[i], -INF_I)
            neg[i] = pick(v == v.max())
    return neg


def semihard_int(Ei, rows, drop_k=None, **rule):
    """semihard_select of integer grid rows E [2B][D] (row 2i anchor, 2i + 1 positive)"""
    return semihard_from_dist(grid_dist(np.asarray(Ei)[0::2], Ei, drop_k), rows, **rule)


def merge_model(calls, k, clamp=True):
    """The per-query list of cdml_knn_merge over a score block streamed in several calls.  ``calls``: (d int64 [nq][nb],
    col0, n_valid, first) in launch order; column c of a call has id col0 + c and counts where id < n_valid.  A call with
    ``first`` starts from the empty list, another one from the list as it stands; an element enters if its (max(d, 0), id)
    is below the list's k-th key, and the k smallest keys stay.  Returns (D, I) int64 [nq][k], INF_I / NO_ID where empty."""
    D = I = None
    for d, col0, n_valid, first in calls:
        d = np.asarray(d, np.int64)
        if clamp:
            d = np.maximum(d, 0)
        nq, nb = d.shape
        ids = col0 + np.arange(nb, dtype=np.int64)
        if first or D is None:
            D = np.full((nq, k), INF_I, dtype=np.int64)
            I = np.full((nq, k), NO_ID, dtype=np.int64)
        for r in range(nq):
            td, ti = D[r, k - 1], I[r, k - 1]
            ok = (ids < n_valid) & ((d[r] < td) | ((d[r] == td) & (ids < ti)))
            ad, ai = np.concatenate([D[r], d[r, ok]]), np.concatenate([I[r], ids[ok]])
            o = np.lexsort((ai, ad))[:k]
            D[r], I[r] = ad[o], ai[o]
    return D, I


def merge_stream(c):
    """(d int64 [nq][sum nb], ids) of a merge case's calls side by side: the whole stream as ONE block, for knn_from_dist"""
    return np.concatenate([x["d"] for x in c["calls"]], axis=1), np.concatenate([x["col0"] + np.arange(x["nb"]) for x in c["calls"]])


def merge_lists_int(list_d, list_i, cands, k, tie_larger=False):
    """cdml_knn_merge_list: per query the k smallest (d, id) of its list (int64 [nq][LIST]) and its candidate set"""
    nq = list_d.shape[0]
    D = np.empty((nq, k), dtype=np.int64)
    I = np.empty((nq, k), dtype=np.int64)
    for r in range(nq):
        ad = np.concatenate([list_d[r], cands[r][:, 0]])
        ai = np.concatenate([list_i[r], cands[r][:, 1]])
        o = np.lexsort((-ai if tie_larger else ai, ad))[:k]
        D[r], I[r] = ad[o], ai[o]
    return D, I


def assert_list_ascending(d, i, what="list"):
    """a whole LIST-entry list (float32 / int32 tensors [nq][LIST]) ascends in (d, id)"""
    d, i = d.detach().cpu().double().numpy(), i.detach().cpu().numpy().astype(np.int64)
    assert not np.isnan(d).any(), "%s: NaN in a list" % what
    ok = (d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] >= i[:, :-1]))
    both_empty = (i[:, 1:] == NO_ID) & (i[:, :-1] == NO_ID)
    strict = (d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] > i[:, :-1])) | both_empty
    assert ok.all() and strict.all(), "%s: not ascending in (d, id) at %s" % (what, np.argwhere(~(ok & strict))[:3].tolist())


# ---- fp32 recomputation in several orders (the host tests: the same bits) -------------------------------------------------
def dist_f32_forms(q_sq, b_sq, score, scale=1.0):
    """[float32 arrays]: d from float32 inputs as the kernels form it -- (qs + bs) - 2 s (two roundings), fma(-2 s, x, qs + bs)
    (the product unrounded), and qs + (bs - 2 s)"""
    qs = np.asarray(q_sq, np.float32)[:, None]
    bs = np.asarray(b_sq, np.float32)[None, :]
    s = np.asarray(score, np.float32)
    two = np.float32(2.0 * scale)
    a = ((qs + bs).astype(np.float32) - (two * s).astype(np.float32)).astype(np.float32)
    b = ((qs + bs).astype(np.float32).astype(np.float64) - np.float64(two) * s.astype(np.float64)).astype(np.float32)
    c = (qs + (bs - (two * s).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return [a, b, c]


def grid_score_f32(q, b, order, chunk=16):
    """q b^T re-associated in float32: k in ``order``, chunk by chunk into one float32 accumulator"""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((q.shape[0], b.shape[0]), dtype=np.float32)
    for i in range(0, len(order), chunk):
        ks = order[i:i + chunk]
        acc = (acc + q[:, ks] @ b[:, ks].T).astype(np.float32)
    return acc


def sqnorm_f32(x, order):
    x = np.asarray(x, np.float32)
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for k in order:
        acc = (acc + x[:, k] * x[:, k]).astype(np.float32)
    return acc


# ---- operands ----------------------------------------------------------------------------------------------------------------
def grid_rows(n, D, rng):
    """integers in [-GRID, GRID], int64 [n][D]"""
    return rng.randint(-GRID, GRID + 1, size=(n, D)).astype(np.int64)


def plant(x, groups):
    """x[dst] = x[src] for every (src, dsts) of ``groups`` (in place; identical rows: bit-identical scores)"""
    for src, dsts in groups:
        for t in dsts:
            x[t] = x[src]
    return x


def strided(v, pad=4, dtype=torch.float32):
    """a [rows][cols] CPU tensor as a view with ld = cols + pad into a poisoned buffer"""
    v = torch.as_tensor(v).to(dtype)
    buf = fp.poisoned((v.shape[0], v.shape[1] + pad), dtype=dtype, device="cpu")
    buf[:, :v.shape[1]] = v
    return buf


def _plane_rows(n, D, form, rng, groups=()):
    """(buffer, plane, planes, n_planes, pairs, dtype) of ``n`` rows as independent planes (exact_gemm.plane_operand) with
    the rows of ``groups`` made identical"""
    n_planes, scales, dtype, pairs = ((3, xg.SCALES_BF16, torch.bfloat16, xg.PAIRS6) if form == "x3"
                                      else (2, xg.SCALES_F16, torch.float16, xg.PAIRS_H2))
    buf, plane, planes = xg.plane_operand(n, D, n_planes, rng, scales, dtype=dtype)
    for p in planes:
        plant(p, groups)
    plant(buf, groups)
    return buf, plane, planes, pairs


H2_OUT_SCALE = 2.0 ** -2          # the fp16 entries' out_scale in the plane cases: d = qs + bs - 2 * 2^-2 * acc
PLANE_UNIT = {"x3": 2.0 ** -11,   # 2 * the smallest term of PAIRS6 under SCALES_BF16 (2^-12)
              "h2": 2.0 ** -9}    # 2 * 2^-2 * the smallest term of PAIRS_H2 under SCALES_F16 (2^-8)


def _scale(form):
    return H2_OUT_SCALE if form == "h2" else 1.0


# ---- cdml_knn_merge: scores given directly ------------------------------------------------------------------------------------
MERGE_KS = (1, 51, 128)
MERGE_NQ = (1, 5, 9)
MERGE_NB = (4, 252, 256, 260, 1024)
MERGE_ORDERS = ("random", "descending", "ascending", "equal", "negative")
MERGE_UNIT = 1.0                  # d, |q|^2, |b|^2 integers; the score (qs + bs - d) / 2 a multiple of 1/2


def merge_block(order, nq, nb, rng, base=0):
    """int64 [nq][nb] raw distances of one stream order: "random" (few distinct values: ties everywhere), "descending" by
    column (strictly: every element enters, the buffer compacts every LIST insertions), "ascending", "equal" (pure id order),
    "negative" (a block of negative raw distances: the clamp makes ties at 0 that go by id)"""
    c, r = np.arange(nb, dtype=np.int64)[None, :], np.arange(nq, dtype=np.int64)[:, None]
    if order == "random":
        return base + rng.randint(0, 40, size=(nq, nb)).astype(np.int64)
    if order == "descending":
        return base + 5000 - c - 3 * r
    if order == "ascending":
        return base + c + 3 * r
    if order == "equal":
        return np.full((nq, nb), base + 7, dtype=np.int64) + 0 * r
    if order == "negative":
        d = rng.randint(-20, 20, size=(nq, nb)).astype(np.int64)
        d[:, nb // 4:nb // 2] = -1 - rng.randint(0, 9, size=(nq, nb // 2 - nb // 4))
        return d
    raise ValueError(order)


def merge_case(order, nq, calls_nb, col0=0, n_valid=None, tag=""):
    """One stream of cdml_knn_merge calls: ``calls_nb`` = the blocks' widths, ids running on from ``col0``.  Per call the
    score s = (qs + bs - d) / 2 with integer qs, bs: a multiple of 1/2, so d = (qs + bs) - 2 s exactly.  ``n_valid``: the
    catalogue's size (default: every column valid)."""
    def make():
        rng = xg.case_rng("merge", order, nq, col0, tag, *calls_nb)
        qs = rng.randint(0, 65, size=nq).astype(np.float64)
        calls, c0 = [], col0
        total = col0 + sum(calls_nb)
        nv = total if n_valid is None else n_valid
        worst = 0.0
        for j, nb in enumerate(calls_nb):
            d = merge_block(order, nq, nb, rng, base=0 if order == "negative" else 2 * j)
            bs = rng.randint(0, 65, size=nb).astype(np.float64)
            s = (qs[:, None] + bs[None, :] - d) / 2.0
            worst = max(worst, assert_select_exact_safe(qs, bs, MERGE_UNIT, score=s))
            calls.append(dict(d=d, col0=c0, nb=nb, b_sq=bs, score=s, first=(j == 0)))
            c0 += nb
        return dict(name="merge %s nq=%d nb=%s col0=%d n_valid=%d" % (order, nq, list(calls_nb), col0, nv), order=order, nq=nq,
                    q_sq=qs, calls=calls, n_valid=nv, unit=MERGE_UNIT, safe=worst)
    return cached(("merge", order, nq, tuple(calls_nb), col0, n_valid, tag), make)


def merge_calls(c):
    """the case as ``merge_model`` takes it"""
    return [(x["d"], x["col0"], c["n_valid"], x["first"]) for x in c["calls"]]


def merge_params():
    """the arguments (order, nq, calls_nb, col0, n_valid, tag) of every stream of tests/test_gpu_exact_select.py::
    test_knn_merge, without building any: each order x nq x nb in one call; n_valid inside a 4-vector and before a whole
    256-column pass; col0 > 0; two and three consecutive calls; fewer valid rows than k"""
    out = []
    for order in MERGE_ORDERS:
        for nq in MERGE_NQ:
            for nb in MERGE_NB:
                out.append((order, nq, (nb,), 0, None, ""))
        out.append((order, 5, (260,), 0, 258, "cut4"))                                   # n_valid inside a 4-vector
        out.append((order, 5, (1024,), 512, 512 + 701, "cutpass"))                       # ... and a whole pass behind it
        out.append((order, 9, (256, 260), 0, None, "two"))
        out.append((order, 5, (252, 1024, 4), 768, 768 + 252 + 1024 + 2, "three"))
        out.append((order, 5, (256,), 0, 40, "short"))                                   # fewer valid rows than k = 51 | 128
    return out


def all_merge_cases():
    return [merge_case(*a) for a in merge_params()]


# ---- the kNN filter and cdml_knn_merge_list: plane operands ------------------------------------------------------------------
FILTER_NQ = 300
FILTER_K = 51
FILTER_CAP = 1024
FILTER_SHAPES = tuple((n_cols, D, col0) for n_cols in (256, 768) for D in (64, 128) for col0 in (0, 512))
FILTER_INVALID = 37               # the last tile's rows from n_cols - 37 on are padding: n_valid cuts a 4-vector


def filter_case(form, n_cols, D, col0, small_cap=False):
    """cdml_knn_filter_x3 | _h2 on independent planes + cdml_knn_merge_list.  nq = 300 (a full row tile + 44 rows).
    |q|^2, |b|^2: integers that put the distances ~ 2.8 sigma of the score above 0 (most positive, a few clamped); identical
    catalogue rows (planes and |b|^2) inside a tile, across the 256 boundary, across n_valid.  tau per query, from the
    oracle: +inf (an empty or short list: every valid row is a candidate), 0, the distance of a planted duplicate (several
    candidates AT tau), or an order statistic of the row's distances.  Every query's running list is built so that its
    k-th entry IS tau (what knn_search passes), ids disjoint from the block's, below them (col0 = 512) or above (col0 = 0).
    ``small_cap``: no +inf rows, one query with more candidates than every other, ``cap`` below exactly that count."""
    def make():
        rng = xg.case_rng("filter", form, n_cols, D, col0, int(small_cap))
        nq, k, unit, scale = FILTER_NQ, FILTER_K, PLANE_UNIT[form], _scale(form)
        n_valid = col0 + n_cols - FILTER_INVALID
        groups = [(5, [6, 200]), (n_cols - 40, [n_cols - 39, n_cols - 30])]
        if n_cols > 256:
            groups += [(255, [256, 257]), (300, [100, 600])]
        Q, plane_q, Ap, pairs = _plane_rows(nq, D, form, rng)
        Bk, plane_b, Bp, _ = _plane_rows(n_cols, D, form, rng, groups)
        sigma = 2.0 * scale * np.sqrt(D * xg.DENSITY ** 2)     # of 2 scale <q, b>: the norms put |q|^2 + |b|^2 ~ 2.8 sigma above 0
        lo, span = int(sigma), int(0.8 * sigma) + 1
        qs = rng.randint(lo, lo + span + 1, size=nq).astype(np.float64)
        bs = plant(rng.randint(lo, lo + span + 1, size=n_cols).astype(np.float64), groups)
        safe = assert_select_exact_safe(qs, bs, unit, Ap, Bp, pairs, scale)
        d = plane_dist(Ap, Bp, pairs, qs, bs, unit, scale)
        ids = col0 + np.arange(n_cols, dtype=np.int64)
        dc = np.maximum(d, 0)
        srt = np.sort(np.where(ids[None, :] < n_valid, dc, INF_I), axis=1)
        tau = np.empty(nq, dtype=np.int64)
        kind = []
        for i in range(nq):
            t = "stat" if small_cap else ("inf", "zero", "dup", "stat", "stat", "stat")[i % 6]
            if t == "zero" and dc[i, :n_cols - FILTER_INVALID].min() > 0:
                t = "stat"                                  # (tau = 0 only where something is clamped: else an empty set)
            kind.append(t)
            m = 60 if (small_cap and i == 123) else 1 + (i * 7) % 40
            tau[i] = {"inf": INF_I, "zero": 0, "dup": dc[i, 5], "stat": srt[i, m - 1]}[t]
        cands = filter_int(d, ids, tau, n_valid)
        counts = np.array([len(c) for c in cands])
        cap = FILTER_CAP
        if small_cap:
            top = np.sort(counts)
            cap = int(top[-1]) - 1
            assert top[-2] <= cap < top[-1], "the small cap must be below exactly one query's count"
        # the running lists [nq][LIST]: k-th entry = tau; beyond k ascending too
        lo, hi = (0, col0) if col0 else (2048, 4096)
        list_d = np.full((nq, LIST), INF_I, dtype=np.int64)
        list_i = np.full((nq, LIST), NO_ID, dtype=np.int64)
        for i in range(nq):
            if tau[i] == INF_I:
                m = (i % 3) * 10                            # fewer than k entries: the k-th is empty
                dv = np.sort(rng.randint(0, 40 * 2048, size=m)).astype(np.int64)
            else:
                head = np.sort(np.append(rng.randint(0, tau[i] + 1, size=k - 1), tau[i]))
                tail = np.sort(tau[i] + rng.randint(0, 4, size=LIST - k)) if i % 2 else np.zeros(0, dtype=np.int64)
                dv = np.concatenate([head, tail]).astype(np.int64)
                m = len(dv)
            iv = rng.choice(np.arange(lo, hi), size=m, replace=False).astype(np.int64)
            o = np.lexsort((iv, dv))
            list_d[i, :m], list_i[i, :m] = dv[o], iv[o]
            assert list_d[i, k - 1] == tau[i]
        wd, wi = merge_lists_int(list_d, list_i, cands, k)
        return dict(name="filter %s n_cols=%d D=%d col0=%d%s" % (form, n_cols, D, col0, " small cap" if small_cap else ""),
                    form=form, nq=nq, n_cols=n_cols, D=D, col0=col0, n_valid=n_valid, k=k, cap=cap, unit=unit, scale=scale,
                    Q=Q, plane_q=plane_q, Ap=Ap, B=Bk, plane_b=plane_b, Bp=Bp, pairs=pairs, q_sq=qs, b_sq=bs, d=d, ids=ids,
                    tau=tau, kind=kind, cands=cands, counts=counts, list_d=list_d, list_i=list_i, want_d=wd, want_i=wi,
                    safe=safe, small_cap=small_cap)
    return cached(("filter", form, n_cols, D, col0, small_cap), make)


def filter_params():
    """(form, n_cols, D, col0, small_cap) of every filter case, without building any"""
    out = [(form,) + s + (False,) for form in ("x3", "h2") for s in FILTER_SHAPES]
    return out + [("x3", 768, 64, 512, True), ("h2", 768, 64, 512, True)]


def all_filter_cases():
    return [filter_case(*a) for a in filter_params()]


# ---- the rank count: plane operands ------------------------------------------------------------------------------------------
RANK_N = 600                      # catalogue rows: not a multiple of 256
RANK_NQ = 520                     # two row tiles + 8: the sweep (512 queries) and 8 constructed ones
RANK_CHUNKS = ((0, 512), (512, 256))     # (col0, n_cols): two column chunks, the counts accumulated
RANK_DUPS = [(50, [310, 590]), (254, [255, 256, 257]), (511, [512]), (20, [420, 421])]
RANK_LOW = (7, 130, 300, 515)     # rows with a very negative |b|^2: their raw distance to most queries is negative (clamped to 0)


def rank_case(form, D=64):
    """cdml_rank_tau_* / cdml_rank_count_* on independent planes: a catalogue of 600 rows; the launched buffer's rows 600 .. 767
    are finite planes with integer |b|^2 like the others (a NaN there would never be counted by a clamp that keeps NaN: only
    ``id < n_valid`` keeps them out, and ``d_pad`` holds their distances),
    |b|^2 integers around a row's score with itself (d(a, a) is small; two anchors get |b|^2 below their own score:
    d(a, duplicate of a) is negative and clamps to 0).  Query i < 512: anchor i, partner (i + 300) % 600 -- self and
    partner ids sweep all 256 column positions of a tile.  Queries 512 ..: a partner that is a duplicate of its anchor
    (tau = 0) with further duplicates below and above it, partners with duplicates below and above."""
    def make():
        rng = xg.case_rng("rank", form, D)
        n, nq, unit, scale = RANK_N, RANK_NQ, PLANE_UNIT[form], _scale(form)
        n_pad = 768
        Bk, plane_b, Bp, pairs = _plane_rows(n_pad, D, form, rng, RANK_DUPS)
        base = int(scale * D * 2 / 3)                        # ~ a row's score with itself, times the form's scale
        bs = rng.randint(base - 3, base + 8, size=n_pad).astype(np.float64)
        self_score = np.array([xg.expected([p[j:j + 1] for p in Bp], [p[j:j + 1] for p in Bp], pairs)[0, 0] for j in range(n_pad)])
        for j in (254, 20):                                 # anchors whose duplicates are at distance 0 (raw: negative)
            bs[j] = np.floor(scale * self_score[j]) - 1
        for j in RANK_LOW:
            bs[j] = -(base + 15.0)
        plant(bs, RANK_DUPS)
        a = np.concatenate([np.arange(512), [254, 256, 255, 20, 420, 10, 310, 590]]).astype(np.int64)
        p = np.concatenate([(np.arange(512) + 300) % n, [256, 254, 257, 421, 20, 310, 50, 310]]).astype(np.int64)
        assert len(a) == nq and (a != p).all()
        Ap = [x[a] for x in Bp]
        qs = bs[a]
        safe = assert_select_exact_safe(qs, bs[:n], unit, Ap, [x[:n] for x in Bp], pairs, scale)
        d_pad = plane_dist(Ap, Bp, pairs, qs, bs, unit, scale)     # (all 768 launched rows: what a wrong n_valid would count)
        d = d_pad[:, :n]
        tau, cnt = rank_int(d, a, p, n)
        return dict(name="rank %s D=%d" % (form, D), form=form, D=D, n=n, n_pad=n_pad, nq=nq, unit=unit, scale=scale, B=Bk,
                    plane_b=plane_b, Bp=Bp, pairs=pairs, b_sq=bs, a=a, p=p, Ap=Ap, q_sq=qs, d=d, d_pad=d_pad, tau=tau, count=cnt, safe=safe)
    return cached(("rank", form, D), make)


RANK_PARAMS = (("x3", 64), ("h2", 64), ("x3", 128), ("h2", 128))


def all_rank_cases():
    return [rank_case(*a) for a in RANK_PARAMS]


# ---- the miner: grid rows ----------------------------------------------------------------------------------------------------
MINER_SHAPES = ((128, 64), (384, 64))        # (B, D): one tile column of four strips | three tile columns, a last row tile of 128 anchors
MINER_VIDEOS = ("many", "twelve", "two")
MINER_H2_SCALE = 2.0 ** 4                    # the fp16 form's scale: |e| <= 4 -> 64, an fp16 integer


def miner_case(B, D, videos):
    """cdml_semihard_select / cdml_semihard_mine_x3 on integer grid rows E [2B][D] with video ids: "many" (5000 videos:
    nearly every row eligible), "twelve", "two" (videos 0 / 1 only: anchors whose pair spans both have NOTHING eligible --
    the only way to have none: every row's video is the anchor's or the positive's).  Planted: an eligible duplicate of a
    positive (d == d_p: not outside under the strict rule), an anchor (4, ..) whose positive is (-4, ..) (d_p is the largest
    distance there is: no outside candidate) with identical farthest rows in two strips, duplicate rows with different
    videos (ties for the closest outside candidate)."""
    def make():
        rng = xg.case_rng("miner", B, D, videos)
        R = 2 * B
        E = grid_rows(R, D, rng)
        nv = {"many": 5000, "twelve": 12, "two": 2}[videos]
        rows = rng.randint(0, nv, size=R).astype(np.int32)
        last = R - 1
        # anchor 3 (rows 6, 7): positive duplicated at rows 40 and R - 20 with another video
        plant(E, [(7, [40, R - 20])])
        # anchor 5 (rows 10, 11): the all-4 row against the all-(-4) row; rows 70 and R - 60 are all -4 too
        E[10], E[11], E[70], E[R - 60] = GRID, -GRID, -GRID, -GRID
        # duplicate rows: ties for the closest / farthest candidate wherever they are it
        plant(E, [(33, [34, 90, last]), (61, [66, 129 % R, R - 65]), (100, [101])])
        if videos == "two":
            rows[:8] = 0
            rows[6], rows[7], rows[10], rows[11] = 0, 0, 0, 0
            for t in (40, R - 20, 70, R - 60, 33, 34, 90, last):
                rows[t] = 1
        else:
            for t, v in ((6, 1), (7, 1), (40, 2), (R - 20, 3), (10, 4), (11, 4), (70, 5), (R - 60, 6)):
                rows[t] = v if videos == "twelve" else 4000 + v
        dist = grid_dist(E[0::2], E)
        unit = 1.0
        qs = (E * E).sum(1).astype(np.float64)
        safe = assert_select_exact_safe(qs[0::2], qs, unit, [E[0::2].astype(np.float64)], [E.astype(np.float64)], xg.PAIRS1)
        assert_h2_exact(E, MINER_H2_SCALE)
        # (the fp16 form's accumulator holds scale^2 <a, c>: the same bound in units of scale^2 / 2)
        neg = semihard_from_dist(dist, rows)
        return dict(name="miner B=%d D=%d %s videos" % (B, D, videos), B=B, D=D, videos=videos, E=E, rows=rows, dist=dist,
                    sqn=qs, dp=dist[np.arange(B), 2 * np.arange(B) + 1], neg=neg, unit=unit, safe=safe)
    return cached(("miner", B, D, videos), make)


def miner_classes(c):
    """per anchor, from the oracle alone: {"tied_closest", "eq_dp", "tied_farthest", "none"} -> bool [B]"""
    dist, rows, B = c["dist"], c["rows"], c["B"]
    d_p = c["dp"]
    elig = (rows[None, :] != rows[0::2, None]) & (rows[None, :] != rows[1::2, None])
    outside = elig & (dist > d_p[:, None])
    has_out = outside.any(1)
    dmin = np.where(outside, dist, INF_I).min(1)
    dmax = np.where(elig, dist, -INF_I).max(1)
    return {"tied_closest": has_out & ((outside & (dist == dmin[:, None])).sum(1) >= 2),
            "eq_dp": (elig & (dist == d_p[:, None])).any(1),
            "tied_farthest": ~has_out & elig.any(1) & ((elig & (dist == dmax[:, None])).sum(1) >= 2),
            "none": ~elig.any(1)}


MINER_PARAMS = tuple((B, D, v) for B, D in MINER_SHAPES for v in MINER_VIDEOS)


def all_miner_cases():
    return [miner_case(*a) for a in MINER_PARAMS]


# ---- the pipelines: grid rows through knn.knn_search and Evaluation.ranks ------------------------------------------------------
PIPE_UNIT = 0.25                  # grid rows k / 4, k in [-4, 4]: distances multiples of 1/16
KNN_N, KNN_NQ, KNN_D = 1100, 300, 64
KNN_KS = (51, 128)
KNN_FIRST = 256                   # b_block = first_block = 256: the filter path runs at this size
KNN_DUPS = [(17, [250, 255, 256, 257, 900]), (3, [4]), (600, [300, 1099]), (700, [40, 701, 1023, 1024])]


def knn_pipeline_case():
    """1100 grid rows, 300 separate queries (D = 64), duplicates below and above the ids they tie with and across the first
    block's end (256) and the tile boundaries; queries 0 .. 7 are catalogue rows themselves (d = 0)."""
    def make():
        rng = xg.case_rng("knnpipe", KNN_N, KNN_NQ, KNN_D)
        bi = plant(grid_rows(KNN_N, KNN_D, rng), KNN_DUPS)
        qi = grid_rows(KNN_NQ, KNN_D, rng)
        qi[:8] = bi[[17, 3, 600, 700, 1, 257, 1099, 512]]
        b, q = bi * PIPE_UNIT, qi * PIPE_UNIT
        unit = PIPE_UNIT ** 2
        safe = assert_select_exact_safe((q * q).sum(1), (b * b).sum(1), unit, [q], [b], xg.PAIRS1)
        for x in (b, q):                                      # precision "f16x2": the scale knn._planes_h2 picks keeps the grid exact
            assert_h2_exact(x, h2_scale_of(x))
        # (its accumulator holds sq sb <q, b>: the same integers times a power of two)
        return dict(name="knn pipeline", bi=bi, qi=qi, b=b.astype(np.float32), q=q.astype(np.float32), unit=unit, safe=safe,
                    d=grid_dist(qi, bi))
    return cached(("knnpipe",), make)


RANKP_N, RANKP_D = 600, 64
RANKP_DUPS = [(50, [310, 590]), (254, [255, 256, 257]), (511, [512]), (20, [420, 421]), (100, [99])]


def rank_pipeline_case():
    """600 grid rows through Evaluation.ranks: 300 random pairs plus pairs between duplicates (tau = 0), pairs whose
    partner has duplicates below and above its id, anchors with duplicates"""
    def make():
        rng = xg.case_rng("rankpipe", RANKP_N, RANKP_D)
        vi = plant(grid_rows(RANKP_N, RANKP_D, rng), RANKP_DUPS)
        a = rng.randint(0, RANKP_N, size=300)
        p = (a + 1 + rng.randint(0, RANKP_N - 1, size=300)) % RANKP_N
        cw = np.concatenate([np.stack([a, p], 1), [[254, 256], [255, 257], [20, 421], [10, 310], [310, 50], [590, 7], [99, 100], [511, 512]]])
        v = vi * PIPE_UNIT
        unit = PIPE_UNIT ** 2
        sq = (v * v).sum(1)
        safe = assert_select_exact_safe(sq, sq, unit, [v], [v], xg.PAIRS1)
        assert_h2_exact(v, h2_scale_of(v))
        return dict(name="rank pipeline", vi=vi, v=v.astype(np.float32), cw=cw.astype(np.int64), unit=unit, safe=safe, d=grid_dist(vi, vi))
    return cached(("rankpipe",), make)


def unit_rows(n, D, rng):
    """rows that are exactly unit on a dyadic grid: 4^j non-zeros of +-2^-j, j = 0 .. 3 (|x|^2 = 4^j 4^-j = 1)"""
    x = np.zeros((n, D), dtype=np.float64)
    for r in range(n):
        j = r % 4
        cols = rng.choice(D, size=4 ** j, replace=False)
        x[r, cols] = rng.choice([-1.0, 1.0], size=4 ** j) * 2.0 ** -j
    return x


UNIT_N, UNIT_NQ, UNIT_D, UNIT_K = 700, 100, 64, 51


def unit_rows_case():
    """the normalised pipeline: unit rows on the dyadic grid (l2norm_fwd must return them bit for bit); distances are
    multiples of 2^-6 (products of +-2^-i and +-2^-j, i, j <= 3)"""
    def make():
        rng = xg.case_rng("unitrows", UNIT_N, UNIT_D)
        b = unit_rows(UNIT_N, UNIT_D, rng)
        plant(b, [(9, [300, 301, 650]), (255, [256])])
        q = unit_rows(UNIT_NQ, UNIT_D, rng)
        q[:4] = b[[9, 255, 2, 699]]
        unit = 2.0 ** -5                                      # 2 <q, b>: multiples of 2 * 2^-6
        safe = assert_select_exact_safe((q * q).sum(1), (b * b).sum(1), unit, [q], [b], xg.PAIRS1)
        assert np.array_equal((b * b).sum(1), np.ones(UNIT_N)) and np.array_equal((q * q).sum(1), np.ones(UNIT_NQ))
        for x in (b, q):
            assert_h2_exact(x, h2_scale_of(x))
        s = q @ b.T
        d = to_units(2.0 - 2.0 * s, unit)
        return dict(name="unit rows", b=b.astype(np.float32), q=q.astype(np.float32), unit=unit, safe=safe, d=d)
    return cached(("unitrows",), make)


# ---- non-finite rows -----------------------------------------------------------------------------------------------------------
NONFINITE_NAN_ROWS = (3, 700)     # one NaN coordinate each: on both sides of the first block (256)
NONFINITE_INF_ROW = 512           # one +inf coordinate
NONFINITE_QUERY = 11              # a NaN query


def nonfinite_knn_case():
    """the kNN pipeline's catalogue with three non-finite rows and one NaN query.  Specified: a catalogue row with a
    non-finite coordinate is nobody's neighbour; a non-finite query gets I = -1, D = +inf throughout; every other result is
    the integer oracle's over the finite rows, original ids kept."""
    def make():
        c = knn_pipeline_case()
        b, q = c["b"].copy(), c["q"].copy()
        for r in NONFINITE_NAN_ROWS:
            b[r, 5] = np.nan
        b[NONFINITE_INF_ROW, 9] = np.inf
        q[NONFINITE_QUERY, 0] = np.nan
        bad = np.array(NONFINITE_NAN_ROWS + (NONFINITE_INF_ROW,))
        finite = np.setdiff1d(np.arange(KNN_N), bad)
        # precision "f16x2": with a NaN or inf in the tensor knn._planes_h2 falls back to scale 1 -- the grid is exact there too
        assert_h2_exact(c["b"], 1.0)
        assert_h2_exact(c["q"], 1.0)
        return dict(name="knn non-finite", b=b, q=q, finite=finite, bad=bad, d=c["d"], unit=c["unit"], safe=c["safe"])
    return cached(("knn-nonfinite",), make)


def nonfinite_want(c, k):
    """(D float32 tensor [nq][k], I int64 tensor): the oracle over the finite rows, ids kept; the NaN query empty"""
    D, I = knn_from_dist(c["d"][:, c["finite"]], c["finite"], k)
    D[NONFINITE_QUERY], I[NONFINITE_QUERY] = INF_I, -1
    return from_units(D, c["unit"]), torch.from_numpy(I)


def nonfinite_rank_case():
    """the rank pipeline's catalogue with rows 3 and 420 NaN and row 512 +inf (420 and 512 are duplicates of partners /
    anchors of the finite case: they must stop counting); no pair touches a non-finite row"""
    def make():
        c = rank_pipeline_case()
        v = c["v"].copy()
        bad = np.array([3, 420, 512])
        v[3, 5] = np.nan
        v[420, 60] = np.nan
        v[512, 9] = np.inf
        cw = c["cw"][~np.isin(c["cw"], bad).any(1)]
        assert_h2_exact(c["v"], 1.0)                          # (the scale knn._planes_h2 falls back to with a NaN in the tensor)
        return dict(name="rank non-finite", v=v, cw=cw, bad=bad, d=c["d"], unit=c["unit"], safe=c["safe"])
    return cached(("rank-nonfinite",), make)


def pipeline_ranks_want(d, queries, bad=()):
    """rank_int for the (anchor, partner) rows Evaluation.ranks returned; rows ``bad`` never counted"""
    a, p = queries[:, 0], queries[:, 1]
    dq = np.asarray(d)[a].copy()
    n = dq.shape[1]
    if len(bad):
        dq[:, np.asarray(bad)] = INF_I                       # behind every partner
    return rank_int(dq, a, p, n)[1]


# ---- knn_search's filter path, from the oracle ---------------------------------------------------------------------------------
def filter_plan(d, k, first_cols, c_chunk, bad=()):
    """(list_cap, largest per-query candidate count of any filter launch) of knn.knn_search on a catalogue with distance
    matrix ``d`` [nq][nb]: the first ``first_cols`` rows give every query its k-th best distance tau, the rest goes through
    filter launches of ``c_chunk`` rows, tau tightened after each; the lists have 64 * 2^j >= 4 k min(nb - first_cols,
    c_chunk) / first_cols slots (knn.py).  ``bad``: rows that never pass (non-finite).  A count above list_cap would send the
    search back through score blocks -- the exact tests would pass without running the filter."""
    d = np.maximum(np.asarray(d, np.int64), 0).copy()
    nb = d.shape[1]
    if len(bad):
        d[:, np.asarray(bad)] = INF_I
    cap, expect = 64, k * min(nb - first_cols, c_chunk) / float(first_cols)
    while cap < 4 * expect:
        cap *= 2
    worst = 0
    for c0 in range(first_cols, nb, c_chunk):
        tau = np.sort(d[:, :c0], axis=1)[:, k - 1:k]
        blk = d[:, c0:c0 + c_chunk]
        worst = max(worst, int(((blk <= tau) & (blk != INF_I)).sum(1).max()))
    return cap, worst


def with_zero_row(d, vi):
    """``d`` [n][n] of grid rows ``vi`` with one more column: the distance to the all-zero padding row Evaluation.ranks
    appends (|a|^2) -- what n_valid + 1 would count"""
    return np.concatenate([d, (np.asarray(vi, np.int64) ** 2).sum(1)[:, None]], axis=1)
