"""Exact-arithmetic operands and models for the triplet tail of csrc/loss.hip: k_l2norm_fwd / k_l2norm_bwd,
k_triplet_hinge / k_triplet_hinge_inbatch, k_vnet_tail<MODE, NCH> with its bf16, three-plane and fp16-plane copies,
k_hinge_indexed_fwd / k_hinge_indexed_bwd<NCH>, k_loss_stats, k_tail_var_final and the elementwise kernels k_lrelu_bwd,
k_ew_fusion_bwd, k_ew_combine, k_pair_dist.

That code is mostly RULES -- the hinge's corner (gradient at t >= 0, hinge and active count at t > 0), lrelu' at +-0, the
norm clamp and the projection term it drops, the in-batch validity masks and the (j, k) slot arithmetic, the indexed
backward's key words -- and a band around Gaussian data hides every one of them.  The operands here put all of it on
dyadic grids:

* rows: ``unit_rows`` (4^j non-zeros of +-2^-j, |x|^2 = 1; 4^j <= D) times 2^s, s in [-3, 3]: |z|^2 = 4^s, the normalised
  row IS the unit row, distances are multiples of a granule G >= 2^-5 (measured per pool), 2 / B is dyadic for B a power of two, and <z, g>,
  c = inv^2 <z, g>, g - z c and dz are short dyadic numbers; two thirds of the coordinates are exactly 0 and a share of
  them -0.0, so lrelu' meets its boundary in nearly every row;
* ``assert_tail_exact_safe``: when zero tolerance is legitimate, computed per case and stored under "safe";
* triplets planted by search in a pool of such rows: t = pos - neg + margin exactly 0, exactly +-1 granule, clearly
  inactive, clearly active; clamped rows (all-zero: ss = 0) in ACTIVE triplets in every role; in-batch id collisions;
  mined rows of every kind for the indexed form (``classes``, asserted by the builders);
* tiny rows (one coordinate 2^-21: ss = 2^-42 below the clamp) beside control rows (2^-19: not clamped): the only rows that
  show whether the projection term is dropped.  Their normalised coordinate is not dyadic, so what it touches through a
  reduction is compared within the standard forward bound ``reduction_bound``; everything elementwise stays bit for bit;
* one numpy model (``tail_model``) for every entry point, float64 on exact values with a rounding to fp32 after every
  elementwise step (a no-op on exact cases, the single rounding of the kernels' operation elsewhere); every rule has a
  switch in ``RULES`` that turns it into one mutation.

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402

EPS = np.float32(1e-12)                                      # kL2Eps (csrc/loss.hip), tf.nn.l2_normalize's epsilon
EPS64 = float(EPS)
INV_C_MODEL = np.float32(1.0 / np.sqrt(np.float64(EPS)))    # 1 / sqrt(1e-12f): one correctly rounded sqrt and one division -> 1 ulp
ALPHA_DYADIC = 0.25                                          # a power of two: every result stays dyadic
ALPHA_REF = 0.2                                              # ops.LRELU_ALPHA: one correctly rounded multiply of an exact operand
ALPHAS = (-1.0, ALPHA_DYADIC, ALPHA_REF)                     # -1: lrelu' off
U = 2.0 ** -24                                               # fp32 unit roundoff
MARGIN = 0.5
TINY, CONTROL = 2.0 ** -21, 2.0 ** -19                       # ss = 2^-42 < 1e-12 < 2^-38
H2_SCALE = 2.0 ** 10                                         # the fp16 planes' scale in the tail cases
cached = xs.cached

# every rule of the tail as one mutation (the host test: each is seen by a committed case of every entry point it concerns)
RULES = ("grad_gt",             # hinge gradient: t > 0 instead of t >= 0
         "count_ge",            # hinge_o / stats[3]: t >= 0 counted as active instead of hinge > 0
         "invalid_reports",     # an invalid triplet still reports max(t, 0)
         "lrelu_ge",            # lrelu': z >= 0 -> 1 instead of z > 0
         "clamp_keeps_proj",    # the clamped branch keeps c = inv^2 <z, g>
         "valid_i_no_va",       # valid_i without vn != va
         "valid_i_no_vp",       # valid_i without vn != vp
         "valid_k_from_j",      # valid_k from the ids of slot j
         "swap_jk",             # j and k exchanged
         "one_over_b",          # 1 / B for 2 / B
         "inactive_key_hit",    # an inactive triplet's mined row counted as a hit
         "hit_row_xor1",        # a hit credited to row r ^ 1
         "neg_minus1_row0",     # neg_row = -1 read as row 0
         "drop_neg_row")        # the negative's own row term dropped (mode 0)
RULES_OF = {"l2norm_bwd": ("lrelu_ge", "clamp_keeps_proj"),
            "hinge": ("grad_gt", "count_ge", "one_over_b", "drop_neg_row"),
            "inbatch": ("grad_gt", "count_ge", "invalid_reports", "valid_i_no_va", "valid_i_no_vp", "valid_k_from_j", "swap_jk", "one_over_b"),
            "indexed": ("grad_gt", "count_ge", "invalid_reports", "one_over_b", "inactive_key_hit", "hit_row_xor1", "neg_minus1_row0")}
RULES_OF["tail0"] = RULES_OF["hinge"] + RULES_OF["l2norm_bwd"]
RULES_OF["tail1"] = RULES_OF["inbatch"] + RULES_OF["l2norm_bwd"]
RULES_OF["indexed_tail"] = RULES_OF["indexed"] + RULES_OF["l2norm_bwd"]


def r32(x):
    """float64 -> nearest fp32 number, as float64: the rounding of one fp32 operation on fp32 operands (a product or a
    short sum of two fp32 numbers is exact in float64, so this is ONE rounding); a no-op on exact values"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def is_f32(x):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(r32(x), x))


def reduction_bound(terms, axis=-1):
    """The standard forward bound of a recursive fp32 sum of n rounded terms in any order: |computed - exact| <=
    (n_terms + 2) 2^-24 sum |terms| (n - 1 additions, two roundings inside a term; first order, the higher orders are
    below 2^-24 of it for n <= 2^14).  ``terms``: the exact terms along ``axis``."""
    t = np.abs(np.asarray(terms, np.float64))
    return (t.shape[axis] + 2) * U * t.sum(axis)


# ---- rows -----------------------------------------------------------------------------------------------------------------
def jmax_of(D):
    j = 0
    while j < 3 and 4 ** (j + 1) <= D:
        j += 1
    return j


def unit_rows(n, D, rng):
    """exact_select.unit_rows; for D < 64 with j limited so that 4^j <= D"""
    if D >= 64:
        return xs.unit_rows(n, D, rng)
    jm = jmax_of(D)
    x = np.zeros((n, D), dtype=np.float64)
    for r in range(n):
        j = r % (jm + 1)
        cols = rng.choice(D, size=4 ** j, replace=False)
        x[r, cols] = rng.choice([-1.0, 1.0], size=4 ** j) * 2.0 ** -j
    return x


def scale_rows(u, rng, s=None, neg_zero=0.3):
    """z = u 2^s per row (s in [-3, 3] unless given), a share of the exact zeros flipped to -0.0"""
    u = np.asarray(u, np.float64)
    s = rng.randint(-3, 4, size=len(u)) if s is None else np.broadcast_to(np.asarray(s), (len(u),))
    z = u * 2.0 ** s[:, None].astype(np.float64)
    z[(z == 0) & (rng.rand(*z.shape) < neg_zero)] = -0.0
    return z, np.asarray(s)


def sqdist(a, b):
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def dyadic(shape, rng, step=2.0 ** -4, span=16, zeros=0.3):
    """multiples of ``step`` in [-span step, span step]; a share exactly 0.0 / -0.0"""
    v = rng.randint(-span, span + 1, size=shape).astype(np.float64) * step
    zero = rng.rand(*shape) < zeros
    v[zero] = np.where(rng.rand(*shape) < 0.5, 0.0, -0.0)[zero]
    return v


# ---- the model -----------------------------------------------------------------------------------------------------------------
def normalize(z, inv_c=None):
    """(e, inv, ss, clamped): inv = 1 / sqrt(max(ss, 1e-12f)); a clamped row (ss <= 1e-12f) gets ``inv_c``"""
    inv_c = float(INV_C_MODEL if inv_c is None else inv_c)
    z = np.asarray(z, np.float64)
    ss = (z * z).sum(1)
    clamped = ss <= EPS64
    inv = np.where(clamped, inv_c, 1.0 / np.sqrt(np.where(clamped, 1.0, ss)))
    return r32(z * inv[:, None]), inv, ss, clamped


def lrelu_factor(z, alpha, rule=()):
    """lrelu'(z) as the kernels apply it: z > 0 ? 1 : alpha (0.0 and -0.0 take alpha); alpha < 0: off"""
    if alpha < 0:
        return np.ones_like(np.asarray(z, np.float64))
    on = (z >= 0) if "lrelu_ge" in rule else (z > 0)
    return np.where(on, 1.0, float(np.float32(alpha)))


def l2norm_bwd_model(z, g, alpha=-1.0, rule=(), inv_c=None, g_tol=None):
    """k_l2norm_bwd / tail_store_row / the indexed backward's tail: dz = inv (g - z c) lrelu'(z), c = inv^2 <z, g> where
    ss > 1e-12f, else 0.  Returns (dz, tol): tol = 0 where every step is exact; where ``g_tol`` (the bound of an inexact
    g) is given, or a row carries a non-dyadic value, the propagated forward bound (see the body)."""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    _, inv, ss, clamped = normalize(z, inv_c)
    terms = z * g
    zg = terms.sum(1)
    keep = ~clamped | ("clamp_keeps_proj" in rule)
    c = np.where(keep, inv * inv * zg, 0.0)
    lr = lrelu_factor(z, alpha, rule)
    d = r32(inv[:, None] * r32(g - r32(z * c[:, None])))
    d = r32(d * lr)
    # the bound: zg off by sum |z| g_tol + reduction_bound; c by inv^2 of that + two roundings; dz by inv lr (g_tol +
    # |z| c_err + four roundings of |g| + |z c|)
    gt = np.zeros_like(g) if g_tol is None else np.asarray(g_tol, np.float64)
    zg_err = (np.abs(z) * gt).sum(1) + reduction_bound(terms)
    c_err = np.where(keep, inv * inv * zg_err + 2 * U * np.abs(c), 0.0)
    tol = inv[:, None] * lr * (gt + np.abs(z) * c_err[:, None] + 4 * U * (np.abs(g) + np.abs(z * c[:, None])))
    return d, tol


def _triplets(c, rule):
    """(tri [B][3], valid [B], extra) of a case under ``rule``"""
    B, kind = c["B"], c["kind"]
    i = np.arange(B)
    if kind == "m0":
        return np.arange(3 * B).reshape(B, 3), np.ones(B, bool), None
    if kind == "m1":
        ids, sh = c["ids"].astype(np.int64), int(c["shift"])
        j, k = (i + sh) % B, (i - sh % B + B) % B
        if "swap_jk" in rule:
            j, k = k, j
        va, vp, vn = ids[2 * i], ids[2 * i + 1], ids[2 * j + 1]
        valid = ((vn != va) | ("valid_i_no_va" in rule)) & ((vn != vp) | ("valid_i_no_vp" in rule))
        kk = j if "valid_k_from_j" in rule else k
        valid_k = (vp != ids[2 * kk]) & (vp != ids[2 * kk + 1])
        return np.stack([2 * i, 2 * i + 1, 2 * j + 1], 1), valid, (k, valid_k)
    nr = c["neg_row"].astype(np.int64)
    if "neg_minus1_row0" in rule:
        nr = np.where(nr < 0, 0, nr)
    valid = nr >= 0
    return np.stack([2 * i, 2 * i + 1, np.where(valid, nr, 2 * i)], 1), valid, nr


def tail_model(c, alpha=-1.0, rule=(), inv_c=None, tail=True):
    """Every output of the tail entry points on case ``c`` (kinds "m0": rows 3i, 3i+1, 3i+2; "m1": in-batch negatives;
    "idx": indexed) under the mutations ``rule``.  e, inv, pos, neg, hinge, valid, key (indexed), de, dz2 (``tail``), stats
    [4] (float32), var (float64), and the bounds pos_tol / de_tol / dz2_tol (all zero on an exact case)."""
    rule = frozenset(rule)
    assert rule <= set(RULES), rule - set(RULES)
    B, kind, margin = c["B"], c["kind"], float(c["margin"])
    z = c["z"]
    e, inv, ss, clamped = normalize(z, inv_c)
    tri, valid, extra = _triplets(c, rule)
    a, p, n = e[tri[:, 0]], e[tri[:, 1]], e[tri[:, 2]]
    tp, tn = r32(a - p) ** 2, r32(a - n) ** 2
    pos, neg = tp.sum(1), tn.sum(1)
    t = pos - neg + margin
    on = (t > 0) if "grad_gt" in rule else (t >= 0)
    hinge = np.where(valid | ("invalid_reports" in rule), np.maximum(t, 0.0), 0.0)
    tb = float(np.float32(1.0 if "one_over_b" in rule else 2.0) / np.float32(B))
    s = (valid & on) * tb
    de = np.zeros_like(e)
    de_abs = np.zeros_like(e)
    n_terms = np.zeros(len(e))
    key = None
    if kind == "m0":
        de[tri[:, 0]] = r32(r32(n - p) * s[:, None])
        de[tri[:, 1]] = r32(r32(p - a) * s[:, None])
        if "drop_neg_row" not in rule:
            de[tri[:, 2]] = r32(r32(a - n) * s[:, None])
    elif kind == "m1":
        k, valid_k = extra
        ak, pk = e[2 * k], e[2 * k + 1]
        tk = (r32(ak - pk) ** 2).sum(1) - (r32(ak - p) ** 2).sum(1) + margin
        sk = (valid_k & ((tk > 0) if "grad_gt" in rule else (tk >= 0))) * tb
        de[tri[:, 0]] = r32(r32(n - p) * s[:, None])
        g1, g2 = r32(r32(p - a) * s[:, None]), r32(r32(ak - p) * sk[:, None])
        de[tri[:, 1]] = r32(g1 + g2)
        de_abs[tri[:, 1]] = np.abs(g1) + np.abs(g2)
        n_terms[tri[:, 1]] = 2
    else:
        nr = extra
        key = np.where(valid & on, nr, -1)
        hit = np.where(valid, nr, -1) if "inactive_key_hit" in rule else key
        de[tri[:, 0]] = r32(r32(n - p) * s[:, None])
        de[tri[:, 1]] = r32(r32(p - a) * s[:, None])
        de_abs[:] = np.abs(de)
        n_terms[:] = 1
        jj = np.nonzero(hit >= 0)[0]                          # ascending triplet order (sums of exact terms: any order)
        tgt = hit[jj]
        term = r32(r32(e[2 * jj] - e[tgt]) * tb)
        if "hit_row_xor1" in rule:
            tgt = tgt ^ 1
        np.add.at(de, tgt, term)
        np.add.at(de_abs, tgt, np.abs(term))
        np.add.at(n_terms, tgt, 1)
    # the bounds.  "npow2": 2 / B is rounded -- a gradient element that sums terms carries (n_terms + 2) 2^-24 sum |terms|.
    # "tiny": only what a tiny row's non-dyadic normalised coordinate enters -- pos / neg of its triplets, the sums of
    # the rows of those triplets (mode 0 sums nothing: its terms are elementwise and stay bit for bit, the tiny row's own
    # dz2 included); every other row of the case stays exact.
    inexact = c.get("inexact")
    dirty_t = c["tiny_rows"][tri].any(1) if inexact == "tiny" else np.zeros(B, bool)
    dirty = np.isin(np.arange(len(e)), tri[dirty_t].ravel())
    de_tol = np.zeros_like(de)
    if inexact == "npow2":
        de_tol = (n_terms[:, None] + 2) * U * de_abs
    elif inexact == "tiny" and kind != "m0":
        de_tol = (n_terms[:, None] + 2) * U * de_abs * dirty[:, None]
    pos_tol = np.maximum(reduction_bound(tp), reduction_bound(tn)) * dirty_t
    out = dict(e=e, inv=inv, ss=ss, clamped=clamped, tri=tri, pos=pos, neg=neg, t=t, hinge=hinge, valid=valid, key=key, de=de,
               de_tol=de_tol, pos_tol=pos_tol, scale=s, on=on, dirty=dirty, dirty_t=dirty_t)
    if kind == "m1":
        out["scale_k"] = sk
    if tail:
        out["dz2"], tol = l2norm_bwd_model(z, de, alpha, rule, inv_c, g_tol=de_tol)
        if inexact == "tiny":
            tol = tol * (dirty & ~(c["tiny_rows"] if kind == "m0" else np.zeros(len(e), bool)))[:, None]
        out["dz2_tol"] = tol if inexact else np.zeros_like(tol)
    active = (valid & (t >= 0)) if "count_ge" in rule else (hinge > 0)
    f = np.float32
    out["stats"] = np.array([f(hinge.sum()) / f(B), f(pos.sum()) / f(B), f(neg.sum()) / f(B), f(active.sum()) / f(B)], dtype=f)
    T = e[tri]                                                # calc_var (train.py:67-71) of the [B][3][D] triplet tensor
    out["var"] = float(np.mean(np.square(T - np.mean(T, axis=(0, 1)))))
    return out


def model_outputs(m, names=("pos", "neg", "hinge", "valid", "key", "de", "dz2", "stats")):
    return [np.asarray(m[k], np.float64) for k in names if m.get(k) is not None]


def differs(m0, m1):
    """a mutation is SEEN: some output differs by more than the two bounds together"""
    for k in ("pos", "neg", "hinge", "valid", "key", "stats"):
        if m0.get(k) is not None and not np.array_equal(np.asarray(m0[k]), np.asarray(m1[k])):
            return True
    for k, tk in (("de", "de_tol"), ("dz2", "dz2_tol")):
        if k in m0 and bool((np.abs(m0[k] - m1[k]) > m0[tk] + m1[tk]).any()):
            return True
    return False


# ---- the safety condition ---------------------------------------------------------------------------------------------------
def _reduction_units(terms, what):
    """sum |terms| of each reduction (last axis) in granules: every term a multiple of one power of two, the sums < 2^24"""
    terms = np.asarray(terms, np.float64)
    terms = terms.reshape(-1, terms.shape[-1])
    if terms.size == 0:
        return 0.0
    m, ex = np.frexp(np.abs(terms))                           # |x| = m 2^ex, m 2^53 an integer (exact_gemm._granule_exp, per reduction)
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2(np.maximum(mi & -mi, 1).astype(np.float64))
    g = np.where(terms != 0, ex - 53 + tz, np.inf).min(-1)    # the granule of each reduction: the largest 2^g dividing its terms
    units = np.where(np.isfinite(g), np.abs(terms).sum(-1) / 2.0 ** np.where(np.isfinite(g), g, 0.0), 0.0)
    worst = float(units.max())
    assert worst < 2.0 ** 24, "%s: the absolute sums reach %g granules: not below 2^24" % (what, worst)
    return worst


def assert_tail_exact_safe(c):
    """Zero tolerance is legitimate on case ``c``: every term of every reduction -- ss, pos, neg, <z, g>, the variance's
    column sums, the sums over the triplets that mined a row -- is an integer multiple of a power-of-two granule and the
    sum of the absolute values of the terms of each reduction stays below 2^24 granules, so any lane order, shuffle tree
    or fma contraction gives the same bits; and every elementwise intermediate (e, the gradient terms, z c, g - z c, dz
    before lrelu') is an fp32 number.  Exempt, and compared otherwise: the clamped rows' products with 1 / sqrt(1e-12f)
    (elementwise, modelled step by step in fp32); on an "npow2" case (2 / B rounded) everything behind the gradient terms;
    on a "tiny" case the reductions that a tiny row's normalised coordinate enters.  Returns the largest reduction in
    granules."""
    z = np.asarray(c["z"], np.float64)
    assert is_f32(z), "an operand is no fp32 number"
    worst = _reduction_units(z * z, "ss")
    if c["kind"] == "rows":                                   # l2norm_fwd / l2norm_bwd: z and a given g
        g = np.asarray(c["g"], np.float64)
        assert is_f32(g)
        ok = ~c["tiny_rows"]
        worst = max(worst, _reduction_units((z * g)[ok], "<z, g>"))
        e, inv, ss, clamped = normalize(z)
        cc = np.where(clamped, 0.0, inv * inv * (z * g).sum(1))
        assert is_f32(e[ok]) and is_f32(cc) and is_f32(z * cc[:, None]) and is_f32(g - z * cc[:, None])
        assert is_f32((inv[:, None] * (g - z * cc[:, None]))[~clamped])
        return max(worst, 1.0)
    inexact = c.get("inexact")
    m = tail_model(c, tail=False)
    e, tri = m["e"], m["tri"]
    a, p, n = e[tri[:, 0]], e[tri[:, 1]], e[tri[:, 2]]
    clean = np.ones(c["B"], bool)
    rows_ok = np.ones(len(z), bool)
    if inexact == "tiny":                                     # a triplet / row that a tiny row's coordinate enters
        tiny = c["tiny_rows"]
        clean = ~tiny[tri].any(1)
        rows_ok = ~np.isin(np.arange(len(z)), tri[~clean].ravel())
    assert is_f32(e[rows_ok])
    worst = max(worst, _reduction_units(((a - p) ** 2)[clean], "pos"), _reduction_units(((a - n) ** 2)[clean], "neg"))
    if c["kind"] in ("m0", "m1") and not inexact:
        worst = max(worst, _reduction_units(np.moveaxis(e[tri], 2, 0).reshape(e.shape[1], -1), "column sums"))
    if inexact == "npow2":
        return worst
    g = m["de"]
    assert is_f32(g[rows_ok]), "a gradient term is no fp32 number"
    if c["kind"] == "idx":                                    # the hub sums: the terms of every row, own term and hits
        key = m["key"]
        jj = np.nonzero((key >= 0) & clean)[0]
        own = np.zeros_like(e)
        own[tri[:, 0]] = (n - p) * m["scale"][:, None]
        own[tri[:, 1]] = (p - a) * m["scale"][:, None]
        own[~rows_ok] = 0.0
        term = (e[2 * jj] - e[key[jj]]) * (2.0 / c["B"])
        gx = min(xg._granule_exp(term), xg._granule_exp(own))
        if gx != np.inf:
            tot = np.abs(own)
            np.add.at(tot, key[jj], np.abs(term))
            w = float(tot[rows_ok].max()) / 2.0 ** gx
            assert w < 2.0 ** 24, "the sums over a row's hits reach %g granules of 2^%d" % (w, gx)
            worst = max(worst, w)
    worst = max(worst, _reduction_units((z * g)[rows_ok], "<z, g>"))
    inv, clamped = m["inv"], m["clamped"]
    cc = np.where(clamped, 0.0, inv * inv * (z * g).sum(1))
    ok = rows_ok & ~clamped
    for v, what in ((cc[ok], "c"), ((z * cc[:, None])[ok], "z c"), ((g - z * cc[:, None])[ok], "g - z c"),
                    ((inv[:, None] * (g - z * cc[:, None]))[ok], "dz")):
        assert is_f32(v), "%s is no fp32 number" % what
    return worst


# ---- planting triplets by search ------------------------------------------------------------------------------------------------
T_CLASSES = {"corner": lambda t, G: t == 0, "plus": lambda t, G: t == G, "minus": lambda t, G: t == -G,
             "active": lambda t, G: t >= 0.125, "inactive": lambda t, G: t <= -0.125, "any": lambda t, G: np.abs(t) >= 0}


def _pool(D, rng, n=96):
    """(pool rows [n + 1][D], dist, G, margin): unit rows and, last, the all-zero row (a clamped row normalises to exactly
    0); their squared distances (exact in float64); the granule G of those distances -- the largest power of two that
    divides them all (2 - 2 <a, p> with <a, p> a multiple of 4^-jmax, coarser where parity helps: integers at D = 4) --
    and a margin ON that grid, max(1/2, G), so that t = pos - neg + margin can be exactly 0 and exactly +-G"""
    if D > 128:                                               # wide rows: the non-zeros live in ~130 "hot" columns spread over the whole
        edge = [q for q in (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 767, 768, D - 2, D - 1) if q < D]      # width, the
        hot = np.unique(np.concatenate([rng.choice(D, 120, replace=False), edge]))          # chunk boundaries among them:
        u = np.zeros((n + 1, D))                              # two drawn rows still overlap, so their distances still
        u[:n, hot] = unit_rows(n, len(hot), rng)              # spread over the grid (at D = 1024 nearly all would be 2)
    else:
        u = np.concatenate([unit_rows(n, D, rng), np.zeros((1, D))])
    sq = (u * u).sum(1)
    dist = sq[:, None] + sq[None, :] - 2.0 * (u @ u.T)
    G = 2.0 ** xg._granule_exp(dist)
    assert 2.0 ** -6 <= G <= 1.0
    return u, dist, G, max(MARGIN, G)


def _search(dist, rng, pred, G, margin, a=None, p=None, n=None, n_real=None, tries=4000):
    """pool indices (a, p, n) with pred(dist[a, p] - dist[a, n] + margin); given entries stay, the others are drawn from
    the first ``n_real`` rows"""
    n_real = dist.shape[0] - 1 if n_real is None else n_real
    if a is None and p is not None and n is not None:         # only the anchor is free: all of them at once
        ok = np.nonzero(pred(dist[:n_real, p] - dist[:n_real, n] + margin, G))[0]
        assert len(ok), "no anchor of the wanted class in the pool"
        return int(ok[rng.randint(len(ok))]), p, n
    for _ in range(tries):
        ai = rng.randint(n_real) if a is None else a
        if p is not None and n is not None:
            if pred(dist[ai, p] - dist[ai, n] + margin, G):
                return ai, p, n
            break
        if n is not None:                                     # the positive is free
            ok = np.nonzero(pred(dist[ai, :n_real] - dist[ai, n] + margin, G))[0]
            if len(ok):
                return ai, int(ok[rng.randint(len(ok))]), n
        else:                                                 # the negative is free (the positive drawn, unless given)
            pi = rng.randint(n_real) if p is None else p
            ok = np.nonzero(pred(dist[ai, pi] - dist[ai, :n_real] + margin, G))[0]
            if len(ok):
                return ai, pi, int(ok[rng.randint(len(ok))])
        if a is not None and (p is not None or n is not None):
            break                                             # (nothing left to draw)
    raise AssertionError("no triplet of the wanted class in the pool")


def _plant_tiny(c, candidates, col, value=TINY):
    """Replace the first row of ``candidates`` that qualifies by zeros with ``value`` at ``col`` (TINY: below the clamp, the
    case becomes "tiny"; +-CONTROL: above it, exact) and return it.  Qualifies: every triplet the row is in stays at
    |t| >= 1/8 for the device's 1 / sqrt(1e-12f) one ulp either side of the model's, and the row's own dz2 shows whether
    the projection term is kept (an active triplet gives it a gradient with <z, g> != 0)."""
    R = len(c["z"])
    tiny_rows = c.setdefault("tiny_rows", np.zeros(R, bool))
    was = c.get("inexact")
    for r in candidates:
        old = c["z"][r].copy()
        c["z"][r] = 0.0
        c["z"][r, col] = value
        if abs(value) == TINY:
            tiny_rows[r] = True
            c["inexact"] = "tiny"
        ok = True
        for inv_c in (np.nextafter(INV_C_MODEL, np.float32(0)), np.nextafter(INV_C_MODEL, np.float32(1e9))):
            m = tail_model(c, inv_c=inv_c, tail=False)
            touched = (m["tri"] == r).any(1)
            ok = ok and bool((np.abs(m["t"][touched]) >= 0.125).all())
        if ok:
            m0 = tail_model(c, ALPHA_DYADIC)
            m1 = tail_model(c, ALPHA_DYADIC, rule=("clamp_keeps_proj",)) if abs(value) == TINY else None
            ok = bool((m0["dz2"][r] != 0).any()) and (m1 is None or
                                                       bool((np.abs(m0["dz2"][r] - m1["dz2"][r]) > m0["dz2_tol"][r] + m1["dz2_tol"][r]).any()))
        if ok:
            return r
        c["z"][r] = old
        tiny_rows[r] = False
        c["inexact"] = was
    raise AssertionError("%s: no row qualifies for a tiny / control row" % c["name"])


M0_PLAN = ("corner", "zero_a", "plus", "minus", "corner", "zero_p", "zero_n", "inactive", "corner", "active", "corner", "plus", "minus")


def hinge_case(B, D, tiny=False):
    """Mode 0 (rows 3i, 3i + 1, 3i + 2): the triplets of M0_PLAN as far as B reaches -- t exactly 0, +-1 granule, clearly
    inactive / active, an all-zero row as anchor, positive and negative of an ACTIVE triplet -- the rest drawn.  ``tiny``:
    three more rows replaced by a tiny row (one coordinate 2^-21) in each role of a triplet with |t| >= 1/8 and three by
    control rows (2^-19) in the same roles of other triplets: an "inexact" case (B >= 16)."""
    def make(attempt):
        rng = xg.case_rng("tail-m0", B, D, int(tiny), attempt)
        pool, dist, G, margin = _pool(D, rng)
        Z = len(pool) - 1
        idx = np.zeros((B, 3), dtype=np.int64)
        plan = [M0_PLAN[i] if i < len(M0_PLAN) else "any" for i in range(B)]
        if B == 1:
            plan = ["corner"]
        for i, want in enumerate(plan):
            for _ in range(64):                              # (three different vectors: no term of the triplet is 0)
                if want.startswith("zero_"):
                    role = {"zero_a": "a", "zero_p": "p", "zero_n": "n"}[want]
                    idx[i] = _search(dist, rng, T_CLASSES["active"], G, margin, **{role: Z})
                else:
                    idx[i] = _search(dist, rng, T_CLASSES[want], G, margin)
                if dist[idx[i, 0], idx[i, 1]] > 0 and dist[idx[i, 0], idx[i, 2]] > 0 and dist[idx[i, 1], idx[i, 2]] > 0:
                    break
            else:
                raise AssertionError("only degenerate triplets of class %s" % want)
        z, s = scale_rows(pool[idx.ravel()], rng)
        c = dict(name="tail m0 B=%d D=%d%s" % (B, D, " tiny" if tiny else ""), kind="m0", B=B, D=D, margin=margin, G=G, z=z, s=s,
                 plan=plan, inexact=None if (B & (B - 1)) == 0 else "npow2")
        if tiny:
            assert B >= 16 and D >= 64
            used = []
            for value in (TINY, -CONTROL):                   # a tiny row, then a control row, as anchor, positive and negative
                for r in range(3):                           # of six triplets
                    row = _plant_tiny(c, [3 * i + r for i in range(len(M0_PLAN), B) if i not in used], 5 + r, value)
                    used.append(row // 3)
        c["safe"] = assert_tail_exact_safe(c)
        c["classes"] = classes(c)
        need = {"corner": 4, "plus": 2, "minus": 2, "inactive": 1, "active": 1, "zero_a": 1, "zero_p": 1, "zero_n": 1} if B >= 16 else \
               {"corner": 1} if B < 8 else {"corner": 2, "plus": 1, "minus": 1, "zero_a": 1, "zero_p": 1, "zero_n": 1, "inactive": 1}
        for k, v in need.items():
            assert len(c["classes"][k]) >= v, "%s: %d triplets of class %s, %d wanted" % (c["name"], len(c["classes"][k]), k, v)
        if c["inexact"] == "npow2":
            _assert_npow2_margin(c)
        return c
    return cached(("tail-m0", B, D, tiny), lambda: _attempts(make))


POOL_BIG = 1024                                              # rows to search in where a rare class (t = +-G) needs them
# (the rare classes first: their slots still have a free positive or negative whatever the shift)
# (at shift = B / 2, j == k: an "inv_vp" slot makes its partner i + B / 2 invalid too -- the partner is the spare "active")
M1_PLAN = {2: ("inv_va", "corner"), 4: ("minus", "corner", "inv_va", "active")}
M1_PLAN_8 = ("plus", "minus", "active", "inv_va", "corner", "inactive", "inv_vp", "corner")


def _attempts(build, tries=24):
    """``build(attempt)`` until one attempt's draw carries every class its builder asserts (a draw that lacks one is
    discarded whole: nothing is patched up afterwards)"""
    err = None
    for attempt in range(tries):
        try:
            return build(attempt)
        except AssertionError as e:
            err = e
    raise AssertionError("no draw out of %d carries every class: %s" % (tries, err))


def inbatch_case(B, D, shift, tiny=False):
    """Mode 1: slot i owns rows 2i (a_i), 2i + 1 (p_i); its negative is p_j, j = (i + shift) % B, and p_i is the negative
    of slot k = (i - shift) % B.  The positives are drawn; the anchors of the planned slots are searched so that t_i is
    exactly 0 / +-1 granule / clearly on one side.  ids are distinct except: slot "inv_va" has id(a_i) = id(p_j) and slot
    "inv_vp" id(p_i) = id(p_j), both on clearly active triplets (so an invalid triplet that still reported or still passed
    gradient shows)."""
    def make(attempt):
        rng = xg.case_rng("tail-m1", B, D, shift, int(tiny), attempt)
        pool, dist, G, margin = _pool(D, rng, n=POOL_BIG)
        plan = (list(M1_PLAN.get(B, M1_PLAN_8)) + ["any"] * max(0, B - 8))[:B]
        n_real = len(pool) - 1
        pi = np.full(B, -1, dtype=np.int64)
        ai = rng.randint(0, n_real, size=B)
        for i, want in enumerate(plan):                       # a positive that an earlier slot fixed stays; the rest is searched
            if want == "any":
                continue
            j = (i + shift) % B
            pred = T_CLASSES["active" if want.startswith("inv_") else want]
            ai[i], pi[i], pi[j] = _search(dist, rng, pred, G, margin, p=None if pi[i] < 0 else int(pi[i]), n=None if pi[j] < 0 else int(pi[j]))
        pi = np.where(pi < 0, rng.randint(0, n_real, size=B), pi)
        idx = np.stack([ai, pi], 1).ravel()
        z, s = scale_rows(pool[idx], rng)
        ids = (1000 + np.arange(2 * B)).astype(np.int32)
        for kind_ in ("inv_vp", "inv_va"):
            for i, want in enumerate(plan):
                j = (i + shift) % B
                if want == kind_:
                    ids[2 * i + (want == "inv_vp")] = ids[2 * j + 1]
        c = dict(name="tail m1 B=%d D=%d shift=%d%s" % (B, D, shift, " tiny" if tiny else ""), kind="m1", B=B, D=D, margin=margin, G=G,
                 z=z, s=s, ids=ids, shift=shift, plan=plan, inexact=None if (B & (B - 1)) == 0 else "npow2")
        if tiny:                                              # a tiny positive (the negative of slot i - shift too) and its control
            assert B >= 32 and D >= 64 and shift == 1
            r = _plant_tiny(c, [2 * i + 1 for i in range(10, B - 1)], 7)
            _plant_tiny(c, [2 * i + 1 for i in range(10, B - 1) if abs(2 * i + 1 - r) > 4], 7, -CONTROL)
        c["safe"] = assert_tail_exact_safe(c)
        c["classes"] = cl = classes(c)
        need = ["inv_va", "valid_i_only", "valid_k_only", "corner"] + (["second_only"] if B == 2 else ["minus"])
        if B >= 8:
            need += ["inv_vp", "both_terms", "second_only", "plus", "inactive"]
        for k in need:
            assert len(cl[k]) >= 1, "%s lacks class %s" % (c["name"], k)
        assert len(cl["both_terms"]) + len(cl["second_only"]) >= 1
        if c["inexact"] == "npow2":
            _assert_npow2_margin(c)
        return c
    return cached(("tail-m1", B, D, shift, tiny), lambda: _attempts(make))


IDX_KINDS = ("mix", "one-row", "chunks")


def indexed_case(B, D, kind="mix", variant=0, tiny=False):
    """Indexed triplets (row 2i, row 2i + 1, row neg_row[i]) over R = 2B rows drawn from a pool of at most 512 rows.
    "mix": neg_row cycles through -1, 2i (own anchor), 2i + 1 (own positive), R - 1, a hub row mined by every other triplet,
    the four rows of one wave; planned triplets (their anchors are nobody's mined row) have t exactly 0, +-1 granule,
    clearly inactive (some of them mine the hub: key -1, they add nothing) or active.  "one-row": every triplet mines row
    77 (B = 1024: more than 512 hits on one wave, the list flush).  "chunks": B > 8192 -- a hub mined by the triplets
    around 8192 (hits on both sides of the key chunk boundary), a second hub mined by every 7th triplet, the last triplets
    of the batch (the short last chunk) active on rows of their own.  B = 1: ``variant`` 0 | 1 | 2 = neg_row -1 | 0 | 1."""
    def make(attempt):
        rng = xg.case_rng("tail-idx", B, D, kind, variant, int(tiny), attempt)
        R = 2 * B
        pool, dist, G, margin = _pool(D, rng, n=512)
        n_real = len(pool) - 1
        idx = rng.randint(0, n_real, size=R)
        nr = np.full(B, -1, dtype=np.int64)
        i = np.arange(B)
        hub = min(77, R - 1) | 1 if R > 2 else 1
        plan = {}
        if B == 1:
            nr[0] = (-1, 0, 1)[variant]
        elif kind == "mix":
            wave0 = 4 * ((R // 2) // 4) if R >= 8 else 0      # the four rows wave0 .. wave0 + 3 (one wave's)
            cyc = [-1, "a", "p", R - 1, hub, wave0, hub, wave0 + 1, hub, min(wave0 + 2, R - 1), hub, min(wave0 + 3, R - 1)]
            for t in range(B):
                v = cyc[t % len(cyc)]
                nr[t] = 2 * t if v == "a" else 2 * t + 1 if v == "p" else v
            if B >= 16:
                plan = {4: "corner", 6: "inactive", 8: "plus", 10: "minus", 16 % B: "corner", 18 % B: "inactive", 3: "corner", 15: "active"}
            elif B == 2:
                nr[:] = (3, -1) if variant == 0 else (1, 0)
                plan = {0: "corner"}
        elif kind == "one-row":
            nr[:] = hub
            plan = {0: "corner", 1: "inactive", 2: "plus", 3: "minus", B - 1: "active", 600 % B: "inactive"}
        else:
            hub2 = (R - 11) | 1
            nr[:] = 2 * rng.randint(0, B, size=B) + 1         # (positives only: every anchor stays free for the search)
            nr[rng.rand(B) < 0.1] = -1
            nr[::7 if (B & (B - 1)) == 0 else 31] = hub2      # (2 / B rounded: a shorter hub keeps the bound below one term)
            nr[8192 - 150:8192 + 150] = hub
            nr[B - 5:] = [1, 3, R - 1, hub, 5]
            plan = {8191: "active", 8192: "active", 8190: "inactive", 8193: "inactive", 8189: "corner", 8194: "corner",
                    B - 1: "active", B - 2: "active", B - 3: "active", B - 4: "corner", B - 5: "active", 0: "inactive", 7: "corner", 14: "plus"}
        if kind == "chunks":                                  # the planned triplets' positives are nobody's mined row: free to search
            nr[np.isin(nr, [2 * t + 1 for t in plan]) & (nr != 2 * i + 1)] = (R - 11) | 1
        hubs = [h for h in (hub, (R - 11) | 1) if kind != "mix" or B >= 8]
        if kind in ("one-row", "chunks"):                     # hub rows with one non-zero (j = 0): short sums over thousands of hits
            for h in hubs:
                idx[h] = 4 * rng.randint(0, n_real // 4)      # (rows r % 4 == 0 of unit_rows have j = 0)
                assert (pool[idx[h]] != 0).sum() == 1
        mined = set(int(v) for v in nr if v >= 0)
        free_a = ~np.isin(2 * i, list(mined))
        free_p = ~np.isin(2 * i + 1, hubs)
        for _ in range(8):                                    # no two rows of a triplet equal (but a mined own row): no term is 0
            n_idx = idx[np.where(nr >= 0, nr, 0)]             # (equal as vectors: the pool holds a +-e_k more than once)
            clash = free_p & (nr >= 0) & (nr != 2 * i + 1) & (dist[idx[2 * i + 1], n_idx] == 0)
            idx[2 * i[clash] + 1] = rng.randint(0, n_real, size=int(clash.sum()))
            n_idx = idx[np.where(nr >= 0, nr, 0)]
            clash = free_a & ((dist[idx[2 * i], idx[2 * i + 1]] == 0) | ((nr >= 0) & (dist[idx[2 * i], n_idx] == 0)))
            idx[2 * i[clash]] = rng.randint(0, n_real, size=int(clash.sum()))
        for t, want in plan.items():                         # search the anchor (it is nobody's mined row), the positive too if free
            if 2 * t in mined or nr[t] < 0 or nr[t] == 2 * t:
                continue
            p_free = (2 * t + 1) not in mined
            idx[2 * t], idx[2 * t + 1], _ = _search(dist, rng, T_CLASSES[want], G, margin, p=None if p_free else int(idx[2 * t + 1]),
                                                    n=int(idx[nr[t]]))
        zp, sp = scale_rows(pool, rng)                        # (one scale and one set of -0.0 per pool row: the builder stays fast)
        z = zp[idx].copy()
        if kind in ("one-row", "chunks"):                     # ... the hub rows at scale 1
            z[hubs] = pool[idx[hubs]]
        c = dict(name="tail idx B=%d D=%d %s%s%s" % (B, D, kind, " v%d" % variant if variant else "", " tiny" if tiny else ""), kind="idx",
                 B=B, D=D, margin=margin, G=G, z=z, neg_row=nr.astype(np.int32), idx_kind=kind, hub=hub,
                 inexact=None if (B & (B - 1)) == 0 else "npow2")
        if tiny:                                              # a tiny row that an active triplet mined, and its control
            assert B == 64 and D >= 64 and kind == "mix"
            r = _plant_tiny(c, [65, 67] + list(range(41, 63, 2)), 7)
            _plant_tiny(c, [q for q in [67, 65] + list(range(41, 63, 2)) if q != r], 7, -CONTROL)
        c["safe"] = assert_tail_exact_safe(c)
        c["classes"] = cl = classes(c)
        if kind == "one-row":
            assert len(cl["hub_hit"]) > 512, "the list flush needs more than 512 hits on one wave"
        if kind == "chunks":
            hits = np.nonzero(tail_model(c, tail=False)["key"] == hub)[0]
            assert (hits < 8192).any() and (hits >= 8192).any(), "the hub's hits do not straddle the key chunk boundary"
            assert len(cl["hub_inactive"]) >= 1 and len(cl["corner"]) >= 1
        if kind == "mix" and B >= 16:
            for k in ("masked", "own_anchor", "own_positive", "last_row", "hub_hit", "hub_inactive", "wave4", "corner", "plus", "minus"):
                assert len(cl[k]) >= 1, "%s lacks class %s" % (c["name"], k)
        if c["inexact"] == "npow2":
            _assert_npow2_margin(c)
        return c
    return cached(("tail-idx", B, D, kind, variant, tiny), lambda: _attempts(make))


def _assert_npow2_margin(c):
    """a batch that is no power of two: 2 / B is rounded and the gradients are compared within their bound -- every single
    term (own or hit) moves some element by at least 2^-3 * 2 / B, more than 4 times the largest bound"""
    m = tail_model(c, ALPHA_REF)
    move = 2.0 ** -3 * 2.0 / c["B"]
    e, tri, key = m["e"], m["tri"], m["key"]
    act = m["scale"] > 0
    a, p, n = e[tri[:, 0]], e[tri[:, 1]], e[tri[:, 2]]
    if c["kind"] != "idx":                                     # modes 0 and 1: the three differences of every active triplet
        for d in (n - p, p - a, a - n):
            assert (np.abs(d[act]).max(1) >= 2.0 ** -3).all(), "a term below the margin"
        # (dz2 = inv (g - z c) lrelu': a term of g reaches the row's dz2 scaled by inv and at least alpha)
        assert (m["dz2_tol"].max(1) * 4 < move * m["inv"] * float(np.float32(ALPHA_REF))).all(), "a dz2 bound is not 4 times below a term"
        return
    own_p = c["neg_row"] == tri[:, 1]                          # (a triplet that mined its own positive: n - p is 0 by definition)
    assert (np.abs((n - p)[act & ~own_p]).max(1) >= 2.0 ** -3).all() and (np.abs((p - a)[act]).max(1) >= 2.0 ** -3).all(), \
        "an own term below the margin"
    jj = np.nonzero(key >= 0)[0]
    dh = np.abs(e[2 * jj] - e[key[jj]]).max(1)
    assert (dh[key[jj] != 2 * jj] >= 2.0 ** -3).all(), "a hit's term below the margin"
    # (a lost term shows if it moves an element by more than twice the bound: computed and expected may each be off by one)
    assert m["de_tol"].max() * 4 < move, "the gradient bound %g is not 4 times below a term %g" % (m["de_tol"].max(), move)


def classes(c):
    """triplet / slot indices per planted class, from the default model alone"""
    m = tail_model(c, tail=False)
    t, G, valid, B = m["t"], c["G"], m["valid"], c["B"]
    i = np.arange(B)
    cl = {"corner": i[valid & (t == 0)], "plus": i[valid & (t == G)], "minus": i[valid & (t == -G)],
          "active": i[valid & (t >= 0.125)], "inactive": i[valid & (t <= -0.125)]}
    cz = m["clamped"]
    tri = m["tri"]
    act = m["scale"] > 0
    if c["kind"] == "m0":
        for r, k in enumerate(("zero_a", "zero_p", "zero_n")):
            cl[k] = i[act & cz[tri[:, r]]]
    elif c["kind"] == "m1":
        ids, sh = c["ids"], c["shift"]
        j, k = (i + sh) % B, (i - sh % B + B) % B
        va, vp, vn = ids[2 * i], ids[2 * i + 1], ids[2 * j + 1]
        sk = m["scale_k"] > 0
        valid_k = valid[k]
        cl.update(inv_va=i[(vn == va) & (vn != vp) & (t > 0)], inv_vp=i[(vn == vp) & (vn != va) & (t > 0)],
                  valid_i_only=i[valid & ~valid_k], valid_k_only=i[~valid & valid_k], both_terms=i[act & sk],
                  second_only=i[~act & sk])
    else:
        nr, key, R, hub = c["neg_row"].astype(np.int64), m["key"], 2 * B, c["hub"]
        w0 = 4 * ((R // 2) // 4)
        cl.update(masked=i[nr < 0], own_anchor=i[nr == 2 * i], own_positive=i[nr == 2 * i + 1], last_row=i[nr == R - 1],
                  hub_hit=i[key == hub], hub_inactive=i[(nr == hub) & (key < 0)],
                  wave4=i[(nr >= w0) & (nr < w0 + 4)] if len(set(nr[(nr >= w0) & (nr < w0 + 4)])) == 4 else i[:0])
    return cl


# ---- l2norm_fwd / l2norm_bwd: rows and a given gradient ----------------------------------------------------------------------------
L2_M, L2_N = (1, 5, 67), (4, 64, 252, 260)


def rows_case(M, N, s_zero=False):
    """z [M][N]: unit rows times 2^s (s cycling through -3 .. 3; ``s_zero``: every s = 0); from M = 5 on row 1 is all zero
    (+-0), row 2 tiny (one coordinate 2^-21), row 3 its control (2^-19).  g: dyadic multiples of 2^-4, +-0 included, non-zero
    at the tiny and the control coordinate."""
    def make():
        rng = xg.case_rng("tail-rows", M, N, int(s_zero))
        s = np.zeros(M, dtype=np.int64) if s_zero else (np.arange(M) + 2) % 7 - 3
        z, s = scale_rows(unit_rows(M, N, rng), rng, s=s)
        g = dyadic((M, N), rng)
        tiny = np.zeros(M, bool)
        col = N // 2 + 1
        if M >= 5:
            z[1] = np.where(rng.rand(N) < 0.5, 0.0, -0.0)
            z[2], z[3] = 0.0, -0.0
            z[2, col], z[3, col] = TINY, -CONTROL
            g[2, col], g[3, col] = 1.0, 0.75
            tiny[2] = True
            s = s.copy()
        c = dict(name="rows M=%d N=%d%s" % (M, N, " s=0" if s_zero else ""), kind="rows", M=M, N=N, z=z, g=g, s=s, tiny_rows=tiny, col=col)
        c["safe"] = assert_tail_exact_safe(c)
        return c
    return cached(("tail-rows", M, N, s_zero), make)


# ---- the elementwise kernels ----------------------------------------------------------------------------------------------------------
EW_M, EW_N = (1, 5), (4, 252, 260)


def ew_case(M, N):
    """dyadic g, a, b (multiples of 2^-4 up to 1, a third of them +-0): every product and sum below is an fp32 number"""
    def make():
        rng = xg.case_rng("tail-ew", M, N)
        g, a, b = (dyadic((M, N), rng) for _ in range(3))
        g[g == 0] = 0.5                                       # a non-zero gradient under every +-0 pre-activation
        a[0, :2], b[0, 2:4] = (0.0, -0.0), (0.0, -0.0)        # (both zeros in both operands, whatever the draw)
        P = 8
        pairs = rng.randint(0, M, size=(P, 2)).astype(np.int32)
        pairs[0] = (M - 1, M - 1)                             # a pair (i, i): distance 0, not counted in means[3]
        c = dict(name="ew M=%d N=%d" % (M, N), kind="ew", M=M, N=N, g=g, a=a, b=b, pairs=pairs, P=P)
        for v in (g * a, g * (b + 1.0), a * b + a + b, g * (a + 1.0)):
            assert is_f32(v)
        d = a[pairs[:, 0]] - a[pairs[:, 1]]
        c["safe"] = max(_reduction_units(d * d, "pair sqdist"), _reduction_units(a[pairs[:, 0]] * a[pairs[:, 1]], "pair dot"), 1.0)
        return c
    return cached(("tail-ew", M, N), make)


def lrelu_bwd_model(g, y, alpha, rule=()):
    return r32(g * lrelu_factor(y, alpha, rule))


def ew_fusion_bwd_model(residual, g, a, b, alpha, rule=()):
    """da = g (b + res) lrelu'(a), db = g (a + res) lrelu'(b), left to right, one rounding per operation"""
    res = 1.0 if residual else 0.0
    return (r32(r32(g * r32(b + res)) * lrelu_factor(a, alpha, rule)), r32(r32(g * r32(a + res)) * lrelu_factor(b, alpha, rule)))


def ew_combine_model(mode, a, b):
    return a * b if mode == 0 else a * b + a + b if mode == 1 else a + b


def pair_dist_model(e, pairs):
    """(sqdist, dot, means [4] float32): means = k_loss_stats over (sqdist, dot, sqdist): mean sqdist twice, mean dot, the
    share of pairs with sqdist > 0"""
    x, y = e[pairs[:, 0]], e[pairs[:, 1]]
    sd, dp = ((x - y) ** 2).sum(1), (x * y).sum(1)
    f, P = np.float32, len(pairs)
    return sd, dp, np.array([f(sd.sum()) / f(P), f(sd.sum()) / f(P), f(dp.sum()) / f(P), f((sd > 0).sum()) / f(P)], dtype=f)


# ---- fp32 recomputation in several orders (the host test: the same bits) ------------------------------------------------------------
def sum_orders_f32(terms):
    """[float32 [rows]] x 3: the last axis summed in fp32 forward, reversed, and 64-lane strided then a shuffle tree"""
    t = np.asarray(terms, np.float32)
    n = t.shape[-1]
    out = []
    for order in (range(n), range(n - 1, -1, -1)):
        acc = np.zeros(t.shape[:-1], np.float32)
        for k in order:
            acc = (acc + t[..., k]).astype(np.float32)
        out.append(acc)
    lanes = np.zeros(t.shape[:-1] + (64,), np.float32)
    for k in range(n):
        lanes[..., k % 64] = (lanes[..., k % 64] + t[..., k]).astype(np.float32)
    w = 64
    while w > 1:
        w //= 2
        lanes = (lanes[..., :w] + lanes[..., w:2 * w]).astype(np.float32)
    out.append(lanes[..., 0])
    return out


# ---- the committed cases ---------------------------------------------------------------------------------------------------------------
HINGE_B, HINGE_D = (1, 2, 4, 8, 64), (4, 64, 252, 260)
TAIL_B, TAIL_D = (2, 8, 64), (4, 64, 252, 256, 260, 512, 516, 1024)
INDEXED_PARAMS = ((1, 64, "mix", 0), (1, 64, "mix", 1), (1, 64, "mix", 2), (2, 64, "mix", 0), (2, 64, "mix", 1), (64, 4, "mix", 0),
                  (1024, 64, "one-row", 0), (16384, 64, "chunks", 0))
NPOW2_PARAMS = ((5, 64, "mix", 0), (67, 260, "mix", 0), (8197, 64, "chunks", 0))


TAIL_NPOW2 = ((5, 64), (67, 260))                           # vnet_tail on batches that are no power of two


def tail_npow2_cases(mode):
    if mode == 0:
        return [hinge_case(B, D) for B, D in TAIL_NPOW2]
    return [inbatch_case(B, D, sh) for B, D in TAIL_NPOW2 for sh in shifts_of(B)]


def shifts_of(B):
    return sorted({1, B // 2, B - 1} - {0})


def hinge_params():
    return [(B, D) for B in HINGE_B for D in HINGE_D]


def inbatch_params(Bs=HINGE_B, Ds=HINGE_D):
    return [(B, D, sh) for B in Bs if B >= 2 for D in Ds for sh in shifts_of(B)]


def tail_params(mode):
    if mode == 0:
        return [(B, D) for B in TAIL_B for D in TAIL_D]
    return inbatch_params(TAIL_B, TAIL_D)


def all_cases(entry):
    """the committed cases of one entry point ("l2norm_bwd", "hinge", "inbatch", "tail0", "tail1", "indexed", "indexed_tail")"""
    if entry == "l2norm_bwd":
        return [rows_case(M, N) for M in L2_M for N in L2_N]
    if entry == "hinge":
        return [hinge_case(*a) for a in hinge_params()]
    if entry == "inbatch":
        return [inbatch_case(*a) for a in inbatch_params()]
    if entry == "tail0":
        return [hinge_case(*a) for a in tail_params(0)] + [hinge_case(64, 64, tiny=True), hinge_case(32, 260, tiny=True)] + tail_npow2_cases(0)
    if entry == "tail1":
        return [inbatch_case(*a) for a in tail_params(1)] + [inbatch_case(64, 64, 1, tiny=True)] + tail_npow2_cases(1)
    return [indexed_case(*a) for a in INDEXED_PARAMS + NPOW2_PARAMS] + [indexed_case(64, 64, "mix", 0, tiny=True)]
