"""Ladder cases and an integer / fp32 model for the N-pair softmax family (csrc/npair.hip, npair_common.h, npair_mixed.hip,
npair_dp.hip; the bf16 W format; the logQ / neg_bias instantiations), compared at ZERO tolerance.

Every stats / grad entry point takes the score matrix S itself, so a test hands the kernels a ladder of logits:

* S holds small integers, multiples of 8; t = 2^-4, so inv_t = 16 is exact and every logit S / t is a multiple of 128;
* every bias (bias[2B], mem_bias[M], lq_u, neg_bias[B]) is an integer multiple of 128;
* in every row term and every column term the counted logits have ONE winner at level ``top``; everything else that counts
  sits at top - 128 k, k >= 1.

With expf(0) == 1, expf(x) == 0 for x <= -128 and logf(1) == 0 (tests/test_gpu_exact_npair.py asserts the three through
the kernels first), lse_add, lse_merge, row_fold, the chunked column pass and the ranks' fold carry (m, s) = (top, 1)
exactly in any order: lse = top bit for bit, the row / column term of W is 1 at the winner and 0 elsewhere (minus 1 on the
diagonal), every W entry is one of {0, +-scale, +-scale / 2} with the host's own fp32 scale = 1.0f / ((float)B * t), and
the rows' partials {top - d, 2 - 2 S_ii, sum (2 - 2 S_ij), count} are integers far below 2^24, so step_scalars' sums are
exact in any order.  Which column wins is then a pure consequence of the RULES: who counts for whom (four id compares, the
diagonal's exemption, empty ring slots), which bias slot a logit loses, where the diagonal sits on a rank, what is halved
under ``symmetric``, which denominator stats[3] takes.  A decoy one level above the winner at a column that must not
count turns a broken rule into another winner: other bits in lse, W and stats.

The model works in LEVELS (int64, one level = 128 logit units = 8 units of S).  A counted logit above the given lse --
what a W kernel sees when IT counts a pair the row pass did not -- is expf(>= 128) = +inf, so a W-only mutation is
visible too (``model(..., lse_rule=())``).  The four stats quotients are formed in np.float32 in step_scalars' order
(t0 / fb, 0.5f * (t0 / fb + t4 / fb), t2 / t3, t3 / den with den formed in fp32 as the three stats kernels form it): hipcc
divides fp32 with correct rounding by default and the build passes no flag that changes that, so they are compared with
``torch.equal`` like everything else.

``assert_npair_exact_safe`` computes the condition under which zero tolerance is legitimate; every builder stores its
result under "safe" and no test runs a case without it.  ``RULES`` lists every rule as a switch that turns the model into
one mutation; tests/test_exact_npair_host.py shows that each one changes the expectation of a committed case of every
entry point it concerns, and that the unmutated model agrees with the fp64 references of the existing tests.

The tie group is the one toleranced part: cases with n = 2, 3, 64, B equal winners, where s == n is still exact but
lse = top + logf(n) and W = expf(-logf(n)) * scale are not.  They are compared with the fp64 model in ulps of the fp32
result.  TIE_MEASURED_ULPS is the largest error the kernels showed on the MI355X and TIE_BOUND_ULPS = 2 * that (one logf,
one add, one expf and one multiply are the only inexact operations, and their error varies with the argument by about as
much); the GPU test prints both.  The winners sit at logit 0, so lse = logf(n) itself.  Measured: lse within 0.82 ulps
for every n; W 0 ulps at n = 2, 1.67 at n = 3 and 6, 0.02 at n = 64 and 5.08 at n = B = 260 -- bound 10.15.  The 5 ulps
are no fault of expf: the fp32 lse = 5.56 carries up to half an ulp (2.4e-7) of rounding, and exp turns an ABSOLUTE
error of its argument into a RELATIVE one of its value, 2.4e-7 = 4 ulps of fp32; it grows with |lse|, which is why the
ladder cases above need a winner, not a tie.

Plain module, numpy and torch on the CPU, no pytest configuration.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402
import footprint as fp  # noqa: E402

T = 2.0 ** -4                   # the temperature: a power of two, inv_t = 16 exact
LV = 128                        # one level in logit units
SU = 8                          # one level in units of S (SU / T == LV)
NEG = -(1 << 40)                # "-inf" of the integer model
F32 = np.float32
TIE_MEASURED_ULPS = 5.077       # largest error of lse / W of the tie cases on the MI355X, in ulps of the fp32 result
TIE_BOUND_ULPS = 2 * TIE_MEASURED_ULPS      # twice the measured value: what test_gpu_exact_npair.py asserts

# bias classes of column j (j % 4 -> R, U, R, W), in levels: (lq of the positive, lq of the anchor).  A row whose winner
# r sits in class R also gets a column u of class U one raw level pair above it (the UNCORRECTED winner: 32 > 31 > 30) and
# a column w of class W (the winner when the row term takes the anchor's slot): corrected 30 | 24 | 25, raw 30 | 32 | 31,
# wrong slot 28 | 27 | 30.
_CLS = np.array([0, 1, 0, 2])
_BP = np.array([0, 8, 6])
_BA = np.array([2, 5, 1])
_MB = np.array([0, 5, 2])       # mem_bias[k] by k % 3: neighbours differ
_NB = np.array([1, 4, 2])       # neg_bias[j] by j % 3
LQ_U = 3                        # the scalar of the uniform block

RULES = (
    "row_drop_a",               # row term: id(p_j) != id(a_i) not tested
    "row_drop_p",               # row term: id(p_j) != id(p_i) not tested
    "col_drop_a",               # column term: id(a_i) != id(a_j) not tested
    "col_drop_p",               # column term: id(a_i) != id(p_j) not tested
    "row_diag_masked",          # the diagonal subject to the row term's mask
    "col_diag_masked",          # the diagonal subject to the column term's mask
    "col_uses_row_rule",        # the column term counts by the row term's rule
    "mem_empty_counts",         # an empty ring slot (mem_id < 0) counts
    "mem_drop_a",               # a slot of the anchor's video counts
    "mem_drop_p",               # a slot of the positive's video counts
    "mem_in_col",               # pair j's column term also folds anchor j's memory logits
    "row_bias_anchor_slot",     # row term less bias[2j] instead of bias[2j + 1]
    "col_bias_pos_slot",        # column term less bias[2i + 1] instead of bias[2i]
    "diag_uncorrected",         # the loss numerators' diagonal logit without its bias
    "mem_bias_shift",           # mem_bias read one slot on
    "neg_bias_shift",           # neg_bias read one column on
    "lq_u_on_inbatch",          # the uniform block's correction applied to the in-batch block too
    "neg_drop_a",               # uniform block: id(n_j) != id(a_i) not tested
    "neg_drop_p",               # uniform block: id(n_j) != id(p_i) not tested
    "neg_diag_exempt",          # uniform block with a special diagonal
    "sym_no_half",              # symmetric: the 0.5 of the in-batch block missing
    "mem_not_halved",           # symmetric: the memory block not halved
    "neg_not_halved",           # symmetric: the uniform block not halved
    "dp_scale_G",               # dp: scale 1 / (G t) instead of 1 / (B t)
    "dp_diag_local",            # dp: the diagonal at column i instead of col0 + i
    "dp_fold_empty_nan",        # dp: an empty colpart (-inf, 0) poisons the ranks' fold
    "dp_fold_last_rank_only",   # dp: the fold keeps the last rank's partial
    "stats_den_no_mem",         # stats[3] without the B M term
    "stats_den_no_neg",         # stats[3] without the B B term (mixed)
    "count_diag",               # the counted negatives include the diagonal
    "mx_rows_ids2",             # mixed: the row rule reads the ids two apart
    "mx_cols_ids2",             # mixed: the column rule reads the ids two apart
)

_ID_ROW = ("row_drop_a", "row_drop_p", "row_diag_masked")
_ID_COL = ("col_drop_a", "col_drop_p", "col_diag_masked", "col_uses_row_rule")
_MEM = ("mem_empty_counts", "mem_drop_a", "mem_drop_p")
_NEGR = ("neg_drop_a", "neg_drop_p", "neg_diag_exempt")
# entry point (group) -> the rules that concern it
RULES_OF = {
    "npair_stats": _ID_ROW + _ID_COL + ("count_diag",),
    "npair_grad": _ID_ROW + _ID_COL + ("sym_no_half",),
    "npair_logq_stats": _ID_ROW + _ID_COL + ("count_diag", "row_bias_anchor_slot", "col_bias_pos_slot", "diag_uncorrected"),
    "npair_logq_grad": _ID_ROW + _ID_COL + ("sym_no_half", "row_bias_anchor_slot", "col_bias_pos_slot"),
    "npair_memory_stats": _ID_ROW + _ID_COL + _MEM + ("count_diag", "mem_in_col", "stats_den_no_mem"),
    "npair_memory_grad": _MEM + ("mem_not_halved",),
    "npair_memory_logq_stats": _ID_ROW + _ID_COL + _MEM + ("count_diag", "mem_in_col", "stats_den_no_mem",
                                                          "row_bias_anchor_slot", "col_bias_pos_slot", "diag_uncorrected",
                                                          "mem_bias_shift"),
    "npair_memory_logq_grad": _MEM + ("mem_not_halved", "mem_bias_shift"),
    "npair_mixed_stats": _ID_ROW + _ID_COL + _MEM + _NEGR + ("count_diag", "stats_den_no_mem", "stats_den_no_neg",
                                                           "row_bias_anchor_slot", "col_bias_pos_slot", "diag_uncorrected",
                                                           "mem_bias_shift", "lq_u_on_inbatch", "mx_rows_ids2", "mx_cols_ids2"),
    "npair_mixed_grad": _ID_ROW + _ID_COL + _MEM + _NEGR + ("sym_no_half", "mem_not_halved", "neg_not_halved",
                                                          "row_bias_anchor_slot", "col_bias_pos_slot", "mem_bias_shift",
                                                          "lq_u_on_inbatch", "mx_rows_ids2", "mx_cols_ids2"),
    "npair_mixed_stats_nb": _NEGR + ("neg_bias_shift", "lq_u_on_inbatch", "stats_den_no_neg", "mx_rows_ids2", "mx_cols_ids2"),
    "npair_mixed_grad_nb": _NEGR + ("neg_bias_shift", "neg_not_halved", "lq_u_on_inbatch", "mx_rows_ids2", "mx_cols_ids2"),
    "npair_dp_local_stats": _ID_ROW + _ID_COL + ("dp_diag_local",),
    "npair_dp_col_fold": ("dp_fold_empty_nan", "dp_fold_last_rank_only"),
    "npair_dp_stats": ("dp_diag_local", "count_diag"),
    "npair_dp_grad": _ID_ROW + _ID_COL + ("sym_no_half", "dp_scale_G", "dp_diag_local"),
}
# entry point (group) -> the chains whose cases launch it
CHAINS_OF = {
    "npair_stats": ("inbatch",), "npair_grad": ("inbatch",), "npair_logq_stats": ("logq",), "npair_logq_grad": ("logq",),
    "npair_memory_stats": ("memory",), "npair_memory_grad": ("memory",), "npair_memory_logq_stats": ("memory_logq",),
    "npair_memory_logq_grad": ("memory_logq",), "npair_mixed_stats": ("mixed", "mixed_lq"),
    "npair_mixed_grad": ("mixed", "mixed_lq"), "npair_mixed_stats_nb": ("mixed_nb",), "npair_mixed_grad_nb": ("mixed_nb",),
    "npair_dp_local_stats": ("dp",), "npair_dp_col_fold": ("dp",), "npair_dp_stats": ("dp",), "npair_dp_grad": ("dp",),
}
# what of the model's output an entry point writes
OUTPUTS_OF = {e: (("W_mem",) if "memory" in e and "grad" in e else ("W",) if "grad" in e else
                  ("lse_col",) if e == "npair_dp_col_fold" else ("stats",) if e == "npair_dp_stats" else
                  ("lse_row", "colpart") if e == "npair_dp_local_stats" else ("lse_row", "lse_col", "stats"))
              for e in RULES_OF}


def up4(n):
    return (int(n) + 3) // 4 * 4


# ---- the model ---------------------------------------------------------------------------------------------------------
def _is_dp(c):
    return c["chain"] == "dp"


def _view(c, rule, rank):
    """masks and logits (levels) of rank ``rank``'s B local rows as the kernels form them, under the mutations ``rule``"""
    B, G, M = c["B"], c["G"], c["M"]
    col0 = rank * B if _is_dp(c) else 0
    rows = col0 + np.arange(B)
    diag = np.arange(B) if "dp_diag_local" in rule else rows
    eye = np.zeros((B, G), bool)
    eye[np.arange(B), diag] = True
    L = c["L"][rows]
    ids, nid, mem_id = c["ids"], c.get("nid"), c.get("mem_id")
    v = {"B": B, "G": G, "M": M, "rows": rows, "diag": diag, "eye": eye, "L": L, "U": c.get("U"), "Lm": c.get("Lm")}
    if ids is None:
        m = np.ones((B, G), bool)
        mc = np.ones((B, G), bool)
        cn = np.ones((B, B), bool) if c.get("U") is not None else None
        cm = np.broadcast_to((mem_id >= 0) | ("mem_empty_counts" in rule), (B, M)).copy() if M else None
    else:
        RA, RP, CP = ids[rows, 0], ids[rows, 1], ids[:, 1]
        QA, CA, CQ = ids[rows, 0], ids[:, 0], ids[:, 1]
        if nid is not None:
            f2 = np.stack([ids[:, 0], ids[:, 1], nid], 1).reshape(-1)[:2 * B].reshape(B, 2)
            if "mx_rows_ids2" in rule:
                RA, RP, CP = f2[:, 0], f2[:, 1], f2[:, 1]
            if "mx_cols_ids2" in rule:
                QA, CA, CQ = f2[:, 0], f2[:, 0], f2[:, 1]

        def row_rule(q, drop_a=False, drop_p=False):
            return ((q[None, :] != RA[:, None]) | drop_a) & ((q[None, :] != RP[:, None]) | drop_p)
        m = row_rule(CP, "row_drop_a" in rule, "row_drop_p" in rule)
        if "row_diag_masked" not in rule:
            m |= eye
        if "col_uses_row_rule" in rule:
            mc = row_rule(CP)
        else:
            mc = ((QA[:, None] != CA[None, :]) | ("col_drop_a" in rule)) & ((QA[:, None] != CQ[None, :]) | ("col_drop_p" in rule))
        if "col_diag_masked" not in rule:
            mc |= eye
        cn = cm = None
        if c.get("U") is not None:
            cn = row_rule(nid, "neg_drop_a" in rule, "neg_drop_p" in rule)
            if "neg_diag_exempt" in rule:
                cn |= np.eye(B, dtype=bool)
        if M:
            cm = row_rule(mem_id, "mem_drop_a" in rule, "mem_drop_p" in rule) & ((mem_id >= 0) | ("mem_empty_counts" in rule))[None, :]
    bias = c.get("bias")
    ba = bp = np.zeros(G, np.int64)
    if bias is not None:
        ba, bp = bias[:, 0], bias[:, 1]
    Xr = L - (ba if "row_bias_anchor_slot" in rule else bp)[None, :]
    Xc = L - (bp if "col_bias_pos_slot" in rule else ba)[rows][:, None]
    lq = c.get("lq")
    if bias is not None and lq is not None and "lq_u_on_inbatch" in rule:
        Xr = Xr - (lq if np.ndim(lq) == 0 else lq[None, :])
    v.update(m=m, mc=mc, cn=cn, cm=cm, Xr=Xr, Xc=Xc)
    Ld = L[np.arange(B), diag]
    v["Ld"] = Ld
    unc = "diag_uncorrected" in rule
    v["d_row"] = Ld - (0 if unc else bp[rows])
    v["d_col"] = Ld - (0 if unc else ba[rows])
    if c.get("U") is not None:
        sub = 0
        if bias is not None and lq is not None:
            sub = lq if np.ndim(lq) == 0 else (np.roll(lq, -1) if "neg_bias_shift" in rule else lq)[None, :]
        v["Xu"] = c["U"] - sub
    if M:
        mb = c.get("mem_bias")
        sub = 0
        if bias is not None and mb is not None:
            sub = (np.roll(mb, -1) if "mem_bias_shift" in rule else mb)[None, :]
        v["Xm"] = c["Lm"] - sub
    return v


def _top(X, mask, axis):
    Xm = np.where(mask, X, NEG)
    top = Xm.max(axis=axis)
    n = (Xm == np.expand_dims(top, axis)).sum(axis=axis)
    return top, np.where(top == NEG, 0, n)


def _row_blocks(v):
    X, K = [v["Xr"]], [v["m"]]
    if v.get("Xu") is not None:
        X.append(v["Xu"])
        K.append(v["cn"])
    if v.get("Xm") is not None:
        X.append(v["Xm"])
        K.append(v["cm"])
    return np.concatenate(X, 1), np.concatenate(K, 1)


def _lse(top, n):
    """(top, n) -> float64 lse in logit units: top * 128 + log n; nobody counted: -inf"""
    with np.errstate(divide="ignore"):
        return np.where(n > 0, top.astype(np.float64) * LV, 0.0) + np.log(n.astype(np.float64))


def tops(c, rule=()):
    """per rank: the row terms' (top, n); for all ranks: the column terms' (top, n) [G], the ranks' partials and the NaN
    flag of a poisoned fold"""
    rule = frozenset(rule)
    world = c["world"]
    out = {"row": [], "colpart": []}
    for r in range(world):
        v = _view(c, rule, r)
        X, K = _row_blocks(v)
        out["row"].append(_top(X, K, 1))
        Xc, mc = v["Xc"], v["mc"]
        if "mem_in_col" in rule and v.get("Xm") is not None:     # (non-dp: B == G) anchor j's memory logits as more "rows" of column j
            Xc, mc = np.concatenate([Xc, v["Xm"].T], 0), np.concatenate([mc, v["cm"].T], 0)
        out["colpart"].append(_top(Xc, mc, 0))
    ct = np.stack([p[0] for p in out["colpart"]])
    cn = np.stack([p[1] for p in out["colpart"]])
    if "dp_fold_last_rank_only" in rule:
        ct, cn = ct[-1:], cn[-1:]
    top = ct.max(0)
    out["col"] = (top, np.where(ct == top[None, :], cn, 0).sum(0))
    out["col_nan"] = (cn == 0).any(0) if "dp_fold_empty_nan" in rule else np.zeros(c["G"], bool)
    return out


def scale_f32(c, rule=()):
    return F32(1.0) / (F32(c["G"] if "dp_scale_G" in rule else c["B"]) * F32(T))


def _ladder(X, top, n, counted):
    """counted ? expf(128 (X - top) - log n) : 0 in the model: 1 / n at the top, 0 below it, +inf above it"""
    d = X - top
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, 1.0 / np.maximum(n, 1), np.where(d > 0, np.inf, 0.0))
    return np.where(counted, e, 0.0)


def model(c, symmetric, rule=(), lse_rule=None):
    """The expectation of every entry point on case ``c``: per rank lists "lse_row" [B], "colpart" [G][2], "W" [B][span]
    (NaN where no launch writes), "W_mem" (the memory block alone), "stats" (np.float32 [4]) and the parts "t"; "lse_col"
    [G] (float64; exact cases: fp32 numbers).  ``rule``: the mutations; ``lse_rule``: the mutations of the lse the W kernels
    are GIVEN (None: the same) -- () models an error of a W kernel alone."""
    rule = frozenset(rule)
    tp = tops(c, rule if lse_rule is None else lse_rule)
    sr = frozenset(rule if lse_rule is None else lse_rule)
    B, G, M, world = c["B"], c["G"], c["M"], c["world"]
    out = {k: [] for k in ("lse_row", "colpart", "W", "W_mem", "stats", "t", "n_row")}
    ctop, cn = tp["col"]
    lse_col = _lse(ctop, cn)
    lse_col[tp["col_nan"]] = np.nan
    out["lse_col"], out["n_col"] = (lse_col if symmetric else None), cn
    scale = scale_f32(c, rule)
    for r in range(world):
        rtop, rn = tp["row"][r]
        out["lse_row"].append(_lse(rtop, rn))
        out["n_row"].append(rn)
        pt, pn = tp["colpart"][r]
        out["colpart"].append(np.stack([np.where(pn > 0, pt * float(LV), -np.inf), pn.astype(np.float64)], 1))
        # ---- W, with the masks and logits of ``rule`` and the lse of ``lse_rule``
        v = _view(c, rule, r)
        eye = v["eye"].astype(np.float64)
        w = _ladder(v["Xr"], rtop[:, None], rn[:, None], v["m"]) - eye
        if symmetric:
            cc = _ladder(v["Xc"], ctop[None, :], cn[None, :], v["mc"])
            cc = np.where(v["mc"] & tp["col_nan"][None, :], np.nan, cc) - eye
            w = (w + cc) if "sym_no_half" in rule else 0.5 * (w + cc)
        span = c["span"]
        W = np.full((B, span), np.nan)
        with np.errstate(invalid="ignore"):
            W[:, :G] = w * float(scale)
        half = lambda name: float(scale) if (not symmetric or name in rule) else 0.5 * float(scale)
        if v.get("Xu") is not None:
            W[:, c["neg_col"]:c["neg_col"] + B] = _ladder(v["Xu"], rtop[:, None], rn[:, None], v["cn"]) * half("neg_not_halved")
        Wm = None
        if M:
            Wm = _ladder(v["Xm"], rtop[:, None], rn[:, None], v["cm"]) * half("mem_not_halved")
            W[:, c["mem_col"]:c["mem_col"] + M] = Wm
        out["W"].append(W)
        out["W_mem"].append(Wm)
        # ---- the step scalars, with the masks and logits of the lse's rule
        v = _view(c, sr, r)
        off = v["m"] & (~v["eye"] if "count_diag" not in sr else True)
        S2 = lambda lev: 2 - 2 * SU * lev
        ns, nc, absum = S2(v["L"])[off].sum(), int(off.sum()), np.abs(S2(v["L"])).sum()
        if v.get("Xu") is not None:
            ns, nc, absum = ns + S2(v["U"])[v["cn"]].sum(), nc + int(v["cn"].sum()), absum + np.abs(S2(v["U"])).sum()
        if M:
            ns, nc, absum = ns + S2(v["Lm"])[v["cm"]].sum(), nc + int(v["cm"].sum()), absum + np.abs(S2(v["Lm"])).sum()
        exact = bool((rn == 1).all()) and (not symmetric or bool((cn[v["diag"]] == 1).all() and not tp["col_nan"][v["diag"]].any()))
        t = None
        st = np.full(4, np.nan, F32)
        if exact:
            p0 = (rtop - v["d_row"]) * LV
            cl = (ctop[v["diag"]] - v["d_col"]) * LV
            t = [int(p0.sum()), int(S2(v["Ld"]).sum()), int(ns), nc, int(cl.sum()) if symmetric else 0]
            out_abs = [int(np.abs(p0).sum()), int(np.abs(S2(v["Ld"])).sum()), int(absum), nc, int(np.abs(cl).sum())]
            t0, t1, t2, t3, t4 = (F32(x) for x in t)
            fb = F32(B)
            if c["chain"].startswith("mixed"):
                den = fb * F32(B - 1) + (F32(0) if "stats_den_no_neg" in sr else fb * fb) \
                    + (F32(0) if "stats_den_no_mem" in sr else fb * F32(M))
                guard = False
            elif _is_dp(c):
                den, guard = fb * F32(G - 1), True
            else:
                den = fb * F32(B - 1) + fb * F32(M) if (M and "stats_den_no_mem" not in sr) else fb * F32(B - 1)
                guard = True
            with np.errstate(divide="ignore", invalid="ignore"):
                st[0] = F32(0.5) * (t0 / fb + t4 / fb) if symmetric else t0 / fb
                st[1] = t1 / fb
                st[2] = t2 / t3 if t3 > 0 else F32(0)
                st[3] = t3 / den if (not guard or den > 0) else F32(0)
            t = {"t": t, "abs": out_abs}
        out["stats"].append(st)
        out["t"].append(t)
    return out


def differs(a, b):
    """two model outputs (arrays, or per-rank lists of them) differ somewhere (NaN == NaN)"""
    if a is None or b is None:
        return (a is None) != (b is None)
    if isinstance(a, list):
        return any(differs(x, y) for x, y in zip(a, b))
    return not np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def entry_output(m, entry):
    return [m[k] for k in OUTPUTS_OF[entry]]


# ---- exactness ---------------------------------------------------------------------------------------------------------
def assert_npair_exact_safe(c):
    """The condition under which zero tolerance is legitimate, computed: S and every logit are fp32 integers on the ladder
    (multiples of 8 / of 128), every row term and every column term has exactly one counted maximum (``tie``: exactly n)
    with every other counted logit at least 128 below it, and every sum of |2 - 2 S| and every loss numerator is below
    2^24.  Returns the largest magnitude met (must be < 2^24)."""
    worst = 0
    for name in ("L", "U", "Lm", "bias", "mem_bias", "lq"):
        a = c.get(name)
        if a is None:
            continue
        a = np.asarray(a)
        assert a.dtype.kind == "i", name
        worst = max(worst, int(np.abs(a).max()) * LV)
    assert T == 2.0 ** -4 and SU / T == LV and float(F32(1.0) / F32(T)) == 1.0 / T
    n_want = c.get("tie", 1)
    for symmetric in (False, True):
        m = model(c, symmetric)
        for r in range(c["world"]):
            v = _view(c, frozenset(), r)
            X, K = _row_blocks(v)
            worst = max(worst, int(np.abs(X).max()) * LV, int(np.abs(v["Xc"]).max()) * LV)
            assert (m["n_row"][r] == n_want).all(), "%s: a row term has %s winners" % (c["name"], sorted(set(m["n_row"][r].tolist())))
            Xs = np.sort(np.where(K, X, NEG), 1)
            if X.shape[1] > n_want:
                assert (Xs[:, -n_want - 1] <= Xs[:, -1] - 1).all()          # (levels are integers: one level = 128)
            if c.get("tie"):
                continue                                                      # (a tie's loss numerators are not integers)
            t = m["t"][r]
            assert t is not None, c["name"]
            assert max(t["abs"]) < 2 ** 24, (c["name"], t)
            worst = max(worst, max(t["abs"]))
        if symmetric:
            assert (m["n_col"] == n_want).all(), "%s: a column term has %s winners" % (c["name"], sorted(set(m["n_col"].tolist())))
    assert worst < 2 ** 24, (c["name"], worst)
    return worst


# ---- builders ----------------------------------------------------------------------------------------------------------
def _set(r, row, col):
    """the permutation r with r[row] = col (the row that had col takes row's old column)"""
    other = int(np.nonzero(r == col)[0][0])
    r[other], r[row] = r[row], col


def _roles(B):
    """which rows play which part: everything at B >= 16, what fits below"""
    if B >= 16:
        return dict(ad=(10, 3), b=(11, 5), c=(12, 8), e=13, mem_w0=1, mem_w1=2, mem_d=3, mem_dp=4, uni_w0=5, uni_w1=6,
                    uni_da=(7, 2), uni_dp=(9, 3), uni_diag=14)
    if B == 6:
        return dict(ad=(0, 1), c=(0, 2), e=5, mem_w0=1, mem_w1=2, mem_d=3, mem_dp=4)
    if B == 4:
        return dict(ad=(0, 1), e=3, mem_w0=1, mem_w1=2, mem_d=3, uni_w0=0)
    if B == 3:
        return dict(ad=(0, 1), e=2)
    return dict(e=0)


def _finish(c):
    c["safe"] = assert_npair_exact_safe(c)
    return c


def _base(chain, B, with_ids, with_bias, G=None, world=1, shift=None):
    """the in-batch block: a permutation of winners at level 30 over a background of 0 with the diagonal at 10 (all before
    the biases), the planted id relations and their decoys"""
    R = world * B                                    # rows of the (global) matrix
    G = R if G is None else G
    roles = _roles(B)
    c = {"chain": chain, "B": B, "G": G, "M": 0, "world": world, "roles": roles, "span": G, "decoys": [], "want": {}}
    ids = None
    if with_ids:
        ids = np.stack([10 + 2 * np.arange(G), 11 + 2 * np.arange(G)], 1).astype(np.int64)
        if "ad" in roles:
            ids[roles["ad"][1], 1] = ids[roles["ad"][0], 0]
        if "b" in roles:
            ids[roles["b"][1], 1] = ids[roles["b"][0], 1]
        if "c" in roles:
            ids[roles["c"][1], 0] = ids[roles["c"][0], 0]
        ids[roles["e"], 1] = ids[roles["e"], 0]
    c["ids"] = ids
    cls = _CLS[np.arange(G) % 4]
    bias = np.stack([_BA[cls], _BP[cls]], 1).astype(np.int64) if with_bias else None
    c["bias"] = bias
    ba, bp = (bias[:, 0], bias[:, 1]) if with_bias else (np.zeros(G, np.int64),) * 2
    s = (7 if R > 7 else 1) if shift is None else shift
    r = (np.arange(R) + s) % R
    if R > 1:
        _set(r, roles["e"], roles["e"])              # a diagonal winner (the pair with id(a) == id(p): its diagonal still counts)
    if world > 1 and R > 4:
        g1 = 20 if B >= 32 else 1
        _set(r, g1, g1 + 1)                          # a winner in the rank's own block, off the diagonal
        _set(r, B + 2, B + 2)                        # a diagonal winner on rank 1: column col0 + i, not i
    L = np.zeros((R, G), np.int64)
    L[np.arange(R), np.arange(R)] = 10 + np.maximum(ba, bp)[:R]
    L[np.arange(R), r] = 30 + bp[r]
    c["winner"], c["three"] = r, np.zeros(R, bool)
    if with_bias and G >= 6:
        for i in range(R):
            j = int(r[i])
            if cls[j] != 0:
                continue
            base = j - j % 4
            if base + 3 >= G:
                base -= 4
            if base < 0:
                continue
            L[i, base + 1], L[i, base + 3] = 32, 31  # the uncorrected winner | the wrong slot's winner
            c["three"][i] = True
    for j in range(R, G):                            # dp padding columns: one counted contender each, below every row's winner
        L[(5 * j) % R, j] = 5
    c["L"] = L
    return c


def _plant_inbatch_decoys(c):
    """one level above the row's / the column's winner at the pairs the planted ids mask (after every block is in place)"""
    roles, ids = c["roles"], c["ids"]
    if ids is None:
        return
    bias = c["bias"]
    ba, bp = (bias[:, 0], bias[:, 1]) if bias is not None else (np.zeros(c["G"], np.int64),) * 2
    for kind in ("c", "b", "ad"):
        if kind not in roles:
            continue
        i, j = roles[kind]
        tp = tops(c)
        rtop, ctop = int(tp["row"][0][0][i]), int(tp["col"][0][j])
        if kind == "ad":                             # id(p_j) == id(a_i): masked in the row term (compare a) and the column term (compare p)
            lev = max(rtop + 1 + bp[j], ctop + 1 + ba[i])
        elif kind == "b":                            # id(p_j) == id(p_i): masked in the row term only
            lev = rtop + 1 + bp[j]
        else:                                        # id(a_i) == id(a_j): masked in the column term only
            lev = ctop + 1 + ba[i]
        c["L"][i, j] = lev
        c["decoys"].append((kind, i, j))


def inbatch_case(B, with_ids, with_bias=False):
    def make():
        c = _base("logq" if with_bias else "inbatch", B, with_ids, with_bias)
        c["name"] = "%s B=%d ids=%s" % (c["chain"], B, with_ids)
        c["lds"] = up4(B) + 4
        _plant_inbatch_decoys(c)
        return _finish(c)
    return xs.cached(("npair", "inbatch", B, with_ids, with_bias), make)


def _add_memory(c, M, col):
    """the ring block: winners in the first and the last slot, an empty slot, a slot of the anchor's and one of the
    positive's video one level above the row's winner, and a counted slot between pair j's column top and row top"""
    B, roles = c["B"], c["roles"]
    c["M"], c["mem_col"] = M, col
    mem_id = 100000 + np.arange(M, dtype=np.int64)
    mem_id[np.arange(M) % 5 == 1] = -1               # empty slots (slot 1 among them)
    mb = _MB[np.arange(M) % 3].astype(np.int64) if c["bias"] is not None else None
    sub = mb if mb is not None else np.zeros(M, np.int64)
    Lm = np.zeros((B, M), np.int64)
    ids = c["ids"]
    if "mem_w0" in roles and B > roles["mem_w1"]:
        Lm[roles["mem_w0"], 0] = 32 + sub[0]
        Lm[roles["mem_w1"], M - 1] = 32 + sub[M - 1]
        Lm[roles["mem_w0"], 2] = 31 + sub[2]         # counted, below the row's winner, above column mem_w0's
        i = roles["mem_d"]
        Lm[i, 1] = 31 + sub[1]                       # the empty slot
        c["decoys"].append(("mem_empty", i, 1))
        if ids is not None:
            mem_id[M - 1] = ids[i, 0]                # the anchor's video
            Lm[i, M - 1] = 31 + sub[M - 1]
            c["decoys"].append(("mem_a", i, M - 1))
            if "mem_dp" in roles:
                i = roles["mem_dp"]
                mem_id[0] = ids[i, 1]                # the positive's video
                Lm[i, 0] = 31 + sub[0]
                c["decoys"].append(("mem_p", i, 0))
    c["mem_id"], c["mem_bias"], c["Lm"] = mem_id, mb, Lm


def memory_case(B, M, with_ids, with_bias=False):
    def make():
        c = _base("memory_logq" if with_bias else "memory", B, with_ids, with_bias)
        c["name"] = "%s B=%d M=%d ids=%s" % (c["chain"], B, M, with_ids)
        _add_memory(c, M, up4(B + 1) + 4)
        c["span"] = c["mem_col"] + M
        c["lds"] = c["span"] + 4
        _plant_inbatch_decoys(c)
        return _finish(c)
    return xs.cached(("npair", "memory", B, M, with_ids, with_bias), make)


def mixed_case(B, M, with_ids, lq):
    """lq: None (uncorrected) | "scalar" (lq_u) | "nb" (neg_bias[B])"""
    def make():
        with_bias = lq is not None
        c = _base({None: "mixed", "scalar": "mixed_lq", "nb": "mixed_nb"}[lq], B, with_ids, with_bias)
        c["name"] = "%s B=%d M=%d ids=%s" % (c["chain"], B, M, with_ids)
        roles, ids = c["roles"], c["ids"]
        c["neg_col"] = B + 4
        c["lq"] = None if lq is None else np.int64(LQ_U) if lq == "scalar" else _NB[np.arange(B) % 3].astype(np.int64)
        sub = np.zeros(B, np.int64) if lq is None else np.broadcast_to(c["lq"], (B,))
        nid = 200000 + np.arange(B, dtype=np.int64)
        U = np.zeros((B, B), np.int64)
        if "uni_w0" in roles:
            U[roles["uni_w0"], 0] = 32 + sub[0]      # a winner in the first uniform column
        if "uni_w1" in roles:
            U[roles["uni_w1"], B - 1] = 32 + sub[B - 1]
        if ids is not None:
            for kind, col in (("uni_da", 0), ("uni_dp", 1)):
                if kind in roles:
                    i, j = roles[kind]
                    nid[j] = ids[i, col]             # the anchor's | the positive's video as a uniform negative
                    U[i, j] = 31 + sub[j]
                    c["decoys"].append((kind, i, j))
            if "uni_diag" in roles:
                i = roles["uni_diag"]
                nid[i] = ids[i, 0]                   # no special diagonal in the uniform block
                U[i, i] = 31 + sub[i]
                c["decoys"].append(("uni_diag", i, i))
        c["U"], c["nid"] = U, (nid if ids is not None else None)
        c["span"] = c["neg_col"] + B
        if M:
            _add_memory(c, M, c["neg_col"] + B + 4)
            c["span"] = c["mem_col"] + M
        else:
            c["mem_col"] = 0
        c["lds"] = c["span"] + 4
        _plant_inbatch_decoys(c)
        return _finish(c)
    return xs.cached(("npair", "mixed", B, M, with_ids, lq), make)


def dp_case(B, G=None, with_ids=True):
    """world = 3 ranks of B pairs: all ranks' row blocks of one global matrix [3B][G]; G > 3B: padding columns"""
    def make():
        world = 3
        c = _base("dp", B, with_ids, False, G=G, world=world, shift=B + 3)
        c["name"] = "dp B=%d G=%d ids=%s" % (B, c["G"], with_ids)
        c["lds"] = c["G"] + 4
        ids = c["ids"]
        c["empty"] = []
        if ids is not None:
            # a column of rank 2 for which NO row of rank 1 (B = 4) / of rank 1's last 256-row chunk (B = 260) counts:
            # those anchors share one video, which is also the column's positive
            rows = np.arange(B, 2 * B) if B <= 4 else np.arange(B + 256, 2 * B)
            j = 2 * B + 1
            ids[rows, 0] = 777
            ids[j, 1] = 777
            if B <= 4:
                c["empty"].append((1, j))
        _plant_inbatch_decoys(c)
        return _finish(c)
    return xs.cached(("npair", "dp", B, G, with_ids), make)


def tie_case(B, n):
    """n equal winners in every row and every column term (a circulant of n diagonals at one level); ids None"""
    def make():
        c = {"chain": "inbatch", "B": B, "G": B, "M": 0, "world": 1, "roles": {}, "span": B, "decoys": [], "ids": None,
             "bias": None, "tie": n, "name": "tie B=%d n=%d" % (B, n), "lds": up4(B) + 4}
        L = np.full((B, B), -1, np.int64)             # the winners at logit 0: lse = logf(n) itself, no large top to round against
        step = max(1, B // n)
        for k in range(n):
            L[np.arange(B), (np.arange(B) + k * step) % B] = 0
        c["L"] = L
        return _finish(c)
    return xs.cached(("npair", "tie", B, n), make)


INBATCH_B = (1, 3, 6, 260, 1030)
MEMORY_B, MEMORY_M = (6, 260), (4, 1028)
MIXED_B, MIXED_M = (4, 260, 1028), (0, 4, 1028)
DP_SHAPES = ((4, None), (260, None), (4, 16))
TIE_SHAPES = ((6, 2), (6, 3), (6, 6), (260, 2), (260, 3), (260, 64), (260, 260))


def case_specs(chain):
    """(builder, arguments) of every committed ladder case of one chain ("inbatch", "logq", "memory", "memory_logq",
    "mixed", "mixed_lq", "mixed_nb", "dp"), unbuilt; every in-batch shape with ids and with ids = None"""
    if chain in ("inbatch", "logq"):
        return [(inbatch_case, (B, w, chain == "logq")) for B in INBATCH_B for w in (True, False)]
    if chain in ("memory", "memory_logq"):
        return [(memory_case, (B, M, w, chain == "memory_logq")) for B in MEMORY_B for M in MEMORY_M for w in (True, False)]
    if chain.startswith("mixed"):
        lq = {"mixed": None, "mixed_lq": "scalar", "mixed_nb": "nb"}[chain]
        return [(mixed_case, (B, M, w, lq)) for B in MIXED_B for M in MIXED_M for w in ((True, False) if B == 260 else (True,))]
    if chain == "dp":
        return [(dp_case, (B, G, w)) for B, G in DP_SHAPES for w in ((True, False) if B == 260 else (True,))]
    raise KeyError(chain)


def all_cases(chain):
    return [make(*args) for make, args in case_specs(chain)]


CHAINS = ("inbatch", "logq", "memory", "memory_logq", "mixed", "mixed_lq", "mixed_nb", "dp")


def tie_cases():
    return [tie_case(B, n) for B, n in TIE_SHAPES]


# ---- what the builders promise -----------------------------------------------------------------------------------------
def winners(c, rank=0):
    """(block, column) of every local row's row-term winner of rank ``rank``: block "in" | "neg" | "mem" """
    v = _view(c, frozenset(), rank)
    X, K = _row_blocks(v)
    j = np.where(K, X, NEG).argmax(1)
    G, B = c["G"], c["B"]
    return [("in", int(x)) if x < G else ("neg", int(x - G)) if (c.get("U") is not None and x < G + B) else
            ("mem", int(x - G - (B if c.get("U") is not None else 0))) for x in j]


def col_winners(c):
    """the global row that wins each in-batch column's term"""
    best = np.full(c["G"], NEG)
    who = np.full(c["G"], -1)
    for r in range(c["world"]):
        v = _view(c, frozenset(), r)
        X = np.where(v["mc"], v["Xc"], NEG)
        i = X.argmax(0)
        val = X[i, np.arange(c["G"])]
        who = np.where(val > best, v["rows"][i], who)
        best = np.maximum(best, val)
    return who


def assert_schedule(c):
    """the winners' placement, by schedule and not by chance, at the sizes that have the path"""
    B, G, M = c["B"], c["G"], c["M"]
    cols, on_diag = set(), False
    for r in range(c["world"]):
        w = winners(c, r)
        cols |= {x[1] for x in w if x[0] == "in"}
        col0 = r * B if _is_dp(c) else 0
        on_diag |= any(x == ("in", col0 + i) for i, x in enumerate(w))
        if r == c["world"] - 1 and B >= 16:
            want = {0, 63, 64, 255, 256, c["world"] * B - 1} if B >= 260 else {0, B - 1}   # (B - 1: the last column of a B % 4 tail)
            assert want <= cols, (c["name"], sorted(want - cols))
            assert on_diag, c["name"] + ": no diagonal winner"
        if _is_dp(c) and B >= 4:
            own = [x[1] for i, x in enumerate(w) if col0 <= x[1] < col0 + B and x[1] != col0 + i]
            other = [x[1] for x in w if not col0 <= x[1] < col0 + B]
            assert other and (r != 0 or own), c["name"]
        if M and B >= 6:
            assert {("mem", 0), ("mem", M - 1)} <= set(w), c["name"]
        if c.get("U") is not None and B >= 16:
            assert {("neg", 0), ("neg", B - 1)} <= set(w), c["name"]
    cw = col_winners(c)
    assert (cw >= 0).all()
    if B >= 260:
        local = set((cw % B).tolist())
        assert {0, 255, 256, B - 1} <= local, c["name"]
    if _is_dp(c):
        owner = np.arange(c["G"]) // B
        assert ((cw // B) != owner)[:3 * B].any(), c["name"]
        m = model(c, True)
        for rank, j in c["empty"]:
            assert np.array_equal(m["colpart"][rank][j], [-np.inf, 0.0]), c["name"]


def assert_decoys(c):
    """every planted decoy is NOT counted where it was planted and sits at least one level above that term's winner"""
    v = _view(c, frozenset(), 0)
    tp = tops(c)
    rtop, ctop = tp["row"][0][0], tp["col"][0]
    kinds = set()
    for kind, i, j in c["decoys"]:
        kinds.add(kind)
        if kind in ("ad", "b"):
            assert not v["m"][i, j] and v["Xr"][i, j] >= rtop[i] + 1, (c["name"], kind)
        if kind in ("ad", "c"):
            assert not v["mc"][i, j] and v["Xc"][i, j] >= ctop[j] + 1, (c["name"], kind)
        if kind.startswith("mem"):
            assert not v["cm"][i, j] and v["Xm"][i, j] == rtop[i] + 1, (c["name"], kind)
        if kind.startswith("uni"):
            assert not v["cn"][i, j] and v["Xu"][i, j] == rtop[i] + 1, (c["name"], kind)
    return kinds


def bias_winner_shares(c):
    """of the rows of a corrected in-batch case: the share whose uncorrected winner differs from the corrected one, and
    the share whose wrong-slot winner differs from both"""
    v = _view(c, frozenset(), 0)
    ok = lambda X: np.where(v["m"], X, NEG).argmax(1)
    good, raw, wrong = ok(v["Xr"]), ok(v["L"]), ok(_view(c, frozenset(("row_bias_anchor_slot",)), 0)["Xr"])
    return float((raw != good).mean()), float(((wrong != good) & (wrong != raw)).mean())


# ---- device operands ---------------------------------------------------------------------------------------------------
def s_matrix(c, rank=0):
    """rank's S fp32 [B][lds]: the blocks at their columns, poison (NaN) in the gaps"""
    B, G, M = c["B"], c["G"], c["M"]
    rows = (rank * B if _is_dp(c) else 0) + np.arange(B)
    S = fp.poisoned((B, c["lds"]), dtype=torch.float32, device="cpu")
    S[:, :G] = xg.f32_exact(c["L"][rows] * float(SU))
    if c.get("U") is not None:
        S[:, c["neg_col"]:c["neg_col"] + B] = xg.f32_exact(c["U"] * float(SU))
    if M:
        S[:, c["mem_col"]:c["mem_col"] + M] = xg.f32_exact(c["Lm"] * float(SU))
    return S


def ids_tensor(c):
    """int32 [2G] (a, p per pair), [3B] (a, p, n per triplet: the mixed chain) or None"""
    if c["ids"] is None:
        return None
    cols = [c["ids"][:, 0], c["ids"][:, 1]] + ([c["nid"]] if c.get("nid") is not None else [])
    return torch.from_numpy(np.stack(cols, 1).reshape(-1).astype(np.int32))


def bias_tensors(c):
    """(bias fp32 [2G], mem_bias fp32 [M], lq_u float | neg_bias fp32 [B]) in logit units, None where the case has none"""
    f = lambda a: None if a is None else torch.from_numpy((np.asarray(a, np.float64) * LV).astype(np.float32).reshape(-1))
    lq = c.get("lq")
    return f(c["bias"]), f(c.get("mem_bias")), (None if lq is None else float(lq) * LV if np.ndim(lq) == 0 else f(lq))


def w_layout(c, fmt):
    """(ldw, plane) for W's format "f32" | "x3" | "bf16": both larger than the span"""
    span = up4(c["span"])
    if fmt == "x3":
        plane = span + 4
        return 2 * plane + span + 8, plane
    return span + 4, 0


def w_buffer(c, fmt, device="cpu"):
    ldw, _ = w_layout(c, fmt)
    return fp.poisoned((c["B"], ldw), dtype=torch.float32 if fmt == "f32" else torch.bfloat16, device=device)


def w_expected(c, fmt, W, cols=None):
    """what a poisoned ``w_buffer`` must hold after the launches that write the columns ``cols`` (a boolean [span]; None:
    every column the model wrote): the fp32 values, their three planes or their round-to-nearest-even, poison elsewhere"""
    ldw, plane = w_layout(c, fmt)
    written = ~np.isnan(W).all(0) if cols is None else cols
    idx = torch.from_numpy(np.nonzero(written)[0])
    w32 = xg.f32_exact(np.where(np.isnan(W), 0.0, W))
    buf = w_buffer(c, fmt)
    if fmt == "f32":
        buf[:, idx] = w32[:, idx]
    elif fmt == "bf16":
        buf[:, idx] = w32[:, idx].to(torch.bfloat16)
    else:
        planes = xg.split_planes(w32)
        assert torch.equal(planes[0].float() + planes[1].float() + planes[2].float(), w32)
        for p, t in enumerate(planes):
            buf[:, p * plane + idx] = t[:, idx]
    return buf


def ulps(got, want):
    """|got - want| in ulps of the fp32 result ``got`` (float64 ``want``)"""
    got = np.asarray(got, np.float32)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(got)).astype(np.float64)


# ---- the chains: embeddings whose scores land on the ladder ------------------------------------------------------------
CHAIN_D = 64


def chain_case(kind, B, world=1):
    """``kind`` "inbatch" | "memory" | "mixed" | "dp": embeddings for ops.npair_loss / npair_mixed_loss / the dp phases whose scores
    S = <a_i, p_j> ARE a ladder.  Pair g has the coordinate k = g % 64 and the layer q = g // 64: a_g = (1 + q) e_k,
    p_g = 8 (1 + (q + k) % nq) e_k (nq layers), so S_ij = 0 across coordinates and (1 + q_i) 8 (1 + ..) within one -- in
    every row and every column distinct multiples of 8, small integers exact in one bf16 plane.  mixed: n_g = 40 e_k on
    layer 0, the zero row elsewhere.  ids: unique, except that on every 16th pair the winner's positive (uniform
    negative) carries the anchor's video, which hands the row to the next level.  The case is a model case (L = S / 8);
    "A", "P", "N" are the rows [world B][64]."""
    def make():
        R, D = world * B, CHAIN_D
        assert R % D == 0
        nq = R // D
        g = np.arange(R)
        k, q = g % D, g // D
        A, P = np.zeros((R, D)), np.zeros((R, D))
        A[g, k] = 1 + q
        P[g, k] = SU * (1 + (q + k) % nq)
        S = A @ P.T
        ids = np.stack([10 + 2 * g, 11 + 2 * g], 1).astype(np.int64)
        top = S.argmax(1)
        for i in range(5, R, 16):
            ids[top[i], 1] = ids[i, 0]
        c = {"chain": "dp" if kind == "dp" else kind, "B": B, "G": R, "M": 0, "world": world, "roles": {}, "decoys": [],
             "ids": ids, "bias": None, "L": (S / SU).astype(np.int64), "span": R, "A": A, "P": P,
             "name": "chain %s B=%d world=%d" % (kind, B, world)}
        assert np.array_equal(c["L"] * float(SU), S)
        if kind == "memory":                          # a ring of M = B rows: 8 (5 + ..) e_k, above every positive of the coordinate
            Mem = np.zeros((R, D))
            Mem[g, k] = SU * (5 + (q + 2 * k) % nq)
            Sm = A @ Mem.T
            mem_id = 300000 + g.astype(np.int64)
            mem_id[g % 7 == 3] = -1                   # empty slots
            for i in range(3, R, 16):
                mem_id[Sm[i].argmax()] = ids[i, 1]    # the row's best slot holds its positive's video
            c.update(M=R, Mem=Mem, Lm=(Sm / SU).astype(np.int64), mem_id=mem_id, mem_col=B, span=B + R, mem_bias=None)
        if kind == "mixed":
            N = np.zeros((R, D))
            N[g[q == 0], k[q == 0]] = 5 * SU
            U = A @ N.T
            nid = 200000 + g.astype(np.int64)
            for i in range(9, R, 16):
                nid[k[i]] = ids[i, 0]                 # (the layer-0 negative of the pair's coordinate)
            c.update(N=N, U=(U / SU).astype(np.int64), nid=nid, neg_col=B, mem_col=2 * B, span=2 * B, lq=None)
        return _finish(c)
    return xs.cached(("npair", "chain", kind, B, world), make)


def chain_de(c, m):
    """per rank the gradient rows the chain must write, from the model's W: dA = W [P; N], dP = W_p^T A (dp: the ranks'
    partials summed in rank order), dN = W_n^T A -- every term a multiple of 2^-5 / B-scale granules far below 2^24, so
    any product order gives these bits; interleaved as the embedded rows are (a, p[, n] per pair)"""
    B, world, G = c["B"], c["world"], c["G"]
    A, P, N = c["A"], c["P"], c.get("N")
    out, parts = [], []
    for r in range(world):
        rows = slice(r * B, (r + 1) * B)
        W = np.where(np.isnan(m["W"][r]), 0.0, m["W"][r])
        gran = float(scale_f32(c)) / 2
        for X in (np.abs(W[:, :G]) @ np.abs(P), np.abs(W[:, :G]).T @ np.abs(A[rows])):
            assert X.max() / gran < 2 ** 24 and np.array_equal(np.round(X / gran), X / gran)
        dA = W[:, :G] @ P
        if N is not None:
            dA = dA + W[:, c["neg_col"]:c["neg_col"] + B] @ N
        if "Mem" in c:                               # (the ring's rows enter dA and get no gradient of their own)
            dA = dA + W[:, c["mem_col"]:c["mem_col"] + c["M"]] @ c["Mem"]
        parts.append(W[:, :G].T @ A[rows])
        out.append([dA, None] + ([W[:, c["neg_col"]:c["neg_col"] + B].T @ A[rows]] if N is not None else []))
    for r in range(world):
        acc = parts[0][r * B:(r + 1) * B].copy()
        for s in range(1, world):
            acc = acc + parts[s][r * B:(r + 1) * B]
        out[r][1] = acc
    res = []
    for blocks in out:
        de = np.empty((len(blocks) * B, CHAIN_D))
        for n, b in enumerate(blocks):
            de[n::len(blocks)] = b
        res.append(de + 0.0)                         # (a sum of -0 products is +0 in an accumulator that starts at +0)
    return res


def chain_rows(c, rank=0):
    """the embedded rows e fp32 [2B | 3B][64] of rank ``rank`` (a, p[, n] per pair) and their ids int32, as tensors"""
    B = c["B"]
    rows = slice(rank * B, (rank + 1) * B)
    blocks = [c["A"][rows], c["P"][rows]] + ([c["N"][rows]] if "N" in c else [])
    e = np.empty((len(blocks) * B, CHAIN_D))
    for n, b in enumerate(blocks):
        e[n::len(blocks)] = b
    cols = [c["ids"][rows, 0], c["ids"][rows, 1]] + ([c["nid"][rows]] if "N" in c else [])
    return xg.f32_exact(e), torch.from_numpy(np.stack(cols, 1).reshape(-1).astype(np.int32))
