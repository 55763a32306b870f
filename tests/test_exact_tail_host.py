"""The exact-arithmetic tail tests' own footing (tests/exact_tail.py), checked without a GPU on the very cases
tests/test_gpu_exact_tail.py launches:

* exactness -- every case has passed ``assert_tail_exact_safe`` (and the check refuses what it must); pos, neg and <z, g>
  recomputed in float32 forward, reversed and 64-lane strided with a shuffle tree give the same bits;
* the models ARE the existing specification: on the same values the default model equals oracle.tower (l2_normalize,
  hinge_loss / hinge_loss_indexed and their backward, l2_normalize_backward, leaky_relu_backward, calc_var) in float64 with
  ``np.array_equal`` -- the oracle stays the specification, the models add none;
* sensitivity -- every single mutation of a rule (exact_tail.RULES) changes the expectation of at least one committed case
  of every entry point and copy format it applies to: the GPU comparison can fail;
* the planted classes, counted per entry point."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_tail as xt  # noqa: E402

from oracle import tower as otower  # noqa: E402

ENTRIES = ("hinge", "inbatch", "tail0", "tail1", "indexed", "indexed_tail")


def cases_of(entry):
    return xt.all_cases("indexed" if entry == "indexed_tail" else entry)


def exact_cases(entry):
    return [c for c in cases_of(entry) if not c.get("inexact")]


# ---- exactness -----------------------------------------------------------------------------------------------------------------
def test_every_case_is_exact_safe():
    """no case without the check; the bound is 2^24 granules, derived in assert_tail_exact_safe"""
    worst = 0.0
    for entry in ("l2norm_bwd",) + ENTRIES:
        for c in cases_of(entry):
            assert 0 < c["safe"] < 2.0 ** 24, c["name"]
            worst = max(worst, c["safe"])
    for M in xt.EW_M:
        for N in xt.EW_N:
            assert 0 < xt.ew_case(M, N)["safe"] < 2.0 ** 24
    assert worst < 2.0 ** 15                                   # (far from the limit: 17 408 granules, the 16 384-triplet hub sums)
    c = dict(xt.hinge_case(8, 64))
    for bad in (1.0 / 3.0, 1.0 + 2.0 ** -30):                   # a row off the grid / not an fp32 number is refused
        z = c["z"].copy()
        z[4, 3] = bad
        with pytest.raises(AssertionError):
            xt.assert_tail_exact_safe(dict(c, z=z))
    z = c["z"].copy()                                           # 2^24 granules are refused: 1 and 2^-13 in one reduction (ss)
    z[0] = 0.0
    z[0, :2] = (1.0, 2.0 ** -13)
    with pytest.raises(AssertionError):
        xt.assert_tail_exact_safe(dict(c, z=z))


def _same_bits(forms, want, what):
    w = np.asarray(want, np.float64).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), want), "%s: the expectation is no fp32 number" % what
    for i, f in enumerate(forms):
        assert f.dtype == np.float32 and np.array_equal(f.view(np.int32), w.view(np.int32)), "%s: order %d differs" % (what, i)


@pytest.mark.parametrize("entry", ("hinge", "inbatch", "tail0", "tail1", "indexed"))
def test_reductions_are_order_independent_in_fp32(entry):
    """pos, neg and <z, g> in float32, three summation orders: the bits of the float64 model (on a "tiny" case: the
    triplets and rows no tiny row enters; on a non-power-of-two batch: pos and neg, the gradient is rounded there)"""
    for c in cases_of(entry):
        if c["B"] > 2048:
            continue                                            # (the two long cases: the same rows as the others, drawn from one pool)
        m = xt.tail_model(c, xt.ALPHA_DYADIC)
        e, tri = m["e"], m["tri"]
        ok_t, ok_r = ~m["dirty_t"], ~m["dirty"]
        a, p, n = e[tri[:, 0]], e[tri[:, 1]], e[tri[:, 2]]
        _same_bits(xt.sum_orders_f32(((a - p) ** 2)[ok_t]), m["pos"][ok_t], c["name"] + " pos")
        _same_bits(xt.sum_orders_f32(((a - n) ** 2)[ok_t]), m["neg"][ok_t], c["name"] + " neg")
        if c.get("inexact") != "npow2":
            zg = (c["z"] * m["de"]).sum(1)
            _same_bits(xt.sum_orders_f32((c["z"] * m["de"])[ok_r]), zg[ok_r], c["name"] + " <z, g>")


def test_rows_cases_are_order_independent_in_fp32():
    for c in xt.all_cases("l2norm_bwd"):
        ok = ~c["tiny_rows"]
        _same_bits(xt.sum_orders_f32((c["z"] ** 2)[ok]), (c["z"] ** 2).sum(1)[ok], c["name"] + " ss")
        _same_bits(xt.sum_orders_f32((c["z"] * c["g"])[ok]), (c["z"] * c["g"]).sum(1)[ok], c["name"] + " <z, g>")


# ---- the models are the oracle ---------------------------------------------------------------------------------------------------
def _oracle_triplets(c, m):
    if c["kind"] == "idx":
        tri, valid = otower.semihard_triplets(c["neg_row"])
        return tri.astype(np.int64), valid
    return m["tri"], m["valid"]


@pytest.mark.parametrize("entry", ("hinge", "inbatch", "tail0", "tail1", "indexed"))
def test_default_model_equals_the_oracle(entry):
    """float64 throughout, ``np.array_equal``.  Two places where the oracle's float64 is finer than one fp32 operation, both
    on clamped rows only: its inv there is 1 / sqrt(1e-12) in float64 (the model's: the fp32 constant's), and its inv g is
    unrounded -- rounded once to fp32 it is the model's value.  A masked triplet's negative is a placeholder on both sides
    (row 0 in oracle.tower.semihard_triplets, the own anchor in the kernel): its neg is not compared, its hinge and
    gradient (both 0) are."""
    for c in exact_cases(entry):
        z = c["z"]
        for alpha in (-1.0, xt.ALPHA_DYADIC):
            m = xt.tail_model(c, alpha)
            e64, inv64 = otower.l2_normalize(z, np.float64)
            live = ~m["clamped"]
            assert np.array_equal(e64, m["e"]) and np.array_equal(inv64[live, 0], m["inv"][live]), c["name"]
            assert np.allclose(inv64[~live, 0], m["inv"][~live], rtol=2.0 ** -23, atol=0)
            tri, valid = _oracle_triplets(c, m)
            w = otower.hinge_loss_indexed(e64, tri, valid, c["margin"], np.float64)
            assert np.array_equal(w["pos_dist"], m["pos"]) and np.array_equal(w["hinge_dist"], m["hinge"]), c["name"]
            assert np.array_equal(w["neg_dist"][valid], m["neg"][valid])
            assert np.array_equal(valid, m["valid"])
            if c["kind"] == "m0":
                wh = otower.hinge_loss(e64[tri], c["margin"], np.float64)
                assert np.array_equal(wh["hinge_dist"][:, 0], m["hinge"]) and np.array_equal(wh["pos_dist"][:, 0], m["pos"])
                dE = np.zeros_like(e64)
                dE[tri.ravel()] = otower.hinge_loss_backward(e64[tri], c["margin"], np.float64).reshape(-1, e64.shape[1])
                assert np.array_equal(dE, otower.hinge_loss_indexed_backward(e64, tri, valid, c["margin"], np.float64))
            else:
                dE = otower.hinge_loss_indexed_backward(e64, tri, valid, c["margin"], np.float64)
            assert np.array_equal(dE, m["de"]), c["name"]
            if (c["B"] & (c["B"] - 1)) == 0:
                assert float(w["hinge_loss"]) == float(m["stats"][0]), c["name"]
                assert float(np.mean(w["hinge_dist"] > 0)) == float(m["stats"][3])
            dz = otower.l2_normalize_backward(z, m["inv"][:, None], dE, np.float64)
            assert xt.is_f32(dz[live])
            if alpha >= 0:
                dz = otower.leaky_relu_backward(z, xt.r32(dz), alpha)
            assert np.array_equal(xt.r32(dz), m["dz2"]), c["name"]
            if c["kind"] != "idx":                              # (the indexed entry points have no variance summary)
                assert otower.calc_var(e64[tri], np.float64) == m["var"]


def test_rows_model_equals_the_oracle():
    for c in xt.all_cases("l2norm_bwd"):
        z, g = c["z"], c["g"]
        e, inv, ss, clamped = xt.normalize(z)
        e64, inv64 = otower.l2_normalize(z, np.float64)
        ok = ~c["tiny_rows"]
        assert np.array_equal(e64[ok], e[ok]) and np.array_equal(inv64[~clamped, 0], inv[~clamped])
        reg = ss == 4.0 ** c["s"]                               # the scaled unit rows: |z|^2 = 4^s, inv = 2^-s (the control row: 2^19)
        assert reg.sum() >= len(z) - 3 and np.array_equal(inv[reg], 2.0 ** -c["s"][reg].astype(np.float64))
        if len(z) >= 5:
            assert clamped[1] and clamped[2] and not clamped[3] and inv[3] == 2.0 ** 19
        for alpha in (-1.0, xt.ALPHA_DYADIC):
            d, _ = xt.l2norm_bwd_model(z, g, alpha)
            dz = otower.l2_normalize_backward(z, inv[:, None], g, np.float64)
            if alpha >= 0:
                dz = otower.leaky_relu_backward(z, xt.r32(dz), alpha)
            assert np.array_equal(xt.r32(dz), d), c["name"]


def test_lrelu_alpha_is_the_reference_default():
    assert xt.ALPHA_REF == otower.LRELU_ALPHA and float(xt.EPS) == float(np.float32(otower.L2_EPS))
    # 1 / sqrt(1e-12f): the fp32 constant sits 4e-21 below 1e-12, the quotient rounds to 10^6 exactly
    assert float(xt.INV_C_MODEL) == 1.0e6


# ---- sensitivity: the mutation table ----------------------------------------------------------------------------------------------
def _planes_differ(d0, d1, kind):
    a, b = torch.from_numpy(d0.astype(np.float32)), torch.from_numpy(d1.astype(np.float32))
    if kind == "h2":
        a, b = (a * xt.H2_SCALE).clamp(-65504.0, 65504.0), (b * xt.H2_SCALE).clamp(-65504.0, 65504.0)
        pa, pb = xg.split_planes(a, 2, torch.float16), xg.split_planes(b, 2, torch.float16)
    else:
        n = 1 if kind == "bf16" else 3
        pa, pb = xg.split_planes(a, n), xg.split_planes(b, n)
    return any(not torch.equal(xg.bits(x), xg.bits(y)) for x, y in zip(pa, pb))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_mutation_is_seen(entry):
    """each rule of exact_tail.RULES_OF[entry], switched alone, changes the expected output of some committed case -- beyond
    the two bounds where a case has any -- and, for the entries that write copies of dz2, the bits of every copy format"""
    tail = entry in ("tail0", "tail1", "indexed_tail")
    formats = {"tail0": ("bf16", "x3", "h2"), "tail1": ("bf16", "x3", "h2"), "indexed_tail": ("bf16", "x3")}.get(entry, ())
    cases = cases_of(entry)
    base = [xt.tail_model(c, xt.ALPHA_DYADIC, tail=tail) for c in cases]
    for rule in xt.RULES_OF[entry]:
        seen, seen_fmt = [], {f: False for f in formats}
        for c, m0 in zip(cases, base):
            m1 = xt.tail_model(c, xt.ALPHA_DYADIC, rule=(rule,), tail=tail)
            if xt.differs(m0, m1):
                seen.append(c["name"])
                if tail and bool((np.abs(m0["dz2"] - m1["dz2"]) > m0["dz2_tol"] + m1["dz2_tol"]).any()) and not c.get("inexact"):
                    for f in formats:
                        seen_fmt[f] = seen_fmt[f] or _planes_differ(m0["dz2"], m1["dz2"], f)
        assert seen, "no committed case of %s sees the mutation %s" % (entry, rule)
        # (count_ge and invalid_reports change hinge and stats[3] only, not dz2; clamp_keeps_proj is seen by the "tiny" cases
        # only, whose copies are compared with those of the device's own dz2)
        if rule not in ("clamp_keeps_proj", "count_ge", "invalid_reports"):
            assert all(seen_fmt.values()), "mutation %s of %s: no exact case changes the copy formats %s" % (
                rule, entry, [f for f, v in seen_fmt.items() if not v])


def test_every_mutation_of_the_row_kernels_is_seen():
    for rule in xt.RULES_OF["l2norm_bwd"]:
        hit = False
        for c in xt.all_cases("l2norm_bwd"):
            d0, t0 = xt.l2norm_bwd_model(c["z"], c["g"], xt.ALPHA_DYADIC)
            d1, t1 = xt.l2norm_bwd_model(c["z"], c["g"], xt.ALPHA_DYADIC, rule=(rule,))
            hit = hit or not np.array_equal(d0, d1)
        assert hit, rule
    for M in xt.EW_M:                                           # lrelu' at +-0 under a non-zero gradient, every elementwise kernel
        for N in xt.EW_N:
            c = xt.ew_case(M, N)
            zero = (c["a"] == 0) & (c["g"] != 0)
            assert zero.any() and np.signbit(c["a"][zero]).any() and (~np.signbit(c["a"][zero])).any(), c["name"]
            assert not np.array_equal(xt.lrelu_bwd_model(c["g"], c["a"], 0.25), xt.lrelu_bwd_model(c["g"], c["a"], 0.25, rule=("lrelu_ge",)))
            for res in (0, 1):
                x0, x1 = xt.ew_fusion_bwd_model(res, c["g"], c["a"], c["b"], 0.25), xt.ew_fusion_bwd_model(res, c["g"], c["a"], c["b"], 0.25, ("lrelu_ge",))
                if res or N > 4 or M > 1:
                    assert not np.array_equal(x0[0], x1[0]) or not np.array_equal(x0[1], x1[1])


# ---- the planted classes ------------------------------------------------------------------------------------------------------------
def class_counts(entry):
    """{class: number of committed cases of ``entry`` that carry it}"""
    out = {}
    for c in cases_of(entry):
        for k, v in c["classes"].items():
            out[k] = out.get(k, 0) + (len(v) > 0)
    return out


def test_planted_classes_are_present():
    """per entry point every class of the issue in at least one committed case (the builders assert the per-case counts);
    the corner triplets have hinge 0, are not counted active and have non-zero gradient rows"""
    want = {"hinge": ("corner", "plus", "minus", "inactive", "active", "zero_a", "zero_p", "zero_n"),
            "tail0": ("corner", "plus", "minus", "inactive", "active", "zero_a", "zero_p", "zero_n"),
            "inbatch": ("corner", "plus", "minus", "inv_va", "inv_vp", "valid_i_only", "valid_k_only", "both_terms", "second_only"),
            "tail1": ("corner", "plus", "minus", "inv_va", "inv_vp", "valid_i_only", "valid_k_only", "both_terms", "second_only"),
            "indexed": ("corner", "plus", "minus", "masked", "own_anchor", "own_positive", "last_row", "hub_hit", "hub_inactive", "wave4")}
    for entry, names in want.items():
        n = class_counts(entry)
        for k in names:
            assert n.get(k, 0) >= 1, "%s: no case carries class %s" % (entry, k)
        for c in cases_of(entry):
            m = xt.tail_model(c, tail=False)
            for i in c["classes"]["corner"]:
                assert m["hinge"][i] == 0 and m["scale"][i] > 0 and np.abs(m["de"][m["tri"][i, 0]]).max() + np.abs(m["de"][m["tri"][i, 1]]).max() > 0
    big = xt.hinge_case(64, 64)["classes"]
    assert len(big["corner"]) >= 4 and len(big["plus"]) >= 2 and len(big["minus"]) >= 2
    shifts = {(c["B"], c["shift"]) for c in cases_of("inbatch")}
    assert (2, 1) in shifts and {(64, 1), (64, 32), (64, 63)} <= shifts
