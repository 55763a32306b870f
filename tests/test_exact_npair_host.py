"""The exact-arithmetic N-pair tests' own footing (tests/exact_npair.py), checked without a GPU on the very cases
tests/test_gpu_exact_npair.py launches:

* exactness -- every committed case has passed ``assert_npair_exact_safe`` (and the check refuses what it must);
* the model IS the existing specification: on the same ladder cases (embeddings A = S, P = the identity, so <a_i, p_j> =
  S_ij) it agrees with npair_ref, npair_logq_ref, npair_memory_ref, npair_mixed_ref and npair_dp_ref to fp64 accuracy;
* sensitivity -- every rule of ``exact_npair.RULES``, switched on, changes the expected lse, W or stats of at least one
  committed case of EVERY entry point it concerns (for a grad entry point as an error of the W kernel alone: the lse it
  is given stays the right one);
* the builders' promises: the winners' placement schedule, the decoys, the bias slots giving three different winners;
* the tie cases have s == n in the model.

Coverage: every template instantiation of the N-pair kernels and the cases (``exact_npair.all_cases(chain)``) that launch
it from tests/test_gpu_exact_npair.py --

  k_npair_rows<MEM=0, BIAS=0>          inbatch (npair_stats)          B in {1, 3, 6, 260, 1030}, ids and ids = None
  k_npair_rows<0, 1>                   logq (npair_logq_stats)        the same shapes
  k_npair_rows<1, 0>                   memory (npair_memory_stats)    B in {6, 260} x M in {4, 1028}
  k_npair_rows<1, 1>                   memory_logq (npair_memory_logq_stats)
  k_npair_cols<BIAS=0, 2> + k_npair_col_fold<0>   inbatch, memory, symmetric (B = 260: two chunks, 1030: five)
  k_npair_cols<1, 2> + k_npair_col_fold<1>        logq, memory_logq, symmetric
  k_npair_cols<0, 3> + k_npair_col_fold<0>        mixed, symmetric (B in {4, 260, 1028})
  k_npair_cols<1, 3> + k_npair_col_fold<1>        mixed_lq, mixed_nb, symmetric
  k_npair_stats                        inbatch, logq (M = 0), memory, memory_logq (M > 0); B = 1030: a second pass of step_scalars
  k_npair_w<kWF32 | kWX3 | kWBf16, BIAS=0>        inbatch and memory (npair_grad_f32 / _x3 / _bf16); B % 4 tails at 1, 3, 6, 1030
  k_npair_w<kWF32 | kWX3 | kWBf16, 1>             logq and memory_logq (npair_logq_grad_*)
  k_npair_mem_w<kWF32 | kWX3 | kWBf16, 0>         memory (npair_memory_grad_*); M = 1028: a second blockIdx.y
  k_npair_mem_w<kWF32 | kWX3 | kWBf16, 1>         memory_logq (npair_memory_logq_grad_*)
  k_mixed_rows<MEM=0, BIAS=0>          mixed, M = 0         k_mixed_rows<1, 0>          mixed, M in {4, 1028}
  k_mixed_rows<0, 1, NB=0>             mixed_lq, M = 0      k_mixed_rows<1, 1, 0>       mixed_lq, M in {4, 1028}
  k_mixed_rows<0, 1, 1>                mixed_nb, M = 0      k_mixed_rows<1, 1, 1>       mixed_nb, M in {4, 1028}
  k_mixed_stats                        every mixed case
  k_mixed_w<kWF32 | kWX3, MEM, BIAS, NB>          the same six (MEM, BIAS, NB) as k_mixed_rows, both formats
  k_npdp_rows, k_npdp_cols, k_npdp_colpart        dp (npair_dp_local_stats), world = 3, B in {4, 260}, G = 3 B and G = 16 > 3 B
  k_npdp_col_fold                      dp (npair_dp_col_fold): three ranks' partials, one of them empty (B = 4)
  k_npdp_stats                         dp (npair_dp_stats), every rank
  k_npdp_w<kWF32 | kWX3>               dp (npair_dp_grad_f32 / _x3), every rank
  k_npdp_pos_fold                      test_gpu_exact_npair.py::test_dp_pos_fold_rank_order (dyadic partials, three ranks)

  the chains (``exact_npair.chain_case``: embeddings whose scores are a ladder; de element by element)
    ops.npair_loss, f32 | f32x3 | bf16          test_chain_inbatch, test_chain_memory (B = 256, D = 64, M = 256; the push checked)
    ops.npair_mixed_loss, f32 | f32x3           test_chain_mixed (B = 256: dN included; no ring, no correction)
    ops.npair_dp_phase1 / 2 / 3, f32 | f32x3    test_chain_dp (world = 3; B = 64 on f32, 256 on f32x3: the facade's tile)

(k_npair_mem_push, k_mixed_split and the logQ gathers move data; their footprint and value tests are elsewhere.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_npair as xn  # noqa: E402
import npair_dp_ref  # noqa: E402
import npair_logq_ref  # noqa: E402
import npair_memory_ref  # noqa: E402
import npair_mixed_ref  # noqa: E402
import npair_ref  # noqa: E402

TOL = dict(rtol=1e-12, atol=1e-12)


def _cases(chain):
    return xn.all_cases(chain)


# ---- exactness ---------------------------------------------------------------------------------------------------------
def test_every_case_is_exact_safe():
    n = 0
    for chain in xn.CHAINS:
        for c in _cases(chain):
            assert 0 < c["safe"] < 2 ** 24, c["name"]
            n += 1
    for c in xn.tie_cases():
        assert 0 <= c["safe"] < 2 ** 24                        # (n = B: every logit is 0)
    assert n >= 60
    c = xn.inbatch_case(6, False)
    L = c["L"].copy()
    L[0, 3] = L[0].max()                                        # a second winner in row 0 is refused
    with pytest.raises(AssertionError):
        xn.assert_npair_exact_safe(dict(c, L=L))
    with pytest.raises(AssertionError):                        # a level that is no integer: a logit off the ladder
        xn.assert_npair_exact_safe(dict(c, L=c["L"] + 0.5))
    with pytest.raises(AssertionError):                        # logits beyond 2^24
        xn.assert_npair_exact_safe(dict(c, L=c["L"] * (1 << 18)))


def test_every_inbatch_shape_comes_with_and_without_ids():
    for chain in ("inbatch", "logq"):
        got = {(c["B"], c["ids"] is not None) for c in _cases(chain)}
        assert got == {(B, w) for B in xn.INBATCH_B for w in (True, False)}


# ---- the model against the fp64 references -----------------------------------------------------------------------------
def _quotients(c, m, r, symmetric):
    """stats[0..3] in fp64 from the model's integer sums"""
    t0, t1, t2, t3, t4 = (float(x) for x in m["t"][r]["t"])
    B, G, M = c["B"], c["G"], c["M"]
    den = B * (G - 1) if c["chain"] == "dp" else B * (B - 1) + B * M + (B * B if c["chain"].startswith("mixed") else 0)
    return np.array([0.5 * (t0 / B + t4 / B) if symmetric else t0 / B, t1 / B, t2 / t3 if t3 else 0.0, t3 / den if den else 0.0])


def _embed(c):
    """A = the rows of S over all blocks, P / N / mem = the unit rows that pick the blocks' columns"""
    B, M = c["B"], c["M"]
    blocks = [c["L"] * float(xn.SU)] + ([c["U"] * float(xn.SU)] if c.get("U") is not None else []) \
        + ([c["Lm"] * float(xn.SU)] if M else [])
    A = np.concatenate(blocks, 1)
    eye = np.eye(A.shape[1])
    P, rest = eye[:B], eye[B:]
    N = rest[:B] if c.get("U") is not None else None
    mem = rest[-M:] if M else None
    return A, P, N, mem


def _flat(a, scale=1.0):
    return None if a is None else np.asarray(a, np.float64).reshape(-1) * scale


@pytest.mark.parametrize("symmetric", (False, True))
@pytest.mark.parametrize("chain", [ch for ch in xn.CHAINS if ch != "dp"])
def test_model_agrees_with_the_fp64_references(chain, symmetric):
    for c in _cases(chain):
        if c["B"] > 300 and not symmetric:
            continue                                            # (the largest shapes: the setting with both terms)
        A, P, N, mem = _embed(c)
        ids = None if c["ids"] is None else c["ids"].reshape(-1)
        bias, mb = _flat(c["bias"], xn.LV), _flat(c.get("mem_bias"), xn.LV)
        if chain == "inbatch":
            ref = npair_ref.npair(A, P, ids, xn.T, symmetric)
        elif chain == "logq":
            ref = npair_logq_ref.npair_logq(A, P, ids, bias, xn.T, symmetric)
        elif chain == "memory":
            ref = npair_memory_ref.npair_memory(A, P, ids, mem, c["mem_id"], xn.T, symmetric)
        elif chain == "memory_logq":
            ref = npair_logq_ref.npair_logq(A, P, ids, bias, xn.T, symmetric, mem=mem, mem_id=c["mem_id"], mem_bias=mb)
        else:
            ids3 = None if ids is None else np.stack([c["ids"][:, 0], c["ids"][:, 1], c["nid"]], 1).reshape(-1)
            lq, Nn = c.get("lq"), N
            if chain == "mixed_nb":                             # (the reference has the scalar only: the vector folded into U)
                A = A.copy()
                A[:, c["B"]:2 * c["B"]] -= lq[None, :] * float(xn.SU)
                lq = 0
            ref = npair_mixed_ref.npair_mixed(A, P, Nn, ids3, xn.T, symmetric, mem=mem, mem_id=c.get("mem_id"), bias=bias,
                                              lq_u=0.0 if lq is None else float(lq) * xn.LV, mem_bias=mb)
        m = xn.model(c, symmetric)
        B, M = c["B"], c["M"]
        assert np.allclose(m["lse_row"][0], ref["lse_row"], **TOL), c["name"]
        if symmetric:
            assert np.allclose(m["lse_col"], ref["lse_col"], **TOL), c["name"]
        un = c["B"] * xn.T                                      # (the model carries the host's fp32 scale 1 / (B t): compared without it)
        W = m["W"][0] / float(xn.scale_f32(c))
        assert np.allclose(W[:, :B], ref["W"] * un, **TOL), c["name"]
        if c.get("U") is not None:
            assert np.allclose(W[:, c["neg_col"]:c["neg_col"] + B], ref["W_n"] * un, **TOL), c["name"]
        if M:
            assert np.allclose(W[:, c["mem_col"]:], ref["W_mem"] * un, **TOL), c["name"]
        q = _quotients(c, m, 0, symmetric)
        keep = [0, 1, 3] if chain == "mixed_nb" else [0, 1, 2, 3]          # (stats[2] reads U itself, not U less its bias)
        assert np.allclose(q[keep], ref["stats"][keep], **TOL), (c["name"], q, ref["stats"])
        st = m["stats"][0].astype(np.float64)
        assert np.allclose(st, q, rtol=2.0 ** -23, atol=0), c["name"]      # (the fp32 quotients: one or two roundings)


@pytest.mark.parametrize("symmetric", (False, True))
def test_dp_model_agrees_with_the_fp64_reference(symmetric):
    for c in _cases("dp"):
        if c["G"] != c["world"] * c["B"] or c["ids"] is None:
            continue                                            # (the reference has no padding columns and needs ids)
        A = c["L"] * float(xn.SU)
        ref = npair_dp_ref.npair_dp(A, np.eye(c["G"]), c["ids"].reshape(-1), c["world"], xn.T, symmetric)
        m = xn.model(c, symmetric)
        if symmetric:
            assert np.allclose(m["lse_col"], ref["lse_col"], **TOL)
        for r in range(c["world"]):
            assert np.allclose(m["lse_row"][r], ref["lse_row"][r], **TOL)
            assert np.array_equal(m["colpart"][r], ref["colpart"][r]), c["name"]
            assert np.allclose(m["W"][r] / float(xn.scale_f32(c)), ref["W"][r] * c["B"] * xn.T, **TOL)
            assert np.allclose(_quotients(c, m, r, symmetric), ref["stats"][r], **TOL)


# ---- sensitivity -------------------------------------------------------------------------------------------------------
def test_every_rule_belongs_to_an_entry_point():
    used = {r for rules in xn.RULES_OF.values() for r in rules}
    assert used == set(xn.RULES)
    assert set(xn.RULES_OF) == set(xn.CHAINS_OF) == set(xn.OUTPUTS_OF)


def _seen(entry, rule):
    w_only = entry.endswith("grad") or entry.endswith("grad_nb")
    cases = [c for chain in xn.CHAINS_OF[entry] for c in _cases(chain)]
    for c in sorted(cases, key=lambda c: abs(c["B"] - 260) + (c["ids"] is None)):      # (the mid-sized cases with ids first)
        for symmetric in (True, False):
            base = xn.model(c, symmetric)
            mut = xn.model(c, symmetric, (rule,), lse_rule=() if w_only else None)
            if xn.differs(xn.entry_output(mut, entry), xn.entry_output(base, entry)):
                return c["name"], symmetric
    return None


@pytest.mark.parametrize("entry", sorted(xn.RULES_OF))
def test_every_rule_changes_every_entry_point_it_concerns(entry):
    """a rule no committed case sees is a failed test"""
    for rule in xn.RULES_OF[entry]:
        hit = _seen(entry, rule)
        assert hit is not None, "%s: no committed case sees the rule %r" % (entry, rule)
        print("%-26s %-22s seen by %s (symmetric=%s)" % (entry, rule, hit[0], hit[1]))


# ---- the builders' promises --------------------------------------------------------------------------------------------
def test_schedule_and_decoys():
    kinds = {}
    for chain in xn.CHAINS:
        for c in _cases(chain):
            xn.assert_schedule(c)
            kinds.setdefault(chain, set()).update(xn.assert_decoys(c))
    inb = {"ad", "b", "c"}
    mem = {"mem_empty", "mem_a", "mem_p"}
    uni = {"uni_da", "uni_dp", "uni_diag"}
    for chain in xn.CHAINS:
        want = inb | (mem if "memory" in chain else set()) | ((mem | uni) if chain.startswith("mixed") else set())
        assert want <= kinds[chain], (chain, sorted(want - kinds[chain]))
    for c in _cases("inbatch"):                                 # the pair with id(a) == id(p): its diagonal wins its row
        if c["ids"] is not None:
            e = c["roles"]["e"]
            assert c["ids"][e, 0] == c["ids"][e, 1] and xn.winners(c)[e] == ("in", e)


def test_bias_slots_give_three_winners():
    for chain in ("logq", "memory_logq", "mixed_lq", "mixed_nb"):
        for c in _cases(chain):
            b = c["bias"]
            assert (b[:, 0] != b[:, 1]).all()
            if c["M"]:
                mb = c["mem_bias"]
                assert (mb[1:] != mb[:-1]).all()
            if chain == "mixed_nb":
                assert len(set(c["lq"].tolist())) == min(3, c["B"]) and (c["lq"][1:] != c["lq"][:-1]).all()
            if c["B"] >= 6:
                raw, wrong = xn.bias_winner_shares(c)
                lost = 8.0 / c["B"]                             # (rows whose winner is a ring slot, a uniform column or a decoy)
                assert raw >= 0.5 - lost and wrong >= 0.5 - lost, (c["name"], raw, wrong)
    for c in _cases("logq"):
        if c["B"] >= 6:
            assert min(xn.bias_winner_shares(c)) >= 0.5, c["name"]


def test_tie_cases_have_s_equal_n():
    for c in xn.tie_cases():
        m = xn.model(c, True)
        n = c["tie"]
        assert (m["n_row"][0] == n).all() and (m["n_col"] == n).all()
        assert np.array_equal(m["colpart"][0][:, 1], np.full(c["B"], float(n)))
        assert np.allclose(m["lse_row"][0], np.log(n), rtol=1e-15)
        ref = npair_ref.npair(c["L"] * float(xn.SU), np.eye(c["B"]), None, xn.T, True)
        assert np.allclose(m["W"][0] / float(xn.scale_f32(c)), ref["W"] * c["B"] * xn.T, **TOL) and np.allclose(m["lse_col"], ref["lse_col"], **TOL)


# ---- the chain cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,world", (("inbatch", 256, 1), ("memory", 256, 1), ("mixed", 256, 1), ("dp", 64, 3), ("dp", 256, 3)))
def test_chain_cases_land_on_the_ladder(kind, B, world):
    """the embeddings' scores ARE the case's ladder, the rows are exact in one bf16 plane, and the expected gradient rows
    are fp32 numbers that the fp64 references give from the embeddings themselves"""
    import torch
    import exact_gemm as xg
    c = xn.chain_case(kind, B, world)
    assert 0 < c["safe"] < 2 ** 24
    A, P, ids = c["A"], c["P"], c["ids"].reshape(-1)
    assert np.array_equal(A @ P.T, c["L"] * float(xn.SU))
    for X in [A, P] + [c[k] for k in ("N", "Mem") if k in c]:
        t = xg.f32_exact(X)
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    for symmetric in (False, True):
        m = xn.model(c, symmetric)
        de = xn.chain_de(c, m)
        for d in de:
            xg.f32_exact(d)
        if kind == "inbatch":
            ref = npair_ref.npair(A, P, ids, xn.T, symmetric)
            want = [npair_ref.interleave(ref["dA"], ref["dP"])]
        elif kind == "memory":
            ref = npair_memory_ref.npair_memory(A, P, ids, c["Mem"], c["mem_id"], xn.T, symmetric)
            want = [npair_ref.interleave(ref["dA"], ref["dP"])]
        elif kind == "mixed":
            ids3 = np.stack([c["ids"][:, 0], c["ids"][:, 1], c["nid"]], 1).reshape(-1)
            ref = npair_mixed_ref.npair_mixed(A, P, c["N"], ids3, xn.T, symmetric)
            want = [npair_mixed_ref.interleave3(ref["dA"], ref["dP"], ref["dN"])]
        else:
            ref = npair_dp_ref.npair_dp(A, P, ids, world, xn.T, symmetric)
            want = [npair_ref.interleave(a, p) for a, p in zip(ref["dA"], ref["dP"])]
        for got, w in zip(de, want):
            assert np.allclose(got, w, **TOL), (c["name"], symmetric)
