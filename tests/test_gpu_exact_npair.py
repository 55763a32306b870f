"""The N-pair softmax family -- csrc/npair.hip, npair_common.h, npair_mixed.hip, npair_dp.hip, every W format, the logQ /
neg_bias instantiations -- against the integer model of tests/exact_npair.py at ZERO tolerance: the kernels are handed a
ladder of logits (S small integers, t = 2^-4, biases multiples of 128, one counted winner per row and column term with
everything else at least 128 below it), so lse, stats and every W entry are exact in any summation order and the rules
-- who counts for whom, which bias slot, where the diagonal sits on a rank, what ``symmetric`` halves, stats[3]'s
denominator, the scalar tail of the W store -- decide every bit.  tests/test_exact_npair_host.py shows on the same cases
that the expectation is the fp64 references' and that it changes under every single mutation of a rule.

The three identities the ladder rests on (expf(0) == 1, expf(x) == 0 for x <= -128, logf(1) == 0) are asserted first,
through the kernels.  Comparisons are ``torch.equal`` on bit patterns: lse and stats in poisoned buffers, W of every
format in poisoned buffers with ldw and plane larger than the span (an unwritten or overwritten cell fails too); every
launch runs twice and must give the same bits.  The W kernels are given the MODEL's lse, so an error of a W kernel alone
shows in W.  One chain test per precision then goes from embeddings (small integers in a few coordinates, exact in one bf16
plane, whose scores land on the ladder) through ops.npair_loss, ops.npair_mixed_loss and the three dp phases and compares
de = [W P ; W^T A] element by element.  The tie group (n equal winners) is the one toleranced part: see exact_npair's
docstring."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_npair as xn  # noqa: E402
import footprint as fp  # noqa: E402

pytestmark = pytest.mark.gpu

from cdml_amd import ops  # noqa: E402

F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16
T = xn.T


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


def _bits_equal(got, want, what):
    g, w = xg.bits(got.cpu()), xg.bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError("%s: %d cells differ, first at %s: got %r, want %r" % (what, bad.shape[0], first,
                                                                                   got.cpu()[first].item(), want[first].item()))


def _vec(n, dev):
    return fp.poisoned((n,), dtype=F32, device=dev)


def _want_vec(n, *parts):
    """a poisoned fp32 vector [n] with the float64 ``parts`` (exact fp32 numbers) from its start"""
    w = fp.poisoned((n,), dtype=F32, device="cpu")
    o = 0
    for p in parts:
        if p is not None:
            w[o:o + len(p)] = xg.f32_exact(p)
            o += len(p)
    return w


def _to(t, dev):
    return None if t is None else t.to(dev)


def _twice(run, check):
    """two launches on the same inputs into fresh poisoned outputs: both meet the expectation bit for bit"""
    for _ in range(2):
        check(run())


class Dev:
    """one case's operands on the device"""

    def __init__(self, c, dev, rank=0):
        assert 0 <= c["safe"] < 2 ** 24                       # no case without assert_npair_exact_safe
        self.c, self.dev = c, dev
        self.S = xn.s_matrix(c, rank).to(dev)
        self.ids = _to(xn.ids_tensor(c), dev)
        bias, mem_bias, lq = xn.bias_tensors(c)
        self.bias, self.mem_bias = _to(bias, dev), _to(mem_bias, dev)
        self.lq = lq.to(dev) if isinstance(lq, torch.Tensor) else (0.0 if lq is None else lq)
        self.mem_id = torch.from_numpy(c["mem_id"].astype(np.int32)).to(dev) if c["M"] else None


def _lse_in(c, m, symmetric, rank, dev):
    """the lse a W kernel is given: the model's (rows, then the columns with ``symmetric``; poison otherwise)"""
    if c["chain"] == "dp":
        return (xg.f32_exact(m["lse_row"][rank]).to(dev), xg.f32_exact(m["lse_col"]).to(dev) if symmetric else None)
    return _want_vec(2 * c["B"], m["lse_row"][0], m["lse_col"] if symmetric else None).to(dev)


def _check_w(c, d, fmt, symmetric, launches, W_model, cols, what):
    ldw, plane = xn.w_layout(c, fmt)
    want = xn.w_expected(c, fmt, W_model, cols)

    def run():
        buf = xn.w_buffer(c, fmt, d.dev)
        for launch in launches:
            launch(buf, plane)
        return buf
    _twice(run, lambda buf: _bits_equal(buf, want, "%s %s W %s symmetric=%s" % (c["name"], what, fmt, symmetric)))


# ---- the identities ------------------------------------------------------------------------------------------------------
def test_math_identities_through_the_kernels(dev):
    """expf(0) == 1 and logf(1) == 0: B = 1 gives lse[0] == S[0][0] / t; expf(x) == 0 for x <= -128: a two-column row
    whose second logit is 128 (and 256) below the first gives the first, bit for bit -- in the row pass, the column pass and W"""
    ws = torch.zeros(max(ops.npair_workspace(2), 16) // 4, dtype=F32, device=dev)
    for s in (0.0, 8.0, -24.0, 0.5, 3.0):
        S = torch.full((1, 4), s, dtype=F32, device=dev)
        lse, stats = _vec(2, dev), _vec(4, dev)
        ops.npair_stats(S, None, 1, T, True, lse, stats, ws)
        assert lse.cpu().tolist() == [s / T, s / T], "expf(0) == 1 / logf(1) == 0 fail on the device: %r" % (lse.cpu().tolist(),)
        assert stats.cpu().tolist() == [0.0, 2.0 - 2.0 * s, 0.0, 0.0]
    for gap in (8.0, 16.0):                                    # S / t apart by 128 | 256
        S = torch.zeros((2, 4), dtype=F32, device=dev)
        S[0, 0], S[0, 1], S[1, 0], S[1, 1] = 16.0, 16.0 - gap, 16.0 - 2 * gap, 16.0
        lse = _vec(4, dev)
        ops.npair_stats(S, None, 2, T, True, lse, _vec(4, dev), ws)
        assert lse.cpu().tolist() == [256.0] * 4, "expf(-%g) != 0 on the device: %r" % (gap / T, lse.cpu().tolist())
        W = fp.poisoned((2, 4), dtype=F32, device=dev)
        ops.npair_grad_f32(S, None, 2, T, False, lse, W)
        assert torch.equal(W[:, :2].cpu(), torch.zeros(2, 2)), W.cpu()     # (1 at the winner less 1 on the diagonal; 0 elsewhere)


# ---- in-batch, logQ, memory, memory + logQ -------------------------------------------------------------------------------
def _inbatch_like(chain):
    """the chain's cases, built when the test runs (xs.cached: the objects the host tests checked)"""
    return [pytest.param(spec, id="%s-%s" % (chain, "-".join(str(a) for a in spec[1]))) for spec in xn.case_specs(chain)]


@pytest.mark.parametrize("symmetric", (False, True))
@pytest.mark.parametrize("c", _inbatch_like("inbatch") + _inbatch_like("logq") + _inbatch_like("memory") + _inbatch_like("memory_logq"))
def test_inbatch_family(dev, c, symmetric):
    c = c[0](*c[1])
    d = Dev(c, dev)
    B, M = c["B"], c["M"]
    m = xn.model(c, symmetric)
    logq, mem = c["bias"] is not None, M > 0
    ws = torch.zeros(max((ops.npair_memory_workspace(B, M) if mem else ops.npair_workspace(B)), 16) // 4, dtype=F32, device=dev)
    want_lse = _want_vec(2 * B, m["lse_row"][0], m["lse_col"] if symmetric else None)
    want_stats = torch.from_numpy(m["stats"][0])

    def stats():
        lse, st = _vec(2 * B, dev), _vec(4, dev)
        if mem and logq:
            ops.npair_memory_logq_stats(d.S, d.ids, B, d.bias, c["mem_col"], d.mem_id, d.mem_bias, T, symmetric, lse, st, ws)
        elif mem:
            ops.npair_memory_stats(d.S, d.ids, B, c["mem_col"], d.mem_id, T, symmetric, lse, st, ws)
        elif logq:
            ops.npair_logq_stats(d.S, d.ids, B, d.bias, T, symmetric, lse, st, ws)
        else:
            ops.npair_stats(d.S, d.ids, B, T, symmetric, lse, st, ws)
        return lse, st

    def check(out):
        _bits_equal(out[0], want_lse, "%s lse symmetric=%s" % (c["name"], symmetric))
        _bits_equal(out[1], want_stats, "%s stats symmetric=%s" % (c["name"], symmetric))
    _twice(stats, check)

    lse = _lse_in(c, m, symmetric, 0, dev)
    cols_in = np.arange(c["span"]) < B
    for fmt in ("f32", "x3", "bf16"):
        def w_in(buf, plane, fmt=fmt):
            if fmt == "bf16":
                ops.npair_grad_bf16(d.S, d.ids, B, T, symmetric, lse, buf, bias=d.bias)
            elif logq:
                (ops.npair_logq_grad_x3 if fmt == "x3" else ops.npair_logq_grad_f32)(
                    d.S, d.ids, B, d.bias, T, symmetric, lse, buf, *((plane,) if fmt == "x3" else ()))
            else:
                (ops.npair_grad_x3 if fmt == "x3" else ops.npair_grad_f32)(
                    d.S, d.ids, B, T, symmetric, lse, buf, *((plane,) if fmt == "x3" else ()))

        def w_mem(buf, plane, fmt=fmt):
            if fmt == "bf16":
                ops.npair_memory_grad_bf16(d.S, d.ids, B, c["mem_col"], d.mem_id, T, symmetric, lse, buf, mem_bias=d.mem_bias)
            elif logq:
                (ops.npair_memory_logq_grad_x3 if fmt == "x3" else ops.npair_memory_logq_grad_f32)(
                    d.S, d.ids, B, c["mem_col"], d.mem_id, d.mem_bias, T, symmetric, lse, buf, *((plane,) if fmt == "x3" else ()))
            else:
                (ops.npair_memory_grad_x3 if fmt == "x3" else ops.npair_memory_grad_f32)(
                    d.S, d.ids, B, c["mem_col"], d.mem_id, T, symmetric, lse, buf, *((plane,) if fmt == "x3" else ()))
        _check_w(c, d, fmt, symmetric, [w_in], m["W"][0], cols_in, "in-batch block")
        if mem:
            _check_w(c, d, fmt, symmetric, [w_mem], m["W"][0], ~cols_in & ~np.isnan(m["W"][0]).all(0), "memory block")
            _check_w(c, d, fmt, symmetric, [w_in, w_mem], m["W"][0], None, "both blocks")


# ---- mixed negatives: scalar lq_u and per-column neg_bias, with and without a memory ---------------------------------------
@pytest.mark.parametrize("symmetric", (False, True))
@pytest.mark.parametrize("c", _inbatch_like("mixed") + _inbatch_like("mixed_lq") + _inbatch_like("mixed_nb"))
def test_mixed_family(dev, c, symmetric):
    c = c[0](*c[1])
    d = Dev(c, dev)
    B, M = c["B"], c["M"]
    m = xn.model(c, symmetric)
    ws = torch.zeros(max(ops.npair_mixed_workspace(B, M), 16) // 4, dtype=F32, device=dev)
    args = (d.S, d.ids, B, c["neg_col"], c["mem_col"], d.mem_id, d.bias, d.lq, d.mem_bias, T, symmetric)
    want_lse = _want_vec(2 * B, m["lse_row"][0], m["lse_col"] if symmetric else None)
    want_stats = torch.from_numpy(m["stats"][0])

    def stats():
        lse, st = _vec(2 * B, dev), _vec(4, dev)
        ops.npair_mixed_stats(*args, lse, st, ws)
        return lse, st

    def check(out):
        _bits_equal(out[0], want_lse, "%s lse symmetric=%s" % (c["name"], symmetric))
        _bits_equal(out[1], want_stats, "%s stats symmetric=%s" % (c["name"], symmetric))
    _twice(stats, check)
    lse = _lse_in(c, m, symmetric, 0, dev)
    _check_w(c, d, "f32", symmetric, [lambda buf, plane: ops.npair_mixed_grad_f32(*args, lse, buf)], m["W"][0], None, "mixed")
    _check_w(c, d, "x3", symmetric, [lambda buf, plane: ops.npair_mixed_grad_x3(*args, lse, buf, plane)], m["W"][0], None, "mixed")


# ---- data-parallel: world = 3, every rank's row block of one global matrix -------------------------------------------------
@pytest.mark.parametrize("symmetric", (False, True))
@pytest.mark.parametrize("c", _inbatch_like("dp"))
def test_dp_family(dev, c, symmetric):
    c = c[0](*c[1])
    B, G, world = c["B"], c["G"], c["world"]
    m = xn.model(c, symmetric)
    ws = torch.zeros(max(ops.npair_dp_workspace(B, G), 16) // 4, dtype=F32, device=dev)
    lse_col_in = xg.f32_exact(m["lse_col"]).to(dev) if symmetric else None
    for rank in range(world):
        d = Dev(c, dev, rank)
        col0 = rank * B
        what = "%s rank %d symmetric=%s" % (c["name"], rank, symmetric)
        want_cp = torch.from_numpy(m["colpart"][rank].astype(np.float32)) if symmetric else fp.poisoned((G, 2), dtype=F32, device="cpu")
        want_stats = torch.from_numpy(m["stats"][rank])

        def local():
            lse_row, colpart, st = _vec(B, dev), fp.poisoned((G, 2), dtype=F32, device=dev), _vec(4, dev)
            ops.npair_dp_local_stats(d.S, d.ids, B, G, col0, T, symmetric, lse_row, colpart, ws)
            ops.npair_dp_stats(d.S, B, G, col0, T, symmetric, lse_col_in, st, ws)
            return lse_row, colpart, st

        def check(out):
            _bits_equal(out[0], xg.f32_exact(m["lse_row"][rank]), what + " lse_row")
            _bits_equal(out[1], want_cp, what + " colpart")
            _bits_equal(out[2], want_stats, what + " stats")
        _twice(local, check)
        lse_row_in = xg.f32_exact(m["lse_row"][rank]).to(dev)
        _check_w(c, d, "f32", symmetric, [lambda buf, plane: ops.npair_dp_grad_f32(d.S, d.ids, B, G, col0, T, symmetric, lse_row_in,
                                                                                  lse_col_in, buf)], m["W"][rank], None, what)
        _check_w(c, d, "x3", symmetric, [lambda buf, plane: ops.npair_dp_grad_x3(d.S, d.ids, B, G, col0, T, symmetric, lse_row_in,
                                                                                lse_col_in, buf, plane)], m["W"][rank], None, what)
    if symmetric:
        cp_all = torch.from_numpy(np.stack(m["colpart"]).astype(np.float32)).to(dev).contiguous()

        def fold():
            lse_col = _vec(G, dev)
            ops.npair_dp_col_fold(cp_all, lse_col)
            return lse_col
        _twice(fold, lambda out: _bits_equal(out, xg.f32_exact(m["lse_col"]), c["name"] + " lse_col"))


def test_dp_pos_fold_rank_order(dev):
    """de[2i + 1] = recv[0][i] + recv[1][i] + recv[2][i] in THAT order: partials 2^24, 1, -2^24 give 0 in rank order and 1
    in any order that adds the two large ones first; rows 2i of de stay untouched"""
    B, D, world = 5, 8, 3
    recv = torch.zeros((world, B, D + 4), dtype=F32)
    recv[0, :, :D], recv[1, :, :D], recv[2, :, :D] = 2.0 ** 24, 1.0, -(2.0 ** 24)
    recv[:, 3, :D] = torch.tensor([1.0, 2.0, 4.0])[:, None] * torch.arange(1, D + 1, dtype=F32)[None, :]
    want = fp.poisoned((2 * B, D + 4), dtype=F32, device="cpu")
    want[1::2, :D] = 0.0                                       # (2^24 + 1 rounds to 2^24 in fp32)
    want[7, :D] = 7.0 * torch.arange(1, D + 1, dtype=F32)
    rd = recv.to(dev)

    def run():
        de = fp.poisoned((2 * B, D + 4), dtype=F32, device=dev)
        ops.npair_dp_pos_fold(rd[:, :, :D], B, D, de[:, :D])
        return de
    _twice(run, lambda de: _bits_equal(de, want, "npair_dp_pos_fold"))


# ---- the tie group: the one toleranced part --------------------------------------------------------------------------------
def test_tie_group(dev):
    """n = 2, 3, 64, B equal winners: s == n is exact, lse = logf(n) and W = expf(-logf(n)) * scale are not; against the fp64
    model in ulps of the fp32 result, bound = twice the largest error measured on the MI355X (exact_npair's docstring)"""
    worst = {"lse": 0.0, "W": 0.0}
    for c in xn.tie_cases():
        d = Dev(c, dev)
        B = c["B"]
        m = xn.model(c, True)
        ws = torch.zeros(max(ops.npair_workspace(B), 16) // 4, dtype=F32, device=dev)
        lse, st = _vec(2 * B, dev), _vec(4, dev)
        ops.npair_stats(d.S, None, B, T, True, lse, st, ws)
        W = fp.poisoned((B, xn.up4(B)), dtype=F32, device=dev)
        ops.npair_grad_f32(d.S, None, B, T, True, lse, W)
        got_lse, got_W = lse.cpu().numpy(), W[:, :B].cpu().numpy()
        want_lse = np.concatenate([m["lse_row"][0], m["lse_col"]])
        want_W = m["W"][0]
        assert np.array_equal(got_W == 0, want_W == 0), c["name"]          # what does not win is exactly 0
        e_lse = float(xn.ulps(got_lse, want_lse)[want_lse != 0].max()) if (want_lse != 0).any() else 0.0
        assert np.array_equal(got_lse[want_lse == 0], want_lse[want_lse == 0])
        nz = want_W != 0
        e_W = float(xn.ulps(got_W[nz], want_W[nz]).max()) if nz.any() else 0.0
        print("%-18s lse %.3f ulps, W %.3f ulps" % (c["name"], e_lse, e_W))
        worst["lse"], worst["W"] = max(worst["lse"], e_lse), max(worst["W"], e_W)
    print("tie group: measured now lse %.3f / W %.3f ulps; recorded %.3f, bound %.3f"
          % (worst["lse"], worst["W"], xn.TIE_MEASURED_ULPS, xn.TIE_BOUND_ULPS))
    assert max(worst.values()) <= xn.TIE_BOUND_ULPS, worst


# ---- one chain per precision: embeddings -> S -> statistics -> W -> de, every element of de ------------------------------
def _check_chain(c, symmetric, rank, lse, stats, W, de, m, want_de, what):
    B, G = c["B"], c["G"]
    _bits_equal(lse[:B], xg.f32_exact(m["lse_row"][rank]), what + " lse_row")
    _bits_equal(stats, torch.from_numpy(m["stats"][rank]), what + " stats")
    _bits_equal(W, xg.f32_exact(np.where(np.isnan(m["W"][rank]), 0.0, m["W"][rank])), what + " W")
    _bits_equal(de, xg.f32_exact(want_de[rank]), what + " de")


@pytest.mark.parametrize("precision", ("f32", "f32x3", "bf16"))
def test_chain_inbatch(dev, precision):
    """ops.npair_loss on embeddings whose scores are a ladder: de = [W P ; W^T A] element by element, the interleave of
    anchor and positive rows included -- the check the Frobenius norm of the band tests stood in for"""
    c = xn.chain_case("inbatch", 256)
    B, D = c["B"], xn.CHAIN_D
    e, rows = (t.to(dev) for t in xn.chain_rows(c))
    ws = ops.NPairWorkspace(B, D, precision, dev)
    for symmetric in (False, True):
        m = xn.model(c, symmetric)
        want_de = xn.chain_de(c, m)
        what = "%s %s symmetric=%s" % (c["name"], precision, symmetric)
        for _ in range(2):
            de, stats = fp.poisoned((2 * B, D), dtype=F32, device=dev), _vec(4, dev)
            _, lse = ops.npair_loss(e, rows, B, D, T, symmetric, precision, de=de, stats=stats, ws=ws)
            _check_chain(c, symmetric, 0, lse, stats, ws.W(), de, m, want_de, what)
            if symmetric:
                _bits_equal(lse[B:2 * B], xg.f32_exact(m["lse_col"]), what + " lse_col")


@pytest.mark.parametrize("precision", ("f32", "f32x3"))
def test_chain_mixed(dev, precision):
    """ops.npair_mixed_loss: de rows (a, p, n) per triplet -- the uniform negatives' gradient rows dN = W_n^T A included"""
    c = xn.chain_case("mixed", 256)
    B, D = c["B"], xn.CHAIN_D
    e3, rows3 = (t.to(dev) for t in xn.chain_rows(c))
    ws = ops.NPairMixed(B, D, precision, dev)
    assert (ws.neg_col, ws.K) == (c["neg_col"], c["span"])
    for symmetric in (False, True):
        m = xn.model(c, symmetric)
        want_de = xn.chain_de(c, m)
        what = "%s %s symmetric=%s" % (c["name"], precision, symmetric)
        for _ in range(2):
            de, stats = fp.poisoned((3 * B, D), dtype=F32, device=dev), _vec(4, dev)
            _, lse = ops.npair_mixed_loss(e3, rows3, B, D, T, symmetric, precision, de=de, stats=stats, ws=ws)
            _check_chain(c, symmetric, 0, lse, stats, ws.W(), de, m, want_de, what)
            if symmetric:
                _bits_equal(lse[B:2 * B], xg.f32_exact(m["lse_col"]), what + " lse_col")


@pytest.mark.parametrize("precision,B", (("f32", 64), ("f32x3", 256)))
def test_chain_dp(dev, precision, B):
    """the three dp phases of world = 3 ranks on one device, the collectives done by copies: every rank's de -- dA = W_r
    P_all, and npair_dp_pos_fold's rank-order sum of the partial positive gradients -- element by element"""
    world = 3
    c = xn.chain_case("dp", B, world)
    G, D = c["G"], xn.CHAIN_D
    ranks = [tuple(t.to(dev) for t in xn.chain_rows(c, r)) for r in range(world)]
    wss = [ops.NPairDP(B, G, D, precision, dev) for _ in range(world)]
    for symmetric in (False, True):
        m = xn.model(c, symmetric)
        want_de = xn.chain_de(c, m)
        des = [fp.poisoned((2 * B, D), dtype=F32, device=dev) for _ in range(world)]
        sts = [_vec(4, dev) for _ in range(world)]
        wire = torch.cat([ops.npair_dp_pack(e, rows, ws).clone() for (e, rows), ws in zip(ranks, wss)])      # all-gather
        for r, ((e, rows), ws) in enumerate(zip(ranks, wss)):
            ws.wire.copy_(wire)
            ops.npair_dp_phase1(e, r, ws, T, symmetric)
        cp_all = torch.stack([ws.colpart for ws in wss])                                                     # all-gather
        for r, ((e, rows), ws) in enumerate(zip(ranks, wss)):
            ws.colpart_all.copy_(cp_all)
            ops.npair_dp_phase2(e, r, ws, T, symmetric, de=des[r], stats=sts[r])
        for r, ws in enumerate(wss):                                                                         # all-to-all
            for s in range(world):
                ws.recv[s].copy_(wss[s].dP_part[r * B:(r + 1) * B])
            ops.npair_dp_phase3(ws, des[r])
            what = "%s %s rank %d symmetric=%s" % (c["name"], precision, r, symmetric)
            _check_chain(c, symmetric, r, ws.lse_row, sts[r], ws.W(), des[r], m, want_de, what)
            if symmetric:
                _bits_equal(ws.lse_col, xg.f32_exact(m["lse_col"]), what + " lse_col")


@pytest.mark.parametrize("precision", ("f32", "f32x3", "bf16"))
def test_chain_memory(dev, precision):
    """ops.npair_loss(memory=...): dA = W [P; Mem] over K = B + M element by element; the ring's rows get no gradient (de
    has the batch's rows alone) and, after the products, the push leaves this step's positives and their ids in the ring"""
    c = xn.chain_case("memory", 256)
    B, D, M = c["B"], xn.CHAIN_D, c["M"]
    e, rows = (t.to(dev) for t in xn.chain_rows(c))
    ring_rows, ring_ids = xg.f32_exact(c["Mem"]), torch.from_numpy(c["mem_id"].astype(np.int32))
    ws = ops.NPairWorkspace(B, D, precision, dev)
    mem = ops.NPairMemory(M, B, D, precision, dev)
    assert (mem.Bp, mem.K) == (c["mem_col"], c["span"])
    for symmetric in (False, True):
        m = xn.model(c, symmetric)
        want_de = xn.chain_de(c, m)
        what = "%s %s symmetric=%s" % (c["name"], precision, symmetric)
        for _ in range(2):
            mem.load(ring_rows, ring_ids)
            de, stats = fp.poisoned((2 * B, D), dtype=F32, device=dev), _vec(4, dev)
            _, lse = ops.npair_loss(e, rows, B, D, T, symmetric, precision, de=de, stats=stats, ws=ws, memory=mem, step=0)
            _check_chain(c, symmetric, 0, lse, stats, mem.W(), de, m, want_de, what)
            if symmetric:
                _bits_equal(lse[B:2 * B], xg.f32_exact(m["lse_col"]), what + " lse_col")
            assert torch.equal(mem.rows, e[1::2, :D]) and torch.equal(mem.ids, rows[1::2]), what + ": the ring after the push"
