"""The kernels that choose instead of sum -- the kNN list kernels, the kNN filter, the rank count, the semi-hard miner --
against integer oracles at zero tolerance, ties included (tests/exact_select.py): inputs whose norms, products and
distances are all exact in fp32 in any order, so which element wins a tie, which side of tau an equal distance falls,
what the clamp does at 0, which ids are excluded and which accumulator element belongs to which (row, column) all show
as a mismatch.  tests/test_exact_select_host.py shows on the same cases that the expectation is the existing
specification, is order-independent, and changes under every single mutation of a rule.  Outputs go into poisoned,
guarded buffers; operands are views with ld > columns and NaN-filled gaps.  No number here is a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import footprint as fp  # noqa: E402

pytestmark = pytest.mark.gpu

from cdml_amd import ops  # noqa: E402

F32, I32 = torch.float32, torch.int32
PRECISIONS = ["f32", "f32x3", "f16x2"]
PLANE_FORMS = ["f32x3", "f16x2"]


@pytest.fixture(scope="module")
def dev(gpu):
    assert ops.knn_list_capacity() == xs.LIST
    return gpu


def assert_bits(got, want, what):
    """bit for bit, with the first mismatch located"""
    got = got.detach().cpu()
    want = want.to(got.dtype) if not want.dtype.is_floating_point else want
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = fp.bits_of(got) != fp.bits_of(want)
    if bool(bad.any()):
        idx = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r"
                             % (what, int(bad.sum()), bad.numel(), idx, got[idx].item(), want[idx].item()))


def vec(v, dev, dtype=F32):
    return torch.as_tensor(np.asarray(v)).to(dtype).to(dev)


def f32_units(d, unit, dev):
    return xs.from_units(d, unit).to(dev)


def guarded(shape, dtype, dev, fill=None):
    g = fp.Guarded(shape, dtype, dev)
    if fill is not None:
        g.fill_from(fill)
    return g


# ---- cdml_knn_merge ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", xs.MERGE_ORDERS)
def test_knn_merge(dev, order):
    """scores given directly (integer-valued fp32, stride wider than nb): every k x nq x nb, n_valid inside a 4-vector and
    before a whole 256-column pass, col0 > 0, two and three consecutive calls, fewer valid rows than k -- the first k
    entries of every list equal the streaming model, the whole list ascends in (d, id)"""
    for c in (c for c in xs.all_merge_cases() if c["order"] == order):
        assert c["safe"] < 2.0 ** 24
        nq = c["nq"]
        q_sq = vec(c["q_sq"], dev)
        calls = [(xs.strided(xs.xg.f32_exact(x["score"]), pad=4).to(dev)[:, :x["nb"]], vec(x["b_sq"], dev), x) for x in c["calls"]]
        for k in xs.MERGE_KS:
            bd, bi = guarded((nq, xs.LIST), F32, dev), guarded((nq, xs.LIST), I32, dev)
            for scores, b_sq, x in calls:
                assert scores.stride(0) > x["nb"]
                ops.knn_merge(scores, nq, x["nb"], x["col0"], c["n_valid"], q_sq, b_sq, k, bd.view, bi.view, first=x["first"])
            D, I = xs.merge_model(xs.merge_calls(c), k)
            what = "%s k=%d" % (c["name"], k)
            assert_bits(bd.view[:, :k], xs.from_units(D, c["unit"]), what + " distances")
            assert_bits(bi.view[:, :k], torch.from_numpy(I), what + " ids")
            xs.assert_list_ascending(bd.view, bi.view, what)
            bd.assert_guards_intact(what + " best_d")
            bi.assert_guards_intact(what + " best_i")


# ---- the kNN filter epilogue and cdml_knn_merge_list ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,n_cols,D,col0,small_cap", xs.filter_params())
def test_knn_filter_and_merge_list(dev, form, n_cols, D, col0, small_cap):
    """three- / two-plane operands: cnt and the candidate SET per query exactly (slot order comes from an atomic: sorted by
    (d, id) first), nothing written past min(cnt, cap); after cdml_knn_merge_list the lists are the exact k best of list and
    candidates, cnt is zero again, overflow 0 -- or, with the small cap, 1 and every query within the cap still exact"""
    c = xs.filter_case(form, n_cols, D, col0, small_cap)
    assert c["safe"] < 2.0 ** 24
    nq, cap, k, unit = c["nq"], c["cap"], c["k"], c["unit"]
    Q, Bk = c["Q"].to(dev), c["B"].to(dev)
    q_sq, b_sq = vec(c["q_sq"], dev), vec(c["b_sq"], dev)
    tau = f32_units(c["tau"], unit, dev)
    cnt = guarded((nq,), I32, dev, torch.zeros(nq, dtype=I32))
    cand = guarded((nq, cap * 2), I32, dev)
    args = (nq, n_cols, D) + ((c["scale"],) if form == "h2" else ()) + (q_sq, b_sq, tau, col0, c["n_valid"], cnt.view, cand.view, cap)
    with fp.frozen(Q, Bk, q_sq, b_sq, tau):
        (ops.knn_filter_h2 if form == "h2" else ops.knn_filter_x3)(Q, c["plane_q"], Bk, c["plane_b"], *args)
    got_n = cnt.payload().cpu().numpy()
    assert np.array_equal(got_n, c["counts"]), "cnt differs for queries %s" % np.nonzero(got_n != c["counts"])[0][:8].tolist()
    slots = cand.payload().cpu().numpy().reshape(nq, cap, 2)
    kept = np.minimum(got_n, cap)
    unused = np.arange(cap)[None, :] >= kept[:, None]
    assert (slots[unused] == fp.poison_scalar(I32, 0)).all(), "a slot past min(cnt, cap) was written"
    for i in range(nq):
        if got_n[i] > cap:
            continue                                        # (the overflowing query keeps an arbitrary cap of its candidates)
        g = slots[i, :kept[i]]
        o = np.lexsort((g[:, 1], g[:, 0].view(np.float32)))
        want_d = xs.from_units(c["cands"][i][:, 0], unit).numpy().view(np.int32)
        assert np.array_equal(g[o, 0], want_d) and np.array_equal(g[o, 1], c["cands"][i][:, 1]), "candidate set of query %d" % i
    cand.assert_guards_intact("cand")
    cnt.assert_guards_intact("cnt")
    # the merge
    bd = guarded((nq, xs.LIST), F32, dev, xs.from_units(c["list_d"], unit))
    bi = guarded((nq, xs.LIST), I32, dev, torch.from_numpy(c["list_i"]))
    overflow = guarded((1,), I32, dev, torch.zeros(1, dtype=I32))
    ops.knn_merge_list(cand.view, cnt.view, cap, nq, k, bd.view, bi.view, overflow.view)
    assert int(overflow.payload().item()) == (1 if small_cap else 0)
    assert not bool(cnt.payload().any()), "cnt is not reset"
    keep = torch.from_numpy(c["counts"] <= cap)
    assert int((~keep).sum()) == (1 if small_cap else 0)
    assert_bits(bd.view[:, :k].cpu()[keep], xs.from_units(c["want_d"], unit)[keep], c["name"] + " distances")
    assert_bits(bi.view[:, :k].cpu()[keep], torch.from_numpy(c["want_i"])[keep], c["name"] + " ids")
    xs.assert_list_ascending(bd.view.cpu()[keep], bi.view.cpu()[keep], c["name"])
    for g, name in ((bd, "best_d"), (bi, "best_i"), (cnt, "cnt"), (overflow, "overflow"), (cand, "cand")):
        g.assert_guards_intact(name)


# ---- the rank epilogue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,D", xs.RANK_PARAMS)
def test_rank_tau_and_count(dev, form, D):
    """520 queries over a catalogue of 600 rows in two column chunks, the counts accumulated onto a non-zero start: tau is
    the integer distance bit for bit, the count rank_int's for EVERY query -- self and partner ids sweep all 256 column
    positions of a tile, partners and anchors have duplicates below and above; the rows 600 .. 767 of the launched buffer
    are finite like the others, so only the n_valid test keeps them out of the counts"""
    c = xs.rank_case(form, D)
    assert c["safe"] < 2.0 ** 24
    nq, n, unit = c["nq"], c["n"], c["unit"]
    Bk = c["B"].to(dev)
    b_sq = vec(c["b_sq"], dev)
    a, p = torch.from_numpy(c["a"]).to(dev), torch.from_numpy(c["p"]).to(dev)
    QA = Bk.index_select(0, a)
    mp = (nq + 255) // 256 * 256
    PP = fp.poisoned((mp, Bk.shape[1]), dtype=Bk.dtype, device=dev)
    PP[:nq] = Bk.index_select(0, p)
    q_sq = b_sq.index_select(0, a)
    p_sq = fp.poisoned(mp, dtype=F32, device=dev)
    p_sq[:nq] = b_sq.index_select(0, p)
    tau = guarded((nq,), F32, dev)
    sc = (c["scale"],) if form == "h2" else ()
    (ops.rank_tau_h2 if form == "h2" else ops.rank_tau_x3)(QA, c["plane_b"], PP, c["plane_b"], nq, D, *sc, q_sq, p_sq, tau.view)
    assert_bits(tau.view, xs.from_units(c["tau"], unit), c["name"] + " tau")
    tau.assert_guards_intact("tau")
    start = 1000 + torch.arange(nq, dtype=I32)
    count = guarded((nq,), I32, dev, start)
    a32, p32 = a.to(I32), p.to(I32)
    with fp.frozen(QA, Bk, b_sq, tau.view, a32, p32):
        for col0, n_cols in xs.RANK_CHUNKS:
            args = (nq, n_cols, D) + sc + (q_sq, b_sq[col0:col0 + n_cols], tau.view, p32, a32, col0, n, count.view)
            (ops.rank_count_h2 if form == "h2" else ops.rank_count_x3)(QA, c["plane_b"], Bk[col0:col0 + n_cols], c["plane_b"], *args)
    got = count.payload().cpu().numpy().astype(np.int64) - start.numpy()
    bad = np.nonzero(got != c["count"])[0]
    assert not len(bad), "%s: %d of %d counts differ; first: query %d (anchor %d, partner %d) got %d, expected %d" % (
        c["name"], len(bad), nq, bad[0], c["a"][bad[0]], c["p"][bad[0]], got[bad[0]], c["count"][bad[0]])
    count.assert_guards_intact("count")


# ---- the miner ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("videos", xs.MINER_VIDEOS)
@pytest.mark.parametrize("B,D", xs.MINER_SHAPES)
def test_semihard_select_and_mine(dev, B, D, videos):
    """cdml_semihard_select (S given directly) and cdml_semihard_mine_x3 (three bf16 planes; two fp16 planes at a power-of-two
    scale) on integer grid rows: neg_row equals semihard_int for EVERY anchor, |e|^2 and d_p bit for bit, the kernels equal
    to each other, a second launch bit-equal"""
    c = xs.miner_case(B, D, videos)
    assert c["safe"] < 2.0 ** 24
    R = 2 * B
    E = torch.from_numpy(c["E"]).to(F32)
    de = xs.strided(E, pad=4).to(dev)[:, :D]
    dr = vec(c["rows"], dev, I32)
    want_neg = torch.from_numpy(c["neg"])
    want_sqn, want_dp = xs.from_units(c["sqn"].astype(np.int64), 1.0), xs.from_units(c["dp"], 1.0)
    S = xs.strided(xs.xg.f32_exact((c["E"][0::2] @ c["E"].T).astype(np.float64)), pad=4).to(dev)[:, :R]
    sq0, neg0 = guarded((R,), F32, dev), guarded((B,), I32, dev)
    with fp.frozen(S, de, dr):
        ops.semihard_select(S, de, dr, B, D, sq0.view, neg0.view)
    assert_bits(neg0.view, want_neg, c["name"] + " semihard_select neg_row")
    assert_bits(sq0.view, want_sqn, c["name"] + " semihard_select sqn")
    neg0.assert_guards_intact("neg_row")
    sq0.assert_guards_intact("sqn")
    plane = D + 8
    for hs in (0.0, xs.MINER_H2_SCALE):
        what = "%s mine h2_scale=%g" % (c["name"], hs)
        outs = []
        for pattern in (0, 1):
            e3 = fp.poisoned((R, (2 if hs else 3) * plane + 8), dtype=torch.float16 if hs else torch.bfloat16, device=dev, pattern=pattern)
            sqn = fp.Guarded((R,), F32, dev, pattern=pattern)
            dpd = fp.Guarded((B,), F32, dev, pattern=pattern)
            neg = fp.Guarded((B,), I32, dev, pattern=pattern)
            ws = fp.poisoned(ops.semihard_mine_x3_workspace(B) // 4 + 4, dtype=F32, device=dev, pattern=pattern)
            with fp.frozen(de, dr):
                ops.semihard_mine_x3(de, dr, B, D, e3, plane, sqn.view, dpd.view, ws, neg.view, h2_scale=hs)
            assert_bits(neg.view, want_neg, what + " neg_row")
            assert_bits(sqn.view, want_sqn, what + " sqn")
            assert_bits(dpd.view, want_dp, what + " dp")
            assert torch.equal(e3[:, :D].float().cpu(), E * (hs or 1.0)), what + ": the high plane is the row"
            for pl in range(1, 2 if hs else 3):
                assert not bool(e3[:, pl * plane:pl * plane + D].float().any()), what + ": plane %d is zero" % pl
            for g, name in ((sqn, "sqn"), (dpd, "dp"), (neg, "neg_row")):
                g.assert_guards_intact(what + " " + name)
            outs.append((neg.payload(), sqn.payload(), dpd.payload()))
        assert all(torch.equal(x, y) for x, y in zip(*outs)), what + ": a second launch differs"
        assert torch.equal(outs[0][0], neg0.payload()), what + ": the fused and the unfused kernel differ"


# ---- the pipelines ----------------------------------------------------------------------------------------------------------------------
KNN_KW = dict(l2_norm=False, b_block=xs.KNN_FIRST, first_block=xs.KNN_FIRST)


def _knn_want(d, n, k, unit):
    D, I = xs.knn_from_dist(d, np.arange(n), k)
    return xs.from_units(D, unit), torch.from_numpy(I)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_knn_search_exact(dev, precision):
    """1100 grid rows, 300 queries, first block 256 (k = 51 goes through the filter path, k = 128 through score blocks):
    (D, I) bit-equal to knn_int, equal with fused=False and with small query / catalogue chunks"""
    from cdml_amd import knn
    c = xs.knn_pipeline_case()
    assert c["safe"] < 2.0 ** 24
    base, q = torch.from_numpy(c["b"]), torch.from_numpy(c["q"])
    for k in xs.KNN_KS:
        want_d, want_i = _knn_want(c["d"], xs.KNN_N, k, c["unit"])
        for kw in (dict(), dict(fused=False), dict(q_block=64, q_chunk=128, c_chunk=512)):
            D, I = knn.knn_search(base, q, k, device=dev, precision=precision, **dict(KNN_KW, **kw))
            what = "knn_search %s k=%d %s" % (precision, k, kw)
            assert_bits(I, want_i, what + " ids")
            assert_bits(D, want_d, what + " distances")


@pytest.mark.parametrize("precision", PLANE_FORMS)
def test_ranks_exact(dev, precision):
    """Evaluation.ranks on 600 grid rows: EVERY position equals rank_int -- no [lo, hi] band -- in any chunking"""
    from cdml_amd.evaluate import Evaluation
    c = xs.rank_pipeline_case()
    assert c["safe"] < 2.0 ** 24
    ev = Evaluation(None, [], device=dev)
    for kw in (dict(), dict(q_chunk=256, c_chunk=512)):
        queries, pos = ev.ranks(c["v"], c["cw"], precision=precision, l2_norm=False, **kw)
        qn = queries.cpu().numpy()
        assert {tuple(r) for r in c["cw"].tolist()} <= {tuple(r) for r in qn.tolist()}
        assert_bits(pos, torch.from_numpy(xs.pipeline_ranks_want(c["d"], qn)), "ranks %s %s" % (precision, kw))


def test_l2norm_returns_dyadic_unit_rows(dev):
    """rows that are exactly unit on a dyadic grid (4^j non-zeros of +-2^-j) come back from cdml_l2norm_fwd bit for bit:
    what the normalised exact case below stands on"""
    c = xs.unit_rows_case()
    x = xs.strided(torch.from_numpy(c["b"]), pad=4).to(dev)[:, :xs.UNIT_D]
    y = fp.Guarded((xs.UNIT_N, xs.UNIT_D), F32, dev, ld=xs.UNIT_D + 4)
    ops.l2norm_fwd(x, xs.UNIT_D, y.view)
    assert_bits(y.view, torch.from_numpy(c["b"]), "l2norm_fwd of unit rows")
    y.assert_guards_intact("y")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_knn_search_exact_normalised(dev, precision):
    from cdml_amd import knn
    c = xs.unit_rows_case()
    assert c["safe"] < 2.0 ** 24
    want_d, want_i = _knn_want(c["d"], xs.UNIT_N, xs.UNIT_K, c["unit"])
    D, I = knn.knn_search(torch.from_numpy(c["b"]), torch.from_numpy(c["q"]), xs.UNIT_K, l2_norm=True, device=dev, precision=precision,
                          b_block=256, first_block=256)
    assert_bits(I, want_i, "normalised knn_search %s ids" % precision)
    assert_bits(D, want_d, "normalised knn_search %s distances" % precision)


# ---- non-finite rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_knn_search_nonfinite_rows(dev, precision, fused):
    """a catalogue row with a NaN or +inf coordinate (on both sides of the first block) is nobody's neighbour, a NaN query
    gets I = -1, D = +inf throughout, every other result is the integer oracle's over the finite rows, ids kept"""
    from cdml_amd import knn
    c = xs.nonfinite_knn_case()
    for k in xs.KNN_KS:
        want_d, want_i = xs.nonfinite_want(c, k)
        D, I = knn.knn_search(torch.from_numpy(c["b"]), torch.from_numpy(c["q"]), k, device=dev, precision=precision, fused=fused, **KNN_KW)
        what = "non-finite knn_search %s fused=%s k=%d" % (precision, fused, k)
        assert_bits(I, want_i, what + " ids")
        assert_bits(D, want_d, what + " distances")


@pytest.mark.parametrize("precision", PLANE_FORMS)
def test_ranks_nonfinite_rows(dev, precision):
    """a non-finite catalogue row is never counted ahead of a partner -- by the fast path and the full rule alike, so in
    any chunking"""
    from cdml_amd.evaluate import Evaluation
    c = xs.nonfinite_rank_case()
    ev = Evaluation(None, [], device=dev)
    for kw in (dict(), dict(q_chunk=256, c_chunk=512)):
        queries, pos = ev.ranks(c["v"], c["cw"], precision=precision, l2_norm=False, **kw)
        want = xs.pipeline_ranks_want(c["d"], queries.cpu().numpy(), c["bad"])
        assert_bits(pos, torch.from_numpy(want), "non-finite ranks %s %s" % (precision, kw))
