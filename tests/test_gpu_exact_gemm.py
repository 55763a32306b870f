"""Every GEMM entry against an integer computation on the host, at zero tolerance (tests/exact_gemm.py): operands whose
partial sums are all exact in fp32, so every walk, tile form, split and slab form must give the same bits -- which plane
pairs are summed and which element is read show as a mismatch, and the probe names the index that was read instead.
tests/test_exact_gemm_host.py shows on the same operands that the expectation is order-independent and that every single
mutation of the pair list or of an index changes at least half of the outputs.  Outputs go into poisoned buffers with
poisoned gaps (compared too); operands are views with ld > columns and NaN-filled plane gaps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import footprint as fp  # noqa: E402

pytestmark = pytest.mark.gpu

from cdml_amd import ops  # noqa: E402

ALPHA = xg.ALPHA
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
WALKS = [("CDML_X3_WALK", "general"), ("CDML_X3_WALK", "f6"), ("CDML_X3_WALK", "r6"), ("CDML_X3_HALFTILES", "2"),
         ("CDML_X3_HALFTILES", "0")]
# (CDML_X3_HALFTILES=2 splits a launch of full rounds + half tiles in two: that takes more than 256 tiles, so at these
# shapes it runs what 1 runs; 0 = full tiles only.  The one-launch rounds kernel is not reached by a small shape.)
_CACHE = {}


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


def cached(key, make):
    """one reference per case, shared by the tests that need it and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def assert_bits(got, want, what):
    """bit-for-bit (poisoned gaps included), with the first mismatch located"""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(xg.bits(got), xg.bits(want)):
        return
    bad = xg.bits(got) != xg.bits(want)
    idx = tuple(int(v) for v in torch.nonzero(bad)[0])
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r"
                         % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx])))


def out_f32(M, N, dev, pattern=0):
    buf = fp.poisoned((M, N + 4), dtype=F32, device=dev, pattern=pattern)
    return buf, buf[:, :N]


def want_f32(v, pattern=0):
    v = xg.f32_exact(v)
    buf = fp.poisoned((v.shape[0], v.shape[1] + 4), dtype=F32, device="cpu", pattern=pattern)
    buf[:, :v.shape[1]] = v
    return buf


def want_vec(v):
    return xg.f32_exact(np.asarray(v, dtype=np.float64))


def ws_bytes(n, dev):
    return fp.poisoned(max(int(n), 16) // 4 + 4, dtype=F32, device=dev)


def to_dev(v, dev, dtype=F32):
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype).to(dev)


def aux_buf(aux, dev, dtype):
    """integer-valued mask source [M][N] as a view into a wider poisoned buffer"""
    M, N = aux.shape
    buf = fp.poisoned((M, N + 8), dtype=dtype, device="cpu")
    buf[:, :N] = torch.from_numpy(aux).to(dtype)
    return buf.to(dev)[:, :N]


def bits_buf(positive, dev):
    """packed sign bits [M][N / 8] as a view into a wider buffer (row stride N / 8 + 16 bytes)"""
    b = xg.pack_bits(positive)
    buf = fp.poisoned((b.shape[0], b.shape[1] + 16), dtype=torch.uint8, device="cpu")
    buf[:, :b.shape[1]] = b
    return buf.to(dev)[:, :b.shape[1]]


def want_bits(positive):
    b = xg.pack_bits(positive)
    buf = fp.poisoned((b.shape[0], b.shape[1] + 16), dtype=torch.uint8, device="cpu")
    buf[:, :b.shape[1]] = b
    return buf


def plane_out(M, N, n, dtype, dev):
    pc = N + 8
    ld = n * pc + 8
    return fp.poisoned((M, ld), dtype=dtype, device=dev), pc, ld


def want_planes(v, n, dtype, pc, ld):
    return xg.plane_buffer(xg.split_planes(xg.f32_exact(v), n, dtype), pc, ld)


def want_ki(v, ldc, plane_c):
    """the k8-interleaved plane output [3][M / 8][ldc][8], planes plane_c elements apart, over poison"""
    M, N = v.shape
    buf = fp.poisoned(3 * plane_c, dtype=BF16, device="cpu")
    for p, t in enumerate(xg.split_planes(xg.f32_exact(v))):
        buf[p * plane_c:p * plane_c + M * ldc].view(M // 8, ldc, 8)[:, :N, :] = t.reshape(M // 8, 8, N).permute(0, 2, 1)
    return buf


# ---- plane GEMM, k-contiguous ------------------------------------------------------------------------------------------
def x3_nt_case(M, N, K, products):
    def make():
        Kl = xg.x3_legal_k(K, products)
        c = xg.plane_case("x3nt", M, N, Kl)
        pairs = xg.PAIRS6 if products == 6 else xg.PAIRS3
        c["K"] = Kl
        c["S"] = xg.expected(c["Ap"], c["Bp"], pairs)
        c["worst"] = xg.assert_exact_safe(c["Ap"], c["Bp"], pairs, c["unit"], extra=xg.BIAS_MAX)
        r = xg.case_rng("x3nt-epi", M, N)
        c["bias"], c["rbias"], c["aux"] = xg.int_bias(N, r), xg.int_bias(M, r), xg.int_aux(M, N, r)
        return c
    return cached(("x3nt", M, N, K, products), make)


def x3_nt_workspace(M, N, K, products, dev):
    return ws_bytes(ops.gemm_bf16x3_workspace(False, M, N, K, products), dev)


@pytest.mark.parametrize("products", [6, 3])
@pytest.mark.parametrize("M,N,K", xg.X3_NT_SHAPES)
def test_x3_nt_every_epilogue(M, N, K, products, dev):
    c = x3_nt_case(M, N, K, products)
    K, S = c["K"], c["S"]
    A, B, pa, pb = c["A"].to(dev), c["B"].to(dev), c["plane_a"], c["plane_b"]
    bias, rbias = to_dev(c["bias"], dev), to_dev(c["rbias"], dev)
    slab = (M, N) == (520, 256)
    ws = x3_nt_workspace(M, N, K, products, dev) if slab else None
    kw = dict(products=products, alpha=ALPHA)
    act = xg.lrelu(S + c["bias"])
    masked = S * np.where(c["aux"] > 0, 1.0, ALPHA)
    with fp.frozen(A, B, names=["A", "B"]):
        buf, C = out_f32(M, N, dev)
        ops.gemm_bf16x3_nt(ops.BE_F32, A, pa, B, pb, C, M, N, K, workspace=ws, **kw)
        assert_bits(buf, want_f32(S), "epilogue 3 (fp32)")
        buf, C = out_f32(M, N, dev, 1)
        ops.gemm_bf16x3_nt(ops.BE_BIAS_LRELU_F32, A, pa, B, pb, C, M, N, K, bias=bias, workspace=ws, **kw)
        assert_bits(buf, want_f32(act, 1), "epilogue 1 (bias + lrelu, fp32)")
        if slab:                                             # the single pass over K (no workspace): the same bits
            buf, C = out_f32(M, N, dev)
            ops.gemm_bf16x3_nt(ops.BE_BIAS_LRELU_F32, A, pa, B, pb, C, M, N, K, bias=bias, **kw)
            assert_bits(buf, want_f32(act), "epilogue 1, single pass")
        out, pc, ld = plane_out(M, N, 3, BF16, dev)
        ops.gemm_bf16x3_nt(ops.BE_BIAS_LRELU_X3, A, pa, B, pb, out, M, N, K, plane_c=pc, bias=bias, **kw)
        assert_bits(out, want_planes(act, 3, BF16, pc, ld), "epilogue 6 (bias + lrelu, planes)")
        out, pc, ld = plane_out(M, N, 3, BF16, dev)
        ops.gemm_bf16x3_nt(ops.BE_MASK_X3, A, pa, B, pb, out, M, N, K, plane_c=pc, aux=aux_buf(c["aux"], dev, BF16), **kw)
        assert_bits(out, want_planes(masked, 3, BF16, pc, ld), "epilogue 7 (mask, planes)")
        out, pc, ld = plane_out(M, N, 3, BF16, dev)
        ops.gemm_bf16x3_nt(ops.BE_ROWBIAS_LRELU_X3, A, pa, B, pb, out, M, N, K, plane_c=pc, bias=rbias, **kw)
        assert_bits(out, want_planes(xg.lrelu(S + c["rbias"][:, None]), 3, BF16, pc, ld), "epilogue 8 (row bias, planes)")
        out, pc, ld = plane_out(M, N, 3, BF16, dev)
        bbuf = fp.poisoned((M, N // 8 + 16), dtype=torch.uint8, device=dev)
        ops.gemm_bf16x3_nt(ops.BE_BIAS_LRELU_X3_BITS, A, pa, B, pb, out, M, N, K, plane_c=pc, bias=bias, aux=bbuf[:, :N // 8], **kw)
        assert_bits(out, want_planes(act, 3, BF16, pc, ld), "epilogue 9 (planes)")
        assert_bits(bbuf, want_bits(act > 0), "epilogue 9 (sign bits)")
        out, pc, ld = plane_out(M, N, 3, BF16, dev)
        ops.gemm_bf16x3_nt(ops.BE_MASKBITS_X3, A, pa, B, pb, out, M, N, K, plane_c=pc, aux=bits_buf(c["aux"] > 0, dev), **kw)
        assert_bits(out, want_planes(masked, 3, BF16, pc, ld), "epilogue 10 (mask from bits, planes)")
        if M % 8 == 0:
            ldc = N + 8
            plane_c = M * ldc + 64
            for aux, want in ((bits_buf(c["aux"] > 0, dev), masked), (None, S)):
                flat = fp.poisoned(3 * plane_c, dtype=BF16, device=dev)
                ops.gemm_bf16x3_nt(ops.BE_MASKBITS_X3_KI, A, pa, B, pb, flat, M, N, K, plane_c=plane_c, aux=aux, ldc=ldc, **kw)
                assert_bits(flat, want_ki(want, ldc, plane_c), "epilogue 12 (k8-interleaved planes, mask %s)" % (aux is not None))
        if (M, N) == (512, 256) and products == 6:
            buf, C = out_f32(M, N, dev)
            cs = fp.poisoned(N, dtype=F32, device=dev)
            ops.gemm_bf16x3_nt(ops.BE_F32, A, pa, B, pb, C, M, N, K, workspace=x3_nt_workspace(M, N, K, 6, dev), colsum=cs, **kw)
            assert_bits(buf, want_f32(S), "epilogue 3 with colsum")
            assert_bits(cs, want_vec(sum(c["Bp"]).sum(1)), "colsum")


@pytest.mark.parametrize("var,value", WALKS)
@pytest.mark.parametrize("M,N,K", xg.X3_NT_SHAPES)
def test_x3_nt_every_walk_gives_the_same_bits(M, N, K, var, value, dev, monkeypatch):
    monkeypatch.setenv(var, value)
    c = x3_nt_case(M, N, K, 6)
    K, S = c["K"], c["S"]
    A, B, pa, pb = c["A"].to(dev), c["B"].to(dev), c["plane_a"], c["plane_b"]
    ws = x3_nt_workspace(M, N, K, 6, dev) if (M, N) == (520, 256) else None
    buf, C = out_f32(M, N, dev)
    ops.gemm_bf16x3_nt(ops.BE_F32, A, pa, B, pb, C, M, N, K, workspace=ws, alpha=ALPHA)
    assert_bits(buf, want_f32(S), "fp32, %s=%s" % (var, value))
    out, pc, ld = plane_out(M, N, 3, BF16, dev)
    ops.gemm_bf16x3_nt(ops.BE_BIAS_LRELU_X3, A, pa, B, pb, out, M, N, K, plane_c=pc, bias=to_dev(c["bias"], dev), alpha=ALPHA)
    assert_bits(out, want_planes(xg.lrelu(S + c["bias"]), 3, BF16, pc, ld), "planes, %s=%s" % (var, value))


# ---- plane GEMM, k-strided ---------------------------------------------------------------------------------------------
def x3_tn_case(M, N, K):
    def make():
        c = xg.tn_window_case(M, N, K)
        for products, pairs in ((6, xg.PAIRS6), (3, xg.PAIRS3)):
            c["S%d" % products] = xg.expected(c["Ap"], c["Bp"], pairs, True)
            xg.assert_exact_safe(c["Ap"], c["Bp"], pairs, c["unit"], True, extra=xg.BIAS_MAX)
        c["bias"] = xg.int_bias(N, xg.case_rng("x3tn-epi", M, N))
        return c
    return cached(("x3tn", M, N, K), make)


@pytest.mark.parametrize("walk", [None, "general"])
@pytest.mark.parametrize("M,N,K", xg.X3_TN_SHAPES)
def test_x3_tn_and_tnk(M, N, K, walk, dev, monkeypatch):
    if walk:
        monkeypatch.setenv("CDML_X3_WALK", walk)
    c = x3_tn_case(M, N, K)
    c0 = xg.TN_COL0
    Aw, Bw, pa, pb = c["A"].to(dev), c["B"].to(dev), c["plane_a"], c["plane_b"]
    A, B = Aw[:, c0:], Bw[:, c0:]                            # the window as a view: plane strides unchanged
    colsum = sum(c["Bp"]).sum(0)
    with fp.frozen(Aw, Bw, names=["A", "B"]):
        for products in (6, 3):
            S = c["S%d" % products]
            ws = ws_bytes(ops.gemm_bf16x3_workspace(True, M, N, K, products), dev)
            buf, C = out_f32(M, N, dev)
            cs = fp.poisoned(N, dtype=F32, device=dev)
            ops.gemm_bf16x3_tn(A, pa, B, pb, C, M, N, K, products=products, workspace=ws, colsum=cs if products == 6 else None)
            assert_bits(buf, want_f32(S), "tn, products %d" % products)
            if products == 6:
                assert_bits(cs, want_vec(colsum), "tn colsum")
            buf, C = out_f32(M, N, dev, 1)
            ops.gemm_bf16x3_tn(A, pa, B, pb, C, M, N, K, products=products, workspace=ws, bias=to_dev(c["bias"], dev), alpha=ALPHA)
            assert_bits(buf, want_f32(xg.lrelu(S + c["bias"]), 1), "tn + bias, products %d" % products)
        if walk:
            return                                           # (the k8-interleaved entry has one walk and does not read the variable)
        # the k8-interleaved entry on the whole operands, the window given as a_col0 / b_col0
        ma, nb = M + c0, N + c0
        Ai = fp.poisoned(3 * K * ma, dtype=BF16, device=dev)
        Bi = fp.poisoned(3 * K * nb, dtype=BF16, device=dev)
        ops.interleave8_bf16x3(Aw, pa, K, ma, Ai)
        ops.interleave8_bf16x3(Bw, pb, K, nb, Bi)
        want_i = xg.interleave8([torch.from_numpy(p).to(BF16) for p in c["Ap_full"]])
        assert_bits(Ai, want_i, "interleave8 of A")
        assert_bits(Bi, xg.interleave8([torch.from_numpy(p).to(BF16) for p in c["Bp_full"]]), "interleave8 of B")
        ws = ws_bytes(ops.gemm_bf16x3_workspace(True, M, N, K, 6), dev)
        buf, C = out_f32(M, N, dev)
        cs = fp.poisoned(N, dtype=F32, device=dev)
        ops.gemm_bf16x3_tnk(Ai, ma, c0, Bi, nb, c0, C, M, N, K, workspace=ws, colsum=cs)
        assert_bits(buf, want_f32(c["S6"]), "tnk")
        assert_bits(cs, want_vec(colsum), "tnk colsum")


# ---- fp16 two-plane form -----------------------------------------------------------------------------------------------
H2_OUT_SCALE, H2_C_SCALE = 2.0 ** -3, 4.0                   # powers of two: out = out_scale * sum, planes of (out * c_scale)


def h2_nt_case(M, N, K):
    def make():
        Kl = xg.x3_legal_k(K, 3)
        c = xg.plane_case("h2nt", M, N, Kl, n_planes=2)
        c["K"] = Kl
        c["S"] = xg.expected(c["Ap"], c["Bp"], xg.PAIRS_H2) * H2_OUT_SCALE
        xg.assert_exact_safe(c["Ap"], c["Bp"], xg.PAIRS_H2, c["unit"], extra=xg.BIAS_MAX / H2_OUT_SCALE)
        r = xg.case_rng("h2nt-epi", M, N)
        c["bias"], c["aux"] = xg.int_bias(N, r), xg.int_aux(M, N, r)
        return c
    return cached(("h2nt", M, N, K), make)


@pytest.mark.parametrize("walk", [None, "general"])
@pytest.mark.parametrize("M,N,K", xg.F16_NT_SHAPES)
def test_f16x2_nt_every_epilogue(M, N, K, walk, dev, monkeypatch):
    if walk:
        monkeypatch.setenv("CDML_X3_WALK", walk)
    c = h2_nt_case(M, N, K)
    K, S = c["K"], c["S"]
    A, B, pa, pb = c["A"].to(dev), c["B"].to(dev), c["plane_a"], c["plane_b"]
    bias = to_dev(c["bias"], dev)
    ws = ws_bytes(ops.gemm_f16x2_workspace(False, M, N, K), dev) if (M, N) == (520, 256) else None
    kw = dict(alpha=ALPHA, c_scale=H2_C_SCALE)
    act = xg.lrelu(S + c["bias"])
    masked = S * np.where(c["aux"] > 0, 1.0, ALPHA)
    buf, C = out_f32(M, N, dev)
    ops.gemm_f16x2_nt(ops.BE_F32, A, pa, B, pb, C, M, N, K, H2_OUT_SCALE, workspace=ws, **kw)
    assert_bits(buf, want_f32(S), "epilogue 3 (fp32)")
    buf, C = out_f32(M, N, dev, 1)
    ops.gemm_f16x2_nt(ops.BE_BIAS_LRELU_F32, A, pa, B, pb, C, M, N, K, H2_OUT_SCALE, bias=bias, workspace=ws, **kw)
    assert_bits(buf, want_f32(act, 1), "epilogue 1 (bias + lrelu, fp32)")
    out, pc, ld = plane_out(M, N, 2, F16, dev)
    ops.gemm_f16x2_nt(ops.BE_BIAS_LRELU_X3, A, pa, B, pb, out, M, N, K, H2_OUT_SCALE, plane_c=pc, bias=bias, **kw)
    assert_bits(out, want_planes(act * H2_C_SCALE, 2, F16, pc, ld), "epilogue 6 (planes)")
    out, pc, ld = plane_out(M, N, 2, F16, dev)
    ops.gemm_f16x2_nt(ops.BE_MASK_X3, A, pa, B, pb, out, M, N, K, H2_OUT_SCALE, plane_c=pc, aux=aux_buf(c["aux"], dev, F16), **kw)
    assert_bits(out, want_planes(masked * H2_C_SCALE, 2, F16, pc, ld), "epilogue 7 (mask, planes)")
    out, pc, ld = plane_out(M, N, 2, F16, dev)
    bbuf = fp.poisoned((M, N // 8 + 16), dtype=torch.uint8, device=dev)
    ops.gemm_f16x2_nt(ops.BE_BIAS_LRELU_X3_BITS, A, pa, B, pb, out, M, N, K, H2_OUT_SCALE, plane_c=pc, bias=bias, aux=bbuf[:, :N // 8], **kw)
    assert_bits(out, want_planes(act * H2_C_SCALE, 2, F16, pc, ld), "epilogue 9 (planes)")
    assert_bits(bbuf, want_bits(act > 0), "epilogue 9 (sign bits)")
    out, pc, ld = plane_out(M, N, 2, F16, dev)
    ops.gemm_f16x2_nt(ops.BE_MASKBITS_X3, A, pa, B, pb, out, M, N, K, H2_OUT_SCALE, plane_c=pc, aux=bits_buf(c["aux"] > 0, dev), **kw)
    assert_bits(out, want_planes(masked * H2_C_SCALE, 2, F16, pc, ld), "epilogue 10 (mask from bits, planes)")


@pytest.mark.parametrize("walk", [None, "general"])
@pytest.mark.parametrize("M,N,K", xg.F16_TN_SHAPES)
def test_f16x2_tn(M, N, K, walk, dev, monkeypatch):
    if walk:
        monkeypatch.setenv("CDML_X3_WALK", walk)
    c = cached(("h2tn", M, N, K), lambda: xg.plane_case("h2tn", M, N, K, n_planes=2, k_strided=True))
    xg.assert_exact_safe(c["Ap"], c["Bp"], xg.PAIRS_H2, c["unit"], True)
    S = xg.expected(c["Ap"], c["Bp"], xg.PAIRS_H2, True) * H2_OUT_SCALE
    A, B = c["A"].to(dev), c["B"].to(dev)
    buf, C = out_f32(M, N, dev)
    cs = fp.poisoned(N, dtype=F32, device=dev)
    ops.gemm_f16x2_tn(A, c["plane_a"], B, c["plane_b"], C, M, N, K, H2_OUT_SCALE, workspace=ws_bytes(ops.gemm_f16x2_workspace(True, M, N, K), dev),
                      colsum=cs, colsum_scale=0.5)
    assert_bits(buf, want_f32(S), "f16x2 tn")
    assert_bits(cs, want_vec(0.5 * sum(c["Bp"]).sum(0)), "f16x2 tn colsum")


# ---- bf16 GEMMs --------------------------------------------------------------------------------------------------------
def bf16_nt_case(M, N, K):
    def make():
        c = xg.int_case("b16nt", M, N, K)
        c["S"] = xg.expected(c["Ap"], c["Bp"], xg.PAIRS1)
        xg.assert_exact_safe(c["Ap"], c["Bp"], xg.PAIRS1, 1.0, extra=xg.BIAS_MAX)
        r = xg.case_rng("b16nt-epi", M, N)
        c["bias"], c["aux"] = xg.int_bias(N, r), xg.int_aux(M, N, r)
        return c
    return cached(("b16nt", M, N, K), make)


def want_bf16(v):
    v = xg.f32_exact(v).bfloat16()
    buf = fp.poisoned((v.shape[0], v.shape[1] + 8), dtype=BF16, device="cpu")
    buf[:, :v.shape[1]] = v
    return buf


def out_bf16(M, N, dev):
    buf = fp.poisoned((M, N + 8), dtype=BF16, device=dev)
    return buf, buf[:, :N]


# (CDML_BF16_TILE=256 only where the 256 x 256 kernel takes the shape: N % 256 == 0, K % 128 == 0)
BF16_NT_PARAMS = [(M, N, K, tile) for (M, N, K) in xg.BF16_NT_SHAPES for tile in (None, "128", "256")
                  if tile != "256" or not (N % 256 or K % 128)]


@pytest.mark.parametrize("mfma", ["32", "16"])
@pytest.mark.parametrize("M,N,K,tile", BF16_NT_PARAMS)
def test_bf16_nt_every_epilogue(M, N, K, tile, mfma, dev, monkeypatch):
    if tile:
        monkeypatch.setenv("CDML_BF16_TILE", tile)
    monkeypatch.setenv("CDML_BF16_MFMA", mfma)
    c = bf16_nt_case(M, N, K)
    S = c["S"]
    A, B = c["A"].to(dev)[:, :K], c["B"].to(dev)[:, :K]
    bias = to_dev(c["bias"], dev)
    act = xg.lrelu(S + c["bias"])
    masked = S * np.where(c["aux"] > 0, 1.0, ALPHA)
    ws = ws_bytes(ops.gemm_bf16_workspace(M, N, K), dev)
    buf, C = out_f32(M, N, dev)
    ops.gemm_bf16_nt(ops.BE_F32, A, B, C, M, N, K, workspace=ws)
    assert_bits(buf, want_f32(S), "epilogue 3 (fp32; split-K where the dispatcher splits)")
    for w in (None, ws):                                     # single pass / split-K over the workspace: the same bits
        buf, C = out_f32(M, N, dev, 1)
        ops.gemm_bf16_nt(ops.BE_BIAS_LRELU_F32, A, B, C, M, N, K, bias=bias, alpha=ALPHA, workspace=w)
        assert_bits(buf, want_f32(act, 1), "epilogue 1 (workspace %s)" % (w is not None))
    buf, C = out_bf16(M, N, dev)
    ops.gemm_bf16_nt(ops.BE_BIAS_LRELU_BF16, A, B, C, M, N, K, bias=bias, alpha=ALPHA)
    assert_bits(buf, want_bf16(act), "epilogue 0 (bias + lrelu, bf16)")
    buf, C = out_bf16(M, N, dev)
    ops.gemm_bf16_nt(ops.BE_MASK_BF16, A, B, C, M, N, K, aux=aux_buf(c["aux"], dev, BF16), alpha=ALPHA)
    assert_bits(buf, want_bf16(masked), "epilogue 2 (mask, bf16)")
    buf, C = out_bf16(M, N, dev)
    ops.gemm_bf16_nt(ops.BE_MASK_BF16, A, B, C, M, N, K, alpha=ALPHA)
    assert_bits(buf, want_bf16(S), "epilogue 2 without a mask")
    if ops.gemm_bf16_epilogue_supported(ops.BE_BIAS_LRELU_BF16_BITS, M, N, K, A.stride(0), B.stride(0), N + 8, N // 8 + 16):
        buf, C = out_bf16(M, N, dev)
        bbuf = fp.poisoned((M, N // 8 + 16), dtype=torch.uint8, device=dev)
        ops.gemm_bf16_nt(ops.BE_BIAS_LRELU_BF16_BITS, A, B, C, M, N, K, bias=bias, alpha=ALPHA, aux=bbuf[:, :N // 8])
        assert_bits(buf, want_bf16(act), "epilogue 4 (bf16)")
        assert_bits(bbuf, want_bits(act > 0), "epilogue 4 (sign bits)")
    if ops.gemm_bf16_epilogue_supported(ops.BE_MASKBITS_BF16, M, N, K, A.stride(0), B.stride(0), N + 8, N // 8 + 16):
        buf, C = out_bf16(M, N, dev)
        ops.gemm_bf16_nt(ops.BE_MASKBITS_BF16, A, B, C, M, N, K, aux=bits_buf(c["aux"] > 0, dev), alpha=ALPHA)
        assert_bits(buf, want_bf16(masked), "epilogue 5 (mask from bits, bf16)")


def bf16_tn_case(tag, M, N, K):
    def make():
        c = xg.int_case(tag, M, N, K, k_strided=True)
        c["S"] = xg.expected(c["Ap"], c["Bp"], xg.PAIRS1, True)
        xg.assert_exact_safe(c["Ap"], c["Bp"], xg.PAIRS1, 1.0, True)
        return c
    return cached((tag, M, N, K), make)


@pytest.mark.parametrize("mfma", ["32", "16"])
@pytest.mark.parametrize("M,N,K", xg.BF16_TN_SHAPES)
def test_bf16_tn(M, N, K, mfma, dev, monkeypatch):
    monkeypatch.setenv("CDML_BF16_MFMA", mfma)
    c = bf16_tn_case("b16tn", M, N, K)
    A, B = c["A"].to(dev)[:, :M], c["B"].to(dev)[:, :N]
    buf, C = out_f32(M, N, dev)
    cs = fp.poisoned(N, dtype=F32, device=dev)
    ops.gemm_bf16_tn(A, B, C, M, N, K, workspace=ws_bytes(ops.gemm_bf16_tn_workspace(M, N, K), dev), colsum=cs)
    assert_bits(buf, want_f32(c["S"]), "bf16 tn")
    assert_bits(cs, want_vec(c["Bp"][0].sum(0)), "bf16 tn colsum")


@pytest.mark.parametrize("mfma", ["32", "16"])
@pytest.mark.parametrize("M1,N1,M2,N2,K", xg.BF16_TN2_SHAPES)
def test_bf16_tn2(M1, N1, M2, N2, K, mfma, dev, monkeypatch):
    monkeypatch.setenv("CDML_BF16_MFMA", mfma)
    c1, c2 = bf16_tn_case("b16tn2a", M1, N1, K), bf16_tn_case("b16tn2b", M2, N2, K)
    nbytes = ops.gemm_bf16_tn2_workspace(M1, N1, M2, N2, K)
    assert nbytes > 0
    b1, C1 = out_f32(M1, N1, dev)
    b2, C2 = out_f32(M2, N2, dev, 1)
    cs1, cs2 = fp.poisoned(N1, dtype=F32, device=dev), fp.poisoned(N2, dtype=F32, device=dev)
    ops.gemm_bf16_tn2(c1["A"].to(dev)[:, :M1], c1["B"].to(dev)[:, :N1], C1, M1, N1, c2["A"].to(dev)[:, :M2], c2["B"].to(dev)[:, :N2], C2, M2, N2,
                      K, ws_bytes(nbytes, dev), colsum1=cs1, colsum2=cs2)
    assert_bits(b1, want_f32(c1["S"]), "tn2, first product")
    assert_bits(b2, want_f32(c2["S"], 1), "tn2, second product")
    assert_bits(cs1, want_vec(c1["Bp"][0].sum(0)), "tn2 colsum 1")
    assert_bits(cs2, want_vec(c2["Bp"][0].sum(0)), "tn2 colsum 2")


# ---- fp32 MFMA kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", xg.FC_SHAPES)
def test_fc_kernels(M, K, N, dev):
    c = cached(("fc", M, K, N), lambda: xg.fc_case(M, K, N))
    r = xg.case_rng("fc-epi", M, K, N)
    Kb = xg.fc_k64(K)
    bias, post = xg.int_bias(N, r), xg.int_aux(M, Kb, r)
    f = c["fwd"]
    xg.assert_exact_safe(f["Ap"], f["Bp"], xg.PAIRS1, 1.0, extra=xg.BIAS_MAX)
    buf, y = out_f32(M, N, dev)
    ops.fc_lrelu_fwd(f["A"].to(dev)[:, :K], f["B"].to(dev)[:, :N], to_dev(bias, dev), y, M, K, N, alpha=ALPHA)
    assert_bits(buf, want_f32(xg.lrelu(xg.expected(f["Ap"], f["Bp"], xg.PAIRS1) + bias)), "fc_lrelu_fwd")
    b = c["bwd_data"]                                        # dx[M][K] = dy[M][N] . W[K][N]^T (times lrelu' of x_post)
    xg.assert_exact_safe(b["Ap"], b["Bp"], xg.PAIRS1, 1.0)
    S = xg.expected(b["Ap"], b["Bp"], xg.PAIRS1)
    dy, W = b["A"].to(dev)[:, :N], b["B"].to(dev)[:, :N]
    buf, dx = out_f32(M, Kb, dev)
    ops.fc_bwd_data(dy, W, aux_buf(post, dev, F32), dx, M, Kb, N, alpha=ALPHA)
    assert_bits(buf, want_f32(S * np.where(post > 0, 1.0, ALPHA)), "fc_bwd_data")
    buf, dx = out_f32(M, Kb, dev, 1)
    ops.fc_bwd_data(dy, W, None, dx, M, Kb, N, alpha=ALPHA)
    assert_bits(buf, want_f32(S, 1), "fc_bwd_data without a mask")
    w = c["bwd_weight"]                                      # dW[K][N] = x[M][K]^T . dy[M][N], db = column sums of dy
    xg.assert_exact_safe(w["Ap"], w["Bp"], xg.PAIRS1, 1.0, True)
    buf, dW = out_f32(Kb, N, dev)
    db = fp.poisoned(N, dtype=F32, device=dev)
    ops.fc_bwd_weight(w["A"].to(dev)[:, :Kb], w["B"].to(dev)[:, :N], dW, db, ws_bytes(ops.fc_bwd_weight_workspace(M, Kb, N), dev), M, Kb, N)
    assert_bits(buf, want_f32(xg.expected(w["Ap"], w["Bp"], xg.PAIRS1, True)), "fc_bwd_weight")
    assert_bits(db, want_vec(w["Bp"][0].sum(0)), "fc_bwd_weight bias gradient")


def test_fc_bwd_weight2_stream_k(dev):
    M, K1, N1, K2, N2 = xg.FC_SK_SHAPE
    nbytes = ops.fc_bwd_weight2_workspace(M, K1, N1, K2, N2)
    assert nbytes > 0, "the stream-K launch does not take the shape"
    c1 = xg.int_case("fcsk1", K1, N1, M, k_strided=True, dtype=F32)
    c2 = xg.int_case("fcsk2", K2, N2, M, k_strided=True, dtype=F32)
    for c in (c1, c2):
        xg.assert_exact_safe(c["Ap"], c["Bp"], xg.PAIRS1, 1.0, True)
    b1, dW1 = out_f32(K1, N1, dev)
    b2, dW2 = out_f32(K2, N2, dev, 1)
    db1, db2 = fp.poisoned(N1, dtype=F32, device=dev), fp.poisoned(N2, dtype=F32, device=dev)
    ops.fc_bwd_weight2(c1["A"].to(dev)[:, :K1], c1["B"].to(dev)[:, :N1], dW1, db1, K1, N1, c2["A"].to(dev)[:, :K2], c2["B"].to(dev)[:, :N2],
                       dW2, db2, K2, N2, M, ws_bytes(nbytes, dev))
    assert_bits(b1, want_f32(xg.expected(c1["Ap"], c1["Bp"], xg.PAIRS1, True)), "fc_bwd_weight2, first layer")
    assert_bits(b2, want_f32(xg.expected(c2["Ap"], c2["Bp"], xg.PAIRS1, True), 1), "fc_bwd_weight2, second layer")
    assert_bits(db1, want_vec(c1["Bp"][0].sum(0)), "db1")
    assert_bits(db2, want_vec(c2["Bp"][0].sum(0)), "db2")


# ---- the probe: one-hot rows against large integers; a mismatch names the index that was read ---------------------------
# Cases: xg.PROBE_CASES (two shapes per entry), the same objects tests/test_exact_gemm_host.py checks; xg.probe_want computes
# assert_exact_safe on the planes the kernel multiplies before every launch.
def probe_ids(cases):
    return [c["name"] for c in cases]


def probe_planes(v, n_planes, dtype, dev):
    """float32 numpy [rows][cols] -> (device plane buffer with poisoned gaps, plane): the torch split"""
    rows, cols = v.shape
    plane = cols + 8
    buf = xg.plane_buffer(xg.split_planes(torch.from_numpy(v), n_planes, dtype), plane, n_planes * plane + 8)
    return buf.to(dev), plane


def project_split3(v, dev):
    """the project's own split of an fp32 operand, into a poisoned buffer; checked against the torch split"""
    rows, cols = v.shape
    plane = cols + 8
    dst = fp.poisoned((rows, 3 * plane + 8), dtype=BF16, device=dev)
    ops.split_f32_bf16x3(torch.from_numpy(v).to(dev), dst, plane)
    want, _ = probe_planes(v, 3, BF16, "cpu")
    assert_bits(dst, want, "split_f32_bf16x3")
    return dst, plane


def project_split2(v, dev):
    rows, cols = v.shape
    plane = cols + 8
    dst = fp.poisoned((rows, 2 * plane + 8), dtype=F16, device=dev)
    ops.split_f32_f16x2(torch.from_numpy(v).to(dev), dst, plane, xg.H2_PROBE_SCALE)
    want, _ = probe_planes(v * np.float32(xg.H2_PROBE_SCALE), 2, F16, "cpu")
    assert_bits(dst, want, "split_f32_f16x2")
    return dst, plane


def mat(v, dev, dtype):
    """a one-plane operand as a view into a wider poisoned buffer"""
    return aux_buf(v.astype(np.float64), dev, dtype)


def check_probe(c, C, src, want, what, buf=None):
    xg.assert_probe(C.double().cpu().numpy(), src, c["pi"], c["k_strided"], want=want, what="%s %s" % (c["name"], what))
    if buf is not None:
        assert_bits(buf, want_f32(want), what)


# (every case under each product count that takes its K: products * K / 64 must be even -- K = 192 under six products only)
X3_NT_PROBES = [(c, products) for c in xg.probe_cases("x3_nt") for products in (6, 3) if (products * c["shape"][2] // 64) % 2 == 0]


@pytest.mark.parametrize("walk", ["r6", "general", "f6"])
@pytest.mark.parametrize("c,products", X3_NT_PROBES, ids=["%s products=%d" % (c["name"], p) for c, p in X3_NT_PROBES])
def test_probe_x3_nt(c, products, walk, dev, monkeypatch):
    M, N, K = c["shape"]
    monkeypatch.setenv("CDML_X3_WALK", walk)
    src, want = xg.probe_want(c, xg.PAIRS6 if products == 6 else xg.PAIRS3)
    A3, pa = probe_planes(c["A"], 3, BF16, dev)
    B3, pb = project_split3(c["B"], dev)
    tag = "products=%d walk=%s" % (products, walk)
    buf, C = out_f32(M, N, dev)
    ops.gemm_bf16x3_nt(ops.BE_F32, A3, pa, B3, pb, C, M, N, K, products=products)
    check_probe(c, C, src, want, "fp32 " + tag, buf)
    out, pc, ld = plane_out(M, N, 3, BF16, dev)
    ops.gemm_bf16x3_nt(ops.BE_MASK_X3, A3, pa, B3, pb, out, M, N, K, products=products, plane_c=pc)
    check_probe(c, sum(out[:, p * pc:p * pc + N].double() for p in range(3)), src, want, "planes " + tag)
    assert_bits(out, want_planes(want, 3, BF16, pc, ld), "x3_nt planes")
    if M % 8 == 0:
        ldc = N + 8
        plane_c = M * ldc + 64
        flat = fp.poisoned(3 * plane_c, dtype=BF16, device=dev)
        ops.gemm_bf16x3_nt(ops.BE_MASKBITS_X3_KI, A3, pa, B3, pb, flat, M, N, K, products=products, plane_c=plane_c, ldc=ldc)
        got = sum(flat[p * plane_c:p * plane_c + M * ldc].view(M // 8, ldc, 8)[:, :N, :].permute(0, 2, 1).reshape(M, N).double()
                  for p in range(3))
        check_probe(c, got, src, want, "k8-interleaved output " + tag)
        assert_bits(flat, want_ki(want, ldc, plane_c), "x3_nt k8-interleaved planes")


@pytest.mark.parametrize("walk", ["r6", "general"])
@pytest.mark.parametrize("c", xg.probe_cases("x3_tn"), ids=probe_ids(xg.probe_cases("x3_tn")))
def test_probe_x3_tn_and_tnk(c, walk, dev, monkeypatch):
    monkeypatch.setenv("CDML_X3_WALK", walk)
    M, N, K = c["shape"]
    A3, pa = probe_planes(c["A"], 3, BF16, dev)
    B3, pb = project_split3(c["B"], dev)
    for products, pairs in ((6, xg.PAIRS6), (3, xg.PAIRS3)):
        src, want = xg.probe_want(c, pairs)
        buf, C = out_f32(M, N, dev)
        ops.gemm_bf16x3_tn(A3, pa, B3, pb, C, M, N, K, products=products, workspace=ws_bytes(ops.gemm_bf16x3_workspace(True, M, N, K, products), dev))
        check_probe(c, C, src, want, "tn products=%d walk=%s" % (products, walk), buf)
    if walk != "r6":
        return                                               # (the k8-interleaved entry has one walk and does not read the variable)
    src, want = xg.probe_want(c, xg.PAIRS6)
    Ai = fp.poisoned(3 * K * M, dtype=BF16, device=dev)
    Bi = fp.poisoned(3 * K * N, dtype=BF16, device=dev)
    ops.interleave8_bf16x3(A3, pa, K, M, Ai)
    ops.interleave8_bf16x3(B3, pb, K, N, Bi)
    buf, C = out_f32(M, N, dev)
    ops.gemm_bf16x3_tnk(Ai, M, 0, Bi, N, 0, C, M, N, K, workspace=ws_bytes(ops.gemm_bf16x3_workspace(True, M, N, K, 6), dev))
    check_probe(c, C, src, want, "tnk", buf)


@pytest.mark.parametrize("walk", ["r6", "general"])
@pytest.mark.parametrize("c", xg.probe_cases("f16x2_nt") + xg.probe_cases("f16x2_tn"),
                         ids=probe_ids(xg.probe_cases("f16x2_nt") + xg.probe_cases("f16x2_tn")))
def test_probe_f16x2(c, walk, dev, monkeypatch):
    monkeypatch.setenv("CDML_X3_WALK", walk)
    (M, N, K), ks = c["shape"], c["k_strided"]
    src, want = xg.probe_want(c, xg.PAIRS_H2)
    A2, pa = probe_planes(c["A"], 2, F16, dev)
    B2, pb = project_split2(c["B"], dev)
    buf, C = out_f32(M, N, dev)
    if ks:
        ops.gemm_f16x2_tn(A2, pa, B2, pb, C, M, N, K, 1.0 / xg.H2_PROBE_SCALE, workspace=ws_bytes(ops.gemm_f16x2_workspace(True, M, N, K), dev))
    else:
        ops.gemm_f16x2_nt(ops.BE_F32, A2, pa, B2, pb, C, M, N, K, 1.0 / xg.H2_PROBE_SCALE)
    check_probe(c, C, src, want, "walk=%s" % walk, buf)


@pytest.mark.parametrize("mfma", ["32", "16"])
@pytest.mark.parametrize("tile", [None, "128", "256"])
@pytest.mark.parametrize("c", xg.probe_cases("bf16_nt"), ids=probe_ids(xg.probe_cases("bf16_nt")))
def test_probe_bf16_nt(c, tile, mfma, dev, monkeypatch):
    if tile:
        monkeypatch.setenv("CDML_BF16_TILE", tile)           # (both probe shapes are legal on both tile sizes)
    monkeypatch.setenv("CDML_BF16_MFMA", mfma)
    M, N, K = c["shape"]
    src, want = xg.probe_want(c, xg.PAIRS1)
    dA, dB = mat(c["A"], dev, BF16), mat(c["B"], dev, BF16)
    buf, C = out_f32(M, N, dev)
    ops.gemm_bf16_nt(ops.BE_F32, dA, dB, C, M, N, K, workspace=ws_bytes(ops.gemm_bf16_workspace(M, N, K), dev))
    check_probe(c, C, src, want, "fp32 tile=%s mfma=%s" % (tile, mfma), buf)
    buf, C = out_bf16(M, N, dev)
    ops.gemm_bf16_nt(ops.BE_MASK_BF16, dA, dB, C, M, N, K, alpha=ALPHA)      # (K = 256, M N >= 2^22, no forced tile: the streaming kernel)
    check_probe(c, C, src, want, "bf16 out tile=%s mfma=%s" % (tile, mfma))
    assert_bits(buf, want_bf16(want), "bf16_nt probe, bf16 out")


@pytest.mark.parametrize("mfma", ["32", "16"])
@pytest.mark.parametrize("c", xg.probe_cases("bf16_tn"), ids=probe_ids(xg.probe_cases("bf16_tn")))
def test_probe_bf16_tn(c, mfma, dev, monkeypatch):
    monkeypatch.setenv("CDML_BF16_MFMA", mfma)
    M, N, K = c["shape"]
    src, want = xg.probe_want(c, xg.PAIRS1)
    buf, C = out_f32(M, N, dev)
    ops.gemm_bf16_tn(mat(c["A"], dev, BF16), mat(c["B"], dev, BF16), C, M, N, K, workspace=ws_bytes(ops.gemm_bf16_tn_workspace(M, N, K), dev))
    check_probe(c, C, src, want, "mfma=%s" % mfma, buf)


@pytest.mark.parametrize("mfma", ["32", "16"])
@pytest.mark.parametrize("which", ["bf16_tn2a", "bf16_tn2b"])
def test_probe_bf16_tn2(which, mfma, dev, monkeypatch):
    """the joint stream-K launch (unit -> tile / k map, fix-up pass): both products one-hot probes at once"""
    monkeypatch.setenv("CDML_BF16_MFMA", mfma)
    (c1,), (c2,) = xg.probe_cases(which + "/1"), xg.probe_cases(which + "/2")
    (M1, N1, K), (M2, N2, K2) = c1["shape"], c2["shape"]
    assert K == K2
    (s1, w1), (s2, w2) = xg.probe_want(c1, xg.PAIRS1), xg.probe_want(c2, xg.PAIRS1)
    nbytes = ops.gemm_bf16_tn2_workspace(M1, N1, M2, N2, K)
    assert nbytes > 0
    b1, C1 = out_f32(M1, N1, dev)
    b2, C2 = out_f32(M2, N2, dev)
    ops.gemm_bf16_tn2(mat(c1["A"], dev, BF16), mat(c1["B"], dev, BF16), C1, M1, N1, mat(c2["A"], dev, BF16), mat(c2["B"], dev, BF16), C2, M2, N2,
                      K, ws_bytes(nbytes, dev))
    check_probe(c1, C1, s1, w1, "first product mfma=%s" % mfma, b1)
    check_probe(c2, C2, s2, w2, "second product mfma=%s" % mfma, b2)


@pytest.mark.parametrize("c", xg.probe_cases("fc_fwd"), ids=probe_ids(xg.probe_cases("fc_fwd")))
def test_probe_fc_fwd(c, dev):
    """x one-hot [M][K], W integers [K][N] (the probe's B = W^T): y[m][n] = lrelu(W[pi(m)][n])"""
    M, N, K = c["shape"]
    src, want = xg.probe_want(c, xg.PAIRS1)
    W = np.ascontiguousarray(c["B"].T)
    buf, y = out_f32(M, N, dev)
    ops.fc_lrelu_fwd(mat(c["A"], dev, F32), mat(W, dev, F32), torch.zeros(N, device=dev), y, M, K, N, alpha=ALPHA)
    check_probe(c, y, xg.lrelu(src), xg.lrelu(want), "fc_lrelu_fwd", buf)      # (an integer below 2^22 times 1/4: exact)


@pytest.mark.parametrize("c", xg.probe_cases("fc_bwd_data"), ids=probe_ids(xg.probe_cases("fc_bwd_data")))
def test_probe_fc_bwd_data(c, dev):
    """dy one-hot [M][N], W integers [K][N]: dx[m][k] = W[k][pi(m)]  (the probe's N = the layer's K, its K the layer's N)"""
    M, Kl, Nl = c["shape"]
    src, want = xg.probe_want(c, xg.PAIRS1)
    buf, dx = out_f32(M, Kl, dev)
    ops.fc_bwd_data(mat(c["A"], dev, F32), mat(c["B"], dev, F32), None, dx, M, Kl, Nl, alpha=ALPHA)
    check_probe(c, dx, src, want, "fc_bwd_data", buf)


@pytest.mark.parametrize("c", xg.probe_cases("fc_bwd_weight"), ids=probe_ids(xg.probe_cases("fc_bwd_weight")))
def test_probe_fc_bwd_weight(c, dev):
    """x [R][K] with one 1 per column, dy integers [R][N]: dW[k][n] = dy[pi(k)][n]"""
    Kl, Nl, R = c["shape"]
    src, want = xg.probe_want(c, xg.PAIRS1)
    buf, dW = out_f32(Kl, Nl, dev)
    db = fp.poisoned(Nl, dtype=F32, device=dev)              # (the column sums of 2^22-sized integers are not exact: not compared)
    ops.fc_bwd_weight(mat(c["A"], dev, F32), mat(c["B"], dev, F32), dW, db, ws_bytes(ops.fc_bwd_weight_workspace(R, Kl, Nl), dev), R, Kl, Nl)
    check_probe(c, dW, src, want, "fc_bwd_weight", buf)


def test_probe_fc_bwd_weight2(dev):
    """the fp32 stream-K pair at FC_SK_SHAPE, both layers one-hot probes at once"""
    (c1,), (c2,) = xg.probe_cases("fc_bwd_weight2/1"), xg.probe_cases("fc_bwd_weight2/2")
    (K1, N1, M), (K2, N2, M2) = c1["shape"], c2["shape"]
    assert (M, K1, N1, K2, N2) == xg.FC_SK_SHAPE and M2 == M
    (s1, w1), (s2, w2) = xg.probe_want(c1, xg.PAIRS1), xg.probe_want(c2, xg.PAIRS1)
    nbytes = ops.fc_bwd_weight2_workspace(M, K1, N1, K2, N2)
    assert nbytes > 0
    b1, dW1 = out_f32(K1, N1, dev)
    b2, dW2 = out_f32(K2, N2, dev)
    db1, db2 = fp.poisoned(N1, dtype=F32, device=dev), fp.poisoned(N2, dtype=F32, device=dev)
    ops.fc_bwd_weight2(mat(c1["A"], dev, F32), mat(c1["B"], dev, F32), dW1, db1, K1, N1, mat(c2["A"], dev, F32), mat(c2["B"], dev, F32),
                       dW2, db2, K2, N2, M, ws_bytes(nbytes, dev))
    check_probe(c1, dW1, s1, w1, "first layer", b1)
    check_probe(c2, dW2, s2, w2, "second layer", b2)
