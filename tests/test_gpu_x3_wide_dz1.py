"""The first layer's weight gradient with dz1 as the WIDE operand (include/cdml_x3_wide.h, cdml_gemm_bf16x3_tn_kb): dz1
k8-interleaved, x_hat row-major as the gather writes it, the kernel's waves tiled 64 x 128 so that two thirds of the fragment
reads are single 16-B reads.  Same images, slots, DMA schedule, product order and K partition as the row-major k-strided
product, so C must have ITS bits, and so must the column sums of dz1 (the bias gradient); against fp64 the column sums keep
the bound of test_split_k_geometry_has_no_empty_split in tests/test_gpu_f32x3.py: 1e-4 absolute."""
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

F32, BF16 = torch.float32, torch.bfloat16
COLSUM_ATOL = 1e-4          # tests/test_gpu_f32x3.py: (cs.double() - B.double().sum(0)).abs().max() < 1e-4
_CACHE = {}


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


def _planes(x, plane):
    """reference split in torch: [rows][hi | mid | lo], `plane` columns apart"""
    hi = x.to(BF16)
    r = x - hi.float()
    mid = r.to(BF16)
    lo = (r - mid.float()).to(BF16)
    out = torch.zeros(x.shape[0], 3 * plane, dtype=BF16, device=x.device)
    for p, t in enumerate((hi, mid, lo)):
        out[:, p * plane:p * plane + x.shape[1]] = t
    return out


def _ws_bytes(M, N, K):
    return max(ops.gemm_bf16x3_workspace(True, M, N, K, 6), 16)


def _slabs(M, N, K):
    """the slab count of the k-strided entries at this shape, from the workspace query: bytes = slabs * M * N * 4 (the slabs)
    + slabs * (M / 256) * 2 * N * 4 (the bias-gradient partials) + N * 4"""
    n = ops.gemm_bf16x3_workspace(True, M, N, K, 6) - 4 * N
    per = 4 * N * (M + 2 * (M // 256))
    assert n % per == 0
    return n // per


def _smallest_split_k():
    """the smallest K (a multiple of 128) at which the one-tile product is split into >= 2 slabs"""
    if "k2" not in _CACHE:
        _CACHE["k2"] = next(K for K in range(128, 1 << 16, 128) if _slabs(256, 256, K) >= 2)
    return _CACHE["k2"]


def _shapes():
    # (M, N, K, lo = column window into a wider x_hat); K of the split case is filled in on the GPU box's own rule
    return [("one tile", 256, 256, 128, 0), ("two slabs", 256, 256, None, 0), ("M 512, window", 512, 256, 256, 256),
            ("N 512", 256, 512, 256, 0)]


def _case(dev, M, N, K, lo):
    """random fp32 operands split into planes (shared by the tests of a shape, never modified): x_hat [K][lo + M + 256]
    row-major planes, dz1 [K][N + 256] row-major planes and k8-interleaved, the product's window at column 256 of dz1 when
    the shape has room for one"""
    key = (M, N, K, lo)
    if key not in _CACHE:
        g = torch.Generator(device=dev); g.manual_seed(M + 3 * N + 7 * K + lo)
        ma, b0 = lo + M + 256, 256
        nb = N + b0
        A = torch.randn(K, ma, device=dev, generator=g) * 0.05
        B = torch.randn(K, nb, device=dev, generator=g) * 0.02
        A3, B3 = _planes(A, ma), _planes(B, nb)
        Bi = fp.poisoned(3 * K * nb, dtype=BF16, device=dev)
        ops.interleave8_bf16x3(B3, nb, K, nb, Bi)
        _CACHE[key] = dict(A=A, B=B, A3=A3, B3=B3, Bi=Bi, ma=ma, nb=nb, b0=b0)
    return _CACHE[key]


@pytest.mark.parametrize("with_colsum", [True, False])
@pytest.mark.parametrize("shape", _shapes(), ids=[s[0] for s in _shapes()])
def test_product_has_the_bits_of_the_row_major_form(shape, with_colsum, dev):
    _, M, N, K, lo = shape
    if K is None:
        K = _smallest_split_k()
        assert _slabs(M, N, K) >= 2 and (K == 128 or _slabs(M, N, K - 128) < 2)
    c = _case(dev, M, N, K, lo)
    ma, nb, b0 = c["ma"], c["nb"], c["b0"]
    ws = fp.poisoned(_ws_bytes(M, N, K) // 4, dtype=F32, device=dev)
    gs = [fp.Guarded((M, N), F32, dev, pattern=p) for p in (0, 1)] + [fp.Guarded((N,), F32, dev, pattern=p) for p in (0, 1)]
    C1, C2, cs1, cs2 = (g.view for g in gs)
    with fp.frozen(c["A3"], c["B3"], c["Bi"], names=["x_hat", "dz1", "dz1 interleaved"]):
        ops.gemm_bf16x3_tn(c["A3"][:, lo:], ma, c["B3"][:, b0:], nb, C1, M, N, K, workspace=ws, colsum=cs1 if with_colsum else None)
        ops.gemm_bf16x3_tn_kb(c["A3"][:, lo:], ma, c["Bi"], nb, b0, C2, M, N, K, workspace=ws, colsum=cs2 if with_colsum else None)
        torch.cuda.synchronize()
    for g in gs:
        g.assert_guards_intact()
    want = c["A"][:, lo:lo + M].double().t() @ c["B"][:, b0:b0 + N].double()
    rel = ((C2.double() - want).abs().max() / want.abs().max()).item()
    print("M %d N %d K %d lo %d: %d slabs, rel max against fp64 %.3g" % (M, N, K, lo, _slabs(M, N, K), rel))
    assert torch.equal(C1.view(torch.int32), C2.view(torch.int32))
    assert rel < 5e-6
    if with_colsum:
        ref = c["B"][:, b0:b0 + N].double().sum(0)
        e1, e2 = (cs1.double() - ref).abs().max().item(), (cs2.double() - ref).abs().max().item()
        print("colsum against fp64: row-major %.3g, wide dz1 %.3g" % (e1, e2))
        assert e2 < COLSUM_ATOL
        assert torch.equal(cs1.view(torch.int32), cs2.view(torch.int32))      # the same partition of K, the same order
    else:                                                    # no colsum asked for: none written
        assert torch.equal(fp.bits_of(cs2), fp.bits_of(fp.poisoned(N, dtype=F32, device=dev, pattern=1)))


@pytest.mark.parametrize("M,N,K", xg.X3_TN_SHAPES)
def test_exact_arithmetic_pins_the_k_index_and_the_store(M, N, K, dev):
    """Operands whose six-product sum is exact in fp32 (tests/exact_gemm.py), as column windows of wider operands, against
    integer host arithmetic: a wrong k, plane pair, row or column (M != N: a transposed or misplaced block) changes the bits.
    The column sums are exact too, so any partition of K must give them."""
    c = xg.tn_window_case(M, N, K)
    S = xg.expected(c["Ap"], c["Bp"], xg.PAIRS6, True)
    xg.assert_exact_safe(c["Ap"], c["Bp"], xg.PAIRS6, c["unit"], True)
    c0 = xg.TN_COL0
    Aw, Bw, pa, pb = c["A"].to(dev), c["B"].to(dev), c["plane_a"], c["plane_b"]
    nb = N + c0
    Bi = fp.poisoned(3 * K * nb, dtype=BF16, device=dev)
    ops.interleave8_bf16x3(Bw, pb, K, nb, Bi)
    ws = fp.poisoned(_ws_bytes(M, N, K) // 4 + 4, dtype=F32, device=dev)
    buf = fp.poisoned((M, N + 4), dtype=F32, device=dev)
    cs = fp.poisoned(N, dtype=F32, device=dev)
    with fp.frozen(Aw, Bi, names=["A", "B interleaved"]):
        ops.gemm_bf16x3_tn_kb(Aw[:, c0:], pa, Bi, nb, c0, buf[:, :N], M, N, K, workspace=ws, colsum=cs)
        torch.cuda.synchronize()
    want = fp.poisoned((M, N + 4), dtype=F32, device="cpu")
    want[:, :N] = xg.f32_exact(S)
    got = buf.cpu()
    bad = xg.bits(got) != xg.bits(want)
    assert not bool(bad.any()), "%d of %d elements differ; first at %s" % (int(bad.sum()), bad.numel(), tuple(torch.nonzero(bad)[0].tolist()))
    assert torch.equal(xg.bits(cs.cpu()), xg.bits(xg.f32_exact(np.asarray(sum(c["Bp"]).sum(0), dtype=np.float64))))


@pytest.mark.parametrize("split", [False, True], ids=["one pass", "slabs"])
def test_write_footprint(split, dev):
    """C (ldc > N), the colsum and the workspace (exactly the queried bytes) in guarded buffers under two poisons: every
    element of C and colsum is stored, nothing beside them is, the operands come back bit-identical."""
    M, N, lo = 512, 256, 256
    # (the slab count is a function of the tile count too: queried for this shape)
    K = next(k for k in range(128, 1 << 16, 128) if _slabs(M, N, k) >= 2) if split else 256
    assert (_slabs(M, N, K) >= 2) == split
    c = _case(dev, M, N, K, lo)
    ma, nb, b0 = c["ma"], c["nb"], c["b0"]
    gC = fp.Guarded((M, N), F32, dev, ld=N + 12)
    gcs = fp.Guarded((N,), F32, dev)
    gws = fp.Guarded((ops.gemm_bf16x3_workspace(True, M, N, K, 6) // 4,), F32, dev)

    def run(pattern):
        for g in (gC, gcs, gws):
            g.rearm(pattern)
        with fp.frozen(c["A3"], c["Bi"], names=["x_hat", "dz1 interleaved"]):
            ops.gemm_bf16x3_tn_kb(c["A3"][:, lo:], ma, c["Bi"], nb, b0, gC.view, M, N, K, workspace=gws.view, colsum=gcs.view)
            torch.cuda.synchronize()
        for g, name in ((gC, "C"), (gcs, "colsum"), (gws, "workspace")):
            g.assert_guards_intact(name)
        return {"C": gC.payload(), "colsum": gcs.payload()}

    got = fp.assert_fully_written(run)
    want = c["A"][:, lo:lo + M].double().t() @ c["B"][:, b0:b0 + N].double()
    assert ((got["C"].double() - want).abs().max() / want.abs().max()).item() < 5e-6
    assert (got["colsum"].double() - c["B"][:, b0:b0 + N].double().sum(0)).abs().max().item() < COLSUM_ATOL


def test_arguments_are_checked(dev):
    from cdml_amd import _lib
    M = N = K = 256
    A3 = torch.zeros(K, 3 * M, dtype=BF16, device=dev)
    Bi = torch.zeros(3 * K * N, dtype=BF16, device=dev)
    C = torch.zeros(M, N, device=dev)
    for bad in (dict(M=200), dict(K=192), dict(b_col0=8), dict(nb=N + 4)):
        a = dict(M=M, N=N, K=K, b_col0=0, nb=N)
        a.update(bad)
        with pytest.raises(_lib.CdmlError):
            ops.gemm_bf16x3_tn_kb(A3, M, Bi, a["nb"], a["b_col0"], C, a["M"], a["N"], a["K"])
    k2 = _smallest_split_k()
    with pytest.raises(_lib.CdmlError, match="workspace"):   # slabs need the workspace
        ops.gemm_bf16x3_tn_kb(torch.zeros(k2, 3 * M, dtype=BF16, device=dev), M, torch.zeros(3 * k2 * N, dtype=BF16, device=dev),
                              N, 0, C, M, N, k2)


def test_train_step_with_wide_dz1_is_the_row_major_step(dev, monkeypatch):
    """TrainStep at the smallest plane shape (F = H = D = 256, B = 128, in-batch, Adam) on the default path -- dz1 held
    k8-interleaved only, dW1 on the wide-dz1 product -- against the row-major path from identical weights and triplets:
    after one step loss, embeddings, gradients and weights have the same bits (gb1 is also held to the colsum bound the
    issue sets); three steps run."""
    from cdml_amd import engine, train
    N, F, B = 3000, 256, 128
    table = engine.FeatureTable.synthetic(N, F, 0, dev)
    rng = np.random.RandomState(1)
    pairs = rng.randint(0, N, size=(2000, 2)).astype(np.int32)
    pairs = torch.from_numpy(pairs[pairs[:, 0] != pairs[:, 1]]).to(dev)
    real = engine.Engine.workspace

    def mk(wide):
        with monkeypatch.context() as m:
            if not wide:
                m.setattr(engine.Engine, "workspace", lambda self, *a, **k: real(self, *a, **dict(k, wide_dz1=False)))
            return train.TrainStep(table, pairs, B, hidden_size=256, output_size=256, mode="inbatch", optimizer="adam",
                                   base_learning_rate=0.01, device=dev, precision="f32x3")
    a, b = mk(False), mk(True)
    assert b.ws.wide_dz1 and b.ws.dz1 is None and b.ws.dz1k is not None and b.ws.xk is None
    assert not a.ws.wide_dz1 and a.ws.dz1 is not None and a.ws.dz1k is None
    assert torch.equal(a.params.flat, b.params.flat)
    a.step(); b.step()
    torch.cuda.synchronize()
    pa, pb = a.params, b.params
    assert torch.equal(a.idx, b.idx) and a.loss() == b.loss()
    assert torch.equal(a.ws.e, b.ws.e) and torch.equal(a.ws.dz1_f32(), b.ws.dz1_f32())
    for name in ("gW1", "gW2", "gb2", "W1", "W2", "b2"):
        assert torch.equal(getattr(pa, name), getattr(pb, name)), name
    d = (pa.gb1.double() - pb.gb1.double()).abs().max().item()
    print("gb1: max |row-major - wide| = %.3g (max |gb1| %.3g)" % (d, pa.gb1.abs().max().item()))
    assert d < COLSUM_ATOL
    assert (pb.gb1.double() - b.ws.dz1_f32().double().sum(0)).abs().max().item() < COLSUM_ATOL
    for _ in range(2):
        a.step(); b.step()
    torch.cuda.synchronize()
    assert np.isfinite(b.loss()) and bool(torch.isfinite(pb.flat).all())
