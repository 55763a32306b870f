"""Every launch of tests/footprint_table.py run into poisoned, guarded buffers (tests/footprint.py): the launch must store
every payload element of its outputs (two runs under two poison patterns, bit-identical, no poison left), write nothing
in front of, behind or in the row / plane gaps of ANY buffer (inputs and workspaces included; workspaces are exactly
the queried size with the guard right behind), leave its inputs bit-identical, and match the fp64 reference at the
tolerance the entry point's own test uses.  Shapes are small: every launch finishes in milliseconds."""
import contextlib
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import footprint_table as table  # noqa: E402
import npair_logq_ref  # noqa: E402
import npair_memory_ref  # noqa: E402
import npair_ref  # noqa: E402
from cdml_amd import ops  # noqa: E402
from oracle import sampler as osampler  # noqa: E402

f32, bf16, f16, i32, i64, u8 = torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8
LAUNCH = {}


def entry(id, variants=(None,)):
    def deco(fn):
        LAUNCH[id] = (fn, tuple(variants))
        return fn
    return deco


class Case:
    """The buffers of one launch under one poison pattern."""

    def __init__(self, dev, pattern):
        self.dev, self.pattern = dev, pattern
        self.bufs, self.roles, self.outs = [], set(), {}
        self.inputs_frozen = contextlib.ExitStack()           # one footprint.frozen per input, entered when it is filled

    def _g(self, name, role, shape, dtype, ld, mask):
        g = fp.Guarded(shape, dtype, self.dev, ld=ld, pattern=self.pattern, mask=mask)
        self.bufs.append((name, g))
        self.roles.add((re.sub(r"\d+$", "", name), role))      # (P0, P1, ... of a launch sequence are one operand of the table)
        return g

    def inp(self, name, t, ld=None, mask=None):
        t = torch.as_tensor(t)
        g = self._g(name, "in", tuple(t.shape), t.dtype, ld, mask).fill_from(t)
        self.inputs_frozen.enter_context(fp.frozen(g.view, names=("input " + name,)))
        return g.view

    def out(self, name, shape, dtype, ld=None, mask=None):
        g = self._g(name, "out", shape, dtype, ld, mask)
        self.outs[name] = g
        return g.view

    def inout(self, name, t, ld=None, mask=None):
        t = torch.as_tensor(t)
        return self._g(name, "inout", tuple(t.shape), t.dtype, ld, mask).fill_from(t).view

    def ws(self, name, nbytes, dtype=f32, zero=False):
        """exactly nbytes (rounded up to one element), the back guard right behind"""
        es = torch.empty((), dtype=dtype).element_size()
        g = self._g(name, "ws", (max((int(nbytes) + es - 1) // es, 1),), dtype, None, None)
        if zero:
            g.view.zero_()
        return g.view

    def payloads(self):
        return {n: g.payload() for n, g in self.outs.items()}

    def assert_guards(self):
        for n, g in self.bufs:
            g.assert_guards_intact(n)

    def assert_inputs_frozen(self):
        """leave the footprint.frozen of every input: each asserts its view (payload and gaps) came back bit-identical"""
        self.inputs_frozen.close()


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    g = torch.Generator(device=_dev())
    g.manual_seed(seed)
    return g


def randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, device=_dev(), generator=_gen(seed)) * scale


def split3(x):
    hi = x.to(bf16)
    r = x - hi.float()
    mid = r.to(bf16)
    return hi, mid, (r - mid.float()).to(bf16)


def planes3(x, plane):
    """[rows][hi | mid | lo], `plane` columns apart, width 2 plane + cols (gap columns zero here: they get poisoned)"""
    out = torch.zeros(x.shape[0], 2 * plane + x.shape[1], dtype=bf16, device=x.device)
    for p, t in enumerate(split3(x)):
        out[:, p * plane:p * plane + x.shape[1]] = t
    return out


def planes2(x, plane, scale):
    xs = x * scale
    hi = xs.to(f16)
    lo = (xs - hi.float()).to(f16)
    out = torch.zeros(x.shape[0], plane + x.shape[1], dtype=f16, device=x.device)
    out[:, :x.shape[1]], out[:, plane:plane + x.shape[1]] = hi, lo
    return out


def scale_of(t, top=2.0 ** 10):
    """the power of two that puts max |t| in (top / 2, top]: the rule tests/test_gpu_f16x2.py scales its fp16 planes by"""
    m = float(t.abs().max())
    return 2.0 ** math.floor(math.log2(top / m)) if m > 0 else 1.0


def pmask(rows, cols, plane, n=3, valid_rows=None):
    m = torch.zeros(rows, (n - 1) * plane + cols, dtype=torch.bool)
    for p in range(n):
        m[:valid_rows, p * plane:p * plane + cols] = True
    return m


def psum(v, cols, plane, n=3):
    return sum(v[:, p * plane:p * plane + cols].double() for p in range(n))


def relmax(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def lrelu(t, a=0.2):
    return torch.maximum(t, a * t)


def interleave(v, rows, cols, plane, ld=None):
    """torch model of cdml_interleave8_bf16x3: row-major planes -> [3][rows / 8][ld][8] (columns >= cols left out)"""
    ps = torch.stack([v[:rows, p * plane:p * plane + cols] for p in range(3)])          # [3, rows, cols]
    return ps.view(3, rows // 8, 8, cols).permute(0, 1, 3, 2).contiguous()              # [3, rows / 8, cols, 8]


# ================================================================================================ gather =====
def _catalogue(c, F=500, N=3000):
    tab = torch.rand(N, F, device=_dev(), generator=_gen(1)) + 0.01
    rng = np.random.RandomState(0)
    pairs = rng.randint(0, N, size=(2000, 2)).astype(np.int32)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    return tab, c.inp("table", tab, ld=F + 4), pairs, c.inp("pairs", torch.from_numpy(pairs).to(_dev()))


def _gather(c, variant, kind):
    mode, steps = variant
    F, Fp, B, seed, step0 = 500, 512, 64, 77, 5
    tab, tabv, pairs, pairsv = _catalogue(c, F)
    R = B * (3 if mode == 0 else 2)
    npl = 2 if kind == "h2" else 3
    x = c.out("x_planes", (steps * R, npl * Fp), f16 if kind == "h2" else bf16)
    idx = c.out("idx", (steps * R,), i32)
    shift = c.out("shift", (steps,), i32) if mode == 1 else None
    xki = c.out("x_ki", (steps, 3 * R * Fp), bf16) if kind == "x3k" else None
    multi = steps > 1
    ops.sample_gather(mode, pairsv, seed, step0, B, tabv, F, idx.view(steps, R) if multi else idx,
                      x.view(steps, R, npl * Fp) if multi else x, shift_out=shift, n_steps=steps,
                      x_ki=None if xki is None else (xki if multi else xki[0]))

    def ref():
        for s in range(steps):
            if mode == 0:
                want = osampler.device_triplets_vec(pairs, tab.shape[0], seed, step0 + s, B).reshape(-1)
            else:
                want, _, _, sh = osampler.device_inbatch(pairs, seed, step0 + s, B)
                assert int(shift[s].item()) == int(sh)
            got = idx[s * R:(s + 1) * R]
            assert np.array_equal(got.cpu().numpy(), np.asarray(want).reshape(-1))
            rows = tab[got.long()].double()
            xh = rows / rows.pow(2).sum(1, keepdim=True).clamp_min(1e-12).sqrt()
            v = x[s * R:(s + 1) * R]
            if kind == "h2":
                assert (psum(v, F, Fp, 2) / 16384.0 - xh).abs().max().item() < 1e-6
                assert bool((v[:, F:Fp] == 0).all()) and bool((v[:, Fp + F:] == 0).all())
                continue
            assert (psum(v, F, Fp) - xh).abs().max().item() < 1e-6
            full = psum(v, Fp, Fp).float()
            assert bool((full[:, F:] == 0).all()), "padding columns are zero"
            assert torch.equal(v.view(torch.int16), planes3(full, Fp).view(torch.int16)), "a valid split"
            if xki is not None:
                assert torch.equal(xki[s].view(torch.int16), interleave(v, R, Fp, Fp).reshape(-1).view(torch.int16))
    return ref


_GV = [(0, 1), (1, 1), (0, 2), (1, 2)]
entry("sample_gather_x3", _GV)(lambda c, v, mp: _gather(c, v, "x3"))
entry("sample_gather_x3k", _GV)(lambda c, v, mp: _gather(c, v, "x3k"))
entry("sample_gather_h2", [(0, 1), (1, 1)])(lambda c, v, mp: _gather(c, v, "h2"))


@entry("gather_rows_x3", [False, True])
def _gather_rows_x3(c, nan_missing, mp):
    n, F, Fp, R = 700, 500, 512, 300
    src = randn(3, n, F)
    idx = torch.randint(0, n, (R,), device=_dev(), generator=_gen(4), dtype=i32)
    idx[7] = -1
    idx[200] = -1
    ok = (idx >= 0).cpu()
    mask = torch.ones(R, 3 * Fp, dtype=torch.bool)
    if not nan_missing:
        mask[~ok] = False                                   # an unanswered request without the flag: the row is left untouched
    out = c.out("planes", (R, 3 * Fp), bf16, mask=mask)
    ops.gather_rows_x3(c.inp("src", src, ld=F + 4), c.inp("idx", idx), F, out, nan_missing=nan_missing)

    def ref():
        rows = torch.zeros(R, Fp, device=_dev())
        rows[:, :F] = src[idx.clamp_min(0).long()]
        assert torch.equal(out[ok].view(torch.int16), planes3(rows, Fp)[ok].view(torch.int16))
        if nan_missing:
            assert bool(torch.isnan(out[~ok].float()).all())
    return ref


# ================================================================================================ splits =====
@entry("split_f32_bf16x3", [(300, 132, False), (200, 96, True)])
def _split3(c, v, mp):
    rows, cols, tr = v
    x = randn(0, rows, cols) * torch.logspace(-6, 3, cols, device=_dev())
    orr, oc = (cols, rows) if tr else (rows, cols)
    plane = (oc + 7) // 8 * 8 + 8
    dst = c.out("dst", (orr, 2 * plane + oc), bf16, ld=3 * plane + 8, mask=pmask(orr, oc, plane))
    ops.split_f32_bf16x3(c.inp("src", x, ld=cols + 4), dst, plane, transpose=tr)

    def ref():
        want = planes3(x.t().contiguous() if tr else x, plane)
        m = pmask(orr, oc, plane).to(_dev())
        assert torch.equal(dst[m].view(torch.int16), want[m].view(torch.int16))
    return ref


@entry("split_f32_f16x2", [(300, 132, False), (200, 96, True)])
def _split2(c, v, mp):
    rows, cols, tr = v
    x = randn(0, rows, cols)
    orr, oc = (cols, rows) if tr else (rows, cols)
    plane = (oc + 7) // 8 * 8 + 8
    dst = c.out("dst", (orr, plane + oc), f16, ld=2 * plane + 8, mask=pmask(orr, oc, plane, 2))
    ops.split_f32_f16x2(c.inp("src", x, ld=cols + 4), dst, plane, 64.0, transpose=tr)

    def ref():
        want = planes2(x.t().contiguous() if tr else x, plane, 64.0)
        m = pmask(orr, oc, plane, 2).to(_dev())
        assert torch.equal(dst[m].view(torch.int16), want[m].view(torch.int16))
    return ref


@entry("interleave8_bf16x3")
def _interleave8(c, mp):
    rows, cols, plane = 72, 264, 272
    src = planes3(randn(2, rows, cols), plane)
    dst = c.out("dst", (3 * rows * cols,), bf16)
    ops.interleave8_bf16x3(c.inp("src", src, ld=3 * plane + 8, mask=pmask(rows, cols, plane)), plane, rows, cols, dst)
    return lambda: _eq16(dst, interleave(src, rows, cols, plane).reshape(-1))


def _eq16(a, b):
    assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ================================================================================= k-contiguous plane GEMMs =====
# (M, CDML_X3_HALFTILES): full-tile launches with the last row tile ending in its first / its second half, and half tiles
_MV = [(300, 0), (1000, 0), (1000, 1)]


def _nt(c, v, mp, epi, h2=False, N=512, K=192, slab=False, colsum=False):
    M, half = v
    mp.setenv("CDML_X3_HALFTILES", str(half))
    npl, dt = (2, f16) if h2 else (3, bf16)
    A, B = randn(1, M, K, scale=0.1), randn(2, N, K, scale=0.1)
    sa, sb, sc = (scale_of(A), scale_of(B), 1.0) if h2 else (1.0, 1.0, 1.0)
    pa = K + 8
    mk = (lambda x, s: planes2(x, pa, s)) if h2 else (lambda x, s: planes3(x, pa))
    Av = c.inp("A", mk(A, sa), ld=npl * pa + 8, mask=pmask(M, K, pa, npl))
    Bv = c.inp("B", mk(B, sb), ld=npl * pa + 8, mask=pmask(N, K, pa, npl))
    rowbias = epi == ops.BE_ROWBIAS_LRELU_X3
    bias = randn(3, M if rowbias else N, scale=0.05)
    prod = A.double() @ B.double().t()
    kw = dict(alpha=0.2)
    if epi in (ops.BE_BIAS_LRELU_F32, ops.BE_BIAS_LRELU_X3, ops.BE_ROWBIAS_LRELU_X3, ops.BE_BIAS_LRELU_X3_BITS):
        kw["bias"] = c.inp("bias", bias)
        want = lrelu(prod + (bias.double()[:, None] if rowbias else bias.double()))
    elif epi == ops.BE_F32:
        want = prod
    else:                                                   # the masked data-gradient epilogues
        h = randn(4, M, N)
        if epi == ops.BE_MASK_X3:
            pc_ = N + 8
            hv = (planes2(h, pc_, 1.0) if h2 else planes3(h, pc_))
            kw["aux"] = c.inp("aux", hv, ld=npl * pc_ + 8, mask=pmask(M, N, pc_, npl))
            pos = hv[:, :N].float() > 0
        else:
            pos = h > 0
            packed = (pos.view(M, N // 8, 8).to(i32) << torch.arange(8, device=_dev(), dtype=i32)).sum(-1).to(u8)
            kw["aux"] = c.inp("bits", packed, ld=N // 8 + 16)
        want = prod * torch.where(pos, 1.0, 0.2).double()
    if h2:
        sc = scale_of(want.float())
        kw.update(out_scale=1.0 / (sa * sb), c_scale=sc)
    if slab or colsum:
        q = ops.gemm_f16x2_workspace(False, M, N, K) if h2 else ops.gemm_bf16x3_workspace(False, M, N, K, 6)
        assert q > 0
        kw["workspace"] = c.ws("workspace", q)
    cs = None
    if colsum:
        cs = kw["colsum"] = c.out("colsum", (N,), f32)
    fn = ops.gemm_f16x2_nt if h2 else ops.gemm_bf16x3_nt
    tol = {ops.BE_BIAS_LRELU_F32: 5e-6, ops.BE_F32: 3e-6, ops.BE_ROWBIAS_LRELU_X3: 3e-6}.get(epi, 2e-6)
    tol = 2e-6 if h2 else tol                               # (test_ragged_rows_and_small_shapes of tests/test_gpu_f16x2.py)
    if epi in (ops.BE_BIAS_LRELU_F32, ops.BE_F32):
        C = c.out("C", (M, N), f32, ld=N + 4)
        fn(epi, Av, pa, Bv, pa, C, M, N, K, **kw)

        def ref():
            assert relmax(C, want) <= tol
            if cs is not None:
                assert relmax(cs, B.double().sum(1)) <= 5e-6
        return ref
    if epi == ops.BE_MASKBITS_X3_KI:
        ldc = N + 8
        m = torch.zeros(3 * (M // 8), ldc * 8, dtype=torch.bool)
        m[:, :N * 8] = True
        C = c.out("C_ki", (3 * (M // 8), ldc * 8), bf16, mask=m)
        fn(epi, Av, pa, Bv, pa, C, M, N, K, plane_c=M * ldc, ldc=ldc, **kw)

        def ref():
            v = C.view(3, M // 8, ldc, 8)[:, :, :N, :]
            got = v.permute(0, 1, 3, 2).reshape(3, M, N).double().sum(0)
            assert relmax(got, want) <= tol
            assert torch.equal(v[0].permute(0, 2, 1).reshape(M, N), got.float().to(bf16)), "hi is the rounding of the sum"
        return ref
    pc = N + 8
    C = c.out("C_planes", (M, (npl - 1) * pc + N), dt, ld=npl * pc + 8, mask=pmask(M, N, pc, npl))
    bits = None
    if epi == ops.BE_BIAS_LRELU_X3_BITS:
        bits = kw["aux"] = c.out("bits", (M, N // 8), u8, ld=N // 8 + 16)
    fn(epi, Av, pa, Bv, pa, C, M, N, K, plane_c=pc, **kw)

    def ref():
        got = psum(C, N, pc, npl) / sc
        assert relmax(got, want) <= tol
        if not h2:
            assert torch.equal(C[:, :N], got.float().to(bf16)), "hi is the rounding of the sum"
        if bits is not None:
            wb = ((got > 0).view(M, N // 8, 8).to(i32) << torch.arange(8, device=_dev(), dtype=i32)).sum(-1).to(u8)
            assert torch.equal(bits, wb)
    return ref


entry("x3_nt_bias_lrelu_f32", _MV)(lambda c, v, mp: _nt(c, v, mp, ops.BE_BIAS_LRELU_F32))
entry("x3_nt_slab_n256", [(300, 0), (300, 1)])(lambda c, v, mp: _nt(c, v, mp, ops.BE_BIAS_LRELU_F32, N=256, K=1344, slab=True))
entry("x3_nt_f32_colsum", [(512, 0)])(lambda c, v, mp: _nt(c, v, mp, ops.BE_F32, colsum=True))
entry("x3_nt_bias_lrelu_x3", _MV)(lambda c, v, mp: _nt(c, v, mp, ops.BE_BIAS_LRELU_X3))
entry("x3_nt_rowbias_lrelu_x3", _MV)(lambda c, v, mp: _nt(c, v, mp, ops.BE_ROWBIAS_LRELU_X3))
entry("x3_nt_bias_lrelu_x3_bits", _MV)(lambda c, v, mp: _nt(c, v, mp, ops.BE_BIAS_LRELU_X3_BITS))
entry("x3_nt_mask_x3", _MV)(lambda c, v, mp: _nt(c, v, mp, ops.BE_MASK_X3))
entry("x3_nt_maskbits_x3", _MV)(lambda c, v, mp: _nt(c, v, mp, ops.BE_MASKBITS_X3))
entry("x3_nt_maskbits_x3_ki", [(328, 0), (1000, 0), (1000, 1)])(lambda c, v, mp: _nt(c, v, mp, ops.BE_MASKBITS_X3_KI))
# (the fp16 form has no half-tile launch: M = 1000 is its "last row tile ends in the second half" case)
_H2V = [(e, 300) for e in (1, 3, 6, 7, 9, 10)] + [(e, 1000) for e in (6, 9, 10)] + [("slab", 300)]


@entry("h2_nt", _H2V)
def _h2_nt(c, v, mp):
    e, M = v
    if e == "slab":
        return _nt(c, (M, 0), mp, ops.BE_BIAS_LRELU_F32, h2=True, N=256, K=1408, slab=True)
    return _nt(c, (M, 0), mp, e, h2=True, K=256)


# =================================================================================== k-strided plane GEMMs =====
def _tn(c, v, mp, h2=False):
    M, N, K, with_bias = v
    npl = 2 if h2 else 3
    X, dY = randn(3, K, M, scale=0.05), randn(4, K, N, scale=0.01)
    sa, sb = (scale_of(X), scale_of(dY)) if h2 else (1.0, 1.0)
    pa, pb = M + 8, N + 8
    mk = (lambda x, p, s: planes2(x, p, s)) if h2 else (lambda x, p, s: planes3(x, p))
    Xv = c.inp("A", mk(X, pa, sa), ld=npl * pa + 8, mask=pmask(K, M, pa, npl))
    Yv = c.inp("B", mk(dY, pb, sb), ld=npl * pb + 8, mask=pmask(K, N, pb, npl))
    q = ops.gemm_f16x2_workspace(True, M, N, K) if h2 else ops.gemm_bf16x3_workspace(True, M, N, K, 6)
    ws = c.ws("workspace", q) if q else None
    C = c.out("C", (M, N), f32, ld=N + 4)
    want = X.double().t() @ dY.double()
    if with_bias:
        bias = randn(5, N, scale=0.01)
        ops.gemm_bf16x3_tn(Xv, pa, Yv, pb, C, M, N, K, workspace=ws, bias=c.inp("bias", bias), alpha=0.2)
        return lambda: _le(relmax(C, lrelu(want + bias.double())), 3e-6)
    cs = c.out("colsum", (N,), f32)
    if h2:
        ops.gemm_f16x2_tn(Xv, pa, Yv, pb, C, M, N, K, 1.0 / (sa * sb), workspace=ws, colsum=cs, colsum_scale=1.0 / sb)
    else:
        ops.gemm_bf16x3_tn(Xv, pa, Yv, pb, C, M, N, K, workspace=ws, colsum=cs)

    def ref():
        rb = dY.double().sum(0)
        if h2:                                              # (test_resident_plane_walk_equals_the_general_loop: 2e-6 for both)
            _le(relmax(C, want), 2e-6)
            _le(relmax(cs, rb), 2e-6)
            return
        _le(relmax(C, want), 5e-6)
        assert (cs.double() - rb).abs().max().item() <= (1e-4 if K > 1024 else 5e-6 * rb.abs().max().item())
    return ref


def _le(a, b):
    assert a <= b, (a, b)


entry("x3_tn", [(512, 256, 384, False), (256, 512, 384, True)])(lambda c, v, mp: _tn(c, v, mp))
entry("x3_tn_split_k", [(256, 256, 3072, False)])(lambda c, v, mp: _tn(c, v, mp))
entry("h2_tn", [(512, 256, 384, False), (256, 256, 3072, False)])(lambda c, v, mp: _tn(c, v, mp, h2=True))


@entry("x3_tnk")
def _tnk(c, mp):
    M, N, K, a0, b0 = 256, 256, 384, 256, 256
    ma, nb = M + a0 + 256, N + b0
    A, B = randn(6, K, ma, scale=0.05), randn(7, K, nb, scale=0.02)
    Ai = interleave(planes3(A, ma), K, ma, ma).reshape(-1)
    Bi = interleave(planes3(B, nb), K, nb, nb).reshape(-1)
    q = ops.gemm_bf16x3_workspace(True, M, N, K, 6)
    C, cs = c.out("C", (M, N), f32, ld=N + 4), c.out("colsum", (N,), f32)
    ops.gemm_bf16x3_tnk(c.inp("A", Ai), ma, a0, c.inp("B", Bi), nb, b0, C, M, N, K, workspace=c.ws("workspace", q) if q else None, colsum=cs)

    def ref():
        _le(relmax(C, A[:, a0:a0 + M].double().t() @ B[:, b0:b0 + N].double()), 5e-6)
        _le(relmax(cs, B[:, b0:b0 + N].double().sum(0)), 5e-6)
    return ref


# ======================================================================================= tail and loss =====
def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def _l2n_bwd(z, g, alpha):
    """d/dz [z rsqrt(max(sum z^2, 1e-12))] applied to g, times leaky-relu'(z) (alpha < 0: none); fp64"""
    n2 = z.pow(2).sum(1, keepdim=True).clamp_min(1e-12)
    inv = n2.rsqrt()
    dz = g * inv - z * (g * z).sum(1, keepdim=True) * inv ** 3
    return dz * torch.where(z > 0, 1.0, alpha).double() if alpha >= 0 else dz


@entry("l2norm_fwd")
def _l2f(c, mp):
    M, N = 301, 200
    x = randn(1, M, N)
    y, inv = c.out("y", (M, N), f32, ld=N + 4), c.out("inv", (M,), f32)
    ops.l2norm_fwd(c.inp("x", x, ld=N + 8), N, y, inv_out=inv)

    def ref():
        n = x.double().pow(2).sum(1, keepdim=True).clamp_min(1e-12).rsqrt()
        assert (y.double() - x.double() * n).abs().max().item() < 1e-6 and relmax(inv, n[:, 0]) < 1e-6
    return ref


@entry("l2norm_bwd", [-1.0, 0.2])
def _l2b(c, alpha, mp):
    M, N = 301, 200
    z, g = randn(1, M, N), randn(2, M, N, scale=0.1)
    dz = c.out("dz", (M, N), f32, ld=N + 4)
    ops.l2norm_bwd(c.inp("z", z, ld=N + 8), c.inp("g", g, ld=N + 4), N, dz, lrelu_alpha=alpha)
    return lambda: _le((dz.double() - _l2n_bwd(z.double(), g.double(), alpha)).abs().max().item(), 1e-6)


def _hinge_ref(e, tri, valid, margin):
    """fp64 hinge over index triplets [B, 3] (valid: counted in the mean either way): pos, neg, hinge, loss, de"""
    a, p, n = e[tri[:, 0]], e[tri[:, 1]], e[tri[:, 2]]
    pos, neg = (a - p).pow(2).sum(1), (a - n).pow(2).sum(1)
    hinge = (margin + pos - neg).clamp_min(0) * valid
    act = ((hinge > 0) * 1.0)[:, None] / tri.shape[0]
    de = torch.zeros_like(e)
    de.index_add_(0, tri[:, 0], act * 2 * (n - p))
    de.index_add_(0, tri[:, 1], act * 2 * (p - a))
    de.index_add_(0, tri[:, 2], act * 2 * (a - n))
    return pos, neg, hinge, hinge.mean(), de


@entry("vnet_tail_planes", [0, 1])
def _tail(c, mode, mp):
    B, D, alpha = 96, 256, 0.2
    R = B * (3 if mode == 0 else 2)
    z = randn(5, R, D)
    ids = torch.arange(R, dtype=i32, device=_dev())
    ids[2 * 9 + 1] = ids[2 * 2 + 1]                           # mode 1: triplet 2's negative (the positive of pair 9) is its positive's video
    shift = torch.tensor([7], dtype=i32, device=_dev())
    pb = D + 8
    e, dz2 = c.out("e", (R, D), f32, ld=D + 4), c.out("dz2", (R, D), f32, ld=D + 4)
    pos, neg, hinge = (c.out(n, (B,), f32) for n in ("pos", "neg", "hinge"))
    valid = c.out("valid", (B,), u8) if mode == 1 else None
    stats = c.out("stats", (8,), f32, mask=torch.arange(8)[None, :] < 4)
    pl = c.out("dz2_planes", (R, 2 * pb + D), bf16, ld=3 * pb + 8, mask=pmask(R, D, pb))
    ops.vnet_tail(mode, c.inp("z", z, ld=D + 8), c.inp("rows", ids), c.inp("shift", shift), B, D, 0.8, e, pos, neg, hinge, dz2,
                  valid=valid, stats=stats, dz2_bf16=pl, plane_bf=pb, alpha=alpha)

    def ref():
        zd = z.double()
        en = zd * zd.pow(2).sum(1, keepdim=True).clamp_min(1e-12).rsqrt()
        i = torch.arange(B, device=_dev())
        if mode == 0:
            tri, ok = torch.stack([3 * i, 3 * i + 1, 3 * i + 2], 1), torch.ones(B, device=_dev()).double()
        else:
            j = (i + 7) % B
            tri = torch.stack([2 * i, 2 * i + 1, 2 * j + 1], 1)
            idl = ids.long()
            ok = ((idl[2 * j + 1] != idl[2 * i]) & (idl[2 * j + 1] != idl[2 * i + 1])).double()
            assert torch.equal(valid, ok.to(u8)) and int(ok.sum()) < B
        p, n, h, loss, de = _hinge_ref(en, tri, ok, 0.8)
        assert (e.double() - en).abs().max().item() < 1e-6
        for got, want in ((pos, p), (neg, n), (hinge, h)):
            assert (got.double() - want).abs().max().item() < 1e-6
        assert abs(stats[0].item() - loss.item()) < 1e-6
        assert (dz2.double() - _l2n_bwd(zd, de, alpha)).abs().max().item() < 1e-6
        m = pmask(R, D, pb).to(_dev())
        _eq16(pl[m], planes3(dz2.contiguous(), pb)[m])
    return ref


def _indexed(c, tail):
    B, D = 128, 64
    z = randn(8, 2 * B, D)
    en = _unit(z)
    neg_row = torch.randint(0, 2 * B, (B,), device=_dev(), generator=_gen(9), dtype=i32)
    neg_row[5] = -1
    neg_row[17] = neg_row[3]                                  # a row mined twice
    ev = c.inp("e", en, ld=D + 4)
    pos, neg, hinge = (c.out(n, (B,), f32) for n in ("pos", "neg", "hinge"))
    stats, de = c.out("stats", (4,), f32), c.out("de", (2 * B, D), f32, ld=D + 4)
    scratch = c.ws("scale_scratch", 4 * B)
    nv = c.inp("neg_row", neg_row)
    dz2 = pl = None
    pb = D + 8
    if tail:
        dz2 = c.out("dz2", (2 * B, D), f32, ld=D + 4)
        pl = c.out("dz2_planes", (2 * B, 2 * pb + D), bf16, ld=3 * pb + 8, mask=pmask(2 * B, D, pb))
        ops.triplet_hinge_indexed(ev, nv, B, D, 0.8, pos, neg, hinge, scratch, stats, de, z=c.inp("z", z, ld=D + 8), dz2=dz2,
                                  dz2_bf16=pl, plane_bf=pb, lrelu_alpha=0.2)
    else:
        ops.triplet_hinge_indexed(ev, nv, B, D, 0.8, pos, neg, hinge, scratch, stats, de)

    def ref():
        i = torch.arange(B, device=_dev())
        ok = (neg_row >= 0).double()
        tri = torch.stack([2 * i, 2 * i + 1, neg_row.clamp_min(0).long()], 1)
        p, n, h, loss, dE = _hinge_ref(en.double(), tri, ok, 0.8)
        assert (pos.double() - p).abs().max().item() < 1e-6
        assert ((neg.double() - n) * ok).abs().max().item() < 1e-6 and (hinge.double() - h).abs().max().item() < 1e-6
        assert abs(stats[0].item() - loss.item()) < 1e-6 and (de.double() - dE).abs().max().item() < 1e-6
        if tail:
            assert (dz2.double() - _l2n_bwd(z.double(), dE, 0.2)).abs().max().item() < 1e-6
            m = pmask(2 * B, D, pb).to(_dev())
            _eq16(pl[m], planes3(dz2.contiguous(), pb)[m])
    return ref


entry("triplet_hinge_indexed")(lambda c, mp: _indexed(c, False))
entry("triplet_hinge_indexed_tail")(lambda c, mp: _indexed(c, True))


@entry("semihard_mine_x3")
def _mine(c, mp):
    B, D = 128, 64
    e = _unit(randn(10, 2 * B, D))
    ids = torch.arange(2 * B, dtype=i32, device=_dev())
    ids[11] = ids[0]                                          # another row of anchor 0's video: never its negative
    pl_ = D + 8
    planes = c.out("e_planes", (2 * B, 2 * pl_ + D), bf16, ld=3 * pl_ + 8, mask=pmask(2 * B, D, pl_))
    sqn, dp, out = c.out("sqn", (2 * B,), f32), c.out("dp", (B,), f32), c.out("neg_row", (B,), i32)
    ws = c.ws("workspace", ops.semihard_mine_x3_workspace(B))
    ops.semihard_mine_x3(c.inp("e", e, ld=D + 4), c.inp("rows", ids), B, D, planes, pl_, sqn, dp, ws, out)

    def ref():
        ed = e.double()
        dist = (ed[0::2, None, :] - ed[None, :, :]).pow(2).sum(-1)               # [B, 2B]
        i = torch.arange(B, device=_dev())
        d_p = dist[i, 2 * i + 1]
        assert (dp.double() - d_p).abs().max().item() < 2e-6 and (sqn.double() - 1).abs().max().item() < 2e-6
        m = pmask(2 * B, D, pl_).to(_dev())
        _eq16(planes[m], planes3(e, pl_)[m])
        idl, tol = ids.long(), 2e-6
        elig = (idl[None, :] != idl[0::2][:, None]) & (idl[None, :] != idl[1::2][:, None])
        got = out.long()
        assert bool((got >= 0).all()) and bool(elig[i, got].all())
        dg = dist[i, got]
        for k in range(B):
            strict = elig[k] & (dist[k] > d_p[k] + tol)
            if bool(strict.any()) and dg[k] > d_p[k] - tol:
                assert dg[k] <= dist[k][strict].min() + tol
            elif not bool((elig[k] & (dist[k] > d_p[k] - tol)).any()):
                assert dg[k] >= dist[k][elig[k]].max() - tol
    return ref


# ========================================================================================== N-pair family =====
NB, NBP, ND, NM, NT = 200, 256, 64, 64, 0.1


def _npair_data(mem=False, logq=False):
    rng = np.random.default_rng(3)
    u = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    A = u(rng.standard_normal((NB, ND)))
    P = u(A + 0.5 * rng.standard_normal((NB, ND)))
    ids = rng.choice(50 * NB, size=2 * NB, replace=False).astype(np.int32)
    ids[2 * 4 + 1] = ids[2 * 9 + 1]
    ids[2 * 20] = ids[2 * 3 + 1]
    d = {"A": A, "P": P, "ids": ids, "S": A @ P.T}
    if mem:
        d["mem"] = u(rng.standard_normal((NM, ND)))
        mid = rng.choice(50 * NB, size=NM).astype(np.int32)
        mid[5], mid[40:48], mid[7] = ids[1], -1, ids[2 * 30]
        d["mem_id"] = mid
        d["S"] = np.concatenate([d["S"], np.zeros((NB, NBP - NB)), A @ d["mem"].T], 1)
    if logq:
        d["bias"] = np.log(rng.uniform(1e-4, 1e-2, 2 * NB)).astype(np.float32)
        d["mem_bias"] = np.log(rng.uniform(1e-4, 1e-2, NM)).astype(np.float32)
    return d


def _npair_ref(d, mem, logq):
    if logq:
        return npair_logq_ref.npair_logq(d["A"], d["P"], d["ids"], d["bias"], NT, True, d.get("mem") if mem else None,
                                         d.get("mem_id") if mem else None, d.get("mem_bias") if mem else None)
    if mem:
        return npair_memory_ref.npair_memory(d["A"], d["P"], d["ids"], d["mem"], d["mem_id"], NT, True)
    return npair_ref.npair(d["A"], d["P"], d["ids"], NT, True)


def _t(x, dtype=f32):
    return torch.as_tensor(np.asarray(x)).to(device=_dev(), dtype=dtype)


def _npair_S(c, d, mem):
    S = _t(d["S"])
    if not mem:
        return c.inp("S", S, ld=NBP + 4)
    m = torch.ones(NB, NBP + NM, dtype=torch.bool)
    m[:, NB:NBP] = False                                      # between the in-batch block and the memory block: not read
    return c.inp("S", S, ld=NBP + NM + 4, mask=m)


def _npair_stats(c, mem, logq):
    d = _npair_data(mem, logq)
    lse = c.out("lse", (2 * NBP,), f32, mask=torch.arange(2 * NBP)[None, :] < 2 * NB)
    stats = c.out("stats", (4,), f32)
    Sv, idv = _npair_S(c, d, mem), c.inp("ids", _t(d["ids"], i32))
    if mem:
        ws = c.ws("workspace", ops.npair_memory_workspace(NB, NM))
        mid = c.inp("mem_id", _t(d["mem_id"], i32))
        if logq:
            ops.npair_memory_logq_stats(Sv, idv, NB, c.inp("bias", _t(d["bias"])), NBP, mid, c.inp("mem_bias", _t(d["mem_bias"])), NT, True, lse, stats, ws)
        else:
            ops.npair_memory_stats(Sv, idv, NB, NBP, mid, NT, True, lse, stats, ws)
    else:
        ws = c.ws("workspace", ops.npair_workspace(NB))
        if logq:
            ops.npair_logq_stats(Sv, idv, NB, c.inp("bias", _t(d["bias"])), NT, True, lse, stats, ws)
        else:
            ops.npair_stats(Sv, idv, NB, NT, True, lse, stats, ws)

    def ref():
        r = _npair_ref(d, mem, logq)
        assert np.abs(lse[:NB].double().cpu().numpy() - r["lse_row"]).max() < 1e-5
        assert np.abs(lse[NB:2 * NB].double().cpu().numpy() - r["lse_col"]).max() < 1e-5
        assert np.abs(stats.double().cpu().numpy() - r["stats"]).max() < 1e-5
    return ref


def _npair_grad(c, x3, mem, logq):
    """mem: the launch writes the memory block of W only; else rows < B, columns < B.  The rest of [Bp][..] keeps the poison."""
    d = _npair_data(mem, logq)
    r = _npair_ref(d, mem, logq)
    lse = np.concatenate([r["lse_row"], r["lse_col"]]).astype(np.float32)
    K = NBP + NM if mem else NBP
    c0, w = (NBP, NM) if mem else (0, NB)
    plane = K + 8
    if x3:
        m = torch.zeros(NBP, 2 * plane + K, dtype=torch.bool)
        for p in range(3):
            m[:NB, p * plane + c0:p * plane + c0 + w] = True
        W = c.out("W", (NBP, 2 * plane + K), bf16, ld=3 * plane + 8, mask=m)
    else:
        m = torch.zeros(NBP, K, dtype=torch.bool)
        m[:NB, c0:c0 + w] = True
        W = c.out("W", (NBP, K), f32, ld=K + 4, mask=m)
    Sv, idv, lv = _npair_S(c, d, mem), c.inp("ids", _t(d["ids"], i32)), c.inp("lse", _t(lse))
    tail = (W, plane) if x3 else (W,)
    sfx = "x3" if x3 else "f32"
    if mem:
        mid = c.inp("mem_id", _t(d["mem_id"], i32))
        if logq:
            getattr(ops, "npair_memory_logq_grad_" + sfx)(Sv, idv, NB, NBP, mid, c.inp("mem_bias", _t(d["mem_bias"])), NT, True, lv, *tail)
        else:
            getattr(ops, "npair_memory_grad_" + sfx)(Sv, idv, NB, NBP, mid, NT, True, lv, *tail)
    elif logq:
        getattr(ops, "npair_logq_grad_" + sfx)(Sv, idv, NB, c.inp("bias", _t(d["bias"])), NT, True, lv, *tail)
    else:
        getattr(ops, "npair_grad_" + sfx)(Sv, idv, NB, NT, True, lv, *tail)

    def ref():
        want = _t(r["W_mem"] if mem else r["W"], torch.float64)
        got = (psum(W[:NB, c0:], w, plane) if x3 else W[:NB, c0:c0 + w].double())
        assert ((got - want).norm() / want.norm()).item() < 1e-4
        assert bool((got[want == 0] == 0).all()), "entries a rule does not count are exactly 0"
    return ref


entry("npair_stats")(lambda c, mp: _npair_stats(c, False, False))
entry("npair_memory_stats")(lambda c, mp: _npair_stats(c, True, False))
entry("npair_logq_stats")(lambda c, mp: _npair_stats(c, False, True))
entry("npair_memory_logq_stats")(lambda c, mp: _npair_stats(c, True, True))
for _n, _a in (("npair_grad_x3", (True, False, False)), ("npair_grad_f32", (False, False, False)),
               ("npair_memory_grad_x3", (True, True, False)), ("npair_memory_grad_f32", (False, True, False)),
               ("npair_logq_grad_x3", (True, False, True)), ("npair_logq_grad_f32", (False, False, True)),
               ("npair_memory_logq_grad_x3", (True, True, True)), ("npair_memory_logq_grad_f32", (False, True, True))):
    entry(_n)(lambda c, mp, _a=_a: _npair_grad(c, *_a))


@entry("npair_memory_push")
def _push(c, mp):
    """three pushes of B = 64 positives into a ring of M = 128 slots (the third wraps onto the first), start = 1: the ring,
    its ids and both plane images change in the step's slots only; everything around them is guard"""
    B, D, M, start = 64, 64, 128, 1
    pr, pt = D + 8, M + 8
    P = [_unit(randn(20 + t, B, D)) for t in range(4)]
    ids = [torch.randint(0, 9999, (2 * B,), device=_dev(), generator=_gen(30 + t), dtype=i32) for t in range(4)]
    mem = c.inout("mem", torch.zeros(M, D, device=_dev()), ld=D + 4)
    mem_id = c.inout("mem_id", torch.full((M,), -1, dtype=i32, device=_dev()))
    R3 = c.inout("R3_image", torch.zeros(M, 2 * pr + D, dtype=bf16, device=_dev()), ld=3 * pr + 8, mask=pmask(M, D, pr))
    T3 = c.inout("T3_image", torch.zeros(D, 2 * pt + M, dtype=bf16, device=_dev()), ld=3 * pt + 8, mask=pmask(D, M, pt))
    step_dev = c.inp("step_dev", torch.tensor([0], dtype=i64, device=_dev()))
    for t in range(4):                                        # step 0 lies before start: no push; step 3 wraps onto step 1's slots
        ops.npair_memory_push(c.inp("P%d" % t, P[t], ld=D + 4), c.inp("ids%d" % t, ids[t]), B, D, t, step_dev, start, mem, mem_id,
                              R3=R3, plane_r=pr, T3=T3, plane_t=pt)

    def ref():
        rows, rid = npair_memory_ref.ring_after(4, start, M, [p.double().cpu().numpy() for p in P], [i[1::2].cpu().numpy() for i in ids])
        assert np.array_equal(mem.double().cpu().numpy(), rows) and np.array_equal(mem_id.cpu().numpy(), rid)
        mr, mt = pmask(M, D, pr).to(_dev()), pmask(D, M, pt).to(_dev())
        _eq16(R3[mr], planes3(mem.contiguous(), pr)[mr])
        _eq16(T3[mt], planes3(mem.t().contiguous(), pt)[mt])
    return ref


def _logq_data():
    rng = np.random.default_rng(5)
    nv, B, M = 1000, 100, 64
    ids = rng.integers(0, nv, 2 * B).astype(np.int32)
    ids[3], ids[8] = -1, nv + 5                               # an empty slot and an id outside the table
    mid = rng.integers(0, nv, M).astype(np.int32)
    mid[10:14] = -1
    return nv, B, M, ids, mid, rng


@entry("logq_table_gather")
def _ltg(c, mp):
    nv, B, M, ids, mid, rng = _logq_data()
    tab = np.log(rng.uniform(1e-5, 1e-2, nv)).astype(np.float32)
    bias, mb = c.out("bias", (2 * B,), f32), c.out("mem_bias", (M,), f32)
    ops.logq_table_gather(c.inp("table", _t(tab)), c.inp("ids", _t(ids, i32)), B, c.inp("mem_id", _t(mid, i32)), bias, mb)

    def ref():
        for got, k in ((bias, ids), (mb, mid)):
            okk = (k >= 0) & (k < nv)
            assert np.array_equal(got.cpu().numpy(), np.where(okk, tab[np.clip(k, 0, nv - 1)], np.float32(0)))
    return ref


@entry("logq_stream_gather")
def _lsg(c, mp):
    nv, B, M, ids, mid, rng = _logq_data()
    last = rng.integers(-1, 50, nv).astype(np.int32)
    gap = rng.uniform(1, 500, nv).astype(np.float32)
    bias, mb = c.out("bias", (2 * B,), f32), c.out("mem_bias", (M,), f32)
    sl, sg = c.out("snap_last", (B,), i32), c.out("snap_gap", (B,), f32)
    ops.logq_stream_gather(c.inp("last", _t(last, i32)), c.inp("gap", _t(gap)), c.inp("ids", _t(ids, i32)), B, c.inp("mem_id", _t(mid, i32)),
                           bias, mb, sl, sg)

    def ref():
        for got, k in ((bias, ids), (mb, mid)):
            okk = (k >= 0) & (k < nv)
            want = np.where(okk, -np.log(gap.astype(np.float64)[np.clip(k, 0, nv - 1)]), 0.0)
            assert np.abs(got.double().cpu().numpy() - want).max() < 1e-6
        pos = ids[1::2]
        okk = (pos >= 0) & (pos < nv)
        assert np.array_equal(sl.cpu().numpy()[okk], last[pos[okk]]) and np.array_equal(sg.cpu().numpy()[okk], gap[pos[okk]])
    return ref


@entry("logq_stream_update")
def _lsu(c, mp):
    """last / gap hold n_videos entries with the guard right behind: the state past n is a guard band"""
    nv, B, M, ids, mid, rng = _logq_data()
    alpha, g0 = 0.05, 10.0
    steps = [rng.integers(0, nv, 2 * B).astype(np.int32) for _ in range(3)]
    steps[1][5], steps[2][7] = nv + 3, -1
    last = c.inout("last", torch.full((nv,), -1, dtype=i32, device=_dev()))
    gap = c.inout("gap", torch.full((nv,), g0, device=_dev()))
    step_dev = c.inp("step_dev", torch.tensor([2], dtype=i64, device=_dev()))
    for t, s in enumerate(steps):
        sv = c.inp("ids%d" % t, _t(s, i32))
        sl, sg = c.ws("snap_last%d" % t, 4 * B, i32), c.ws("snap_gap%d" % t, 4 * B)
        bias = c.ws("bias%d" % t, 8 * B)
        ops.logq_stream_gather(last, gap, sv, B, None, bias, None, sl, sg)
        ops.logq_stream_update(last, gap, sv, B, sl, sg, alpha, t, step_dev)

    def ref():
        wl, wg = npair_logq_ref.estimator_after([s[1::2] for s in steps], nv, B, alpha, g0=g0, t0=2)
        assert np.array_equal(last.cpu().numpy(), wl) and np.array_equal(gap.cpu().numpy(), wg)
    return ref


@entry("logq_stream_reset")
def _lsr(c, mp):
    nv = 1001
    last, gap = c.out("last", (nv,), i32), c.out("gap", (nv,), f32)
    ops.logq_stream_reset(last, gap, 7.5)
    return lambda: (_le(int((last != -1).sum()), 0), _le(int((gap != 7.5).sum()), 0))


# ================================================================================================ optimizers =====
def _adam_ref(w, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    w, g, m, v = (x.double() for x in (w, g, m, v))
    m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
    return w - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (v.sqrt() + eps), m, v


@entry("adam_step")
def _adam(c, mp):
    n = 1003
    w0, g, m0, v0 = randn(1, n), randn(2, n, scale=1e-3), randn(3, n, scale=1e-4), randn(4, n, scale=1e-4).abs()
    w, m, v = c.inout("w", w0), c.inout("m", m0), c.inout("v", v0)
    t_dev = c.inout("t_dev", torch.tensor([2], dtype=i64, device=_dev()))
    tick = c.inout("tickets", torch.zeros(ops.TICKET_WORDS, dtype=i32, device=_dev()))
    ops.adam_step(w, c.inp("g", g), m, v, 0.01, 1, t_dev=t_dev, advance_tickets=tick)

    def ref():
        ww, wm, wv = _adam_ref(w0, g, m0, v0, 3, 0.01)
        assert (w.double() - ww).abs().max().item() < 1e-6 and relmax(m, wm) < 2e-6 and relmax(v, wv) < 2e-6
        assert int(t_dev.item()) == 3 and int(tick.abs().sum().item()) == 0
    return ref


def _copies(c, K, N):
    pt, pc = K + 8, N + 8
    wt = c.out("wt", (N, 2 * pt + K), bf16, ld=3 * pt + 8, mask=pmask(N, K, pt))
    wc = c.out("wc", (K, 2 * pc + N), bf16, ld=3 * pc + 8, mask=pmask(K, N, pc))
    return wt, pt, wc, pc


def _check_copies(W, wt, pt, wc, pc):
    K, N = W.shape
    mt, mc = pmask(N, K, pt).to(_dev()), pmask(K, N, pc).to(_dev())
    _eq16(wt[mt], planes3(W.t().contiguous(), pt)[mt])
    _eq16(wc[mc], planes3(W.contiguous(), pc)[mc])


@entry("adam_matrix_planes")
def _adam_planes(c, mp):
    K, N = 128, 192
    W0, g, m0, v0 = randn(1, K, N, scale=0.05), randn(2, K, N, scale=1e-3), randn(3, K, N, scale=1e-4), randn(4, K, N, scale=1e-4).abs()
    b0, gb = randn(5, N, scale=0.05), randn(6, N, scale=1e-3)
    W, m, v = c.inout("W", W0), c.inout("m", m0), c.inout("v", v0)
    b, mb, vb = c.inout("b", b0), c.inout("mb", torch.zeros(N, device=_dev())), c.inout("vb", torch.zeros(N, device=_dev()))
    wt, pt, wc, pc = _copies(c, K, N)
    ops.adam_matrix_bf16(W, c.inp("g", g), m, v, 0.01, 2, wt=wt, wc=wc, bias=(b, c.inp("gb", gb), mb, vb), plane_t=pt, plane_c=pc)

    def ref():
        assert (W.double() - _adam_ref(W0, g, m0, v0, 2, 0.01)[0]).abs().max().item() < 1e-6
        assert (b.double() - _adam_ref(b0, gb, 0 * b0, 0 * b0, 2, 0.01)[0]).abs().max().item() < 1e-6
        _check_copies(W, wt, pt, wc, pc)
    return ref


@entry("momentum_matrix")
def _mom(c, mp):
    K, N = 128, 192
    W0, g, a0 = randn(1, K, N, scale=0.05), randn(2, K, N, scale=1e-3), randn(3, K, N, scale=1e-4)
    W, acc = c.inout("W", W0), c.inout("acc", a0)
    b0, gb = randn(5, N, scale=0.05), randn(6, N, scale=1e-3)
    b, ab = c.inout("b", b0), c.inout("ab", torch.zeros(N, device=_dev()))
    wt, pt, wc, pc = _copies(c, K, N)
    ops.momentum_matrix(W, c.inp("g", g), acc, 0.05, wt=wt, wc=wc, plane_t=pt, plane_c=pc, bias=(b, c.inp("gb", gb), ab))

    def ref():
        a = a0.double() * 0.9 + g.double()
        assert (acc.double() - a).abs().max().item() < 1e-6
        assert (W.double() - (W0.double() - (g.double() * 0.05 + a * 0.9 * 0.05))).abs().max().item() < 1e-6
        assert (b.double() - (b0.double() - (gb.double() * 0.05 + gb.double() * 0.9 * 0.05))).abs().max().item() < 1e-6
        _check_copies(W, wt, pt, wc, pc)
    return ref


@entry("lars_matrix")
def _lars(c, mp):
    K, N = 128, 192
    segs = [(0, K * N), (K * N, N)]
    n = K * N + N
    w0, g, a0 = randn(1, n, scale=0.05), randn(2, n, scale=1e-3), randn(3, n, scale=1e-4)
    w, acc, gv = c.inout("w", w0), c.inout("acc", a0), c.inp("g", g)
    scratch = c.ws("scratch", 4 * ops.lars_multi_scratch_floats(), zero=True)
    norms = c.out("norms", (4,), f32)
    wt, pt, wc, pc = _copies(c, K, N)
    ops.lars_multi_norms(w, gv, segs, scratch)
    ops.lars_matrix(w, gv, acc, segs, 0, 1, K, N, 0.5, scratch, wt=wt, wc=wc, plane_t=pt, plane_c=pc, norms_out=norms)

    def ref():
        for k, (o, sz) in enumerate(segs):
            ww, gg, aa = (x[o:o + sz].double() for x in (w0, g, a0))
            wn, gn = ww.norm(), gg.norm()
            trust = 1e-3 * wn / (gn + 1e-4 * wn)
            a = 0.9 * aa + 0.5 * trust * (gg + 1e-4 * ww)
            assert (acc[o:o + sz].double() - a).abs().max().item() < 1e-6 and (w[o:o + sz].double() - (ww - a)).abs().max().item() < 1e-6
            assert abs(norms[2 * k].item() / wn.item() - 1) < 1e-5 and abs(norms[2 * k + 1].item() / gn.item() - 1) < 1e-5
        _check_copies(w[:K * N].view(K, N), wt, pt, wc, pc)
    return ref


@entry("grad_prepare")
def _gprep(c, mp):
    n = 7001
    w, g0 = randn(1, n), randn(2, n, scale=1e-2)
    g = c.inout("g", g0)
    norms = c.out("norms", (2,), f32)
    scratch = c.ws("scratch", 4 * ops.lars_scratch_floats(), zero=True)
    ops.grad_prepare(g, c.inp("w", w), 0.3, 0.5, scratch, norms)

    def ref():
        want = g0.double() + 0.3 * w.double()
        gn = want.norm()
        assert abs(norms[0].item() / gn.item() - 1) < 1e-5 and abs(norms[1].item() / w.double().pow(2).sum().item() - 1) < 1e-5
        want = want * 0.5 / max(gn.item(), 0.5)
        assert (g.double() - want).abs().max().item() <= 2e-6 * want.abs().max().item() + 1e-9
    return ref


# ============================================================================================ export and eval =====
@entry("row_sqnorm")
def _sqn(c, mp):
    n, D = 301, 200
    x = randn(1, n, D)
    out = c.out("out", (n,), f32)
    ops.row_sqnorm(c.inp("x", x, ld=D + 4), D, out)
    return lambda: _le(relmax(out, x.double().pow(2).sum(1)), 1e-6)


def _knn_data(nq=300, nb=768, D=64):
    Q, Bk = _unit(randn(1, nq, D)), _unit(randn(2, nb, D))
    d = (Q.double().pow(2).sum(1)[:, None] + Bk.double().pow(2).sum(1)[None, :] - 2 * Q.double() @ Bk.double().t()).clamp_min(0)
    return Q, Bk, d


def _topk(d, k):
    """fp64 top-k by (distance, id)"""
    order = torch.argsort(d, dim=1, stable=True)[:, :k]
    return d.gather(1, order), order


@entry("knn_merge")
def _kmerge(c, mp):
    nq, nb, D, k, n_valid, L = 300, 768, 64, 20, 700, ops.knn_list_capacity()
    Q, Bk, d = _knn_data(nq, nb, D)
    S = Q @ Bk.t()
    qs, bs = Q.pow(2).sum(1), Bk.pow(2).sum(1)
    bd, bi = c.out("best_d", (nq, L), f32), c.out("best_i", (nq, L), i32)
    for c0 in (0, 384):
        ops.knn_merge(c.inp("scores%d" % c0, S[:, c0:c0 + 384].contiguous(), ld=388), nq, 384, c0, n_valid, c.inp("q_sq%d" % c0, qs),
                      c.inp("b_sq%d" % c0, bs[c0:c0 + 384].contiguous()), k, bd, bi, first=(c0 == 0))

    def ref():
        wd, wi = _topk(d[:, :n_valid], k)
        assert (bd[:, :k].double() - wd).abs().max().item() < 1e-5
        assert (d[:, :n_valid].gather(1, bi[:, :k].long()) - wd).abs().max().item() < 1e-5 and float((bi[:, :k] == wi).float().mean()) > 0.99
    return ref


def _filter(c, cap, merge):
    nq, nb, D, k, n_valid, col0, L = 300, 768, 64, 10, 700, 1000, ops.knn_list_capacity()
    Q, Bk, d = _knn_data(nq, nb, D)
    d = d[:, :n_valid]
    tau = torch.sort(d, 1).values[:, 39].float()                                 # the 40th best distance: ~40 pass per query
    qs, bs = Q.pow(2).sum(1), Bk.pow(2).sum(1)
    pl = D + 8
    cnt = c.inout("cnt", torch.zeros(nq, dtype=i32, device=_dev()))
    cand = c.inout("cand", torch.full((nq * cap * 2,), -7, dtype=i32, device=_dev()))   # the guard right after cap entries per the last query
    ops.knn_filter_x3(c.inp("Q", planes3(Q, pl), ld=3 * pl + 8, mask=pmask(nq, D, pl)), pl,
                      c.inp("B", planes3(Bk, pl), ld=3 * pl + 8, mask=pmask(nb, D, pl)), pl, nq, nb, D, c.inp("q_sq", qs), c.inp("b_sq", bs),
                      c.inp("tau", tau), col0, col0 + n_valid, cnt, cand, cap)
    if not merge:
        def ref():
            n = cnt.long()
            want = (d <= tau.double()[:, None] + 1e-5).sum(1)
            low = (d <= tau.double()[:, None] - 1e-5).sum(1)
            assert bool((n <= want).all()) and bool((n >= low).all())
            assert bool((n > cap).all()) if cap < 30 else bool((n <= cap).all())
            cv = cand.view(nq, cap, 2)
            for q in (0, 131, nq - 1):
                m = min(int(n[q]), cap)
                ids = cv[q, :m, 1].long() - col0
                assert bool(((ids >= 0) & (ids < n_valid)).all()) and len(set(ids.tolist())) == m
                assert (cv[q, :m, 0].contiguous().view(f32).double() - d[q, ids]).abs().max().item() < 1e-5
                assert bool((cv[q, m:] == -7).all()), "slots past the count are not written"
        return ref
    bd0, bi0 = torch.full((nq, L), float("inf"), device=_dev()), torch.full((nq, L), 2 ** 31 - 1, dtype=i32, device=_dev())
    bd, bi = c.inout("best_d", bd0), c.inout("best_i", bi0)
    over = c.inout("overflow", torch.zeros(1, dtype=i32, device=_dev()))
    ops.knn_merge_list(cand, cnt, cap, nq, k, bd, bi, over)

    def ref2():
        assert int(cnt.abs().sum().item()) == 0, "cnt back to 0"
        assert int(over.item()) == (1 if cap < 30 else 0)
        if cap >= 30:
            wd, wi = _topk(d, k)
            assert (bd[:, :k].double() - wd).abs().max().item() < 1e-5 and float((bi[:, :k].long() - col0 == wi).float().mean()) > 0.99
    return ref2


entry("knn_filter_x3", [64, 16])(lambda c, cap, mp: _filter(c, cap, False))
entry("knn_merge_list", [64, 16])(lambda c, cap, mp: _filter(c, cap, True))


def _rank_data(c):
    nq, nb, D, n_valid = 300, 768, 64, 700
    Bk = _unit(randn(2, nb, D))
    Bk[n_valid:] = 0
    g = _gen(3)
    a = torch.randint(0, n_valid, (nq,), device=_dev(), generator=g)
    p = (a + 1 + torch.randint(0, n_valid - 1, (nq,), device=_dev(), generator=g)) % n_valid
    pl = D + 8
    Qv = c.inp("Q", planes3(Bk[a], pl), ld=3 * pl + 8, mask=pmask(nq, D, pl))
    bs = Bk.pow(2).sum(1)
    return nq, nb, D, n_valid, Bk, a, p, pl, Qv, bs


@entry("rank_tau_x3")
def _rtau(c, mp):
    nq, nb, D, n_valid, Bk, a, p, pl, Qv, bs = _rank_data(c)
    PP = torch.zeros(512, D, device=_dev())
    PP[:nq] = Bk[p]
    psq = torch.zeros(512, device=_dev())
    psq[:nq] = bs[p]
    tau = c.out("tau", (nq,), f32)
    ops.rank_tau_x3(Qv, pl, c.inp("P", planes3(PP, pl), ld=3 * pl + 8, mask=pmask(512, D, pl)), pl, nq, D, c.inp("q_sq", bs[a]), c.inp("p_sq", psq), tau)
    return lambda: _le((tau.double() - (Bk[a].double() - Bk[p].double()).pow(2).sum(1)).abs().max().item(), 1e-5)


@entry("rank_count_x3")
def _rcount(c, mp):
    nq, nb, D, n_valid, Bk, a, p, pl, Qv, bs = _rank_data(c)
    dd = (Bk[a].double()[:, None, :] - Bk.double()[None, :n_valid, :]).pow(2).sum(-1)          # [nq, n_valid]
    i = torch.arange(nq, device=_dev())
    tau = dd[i, p].float()
    count = c.inout("count", torch.full((nq,), 5, dtype=i32, device=_dev()))
    Bv = c.inp("B", planes3(Bk, pl), ld=3 * pl + 8, mask=pmask(nb, D, pl))
    qv, bv, tv = c.inp("q_sq", bs[a]), c.inp("b_sq", bs), c.inp("tau", tau)
    pv, av = c.inp("pos_id", p.to(i32)), c.inp("self_id", a.to(i32))
    for c0, nc in ((0, 256), (256, 512)):                     # two launches accumulate; n_valid = 700 lies inside the last tile
        ops.rank_count_x3(Qv, pl, Bv[c0:c0 + nc], pl, nq, nc, D, qv, bv[c0:c0 + nc], tv, pv, av, c0, n_valid, count)

    def ref():
        j = torch.arange(n_valid, device=_dev())[None, :]
        other = (j != a[:, None]) & (j != p[:, None])
        t = tau.double()[:, None]
        sure = (other & (dd < t - 1e-5)).sum(1)
        maybe = (other & (dd < t + 1e-5)).sum(1)
        got = count.long() - 5
        assert bool((got >= sure).all()) and bool((got <= maybe).all())
        exact = (other & ((dd.float() < tau[:, None]) | ((dd.float() == tau[:, None]) & (j < p[:, None])))).sum(1)
        assert float((got == exact).float().mean()) > 0.98
    return ref


@entry("knn_desim_prep", [i32, i64])
def _dprep(c, dt, mp):
    n_f, kf, kp, end, thr = 257, 40, 32, 30, 0.5
    g = _gen(4)
    fI = torch.randint(-1, n_f, (n_f, kf), device=_dev(), generator=g).to(dt)
    fI[:, 3] = torch.arange(n_f, device=_dev()).to(dt)        # the row itself
    fD = torch.rand(n_f, kf, device=_dev(), generator=g)
    fD[4, 6] = thr                                            # == threshold is kept
    out = c.out("out", (n_f, kp), i32)
    ops.knn_desim_prep(c.inp("fI", fI, ld=kf + 4), c.inp("fD", fD, ld=kf + 4), end, thr, out)

    def ref():
        t = torch.arange(kp, device=_dev())[None, :]
        I, Dd = torch.full((n_f, kp), -1, device=_dev(), dtype=torch.long), torch.full((n_f, kp), 9.0, device=_dev())
        I[:, :end], Dd[:, :end] = fI[:, :end].long(), fD[:, :end]
        keep = (t < end) & ~(Dd > thr) & (I != torch.arange(n_f, device=_dev())[:, None]) & (I >= 0)
        assert torch.equal(out.long(), torch.where(keep, I, torch.full_like(I, -1)))
    return ref


@entry("knn_desim")
def _desim(c, mp):
    nq, ke, kp, n_f, row0 = 150, 20, 32, 400, 3
    rng = np.random.RandomState(6)
    eI = rng.randint(-1, n_f + 20, size=(nq, ke)).astype(np.int32)
    ff = rng.randint(-1, n_f, size=(n_f, kp)).astype(np.int32)
    for r in range(0, nq, 3):                                 # plant near-duplicates: a later column listed by an earlier one
        if 0 <= eI[r, 1] < n_f:
            ff[eI[r, 1], 5] = eI[r, 7]
    eI[4, 2] = row0 + 4                                       # the query itself
    out = c.out("out", (nq, ke), i32, ld=ke + 4)
    ops.knn_desim(c.inp("eI", _t(eI, i32), ld=ke + 4), c.inp("f_filtered", _t(ff, i32)), out, row0=row0)

    def ref():
        want = np.full((nq, ke), -1, np.int32)
        for i in range(nq):
            keep = [(0 <= v < n_f) for v in eI[i]]
            for a_ in range(ke):
                if keep[a_]:
                    near = set(ff[eI[i, a_]].tolist())
                    for b_ in range(a_ + 1, ke):
                        if keep[b_] and eI[i, b_] in near:
                            keep[b_] = False
            for a_ in range(ke):
                if keep[a_] and eI[i, a_] != row0 + i:
                    want[i, a_] = eI[i, a_]
        assert np.array_equal(out.cpu().numpy(), want)
    return ref


# ==================================================================================================== the test =====
@pytest.mark.gpu
@pytest.mark.parametrize("eid,variant", [(e["id"], v) for e in table.ENTRIES for v in LAUNCH.get(e["id"], (None, (None,)))[1]],
                         ids=lambda x: str(x))
def test_footprint(gpu, eid, variant, monkeypatch):
    fn = LAUNCH[eid][0]
    cases = []

    def run(pattern):
        c = Case(gpu, pattern)
        ref = fn(c, variant, monkeypatch) if variant is not None else fn(c, monkeypatch)
        torch.cuda.synchronize()
        cases.append((c, ref))
        return c.payloads()

    fp.assert_fully_written(run)
    for c, _ in cases:
        c.assert_guards()
    for c, _ in cases:
        c.assert_inputs_frozen()
    cases[-1][1]()                                          # the reference comparison
    declared = set(table.OPERANDS[eid])                     # the table's operand list is the launch's: names and roles
    for c, _ in cases:
        assert c.roles <= declared, "operands the table does not declare for %s: %s" % (eid, sorted(c.roles - declared))
    _USED.setdefault(eid, set()).update(cases[-1][0].roles)


_USED = {}


@pytest.mark.gpu
def test_every_declared_operand_is_used_by_some_variant(gpu):
    """runs after test_footprint (file order): an operand the table lists and no variant of the entry allocates has drifted"""
    assert set(_USED) == {e["id"] for e in table.ENTRIES}, "run the whole file: this test reads what test_footprint recorded"
    for e in table.ENTRIES:
        unused = set(table.OPERANDS[e["id"]]) - _USED[e["id"]]
        assert not unused, "%s: declared in the table, allocated by no variant: %s" % (e["id"], sorted(unused))
