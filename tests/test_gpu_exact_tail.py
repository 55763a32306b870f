"""The triplet tail of csrc/loss.hip -- l2norm forward / backward, the hinge kernels, the fused tail with its bf16,
three-plane and fp16-plane copies, the indexed hinge with its key scan, the statistics, the elementwise kernels -- against
the models of tests/exact_tail.py at zero tolerance: operands on dyadic grids whose every reduction is exact in fp32 in
any order, so the hinge's corner (gradient at t >= 0, hinge and active count at t > 0), lrelu' at +0 / -0, the norm clamp
and the projection term it drops, the in-batch validity masks and slot arithmetic, and the indexed backward's keys,
chunks, list flush and row-to-wave mapping all show as a mismatch.  tests/test_exact_tail_host.py shows on the same cases
that the expectation is the existing specification (oracle.tower), is order-independent, and changes under every single
mutation of a rule.

Comparisons are ``torch.equal`` on values (bit patterns for the 16-bit copies) except, as exact_tail states and bounds:
1 / sqrt(1e-12f) is read once from the device (within 1 ulp of the correctly rounded value) and used by the model; what a
tiny row's non-dyadic normalised coordinate enters through a reduction, and the gradients of a batch that is no power of
two (2 / B is rounded), are compared within the forward bound ``exact_tail.reduction_bound`` propagates -- rows that must
be exactly zero still are.  stats[4] is within 1 fp32 ulp of the float64 model (the column sums are exact; only the order
of the double operations is free).  Measured on the MI355X: sqrt and division are exact at the powers of four, so the rows
keep their scales 2^s, s in [-3, 3] (|z|^2 = 4^s returns the unit row and inv = 2^-s bit for bit), and the device's
1 / sqrt(1e-12f) is 1 000 000.0, the model's value.  Outputs go into poisoned, guarded buffers with padded leading dimensions and plane
gaps; inputs are views with NaN-filled gaps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402
import exact_tail as xt  # noqa: E402
import footprint as fp  # noqa: E402

pytestmark = pytest.mark.gpu

from cdml_amd import ops  # noqa: E402

F32, I32, U8, BF16, F16 = torch.float32, torch.int32, torch.uint8, torch.bfloat16, torch.float16
PAD = 4


@pytest.fixture(scope="module")
def dev(gpu):
    assert ops.LRELU_ALPHA == xt.ALPHA_REF
    return gpu


@pytest.fixture(scope="module")
def inv_c(dev):
    """1 / sqrt(max(0, 1e-12f)) as this device computes it, read from l2norm_fwd on an all-zero row: within 1 ulp of
    float32(1 / sqrt(float64(float32(1e-12)))) -- one correctly rounded sqrt and one division"""
    x = torch.zeros((1, 4), dtype=F32, device=dev)
    y, inv = fp.Guarded((1, 4), F32, dev), fp.Guarded((1,), F32, dev)
    ops.l2norm_fwd(x, 4, y.view, inv.view)
    got = np.float32(inv.payload().cpu().numpy()[0])
    assert abs(float(got) - float(xt.INV_C_MODEL)) <= float(np.spacing(xt.INV_C_MODEL)), (got, xt.INV_C_MODEL)
    print("device 1/sqrt(1e-12f) = %r (model %r)" % (float(got), float(xt.INV_C_MODEL)))
    return float(got)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def dev_in(v, dev):
    """an exact float64 operand [rows][cols] as an fp32 device view with ld = cols + PAD and a poisoned gap"""
    v = np.asarray(v, np.float64)
    return xs.strided(xg.f32_exact(v), pad=PAD).to(dev)[:, :v.shape[1]]


def rows_out(rows, cols, dev, dtype=F32):
    return fp.Guarded((rows, cols), dtype, dev, ld=cols + PAD)


def vec_out(n, dev, dtype=F32, mask=None):
    return fp.Guarded((n,), dtype, dev, mask=mask)


def _first(bad):
    return tuple(int(v) for v in torch.nonzero(bad)[0])


def assert_equal(g, want, what):
    """the payload of a guarded output equals the (exact) expectation, value for value; the guards are intact"""
    got = g.payload().cpu() if isinstance(g, fp.Guarded) else g.detach().cpu()
    w = xg.f32_exact(want) if got.dtype == F32 else torch.as_tensor(np.asarray(want)).to(got.dtype)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    if not torch.equal(got, w):
        bad = ~((got == w) | (torch.isnan(got.float()) & torch.isnan(w.float())))
        i = _first(bad)
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.numel(), i, got[i].item(), w[i].item()))
    if isinstance(g, fp.Guarded):
        g.assert_guards_intact(what)


def assert_within(g, want, tol, what):
    """|got - want| <= tol element by element (float64); where tol is 0 the element is exact"""
    got = (g.payload() if isinstance(g, fp.Guarded) else g).detach().cpu().double().numpy()
    want, tol = np.asarray(want, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(want))
    assert got.shape == want.shape and not np.isnan(got).any(), what
    bad = ~(np.abs(got - want) <= tol)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements outside their bound; first at %s: got %r, expected %r, bound %g (%d of them exact)"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i], tol[i], int((bad & (tol == 0)).sum())))
    if isinstance(g, fp.Guarded):
        g.assert_guards_intact(what)


def assert_bits(got, want, what):
    """a 16-bit buffer, gaps included, bit for bit"""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = xg.bits(got) != xg.bits(want)
    if bool(bad.any()):
        i = _first(bad)
        sign_only = int(((xg.bits(got) ^ xg.bits(want)) == -32768)[bad].sum())
        raise AssertionError("%s: %d of %d elements differ (%d in the sign bit alone); first at %s: got %r, expected %r"
                             % (what, int(bad.sum()), bad.numel(), sign_only, i, got[i].item(), want[i].item()))


def copy_buffer(fmt, R, D, dev):
    """(buffer, plane, h2_scale) of a dz2 copy format: "bf16" [R][D + PAD]; "x3" three bf16 planes D + PAD apart; "h2" two fp16
    planes; all poisoned"""
    if fmt == "bf16":
        return fp.poisoned((R, D + PAD), dtype=BF16, device=dev), 0, 0.0
    plane = D + PAD
    if fmt == "x3":
        return fp.poisoned((R, 3 * plane + PAD), dtype=BF16, device=dev), plane, 0.0
    return fp.poisoned((R, 2 * plane + PAD), dtype=F16, device=dev), plane, xt.H2_SCALE


def copy_want(fmt, dz2_f32, plane, ld):
    """the copy of an fp32 dz2 (CPU tensor) by the exact_gemm helpers, over the poison: gaps must keep it"""
    if fmt == "bf16":
        return xg.plane_buffer([dz2_f32.to(BF16)], ld, ld)
    if fmt == "x3":
        return xg.plane_buffer(xg.split_planes(dz2_f32, 3), plane, ld)
    sv = (dz2_f32 * xt.H2_SCALE).clamp(-65504.0, 65504.0)
    return xg.plane_buffer(xg.split_planes(sv, 2, F16), plane, ld)


# ---- l2norm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", xt.L2_M)
@pytest.mark.parametrize("N", xt.L2_N)
def test_l2norm_fwd(dev, inv_c, M, N):
    """|z|^2 = 4^s returns the unit rows and inv = 2^-s bit for bit; the zero row 0 and the device's 1 / sqrt(1e-12f); the
    tiny row 2^-21 times that (an exact scaling); the control row -1 and 2^19"""
    c = xt.rows_case(M, N)
    assert c["safe"] < 2.0 ** 24
    x = dev_in(c["z"], dev)
    y, inv = rows_out(M, N, dev), vec_out(M, dev)
    with fp.frozen(x):
        ops.l2norm_fwd(x, N, y.view, inv.view)
    e, inv_m, ss, clamped = xt.normalize(c["z"], inv_c)
    assert_equal(inv, inv_m, c["name"] + " inv")
    assert_equal(y, e, c["name"] + " y")
    reg = ss == 4.0 ** c["s"]
    assert torch.equal(inv.payload().cpu()[torch.from_numpy(reg)], xg.f32_exact(2.0 ** -c["s"][reg].astype(np.float64)))


@pytest.mark.parametrize("alpha", xt.ALPHAS)
@pytest.mark.parametrize("M", xt.L2_M)
@pytest.mark.parametrize("N", xt.L2_N)
def test_l2norm_bwd(dev, inv_c, M, N, alpha):
    """dz = inv (g - z c) lrelu'(z): exact rows bit for bit; the zero and the tiny row inv_c g (no projection term: the
    tiny row's <z, g> is not 0), the control row with its term; lrelu' off, 1/4, 0.2"""
    c = xt.rows_case(M, N)
    assert c["safe"] < 2.0 ** 24
    z, g = dev_in(c["z"], dev), dev_in(c["g"], dev)
    dz = rows_out(M, N, dev)
    with fp.frozen(z, g):
        ops.l2norm_bwd(z, g, N, dz.view, lrelu_alpha=alpha)
    want, _ = xt.l2norm_bwd_model(c["z"], c["g"], alpha, inv_c=inv_c)
    assert_equal(dz, want, "%s alpha=%g dz" % (c["name"], alpha))


# ---- the hinge kernels -----------------------------------------------------------------------------------------------------------------
def _check_corner(c, m, hinge, de, stats):
    """corner triplets: hinge == 0, not counted in stats[3], non-zero gradient rows"""
    h, d = hinge.payload().cpu().numpy(), de.payload().cpu().numpy()
    for i in c["classes"]["corner"]:
        assert h[i] == 0.0 and np.abs(d[m["tri"][i, 0]]).max() + np.abs(d[m["tri"][i, 1]]).max() > 0, "%s: corner triplet %d" % (c["name"], i)
    assert float(stats.payload().cpu()[3]) == float((h > 0).sum()) / c["B"]


@pytest.mark.parametrize("B,D", xt.hinge_params())
def test_triplet_hinge(dev, B, D):
    c = xt.hinge_case(B, D)
    assert c["safe"] < 2.0 ** 24
    m = xt.tail_model(c, tail=False)
    e = dev_in(m["e"], dev)
    pos, neg, hinge, stats = vec_out(B, dev), vec_out(B, dev), vec_out(B, dev), vec_out(4, dev)
    de = rows_out(3 * B, D, dev)
    with fp.frozen(e):
        ops.triplet_hinge(e, B, D, c["margin"], pos.view, neg.view, hinge.view, stats.view, de.view)
    for g, k in ((pos, "pos"), (neg, "neg"), (hinge, "hinge"), (de, "de"), (stats, "stats")):
        assert_equal(g, m[k], "%s %s" % (c["name"], k))
    _check_corner(c, m, hinge, de, stats)


@pytest.mark.parametrize("B,D,shift", xt.inbatch_params())
def test_triplet_hinge_inbatch(dev, B, D, shift):
    c = xt.inbatch_case(B, D, shift)
    assert c["safe"] < 2.0 ** 24
    m = xt.tail_model(c, tail=False)
    e = dev_in(m["e"], dev)
    ids, sh = torch.from_numpy(c["ids"]).to(dev), torch.tensor([shift], dtype=I32, device=dev)
    pos, neg, hinge, stats = vec_out(B, dev), vec_out(B, dev), vec_out(B, dev), vec_out(4, dev)
    valid, de = vec_out(B, dev, U8), rows_out(2 * B, D, dev)
    with fp.frozen(e, ids, sh):
        ops.triplet_hinge_inbatch(e, ids, sh, B, D, c["margin"], pos.view, neg.view, hinge.view, valid.view, stats.view, de.view)
    for g, k in ((pos, "pos"), (neg, "neg"), (hinge, "hinge"), (valid, "valid"), (de, "de"), (stats, "stats")):
        assert_equal(g, m[k], "%s %s" % (c["name"], k))
    _check_corner(c, m, hinge, de, stats)


# ---- the fused tail ------------------------------------------------------------------------------------------------------------------
TAIL_RUNS = (("none", xt.ALPHA_DYADIC, False), ("none", xt.ALPHA_REF, True), ("bf16", xt.ALPHA_REF, False),
             ("x3", xt.ALPHA_DYADIC, False), ("h2", xt.ALPHA_REF, True))        # (copy format, alpha, with the variance)


def _run_tail(c, dev, fmt, alpha, with_var):
    """one launch of vnet_tail into fresh poisoned outputs -> dict of the guarded outputs, the copy buffer and its geometry"""
    B, D, mode = c["B"], c["D"], 0 if c["kind"] == "m0" else 1
    R = len(c["z"])
    z = dev_in(c["z"], dev)
    ids = sh = None
    if mode:
        ids, sh = torch.from_numpy(c["ids"]).to(dev), torch.tensor([c["shift"]], dtype=I32, device=dev)
    o = dict(e=rows_out(R, D, dev), dz2=rows_out(R, D, dev), pos=vec_out(B, dev), neg=vec_out(B, dev), hinge=vec_out(B, dev),
             stats=vec_out(5, dev, mask=torch.tensor([[True] * 4 + [with_var]])), valid=vec_out(B, dev, U8) if mode else None)
    bf, plane, h2 = copy_buffer(fmt, R, D, dev) if fmt != "none" else (None, 0, 0.0)
    ws = fp.poisoned(ops.vnet_tail_workspace_floats(B, D), dtype=F32, device=dev) if with_var else None
    with fp.frozen(z):
        ops.vnet_tail(mode, z, ids, sh, B, D, c["margin"], o["e"].view, o["pos"].view, o["neg"].view, o["hinge"].view, o["dz2"].view,
                      valid=None if o["valid"] is None else o["valid"].view, stats=o["stats"].view, dz2_bf16=bf, var_ws=ws,
                      alpha=alpha, plane_bf=plane, h2_scale=h2)
    o.update(bf=bf, plane=plane, z=z, ids=ids, sh=sh)
    return o


def _check_stats(o, m, with_var, what, tol=None):
    st = o["stats"].flat[0].detach().cpu()
    if tol is None:
        assert torch.equal(st[:4], torch.from_numpy(m["stats"])), (what, st, m["stats"])
    else:
        assert (np.abs(st[:4].double().numpy() - m["stats"].astype(np.float64)) <= tol).all(), (what, st, m["stats"], tol)
    if with_var:
        v32 = np.float32(m["var"])
        assert abs(float(st[4]) - m["var"]) <= float(np.spacing(v32)), (what, float(st[4]), m["var"])
    o["stats"].assert_guards_intact(what + " stats")


def _tail_cases(mode, D):
    if mode == 0:
        return [xt.hinge_case(B, D) for B in xt.TAIL_B]
    return [xt.inbatch_case(B, D, sh) for B in xt.TAIL_B for sh in xt.shifts_of(B)]


@pytest.mark.parametrize("D", xt.TAIL_D)
@pytest.mark.parametrize("mode", (0, 1))
def test_vnet_tail(dev, inv_c, mode, D):
    """modes 0 and 1, the three NCH buckets, B in {2, 8, 64} (every shift), without a copy, with the bf16 copy, the three
    planes (plane = D + 4) and the fp16 planes at scale 2^10 -- where the zero rows' gradients saturate to (+-65 504, 0);
    stats[0..3] exact, stats[4] within 1 ulp; and the separate kernels (l2norm_fwd, triplet_hinge / _inbatch, l2norm_bwd)
    give the same bits: on exact operands no contraction can differ"""
    for c in _tail_cases(mode, D):
        assert c["safe"] < 2.0 ** 24 and not c["inexact"]
        B, R = c["B"], len(c["z"])
        for fmt, alpha, with_var in TAIL_RUNS:
            what = "%s %s alpha=%g" % (c["name"], fmt, alpha)
            m = xt.tail_model(c, alpha, inv_c=inv_c)
            o = _run_tail(c, dev, fmt, alpha, with_var)
            for k in ("e", "pos", "neg", "hinge", "dz2") + (("valid",) if mode else ()):
                assert_equal(o[k], m[k], "%s %s" % (what, k))
            _check_stats(o, m, with_var, what)
            if fmt != "none":
                w32 = xg.f32_exact(m["dz2"])
                assert_bits(o["bf"], copy_want(fmt, w32, o["plane"], o["bf"].shape[1]), what + " copy")
                if fmt == "h2" and m["clamped"].any() and B >= 8:                     # the saturating branch, on purpose
                    zr = np.nonzero(m["clamped"])[0]
                    sat = np.abs(m["dz2"][zr]) * xt.H2_SCALE > 65504.0
                    assert sat.any() and (sat == (m["dz2"][zr] != 0)).all(), what
                    hi = o["bf"][:, :D].float().cpu().numpy()[zr]
                    lo = o["bf"][:, o["plane"]:o["plane"] + D].float().cpu().numpy()[zr]
                    assert (np.abs(hi[sat]) == 65504.0).all() and (lo[sat] == 0).all(), what
        # the separate kernels on the same case: equal bits
        alpha = xt.ALPHA_REF
        o = _run_tail(c, dev, "none", alpha, False)
        e0, de0, dz0 = rows_out(R, D, dev), rows_out(R, D, dev), rows_out(R, D, dev)
        p0, n0, h0, s0 = vec_out(B, dev), vec_out(B, dev), vec_out(B, dev), vec_out(4, dev)
        ops.l2norm_fwd(o["z"], D, e0.view)
        if mode:
            ops.triplet_hinge_inbatch(e0.view, o["ids"], o["sh"], B, D, c["margin"], p0.view, n0.view, h0.view, None, s0.view, de0.view)
        else:
            ops.triplet_hinge(e0.view, B, D, c["margin"], p0.view, n0.view, h0.view, s0.view, de0.view)
        ops.l2norm_bwd(o["z"], de0.view, D, dz0.view, lrelu_alpha=alpha)
        for a, b, k in ((e0, "e", "e"), (p0, "pos", "pos"), (n0, "neg", "neg"), (h0, "hinge", "hinge"), (dz0, "dz2", "dz2")):
            assert torch.equal(a.payload(), o[b].payload()), "%s: fused and separate kernels differ in %s" % (c["name"], k)
        assert torch.equal(s0.payload(), o["stats"].flat[0, :4])


def _tiny_cases(mode):
    return [xt.hinge_case(64, 64, tiny=True), xt.hinge_case(32, 260, tiny=True)] if mode == 0 else [xt.inbatch_case(64, 64, 1, tiny=True)]


@pytest.mark.parametrize("mode", (0, 1))
def test_vnet_tail_tiny_rows(dev, inv_c, mode):
    """a tiny row (one coordinate 2^-21: clamped, but <z, g> != 0) beside its control (2^-19: not clamped) in active
    triplets: e is elementwise and exact everywhere; in mode 0 so is the tiny row's own dz2 (no projection term) -- the
    other rows of its triplets carry its non-dyadic coordinate through pos, neg and <z, g> and are compared within the
    propagated forward bound; every row and triplet it does not touch stays bit for bit; the copies are those of the dz2
    this launch wrote"""
    for c in _tiny_cases(mode):
        assert c["safe"] < 2.0 ** 24 and c["inexact"] == "tiny"
        B, D, R = c["B"], c["D"], len(c["z"])
        for fmt, alpha, with_var in (("none", xt.ALPHA_DYADIC, False), ("x3", xt.ALPHA_REF, False), ("bf16", xt.ALPHA_REF, False)):
            what = "%s %s alpha=%g" % (c["name"], fmt, alpha)
            m = xt.tail_model(c, alpha, inv_c=inv_c)
            assert (np.abs(m["t"][m["dirty_t"]]) >= 0.125).all() and (m["dz2_tol"][~m["dirty"]] == 0).all()
            assert (m["dz2"][c["tiny_rows"]] != 0).any()
            if mode == 0:
                assert (m["dz2_tol"][c["tiny_rows"]] == 0).all()
            o = _run_tail(c, dev, fmt, alpha, with_var)
            assert_equal(o["e"], m["e"], what + " e")
            if mode:
                assert_equal(o["valid"], m["valid"], what + " valid")
            assert_within(o["pos"], m["pos"], m["pos_tol"], what + " pos")
            assert_within(o["neg"], m["neg"], m["pos_tol"], what + " neg")
            assert_within(o["hinge"], m["hinge"], (2 * m["pos_tol"] + 8 * xt.U) * m["dirty_t"], what + " hinge")   # (two more additions, |.| <= 4)
            assert_within(o["dz2"], m["dz2"], m["dz2_tol"], what + " dz2")
            tol = (2 * m["pos_tol"].sum() + xt.reduction_bound(np.stack([m["hinge"], m["pos"], m["neg"]])).max()) / B + xt.U
            _check_stats(o, m, with_var, what, tol=tol)
            if fmt != "none":
                assert_bits(o["bf"], copy_want(fmt, o["dz2"].payload().cpu(), o["plane"], o["bf"].shape[1]), what + " copy")


@pytest.mark.parametrize("mode", (0, 1))
def test_vnet_tail_batch_no_power_of_two(dev, inv_c, mode):
    """B = 5 (D = 64) and B = 67 (D = 260): 2 / B is rounded, so the gradients are not order-free -- e, pos, neg, hinge,
    valid and stats[0..3] (one correctly rounded division) bit for bit; dz2 within its propagated bound, rows that must be
    exactly zero exactly zero (the builder asserts that a lost or misplaced term moves an element by four times the
    bound); the copies are those of the dz2 this launch wrote"""
    for c in xt.tail_npow2_cases(mode):
        assert c["safe"] < 2.0 ** 24 and c["inexact"] == "npow2"
        for fmt, alpha, with_var in (("none", xt.ALPHA_DYADIC, True), ("x3", xt.ALPHA_REF, False), ("bf16", xt.ALPHA_REF, False)):
            what = "%s %s alpha=%g" % (c["name"], fmt, alpha)
            m = xt.tail_model(c, alpha, inv_c=inv_c)
            o = _run_tail(c, dev, fmt, alpha, with_var)
            for k in ("e", "pos", "neg", "hinge") + (("valid",) if mode else ()):
                assert_equal(o[k], m[k], "%s %s" % (what, k))
            _check_stats(o, m, with_var, what)
            zero_rows = (m["dz2"] == 0).all(1) & (m["dz2_tol"] == 0).all(1)
            assert zero_rows.any() and (m["dz2_tol"][~zero_rows].max(1) > 0).all()
            assert_within(o["dz2"], m["dz2"], m["dz2_tol"], what + " dz2")
            if fmt != "none":
                assert_bits(o["bf"], copy_want(fmt, o["dz2"].payload().cpu(), o["plane"], o["bf"].shape[1]), what + " copy")


# ---- the indexed hinge -----------------------------------------------------------------------------------------------------------------
IDX_PARAMS = [a + (False,) for a in xt.INDEXED_PARAMS + xt.NPOW2_PARAMS] + [(64, 64, "mix", 0, True)]


@pytest.mark.parametrize("B,D,kind,variant,tiny", IDX_PARAMS)
def test_triplet_hinge_indexed(dev, inv_c, B, D, kind, variant, tiny):
    """neg_row in {-1, own anchor, own positive, R - 1, a hub, the four rows of one wave}; inactive triplets that mined the
    hub (key -1: they add nothing); 1 024 anchors on one row (the 512-entry flush); 16 384 triplets (two key chunks, a hub
    across the boundary); batches that are no power of two (8 197: a last chunk of 5 keys) -- pos, neg, hinge, the key words
    and stats bit for bit, the gradients bit for bit (power-of-two batches) or within their bound with exact zeros; then
    the fused tail with the bf16 copy and the three planes"""
    c = xt.indexed_case(B, D, kind, variant, tiny)
    assert c["safe"] < 2.0 ** 24
    R, inexact = 2 * B, c["inexact"]
    e_in = None
    for fmt, alpha in ((None, -1.0), ("bf16", xt.ALPHA_REF), ("x3", xt.ALPHA_DYADIC)):
        what = "%s %s" % (c["name"], fmt or "no tail")
        m = xt.tail_model(c, alpha, inv_c=inv_c, tail=fmt is not None)
        if e_in is None:
            e_in, z_in = dev_in(m["e"], dev), dev_in(c["z"], dev)
            nr = torch.from_numpy(c["neg_row"]).to(dev)
        pos, neg, hinge, key, stats = vec_out(B, dev), vec_out(B, dev), vec_out(B, dev), vec_out(B, dev), vec_out(4, dev)
        de = rows_out(R, D, dev)
        dz2 = bf = None
        plane = 0
        with fp.frozen(e_in, z_in, nr):
            if fmt is None:
                ops.triplet_hinge_indexed(e_in, nr, B, D, c["margin"], pos.view, neg.view, hinge.view, key.view, stats.view, de.view)
            else:
                dz2 = rows_out(R, D, dev)
                bf, plane, _ = copy_buffer(fmt, R, D, dev)
                ops.triplet_hinge_indexed(e_in, nr, B, D, c["margin"], pos.view, neg.view, hinge.view, key.view, stats.view, de.view,
                                          z=z_in, dz2=dz2.view, dz2_bf16=bf, plane_bf=plane, lrelu_alpha=alpha)
        if inexact == "tiny":
            assert_within(pos, m["pos"], m["pos_tol"], what + " pos")
            assert_within(neg, m["neg"], m["pos_tol"], what + " neg")
            assert_within(hinge, m["hinge"], (2 * m["pos_tol"] + 8 * xt.U) * m["dirty_t"], what + " hinge")
        else:
            for g, k in ((pos, "pos"), (neg, "neg"), (hinge, "hinge"), (stats, "stats")):
                assert_equal(g, m[k], "%s %s" % (what, k))
        got_key = key.payload().view(I32).cpu().numpy()
        assert np.array_equal(got_key, m["key"]), "%s: key words differ for triplets %s" % (what, np.nonzero(got_key != m["key"])[0][:8].tolist())
        key.assert_guards_intact(what + " key")
        if inexact:
            assert_within(de, m["de"], m["de_tol"], what + " de")
        else:
            assert_equal(de, m["de"], what + " de")
        if fmt is not None:
            if inexact:
                assert_within(dz2, m["dz2"], m["dz2_tol"], what + " dz2")
                w32 = dz2.payload().cpu()                       # the copies: those of the dz2 this launch wrote
            else:
                assert_equal(dz2, m["dz2"], what + " dz2")
                w32 = xg.f32_exact(m["dz2"])
            assert_bits(bf, copy_want(fmt, w32, plane, bf.shape[1]), what + " copy")


# ---- the elementwise kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", xt.EW_M)
@pytest.mark.parametrize("N", xt.EW_N)
def test_elementwise_kernels(dev, M, N):
    """lrelu_bwd, ew_fusion_bwd (residual 0 and 1), ew_combine (modes 0 - 2), pair_dist with its means (P = 8, a pair (i, i)):
    dyadic inputs with 0.0 and -0.0 under non-zero gradients, against the single-rounding fp32 model"""
    c = xt.ew_case(M, N)
    assert c["safe"] < 2.0 ** 24
    g, a, b = dev_in(c["g"], dev), dev_in(c["a"], dev), dev_in(c["b"], dev)
    for alpha in (xt.ALPHA_DYADIC, xt.ALPHA_REF):
        out = rows_out(M, N, dev)
        with fp.frozen(g, a):
            ops.lrelu_bwd(g, a, out.view, M, N, alpha=alpha)
        assert_equal(out, xt.lrelu_bwd_model(c["g"], c["a"], alpha), "%s lrelu_bwd alpha=%g" % (c["name"], alpha))
        for res in (0, 1):
            da, db = rows_out(M, N, dev), rows_out(M, N, dev)
            with fp.frozen(g, a, b):
                ops.ew_fusion_bwd(res, g, a, b, da.view, db.view, M, N, alpha=alpha)
            wa, wb = xt.ew_fusion_bwd_model(res, c["g"], c["a"], c["b"], alpha)
            assert_equal(da, wa, "%s ew_fusion_bwd res=%d alpha=%g da" % (c["name"], res, alpha))
            assert_equal(db, wb, "%s ew_fusion_bwd res=%d alpha=%g db" % (c["name"], res, alpha))
    for mode in (0, 1, 2):
        out = rows_out(M, N, dev)
        with fp.frozen(a, b):
            ops.ew_combine(mode, a, b, out.view, M, N)
        assert_equal(out, xt.ew_combine_model(mode, c["a"], c["b"]), "%s ew_combine mode %d" % (c["name"], mode))
    pairs = torch.from_numpy(c["pairs"]).to(dev)
    sd, dp, means = vec_out(c["P"], dev), vec_out(c["P"], dev), vec_out(4, dev)
    with fp.frozen(a, pairs):
        ops.pair_dist(a, pairs, N, sd.view, dp.view, means.view)
    wsd, wdp, wm = xt.pair_dist_model(c["a"], c["pairs"])
    assert wsd[0] == 0 and float(wm[3]) < 1.0
    assert_equal(sd, wsd, c["name"] + " pair sqdist")
    assert_equal(dp, wdp, c["name"] + " pair dot")
    assert_equal(means, wm, c["name"] + " pair means")
