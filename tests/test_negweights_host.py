"""Weighted negatives, host side: the quantisation properties and the tables of cdml_amd.negweights, the invariants of the
draw's host model (tests/negweights_ref.py), the refusals of TrainStep and the wrappers by name, and the argument checks of
include/cdml_negweights.h through the C ABI without a GPU."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import negweights_ref as ref  # noqa: E402
from oracle import sampler as osampler  # noqa: E402

T32 = 2 ** 32

TABLES = {
    "equal3": lambda: ref.equal_weights(3),
    "equal70001": lambda: ref.equal_weights(70001),
    "zipf1000": lambda: ref.zipf_weights(1000, 1),
    "zipf200000": lambda: ref.zipf_weights(200000, 2),
    "halfzero": lambda: ref.half_zero_weights(5000, 3),
}


@pytest.fixture(scope="module")
def nw_mod():
    from cdml_amd import negweights
    return negweights


@pytest.mark.parametrize("name", sorted(TABLES))
def test_quantisation_properties(nw_mod, name):
    """sum = 2^32 exactly, zero <=> zero, every positive entry within 2 quanta of 1 + w / sum(w) (2^32 - |P|)."""
    w = TABLES[name]()
    nw = nw_mod.NegativeWeights.from_weights(torch.from_numpy(w))
    q = nw.quanta.numpy()
    assert q.dtype == np.int64 and q.shape == w.shape
    assert int(q.sum()) == T32
    assert np.array_equal(q == 0, w == 0)
    assert (q >= 0).all()
    dev = np.abs(q - ref.ideal_quanta(w))[w > 0]
    print(name, "largest deviation from the ideal, in quanta:", dev.max())
    assert dev.max() <= 2.0
    if name == "halfzero":
        assert w[0] == 0 and w[-1] == 0 and (w == 0).sum() == len(w) // 2
        assert nw.n_live == int(np.flatnonzero(w)[-1]) + 1 < len(w)
    # the tables that derive from the quanta
    start, n_live = ref.start_of(q)
    assert nw.n_live == n_live and nw.start.dtype == torch.int32 and nw.start.numel() == n_live
    assert np.array_equal(ref.as_start(nw.start.numpy()), start)
    want_lq = (np.log(np.maximum(q, 1).astype(np.float64)) - 32 * np.log(2.0)).astype(np.float32)
    assert nw.lq.dtype == torch.float32 and np.array_equal(nw.lq.numpy(), want_lq) and np.isfinite(want_lq).all()
    assert nw.coarse.dtype == torch.int32 and nw.coarse.numel() == 2 ** 16 + 1 and nw.bits == 16


@pytest.mark.parametrize("bits", [8, 16, 20])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_owner_and_the_coarse_bracket(nw_mod, name, bits):
    w = TABLES[name]()
    nw = nw_mod.NegativeWeights.from_weights(w, bits=bits)
    q = nw.quanta.numpy()
    start = ref.as_start(nw.start.numpy())
    live = np.flatnonzero(q)
    assert np.array_equal(ref.owner(start, start[live]), live)
    assert np.array_equal(ref.owner(start, start[live] + q[live] - 1), live)
    assert ref.owner(start, 0) == live[0] and ref.owner(start, T32 - 1) == live[-1] == nw.n_live - 1
    assert np.array_equal(nw.owner(start[live]), live)                     # the module's own host search agrees
    coarse = nw.coarse.numpy()
    assert coarse[-1] == nw.n_live - 1 and coarse[0] == live[0]
    shift = 32 - bits
    assert np.array_equal(coarse[:-1], ref.owner(start, np.arange(2 ** bits, dtype=np.int64) << shift))
    r = np.random.default_rng(bits).integers(0, T32, size=200000, dtype=np.int64)
    r[:4] = (0, T32 - 1, (1 << shift) - 1, 1 << shift)
    v = ref.owner(start, r)
    assert (coarse[r >> shift] <= v).all() and (v <= coarse[(r >> shift) + 1]).all()
    assert (q[v] > 0).all()                                                # a word never lands on a row of weight 0


def test_from_counts_is_the_unigram_family(nw_mod):
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1000, size=4000).astype(np.float64)
    c[:7] = 0
    a = nw_mod.NegativeWeights.from_counts(c, power=0.75)
    b = nw_mod.NegativeWeights.from_weights(np.where(c > 0, c ** 0.75, 0.0))
    assert torch.equal(a.quanta, b.quanta) and (a.quanta[:7] == 0).all()
    # a mixture with uniform gives every row mass; at uniform_mix = 1 it is the equal table
    m = nw_mod.NegativeWeights.from_counts(c, power=0.75, uniform_mix=0.25)
    assert (m.quanta > 0).all()
    want = 0.75 * np.where(c > 0, c ** 0.75, 0.0) / (c[c > 0] ** 0.75).sum() + 0.25 / len(c)
    assert np.abs(m.quanta.numpy() - ref.ideal_quanta(want)).max() <= 2.0
    u = nw_mod.NegativeWeights.from_counts(c, uniform_mix=1.0)
    assert torch.equal(u.quanta, nw_mod.NegativeWeights.from_weights(np.ones(len(c))).quanta)
    # equal weights: lq is -log(n) to fp32 rounding
    assert np.abs(u.lq.numpy() + np.log(len(c))).max() < 1e-6
    for kw in (dict(power=-1.0), dict(uniform_mix=1.5), dict(power=float("inf"))):
        with pytest.raises(ValueError):
            nw_mod.NegativeWeights.from_counts(c, **kw)
    with pytest.raises(ValueError, match="bits"):
        nw_mod.NegativeWeights.from_weights(np.ones(10), bits=7)
    with pytest.raises(ValueError, match="bits"):
        nw_mod.NegativeWeights.from_weights(np.ones(10), bits=25)
    with pytest.raises(ValueError, match="2\\^32"):
        nw_mod.NegativeWeights(np.ones(10, dtype=np.int64))


def _pairs(rng, n_rows, n=64):
    a = rng.integers(0, n_rows, size=n)
    p = (a + 1 + rng.integers(0, n_rows - 1, size=n)) % n_rows
    return np.stack([a, p], 1).astype(np.int32)


@pytest.mark.parametrize("name", ["equal3", "zipf1000", "halfzero"])
def test_model_never_returns_the_pair_nor_a_row_of_weight_zero(nw_mod, name):
    w = TABLES[name]()
    n_rows = len(w)
    nw = nw_mod.NegativeWeights.from_weights(w)
    start = ref.as_start(nw.start.numpy())
    pairs = _pairs(np.random.default_rng(6), n_rows)
    for step in (0, 3, 2 ** 32 + 5):
        got, kind = ref.weighted_triplets(pairs, n_rows, 99, step, 48, start, slot0=48, batch_global=96)
        assert (got[:, 2] != got[:, 0]).all() and (got[:, 2] != got[:, 1]).all()
        assert (got[:, 2] >= 0).all() and (got[:, 2] < n_rows).all()
        assert (w[got[kind == 1, 2]] > 0).all()
        assert kind.sum() > 40                                            # the weighted draw is the rule, the fall-back rare
        want = osampler.device_triplets(pairs, n_rows, 99, step, 48, slot0=48, batch_global=96)
        assert np.array_equal(got[:, :2], want[:, :2])                    # the pair stream is the uniform sampler's


def test_model_falls_back_to_the_mode0_id_when_all_mass_sits_on_the_pair():
    n_rows = 500
    pairs = _pairs(np.random.default_rng(7), n_rows, 32)
    for i, (a, p) in enumerate(pairs):
        q = np.zeros(n_rows, dtype=np.int64)
        q[a] = q[p] = 2 ** 31
        start, _ = ref.start_of(q)
        got = ref.weighted_negative(5, 1, i, int(a), int(p), n_rows, start)
        assert got == (osampler.uniform_negative(5, 1, i, int(a), int(p), n_rows), 0)
    # ... and a third row with a visible share is what the draw returns
    a, p = (int(v) for v in pairs[0])
    third = next(v for v in range(n_rows) if v not in (a, p))
    q = np.zeros(n_rows, dtype=np.int64)
    q[a] = q[p] = 2 ** 30
    q[third] = 2 ** 31
    start, _ = ref.start_of(q)
    assert ref.weighted_negative(5, 1, 0, a, p, n_rows, start) == (third, 1)


def test_train_step_refusals_name_the_argument(nw_mod):
    from cdml_amd import train
    table = types.SimpleNamespace(n_rows_global=1000, data=torch.zeros(1), feature_size=8)
    pairs = torch.zeros((4, 2), dtype=torch.int32)
    w = torch.ones(1000)
    mk = lambda **kw: train.TrainStep(table, pairs, 256, device="cpu", negative_weights=kw.pop("w", w), **kw)
    with pytest.raises(ValueError, match="negative_weights.*negative_lists"):
        mk(mode="uniform", negative_lists=torch.full((1000, 8), -1, dtype=torch.int32))
    with pytest.raises(ValueError, match="negative_weights.*uniform_logq"):
        mk(mode="npair", uniform_negatives=True, logq="stream", uniform_logq=-3.0)
    for name in ("exchange", "grad_sync", "npair_sync"):
        with pytest.raises(ValueError, match="negative_weights.*" + name):
            mk(mode="uniform", **{name: object()})
        with pytest.raises(ValueError, match="negative_weights.*" + name):
            mk(mode="npair", uniform_negatives=True, **{name: object()})
    with pytest.raises(ValueError, match="negative_weights.*train_table"):
        mk(mode="uniform", train_table=True)
    with pytest.raises(ValueError, match="negative_weights.*f16x2"):
        mk(mode="uniform", precision="f16x2")
    for kw in (dict(mode="inbatch"), dict(mode="semihard"), dict(mode="npair")):
        with pytest.raises(ValueError, match="negative_weights.*draws a negative.*%s" % kw["mode"]):
            mk(**kw)
    with pytest.raises(ValueError, match="negative_weights.*one weight per catalogue row"):
        mk(mode="uniform", w=torch.ones(999))
    with pytest.raises(ValueError, match="negative_weights.*one weight per catalogue row"):
        mk(mode="uniform", w=torch.ones((1000, 2)))
    with pytest.raises(ValueError, match="negative_weights.*one weight per catalogue row"):
        mk(mode="uniform", w=nw_mod.NegativeWeights.from_weights(np.ones(999)))
    neg = torch.ones(1000)
    neg[17] = -0.5
    with pytest.raises(ValueError, match="negative_weights must be >= 0.*row 17"):
        mk(mode="uniform", w=neg)
    nan = torch.ones(1000)
    nan[3] = float("nan")
    with pytest.raises(ValueError, match="negative_weights must be finite"):
        mk(mode="uniform", w=nan)
    two = torch.zeros(1000)
    two[5] = two[9] = 1.0
    with pytest.raises(ValueError, match="negative_weights.*at least 3.*got 2"):
        mk(mode="uniform", w=two)
    # the mixed chain's own refusals still come where they apply
    with pytest.raises(ValueError, match="precision"):
        mk(mode="npair", uniform_negatives=True, precision="bf16")


def test_train_config_carries_the_weights():
    from cdml_amd.config import TrainConfig
    c = TrainConfig(mode="inbatch", negative_weights=[1.0, 0.0, 2.5])
    assert TrainConfig.from_json(c.to_json()) == c and TrainConfig().negative_weights is None
    table = types.SimpleNamespace(n_rows_global=3, data=torch.zeros(1), feature_size=8)
    with pytest.raises(ValueError, match="negative_weights.*draws a negative.*inbatch"):      # (the step was handed them)
        c.train_step(table, torch.zeros((4, 2), dtype=torch.int32), device="cpu")


def test_wrapper_refusals(nw_mod):
    from cdml_amd import ops
    nw = nw_mod.NegativeWeights.from_weights(np.ones(100), bits=8)
    t = nw.tables("cpu")
    assert t.n_live == 100 and t.bits == 8 and t.coarse.numel() == 257
    padded = nw_mod.NegativeWeights.from_weights(ref.half_zero_weights(100, 1), bits=8).tables("cpu", pad_to=100)
    assert padded.n_live == 100 and padded.start.numel() == 100 and int(padded.start[-1]) == -1
    with pytest.raises(ValueError, match="pad_to"):
        nw.tables("cpu", pad_to=50)
    with pytest.raises(ValueError, match="coarse table"):
        ops._weighted_args(t._replace(bits=9), 100)
    with pytest.raises(ValueError, match="bits"):
        ops._weighted_args(t._replace(bits=30), 100)
    with pytest.raises(ValueError, match="n_live"):
        ops._weighted_args(t._replace(n_live=101), 100)
    with pytest.raises(ValueError, match="n_live"):
        ops._weighted_args(t, 99)
    e3 = torch.zeros((768, 64))
    with pytest.raises(ValueError, match="neg_bias.*lq_u"):
        ops.npair_mixed_loss(e3, None, 256, 64, ws=types.SimpleNamespace(Bp=256, Dp=64, precision="f32x3", ring=None),
                             logq=torch.zeros(512), lq_u=-2.0, neg_bias=torch.zeros(256))
    with pytest.raises(ValueError, match="neg_bias must be a fp32 tensor"):
        ops.npair_mixed_loss(e3, None, 256, 64, ws=types.SimpleNamespace(Bp=256, Dp=64, precision="f32x3", ring=None),
                             logq=torch.zeros(512), neg_bias=torch.zeros(255))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cdml_negweights.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_table_and_library_agree():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    syms = _header_symbols()
    assert syms == sorted(_lib.SIGNATURES_NEGW) and len(syms) == 8
    for s in syms:
        assert hasattr(lib, s), s
    assert not set(syms) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_HARDNEG) | set(_lib.SIGNATURES_MIXED))


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first

    def ids(pairs=p, start=p, coarse=p, n_live=1000, bits=16, idx=p, n_rows=1000, batch=32):
        return lib.cdml_sample_weighted, (pairs, 64, n_rows, 1, 0, None, batch, 0, batch, start, n_live, coarse, bits, idx,
                                          None, None)

    def fused(name, start=p, coarse=p, n_live=1000, bits=16, n_steps=1, kss=0, kind=None, table=p, x=p, ld=64, xki=False,
              F=64):
        fn = getattr(lib, name)
        a = (p, 64, 1, 0, None, 32, 0, 32, table, 1000, 64, F, start, n_live, coarse, bits, p, kind, x, ld, n_steps,
             32 * 3 * ld, 96, kss, None)
        if name.endswith("_x3"):
            a += (p if xki else None, 0)
        return fn, a + (None,)

    cases = [(ids(start=None), b"tables are null"), (ids(coarse=None), b"tables are null"), (ids(n_live=2), b"n_live = 2"),
             (ids(n_live=1001), b"n_live = 1001"), (ids(bits=7), b"bits = 7"), (ids(bits=25), b"bits = 25"),
             (ids(pairs=None), b"bad argument"), (ids(idx=None), b"bad argument"), (ids(n_rows=2), b"n_rows"),
             (ids(batch=0), b"bad argument")]
    for name, ld in (("cdml_sample_gather_weighted", 64), ("cdml_sample_gather_weighted_x3", 192),
                     ("cdml_sample_gather_weighted_f16", 64)):
        who = name[5:].encode()
        cases += [(fused(name, ld=ld, start=None), who + b": the start / coarse tables are null"),
                  (fused(name, ld=ld, coarse=None), who + b": the start / coarse tables are null"),
                  (fused(name, ld=ld, n_live=2), b"outside [3, n_rows"), (fused(name, ld=ld, n_live=1001), b"outside [3, n_rows"),
                  (fused(name, ld=ld, bits=7), b"outside [8, 24]"), (fused(name, ld=ld, bits=25), b"outside [8, 24]"),
                  (fused(name, ld=ld, n_steps=2, kss=31, kind=p), b"kind_step_stride"),
                  (fused(name, ld=ld, table=None), b"bad argument"), (fused(name, ld=ld, x=None), b"bad argument"),
                  (fused(name, ld=ld, n_steps=65), b"n_steps")]
    for (fn, args), msg in cases:
        rc = fn(*args)
        assert rc == -1, (rc, args)                       # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())
    fn, args = fused("cdml_sample_gather_weighted", ld=64, F=4000)
    assert fn(*args) < 0 and b"feature size" in lib.cdml_last_error()
    fn, args = fused("cdml_sample_gather_weighted_x3", ld=190)
    assert fn(*args) < 0 and b"out_stride" in lib.cdml_last_error()
    fn, args = fused("cdml_sample_gather_weighted_x3", ld=192, xki=True)       # plane 64 is no multiple of 256
    assert fn(*args) < 0 and b"x_ki" in lib.cdml_last_error()
    # mode 3 is reachable only through these entry points
    rc = lib.cdml_sample_gather(3, p, 64, 1, 0, None, 32, 0, 32, p, 1000, 64, 64, p, None, p, 64, 1, 0, 0, None, None)
    assert rc == -1 and b"mode must be 0 or 1" in lib.cdml_last_error()

    # the mixed chain's vector form: neg_bias is required with bias, must be 16-B aligned, and is not looked at without
    S = lse = ws = C.c_void_p(4096)
    st = lambda bias, nb: lib.cdml_npair_mixed_stats_nb(S, 512, None, 256, 256, 0, None, 0, bias, nb, None, 0.1, 1, lse, p, ws,
                                                        0, None)
    assert st(p, None) == -1 and b"npair_mixed_stats_nb" in lib.cdml_last_error() and b"neg_bias" in lib.cdml_last_error()
    assert st(p, C.c_void_p(260)) == -1 and b"neg_bias" in lib.cdml_last_error()
    assert st(None, None) == -1 and b"workspace" in lib.cdml_last_error()      # past the bias checks: the short workspace
    for name, tail in (("cdml_npair_mixed_grad_x3_nb", (p, 3 * 512, 512, None)), ("cdml_npair_mixed_grad_f32_nb", (S, 512, None))):
        fn = getattr(lib, name)
        assert fn(S, 512, None, 256, 256, 0, None, 0, p, None, None, 0.1, 1, lse, *tail) == -1
        assert name[5:].encode() in lib.cdml_last_error() and b"neg_bias" in lib.cdml_last_error()
        assert fn(S, 512, None, 255, 256, 0, None, 0, p, p, None, 0.1, 1, lse, *tail) == -1
        assert b"multiple of 4" in lib.cdml_last_error()
    nbias = lambda lq=p, ids3=p, B=256, off=0.0, out=p, n=1000: lib.cdml_negw_bias(lq, n, ids3, B, off, out, None)
    for kw, msg in ((dict(lq=None), b"null"), (dict(ids3=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"positive"),
                    (dict(n=0), b"positive"), (dict(off=float("inf")), b"finite")):
        assert nbias(**kw) == -1 and b"negw_bias" in lib.cdml_last_error() and msg in lib.cdml_last_error()
