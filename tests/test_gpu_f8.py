"""The fp8 catalogue on the MI355X (include/cdml_f8.h): the HIP quantiser against the host quantiser bit for bit; the fp8
gathers (unfused, fused in the four sampler modes) against the fp16 gathers of the SAME values bit for bit -- every e4m3
value is an fp16 value, and the fp8 row policy runs the fp16 one's instructions after an exact conversion -- and against
fp64 on the codes at the fp16 gather's own tolerance; TrainStep and Prediction on a FeatureTableF8 against the same on
its as_f16() from the same seeds; from_table / synthetic / from_numpy against one another."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f8_ref as ref  # noqa: E402
import negweights_ref as nwref  # noqa: E402
from oracle import synth as osynth, tower as otower  # noqa: E402

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, negweights, ops, predict, train
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.ebf, ns.negweights, ns.ops, ns.predict, ns.train, ns.dev = engine, engine_bf16, negweights, ops, predict, train, gpu
    return ns


def _bits(t):
    return t.view(torch.int16)


def _up(v, m):
    return (v + m - 1) // m * m


# ---- the quantiser ----
@pytest.mark.parametrize("F", [7, 520, 1500])
@pytest.mark.parametrize("src", ["f32", "f16"])
def test_device_quantiser_is_the_host_quantiser(cd, F, src):
    """Codes (NaN codes as codes) and scales bit for bit, the destination's pad columns 0, from a poisoned destination; the
    source's own pad (7.0) is never read into a row."""
    x = ref.sample_rows(F)
    if src == "f16":
        with np.errstate(over="ignore"):
            x = x.astype(np.float16)
    want_codes, want_scale = cd.ebf.quantize_f8_host(x.astype(np.float32))
    assert np.array_equal(want_codes, ref.quantize(x.astype(np.float32))[0])
    n = x.shape[0]
    s = torch.full((n, _up(F, 8) + 8), 7.0, dtype=torch.float32 if src == "f32" else torch.float16, device=cd.dev)
    s[:, :F] = torch.from_numpy(x).to(cd.dev)
    codes = torch.full((n, _up(F, 128)), 0xA5, dtype=torch.uint8, device=cd.dev)
    scale = torch.full((n,), float("nan"), dtype=torch.float32, device=cd.dev)
    cd.ops.quantize_rows_f8(s, F, codes.view(F8), scale)
    got = codes.cpu().numpy()
    assert np.array_equal(scale.cpu().numpy().view(np.uint32), want_scale.view(np.uint32))
    bad = np.argwhere(got[:, :F] != want_codes)
    assert bad.size == 0, (bad[:5], got[:, :F][tuple(bad[0])], want_codes[tuple(bad[0])], x[tuple(bad[0])])
    assert not got[:, F:].any()


# ---- the unfused gather ----
def _random_table(cd, N, F, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, F)).astype(np.float32) ** 3
    x[1] = 0                                              # a zero row stays zero
    x[2] = x[2] * np.float32(1e-9)                        # a tiny row is a row like any other: the scale cancels
    return cd.ebf.FeatureTableF8.from_numpy(x, cd.dev)


@pytest.mark.parametrize("F", [8, 512, 520, 1500, 1536, 1544, 4096])
def test_gather_rows_f8_is_the_fp16_gather_of_the_same_values(cd, F):
    N = 500
    t8 = _random_table(cd, N, F, F)
    t16 = t8.as_f16()
    assert t8.data.shape[1] == _up(F, 128) and t8.data.dtype == F8 and int(t8.data.view(torch.uint8)[:, F:].sum()) == 0
    codes = t8.codes().cpu().numpy()
    assert np.array_equal(t16.data[:, :F].double().cpu().numpy(), ref.decode(codes))          # as_f16 is exact
    idx_np = np.random.RandomState(0).randint(0, N, size=130).astype(np.int32)
    idx_np[:3] = (1, 2, 1)
    idx = torch.as_tensor(idx_np).to(cd.dev)
    ld = _up(F, 8) + 16
    x8 = torch.full((130, ld), 7.0, dtype=torch.bfloat16, device=cd.dev)
    x16 = torch.full((130, ld), 7.0, dtype=torch.bfloat16, device=cd.dev)
    cd.ops.gather_rows_f8(t8.data, 0, idx, F, x8)
    cd.ops.gather_rows_f16(t16.data, 0, idx, F, x16)
    assert torch.equal(_bits(x8), _bits(x16))
    assert float(x8[:, F:].float().abs().max()) == 0 and float(x8[0].float().abs().max()) == 0
    want = otower.l2_normalize(ref.decode(codes)[idx_np], np.float64)[0]
    np.testing.assert_allclose(x8[:, :F].float().cpu().numpy(), want, rtol=2 ** -8, atol=1e-6)
    assert abs(float(x8[1, :F].float().norm()) - 1) < 1e-2


def test_every_code_gathers_as_its_fp16_value(cd):
    """Row r carries code r at several columns (the first and last lane of a chunk, both sides of a chunk edge, the ragged
    end) among random codes: all 256 codes, subnormals and -0 included, pass through the conversion.  The two rows with NaN
    codes carry NaN in both outputs, at exactly the columns of the NaN codes: the fp16 gather's fmaxf(ss, 1e-12f) drops a NaN
    sum of squares, so the other columns of such a row are the codes times 1e6 -- in both gathers, bit for bit."""
    F, cols = 1500, [0, 7, 8, 511, 512, 777, 1496, 1499]
    rng = np.random.default_rng(5)
    c = rng.integers(0, 256, size=(256, F)).astype(np.uint8)
    c[(c & 0x7F) == 0x7F] = 0x3A
    c[np.arange(256)[:, None], np.array(cols)[None, :]] = np.arange(256, dtype=np.uint8)[:, None]
    data = torch.zeros((256, 1536), dtype=torch.uint8, device=cd.dev)
    data[:, :F] = torch.from_numpy(c).to(cd.dev)
    t8 = cd.ebf.FeatureTableF8(data.view(F8), F)
    t16 = t8.as_f16()
    idx = torch.arange(256, dtype=torch.int32, device=cd.dev)
    x8 = torch.full((256, 1536), 7.0, dtype=torch.bfloat16, device=cd.dev)
    x16 = torch.full((256, 1536), 7.0, dtype=torch.bfloat16, device=cd.dev)
    cd.ops.gather_rows_f8(t8.data, 0, idx, F, x8)
    cd.ops.gather_rows_f16(t16.data, 0, idx, F, x16)
    nan = torch.zeros(256, dtype=torch.bool, device=cd.dev)
    nan[[0x7F, 0xFF]] = True
    assert torch.equal(_bits(x8[~nan]), _bits(x16[~nan]))
    assert bool(torch.isfinite(x8[~nan].float()).all())
    want_nan = torch.zeros((2, 1536), dtype=torch.bool, device=cd.dev)
    want_nan[:, cols] = True
    n8, n16 = torch.isnan(x8[nan].float()), torch.isnan(x16[nan].float())
    assert torch.equal(n8, want_nan) and torch.equal(n16, want_nan)
    assert torch.equal(_bits(x8[nan])[~want_nan], _bits(x16[nan])[~want_nan])
    want = otower.l2_normalize(ref.decode(c)[~nan.cpu().numpy()], np.float64)[0]
    np.testing.assert_allclose(x8[~nan][:, :F].float().cpu().numpy(), want, rtol=2 ** -8, atol=1e-6)


# ---- the fused sampler + gather ----
@pytest.fixture(scope="module")
def tables(cd):
    t8 = cd.ebf.FeatureTableF8.synthetic(3000, 1500, 0, cd.dev)
    return t8, t8.as_f16()


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_f8_equals_separate_and_the_fp16_entry(cd, tables, mode):
    """N = 3000, F = 1500, B = 133, three steps per launch: ids, shifts and rows == the sampler kernel + gather_rows_f8, and
    == cdml_sample_gather_f16 on as_f16(), bit for bit."""
    N, F, B, K = 3000, 1500, 133, 3
    t8, t16 = tables
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0)).to(cd.dev)
    R = B * (3 if mode == 0 else 2)
    out = []
    for t in (t8, t16):
        x = torch.full((K, R, 1536), 7.0, dtype=torch.bfloat16, device=cd.dev)
        idx = torch.full((K, R), -1, dtype=torch.int32, device=cd.dev)
        shift = torch.full((K,), -1, dtype=torch.int32, device=cd.dev)
        cd.ops.sample_gather(mode, pairs, 1234, 5, B, t.data, F, idx, x, shift_out=shift, n_steps=K)
        out.append((x, idx, shift))
    (x, idx, shift), (x16, idx16, shift16) = out
    assert torch.equal(idx, idx16) and torch.equal(_bits(x), _bits(x16))
    assert mode == 0 or torch.equal(shift, shift16)
    for s in range(K):
        i1 = torch.full((R,), -1, dtype=torch.int32, device=cd.dev)
        s1 = torch.full((1,), -1, dtype=torch.int32, device=cd.dev)
        if mode == 0:
            cd.ops.sample_uniform(pairs, N, 1234, 5 + s, B, i1)
        else:
            cd.ops.sample_inbatch(pairs, 1234, 5 + s, B, i1, s1)
            assert int(s1.item()) == int(shift[s].item())
        x1 = torch.full((R, 1536), 7.0, dtype=torch.bfloat16, device=cd.dev)
        cd.ops.gather_rows_f8(t8.data, 0, i1, F, x1)
        assert torch.equal(i1, idx[s]) and torch.equal(_bits(x1), _bits(x[s]))
    assert float(x[:, :, 1500:].float().abs().max()) == 0 and float(x.float().abs().sum()) > 0


@pytest.mark.parametrize("mode", [2, 3])
def test_fused_f8_listed_and_weighted_equal_the_fp16_entries(cd, mode):
    """Sampler modes 2 and 3 at the sizes of tests/test_gpu_hardneg.py / test_gpu_negweights.py (1000 rows, 256 triplets, two
    steps per launch; their planted lists, their zipf weights): ids, kind_out and rows == the _f16 entry on as_f16()."""
    from test_gpu_hardneg import _planted
    N, F, batch, n_steps, L = 1000, 1500, 256, 2, 8
    t8 = cd.ebf.FeatureTableF8.synthetic(N, F, 5, cd.dev)
    pairs_np, lists_np = _planted(N, L, L + 4, 400, seed=10)
    pairs = torch.from_numpy(pairs_np).to(cd.dev)
    lists = torch.from_numpy(lists_np).to(cd.dev)[:, :L]
    nw = cd.negweights.NegativeWeights.from_weights(nwref.zipf_weights(N, 13)).tables(cd.dev)
    out = []
    for t in (t8, t8.as_f16()):
        x = torch.full((n_steps, 3 * batch, 1512), 7.0, dtype=torch.bfloat16, device=cd.dev)
        idx = torch.full((n_steps, 3 * batch), -9, dtype=torch.int32, device=cd.dev)
        kind = torch.full((n_steps, batch), -9, dtype=torch.int32, device=cd.dev)
        if mode == 2:
            cd.ops.sample_gather_listed(pairs, 31, 4, batch, t.data, F, lists, 1.0, idx, x, kind_out=kind, n_steps=n_steps)
        else:
            cd.ops.sample_gather_weighted(pairs, 31, 4, batch, t.data, F, nw, idx, x, kind_out=kind, n_steps=n_steps)
        out.append((x, idx, kind))
    (x, idx, kind), (x16, idx16, kind16) = out
    assert torch.equal(idx, idx16) and torch.equal(kind, kind16) and torch.equal(_bits(x), _bits(x16))
    assert 0 < int(kind.sum()) and int(idx.min()) >= 0 and int(kind.min()) >= 0
    for s in range(n_steps):
        want = torch.zeros_like(x[s])
        cd.ops.gather_rows_f8(t8.data, 0, idx[s], F, want)
        assert torch.equal(_bits(want), _bits(x[s]))


# ---- the training step ----
N_T, F_T = 8000, 1500


@pytest.fixture(scope="module")
def train_tables(cd):
    feats = osynth.features_numpy(N_T, F_T, seed=0).astype(np.float32)
    t8 = cd.ebf.FeatureTableF8.from_numpy(feats, cd.dev)
    return t8, t8.as_f16(), torch.as_tensor(osynth.cowatch_pairs(N_T, 2500, 0)).to(cd.dev)


def _run(cd, table, pairs, B, steps=3, **kw):
    ts = cd.train.TrainStep(table, pairs, B, hidden_size=640, output_size=128, device=cd.dev, base_learning_rate=0.01, **kw)
    losses, ids = [], []
    for _ in range(steps):
        ts.step()
        losses.append(ts.loss())
        ids.append(ts.idx.clone())
    torch.cuda.synchronize()
    return ts, losses, ids, [t.clone() for t in ts.params.unpadded()]


def _same(a, b):
    (_, la, ia, wa), (_, lb, ib, wb) = a, b
    assert la == lb and all(np.isfinite(la)), (la, lb)
    assert all(torch.equal(x, y) for x, y in zip(ia, ib))
    assert all(torch.equal(x, y) for x, y in zip(wa, wb))


CASES = {
    "uniform": dict(B=128, mode="uniform"),
    "inbatch": dict(B=128, mode="inbatch"),
    "semihard": dict(B=128, mode="semihard"),
    "npair": dict(B=256, mode="npair", memory_size=256, logq="stream"),
    "weighted": dict(B=128, mode="uniform", negative_weights=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_train_step_on_fp8_is_the_step_on_its_fp16_values(cd, train_tables, case):
    """precision "auto" on the fp8 table == the fp16 table of the same values from the same seeds, three steps: every loss,
    every idx and the four weight tensors torch.equal."""
    t8, t16, pairs = train_tables
    kw = dict(CASES[case])
    if kw.pop("negative_weights", None):
        kw["negative_weights"] = torch.from_numpy(nwref.zipf_weights(N_T, 1))
    a = _run(cd, t8, pairs, precision="auto", **kw)
    assert a[0].precision == "bf16" and a[0].table is t8
    assert a[0].gather_ahead == _run(cd, t16, pairs, steps=0, **kw)[0].gather_ahead
    _same(a, _run(cd, t16, pairs, **kw))
    assert len(set(a[1])) == 3                            # (it trains: three different losses)


def test_train_step_graph_replay_on_fp8(cd, train_tables):
    t8, _, pairs = train_tables
    _same(_run(cd, t8, pairs, 128, steps=4, mode="uniform", use_graph=True), _run(cd, t8, pairs, 128, steps=4, mode="uniform"))


def test_train_step_refuses_what_an_fp8_table_does_not_do(cd, train_tables):
    t8, _, pairs = train_tables
    with pytest.raises(ValueError, match="an fp8 catalogue is read-only"):
        cd.train.TrainStep(t8, pairs, 128, device=cd.dev, train_table=True)
    with pytest.raises(ValueError, match="precision 'bf16' goes with an fp16 FeatureTableF16"):
        cd.train.TrainStep(t8, pairs, 128, device=cd.dev, precision="f32x3")


# ---- inference ----
def test_prediction_embeds_an_fp8_table(cd):
    N, F = 1000, 1500
    t8 = cd.ebf.FeatureTableF8.synthetic(N, F, 2, cd.dev)
    params = cd.engine.VNetParams(cd.ebf.layout_bf16(F, 640, 128), cd.dev)
    pred = cd.predict.Prediction(params=params, precision="bf16")
    got = pred.embed_table(t8, 384).clone()
    want = pred.embed_table(t8.as_f16(), 384)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert float((got.norm(dim=1) - 1).abs().max()) < 1e-3
    assert np.array_equal(pred.run_features(t8, 512), got.cpu().numpy())
    with pytest.raises(ValueError, match="reads an fp16 FeatureTableF16"):
        pred.embed_table(cd.engine.FeatureTable.synthetic(64, F, 2, cd.dev), 64)


# ---- the three constructors ----
def test_from_table_from_numpy_and_synthetic_agree(cd):
    x = ref.sample_rows(520)
    x[10] = 1                                             # (finite data: an fp32 FeatureTable holds it as it is)
    a = cd.ebf.FeatureTableF8.from_numpy(x, cd.dev)
    b = cd.ebf.FeatureTableF8.from_table(cd.engine.FeatureTable.from_numpy(x, cd.dev), chunk_rows=128)
    assert torch.equal(a.data.view(torch.uint8), b.data.view(torch.uint8)) and torch.equal(a.scale, b.scale)
    assert a.data.shape == (300, 640) and a.feature_size == 520 and a.n_rows_global == 300
    deq = a.dequantize(torch.tensor([0, 5, 299], device=cd.dev)).double().cpu().numpy()
    codes, scale = ref.quantize(x)
    assert np.array_equal(deq, (ref.decode(codes) * scale.astype(np.float64)[:, None])[[0, 5, 299]])
    assert np.all(np.linalg.norm(a.dequantize().double().cpu().numpy() - x, axis=1) <= ref.error_bound(x, scale))
    # synthetic: fp16 chunks through the quantiser, two chunk edges crossed; the fp16 table never exists whole
    N, F = 70000, 136
    s = cd.ebf.FeatureTableF8.synthetic(N, F, 7, cd.dev)
    t = cd.ebf.FeatureTableF8.from_table(cd.ebf.FeatureTableF16.synthetic(N, F, 7, cd.dev))
    assert torch.equal(s.data.view(torch.uint8), t.data.view(torch.uint8)) and torch.equal(s.scale, t.scale)
    # U[0,1) rounded to fp16: a row's maximum lies in [0.5, 1], so its scale is 2^-8, or 2^-7 where an element rounded to 1
    assert set(s.scale.unique().tolist()) <= {2.0 ** -8, 2.0 ** -7} and int((s.codes() & 0x7F).max(1).values.min()) >= 0x70
    sharded = cd.ebf.FeatureTableF8.synthetic(1000, F, 7, cd.dev, row0=65000, n_rows_global=N)
    assert torch.equal(sharded.data.view(torch.uint8), s.data.view(torch.uint8)[65000:66000]) and sharded.row0 == 65000
