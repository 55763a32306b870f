"""Write footprint of the fp8 catalogue's six entry points (include/cdml_f8.h) with tests/footprint.py's poisoned, guarded
buffers: the three fused gathers and cdml_gather_rows_f8 write idx_out, kind_out, shift_out and x_out in full under two
poison patterns and nothing beyond them (per-step padding, rows past the batch, row gaps, guard bands); the two quantisers
write their codes -- a strided slice of a larger buffer -- and scales in full and nothing around the slice; the pairs, the
lists, the weight tables, the catalogue and the quantisers' sources come back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f8_ref as ref  # noqa: E402
import footprint as fp  # noqa: E402
import negweights_ref as nwref  # noqa: E402

pytestmark = pytest.mark.gpu
N_ROWS = 1000
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine_bf16, negweights, ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.ebf, ns.negweights, ns.ops, ns.dev = engine_bf16, negweights, ops, gpu
    return ns


def _pairs(seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_ROWS, size=333)
    return np.stack([a, (a + 1 + rng.integers(0, N_ROWS - 1, size=333)) % N_ROWS], 1).astype(np.int32)


@pytest.mark.parametrize("entry", ["uniform", "inbatch", "listed", "weighted"])
@pytest.mark.parametrize("batch,F,n_steps", [(37, 72, 1), (256, 1500, 2)])
def test_footprint_fused(cd, entry, batch, F, n_steps):
    ops, dev = cd.ops, cd.dev
    table = cd.ebf.FeatureTableF8.synthetic(N_ROWS, F, 2, dev)
    pairs = torch.from_numpy(_pairs(batch + F)).to(dev)
    rng = np.random.default_rng(F)
    lists = torch.from_numpy(rng.integers(-1, N_ROWS, size=(N_ROWS, 8)).astype(np.int32)).to(dev)
    tables = cd.negweights.NegativeWeights.from_weights(nwref.half_zero_weights(N_ROWS, 3), bits=8).tables(dev)
    R = batch * (2 if entry == "inbatch" else 3)
    cols = ld = (F + 7) // 8 * 8 + 16                      # (a row is written through out_stride: columns >= F are zeroed)
    rows_per_step = R + 3
    xmask = torch.zeros((n_steps * rows_per_step, cols), dtype=torch.bool)
    imask = torch.zeros((n_steps, R + 5), dtype=torch.bool)
    kmask = torch.zeros((n_steps, batch + 3), dtype=torch.bool)
    for s in range(n_steps):
        xmask[s * rows_per_step:s * rows_per_step + R] = True
        imask[s, :R] = True
        kmask[s, :batch] = True
    gx = fp.Guarded((n_steps * rows_per_step, cols), torch.bfloat16, dev, ld=ld, mask=xmask)
    gi = fp.Guarded((n_steps, R + 5), torch.int32, dev, mask=imask)
    gk = fp.Guarded((n_steps, batch + 3), torch.int32, dev, mask=kmask) if entry in ("listed", "weighted") else None
    gs = fp.Guarded((n_steps,), torch.int32, dev) if entry == "inbatch" else None

    def run(pattern):
        for g in (gx, gi, gk, gs):
            if g is not None:
                g.rearm(pattern)
        x = gx.flat.view(n_steps, rows_per_step, ld)[:, :R, :cols]
        idx = gi.flat[:, :R]
        kind = gk.flat[:, :batch] if gk is not None else None
        one = n_steps == 1
        x, idx, kind = (x[0], idx[0], None if kind is None else kind[0]) if one else (x, idx, kind)
        with fp.frozen(pairs, lists, tables.start, tables.coarse, table.data, table.scale,
                       names=["pairs", "lists", "start", "coarse", "table", "scale"]):
            if entry == "listed":
                ops.sample_gather_listed(pairs, 5, 2, batch, table.data, F, lists, 0.75, idx, x, kind_out=kind, n_steps=n_steps)
            elif entry == "weighted":
                ops.sample_gather_weighted(pairs, 5, 2, batch, table.data, F, tables, idx, x, kind_out=kind, n_steps=n_steps)
            else:
                ops.sample_gather(1 if entry == "inbatch" else 0, pairs, 5, 2, batch, table.data, F, idx, x,
                                  shift_out=None if gs is None else gs.view, n_steps=n_steps)
            torch.cuda.synchronize()
        out = {"x": gx.payload(), "idx": gi.payload()}
        for g, name in ((gx, "x_out"), (gi, "idx_out"), (gk, "kind_out"), (gs, "shift_out")):
            if g is not None:
                g.assert_guards_intact(name)
                out[name] = g.payload()
        return out

    got = fp.assert_fully_written(run)
    assert bool(torch.isfinite(got["x"].float()).all())
    rows = got["x"].view(-1, cols)
    assert rows.shape[0] == n_steps * R and bool((rows[:, F:] == 0).all()) and bool((rows[:, :F] != 0).any())
    ids = got["idx"]
    assert int(ids.min()) >= 0 and int(ids.max()) < N_ROWS
    if gk is not None:
        assert set(got["kind_out"].unique().tolist()) <= {0, 1} and int(got["kind_out"].sum()) > 0
    if gs is not None:
        assert 1 <= int(got["shift_out"].min()) and int(got["shift_out"].max()) < batch


@pytest.mark.parametrize("n_idx,F", [(37, 72), (130, 1500), (5, 4096)])
def test_footprint_gather_rows_f8(cd, n_idx, F):
    ops, dev = cd.ops, cd.dev
    table = cd.ebf.FeatureTableF8.synthetic(N_ROWS, F, 2, dev)
    idx_np = np.random.default_rng(n_idx).integers(0, N_ROWS, size=n_idx).astype(np.int32)
    idx_np[3] = -1                                          # a padding slot: its row is left untouched
    idx = torch.from_numpy(idx_np).to(dev)
    cols = ld = (F + 7) // 8 * 8 + 8                        # (a row is written through out_stride: columns >= F are zeroed)
    mask = torch.ones((n_idx, cols), dtype=torch.bool)
    mask[3] = False
    gx = fp.Guarded((n_idx, cols), torch.bfloat16, dev, ld=ld, mask=mask)

    def run(pattern):
        gx.rearm(pattern)
        with fp.frozen(idx, table.data, table.scale, names=["idx", "table", "scale"]):
            ops.gather_rows_f8(table.data, 0, idx, F, gx.view)
            torch.cuda.synchronize()
        gx.assert_guards_intact("x_out")
        return gx.payload()

    got = fp.assert_fully_written(run)["out"].view(n_idx - 1, cols)
    assert bool(torch.isfinite(got.float()).all()) and bool((got[:, F:] == 0).all()) and bool((got[:, :F] != 0).any())


@pytest.mark.parametrize("src", ["f32", "f16"])
@pytest.mark.parametrize("n,F", [(5, 7), (300, 520), (133, 1500)])
def test_footprint_quantisers(cd, src, n, F):
    """The destination: rows [2, 2 + n) and columns [128, 128 + round_up(F, 128)) of a larger code buffer -- its own stride,
    independent of the source's; the scales: a guarded vector."""
    ops, dev = cd.ops, cd.dev
    x = ref.sample_rows(F, n=max(n, 14))[:n]
    if src == "f16":
        with np.errstate(over="ignore"):
            x = x.astype(np.float16)
    s = torch.zeros((n, (F + 7) // 8 * 8 + 8), dtype=torch.float32 if src == "f32" else torch.float16, device=dev)
    s[:, :F] = torch.from_numpy(x).to(dev)
    W = (F + 127) // 128 * 128
    big_rows, big_cols = n + 4, W + 256
    mask = torch.zeros((big_rows, big_cols), dtype=torch.bool)
    mask[2:2 + n, 128:128 + W] = True
    gc = fp.Guarded((big_rows, big_cols), torch.uint8, dev, ld=big_cols + 64, mask=mask)
    gs = fp.Guarded((n,), torch.float32, dev)

    def run(pattern):
        gc.rearm(pattern), gs.rearm(pattern)
        with fp.frozen(s, names=["src"]):
            ops.quantize_rows_f8(s, F, gc.view[2:2 + n, 128:128 + W].view(F8), gs.view)
            torch.cuda.synchronize()
        gc.assert_guards_intact("codes"), gs.assert_guards_intact("scale")
        return {"codes": gc.payload(), "scale": gs.payload()}

    got = fp.assert_fully_written(run)
    want_codes, want_scale = cd.ebf.quantize_f8_host(x.astype(np.float32))
    codes = got["codes"].view(n, W).cpu().numpy()
    assert np.array_equal(codes[:, :F], want_codes) and not codes[:, F:].any()
    assert np.array_equal(got["scale"].cpu().numpy().view(np.uint32), want_scale.view(np.uint32))
