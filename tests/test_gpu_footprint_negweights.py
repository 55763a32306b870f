"""Write footprint of the weighted negatives' launches (include/cdml_negweights.h) with tests/footprint.py's poisoned, guarded
buffers: the four fused forms and cdml_sample_weighted write idx_out, kind_out, x_out and x_ki in full under two poison
patterns and nothing beyond them (the per-step padding, rows past the batch, the guard bands); cdml_negw_bias writes its B
floats; the three _nb launches of the mixed N-pair chain write lse, stats and the blocks of W, not the gap between them;
pairs, the weight tables, the catalogue and every operand come back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import negweights_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
N_ROWS = 1000


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, negweights, ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.engine_bf16, ns.negweights, ns.ops, ns.dev = engine, engine_bf16, negweights, ops, gpu
    return ns


def _inputs(cd, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_ROWS, size=333)
    pairs = np.stack([a, (a + 1 + rng.integers(0, N_ROWS - 1, size=333)) % N_ROWS], 1).astype(np.int32)
    nw = cd.negweights.NegativeWeights.from_weights(ref.half_zero_weights(N_ROWS, seed), bits=8)
    return pairs, nw, torch.from_numpy(pairs).to(cd.dev), nw.tables(cd.dev)


def _model(pairs_np, nw, seed, step, batch, n_steps):
    start = ref.as_start(nw.start.numpy())
    out = [ref.weighted_triplets(pairs_np, N_ROWS, seed, step + s, batch, start) for s in range(n_steps)]
    return np.concatenate([o[0].reshape(-1) for o in out]), np.concatenate([o[1] for o in out])


def _check(cd, fmt, batch, F, n_steps, extra_rows=0):
    """One weighted launch of row format ``fmt`` into guarded buffers, under both poisons; returns the second run's payloads."""
    ops, dev = cd.ops, cd.dev
    pairs_np, nw, pairs, tables = _inputs(cd, batch + F)
    R = 3 * batch
    if fmt == "f16":
        table = cd.engine_bf16.FeatureTableF16.synthetic(N_ROWS, F, 2, dev)
        cols = ld = (F + 7) // 8 * 8 + 16                      # (a row is written through out_stride: columns >= F are zeroed)
        xdt = torch.bfloat16
    else:
        table = cd.engine.FeatureTable.synthetic(N_ROWS, F, 2, dev)
        if fmt == "f32":
            cols = ld = (F + 3) // 4 * 4 + 8
            xdt = torch.float32
        else:
            plane = (F + 255) // 256 * 256
            cols, ld, xdt = 3 * plane, 3 * plane, torch.bfloat16
    rows_per_step = R + extra_rows
    xmask = torch.zeros((n_steps * rows_per_step, cols), dtype=torch.bool)
    imask = torch.zeros((n_steps, R + 5), dtype=torch.bool)
    kmask = torch.zeros((n_steps, batch + 3), dtype=torch.bool)
    for s in range(n_steps):
        xmask[s * rows_per_step:s * rows_per_step + R] = True
        imask[s, :R] = True
        kmask[s, :batch] = True
    gx = fp.Guarded((n_steps * rows_per_step, cols), xdt, dev, ld=ld, mask=xmask)
    gi = fp.Guarded((n_steps, R + 5), torch.int32, dev, mask=imask)
    gk = fp.Guarded((n_steps, batch + 3), torch.int32, dev, mask=kmask)
    gki = fp.Guarded((n_steps * 3 * R * (cols // 3),), torch.bfloat16, dev) if fmt == "x3k" else None

    def run(pattern):
        for g in (gx, gi, gk, gki):
            if g is not None:
                g.rearm(pattern)
        x = gx.flat.view(n_steps, rows_per_step, ld)[:, :R, :cols]
        idx, kind = gi.flat[:, :R], gk.flat[:, :batch]
        xk = gki.view.view(n_steps, -1) if gki is not None else None
        one = n_steps == 1
        with fp.frozen(pairs, tables.start, tables.coarse, table.data, names=["pairs", "start", "coarse", "table"]):
            ops.sample_gather_weighted(pairs, 5, 2, batch, table.data, F, tables, idx[0] if one else idx,
                                       x[0] if one else x, kind_out=kind[0] if one else kind, n_steps=n_steps,
                                       x_ki=None if xk is None else (xk[0] if one else xk))
            torch.cuda.synchronize()
        for g, name in ((gx, "x_out"), (gi, "idx_out"), (gk, "kind_out"), (gki, "x_ki")):
            if g is not None:
                g.assert_guards_intact(name)
        out = {"x": gx.payload(), "idx": gi.payload(), "kind": gk.payload()}
        if gki is not None:
            out["x_ki"] = gki.payload()
        return out

    got = fp.assert_fully_written(run)
    want_idx, want_kind = _model(pairs_np, nw, 5, 2, batch, n_steps)
    assert np.array_equal(got["idx"].cpu().numpy(), want_idx) and np.array_equal(got["kind"].cpu().numpy(), want_kind)
    assert want_kind.all()
    assert bool(torch.isfinite(got["x"].float()).all())
    if fmt in ("f32", "f16"):                             # cdml.h: columns F .. out_stride - 1 of every row are zeroed
        rows = got["x"].view(-1, cols)
        assert rows.shape[0] == n_steps * R and bool((rows[:, F:] == 0).all()) and bool((rows[:, :F] != 0).any())
    return got


@pytest.mark.parametrize("batch", [37, 256])
@pytest.mark.parametrize("n_steps", [1, 2])
def test_footprint_fp32_rows(cd, batch, n_steps):
    _check(cd, "f32", batch, 72, n_steps, extra_rows=3)


@pytest.mark.parametrize("fmt", ["x3", "x3k", "f16"])
def test_footprint_plane_and_fp16_forms(cd, fmt):
    got = _check(cd, fmt, 256, 256, 2, extra_rows=8)
    if fmt == "x3k":
        assert bool(torch.isfinite(got["x_ki"].float()).all())


def test_footprint_ids_only(cd):
    ops, dev = cd.ops, cd.dev
    pairs_np, nw, pairs, tables = _inputs(cd, 1)
    for batch in (37, 256):
        gi = fp.Guarded((3 * batch,), torch.int32, dev)
        gk = fp.Guarded((batch,), torch.int32, dev)

        def run(pattern):
            gi.rearm(pattern), gk.rearm(pattern)
            with fp.frozen(pairs, tables.start, tables.coarse, names=["pairs", "start", "coarse"]):
                ops.sample_weighted(pairs, N_ROWS, 5, 2, batch, tables, gi.view, kind_out=gk.view)
                torch.cuda.synchronize()
            gi.assert_guards_intact("idx_out"), gk.assert_guards_intact("kind_out")
            return {"idx": gi.payload(), "kind": gk.payload()}

        got = fp.assert_fully_written(run)
        want_idx, want_kind = _model(pairs_np, nw, 5, 2, batch, 1)
        assert np.array_equal(got["idx"].cpu().numpy(), want_idx) and np.array_equal(got["kind"].cpu().numpy(), want_kind)


def test_footprint_negw_bias(cd):
    ops, dev = cd.ops, cd.dev
    _, nw, _, tables = _inputs(cd, 2)
    rng = np.random.default_rng(3)
    for B in (37, 256):
        ids_np = rng.integers(0, N_ROWS, size=3 * B + 7).astype(np.int32)
        ids_np[3 * 5 + 2] = N_ROWS + 1
        ids = torch.from_numpy(ids_np).to(dev)
        g = fp.Guarded((B,), torch.float32, dev)

        def run(pattern):
            g.rearm(pattern)
            with fp.frozen(tables.lq, ids, names=["lq", "ids3"]):
                ops.negw_bias(tables.lq, ids, B, -0.5, g.view)
                torch.cuda.synchronize()
            g.assert_guards_intact("neg_bias")
            return g.payload()

        got = fp.assert_fully_written(run)["out"].cpu().numpy()
        want = nw.lq.numpy()[np.clip(ids_np[2:3 * B:3], 0, N_ROWS - 1)] + np.float32(-0.5)
        want[5] = 0
        assert np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("M", [0, 256])
@pytest.mark.parametrize("symmetric", [True, False])
def test_footprint_mixed_nb_launches(cd, M, symmetric):
    """cdml_npair_mixed_stats_nb, _grad_x3_nb and _grad_f32_nb at B = 256 with gaps between the blocks of S and W: lse
    ([B] or [2B] with the column term), stats[0..3] and W's three blocks are written in full, the gaps and guards are not."""
    ops, dev = cd.ops, cd.dev
    B, gap, t = 256, 8, 0.1
    neg_col = B + gap
    mem_col = neg_col + B + gap
    span = mem_col + M if M else neg_col + B
    rng = np.random.default_rng(M + symmetric)
    S = torch.from_numpy(rng.uniform(-1, 1, (B, span + 4)).astype(np.float32)).to(dev)
    ids_np = rng.choice(50 * B, size=3 * B, replace=False).astype(np.int32)
    ids_np[3 * 9 + 2] = ids_np[3 * 4]                                       # a negative that is another row's anchor
    ids = torch.from_numpy(ids_np).to(dev)
    mem_id = torch.from_numpy(rng.integers(-1, 50 * B, size=M).astype(np.int32)).to(dev) if M else None
    f = lambda n: torch.from_numpy(rng.normal(-8, 1, n).astype(np.float32)).to(dev)
    bias, nb, mem_bias = f(2 * B), f(B), (f(M) if M else None)
    ws = torch.zeros(ops.npair_mixed_workspace(B, M) // 4, dtype=torch.float32, device=dev)
    n_lse = 2 * B if symmetric else B
    g_lse = fp.Guarded((n_lse,), torch.float32, dev)
    g_st = fp.Guarded((4,), torch.float32, dev)
    wmask = torch.zeros((B, span), dtype=torch.bool)
    wmask[:, :B] = True
    wmask[:, neg_col:neg_col + B] = True
    if M:
        wmask[:, mem_col:] = True
    ldw = span + 12
    g_w = fp.Guarded((B, span), torch.float32, dev, ld=ldw, mask=wmask)
    plane = span + 4
    m3 = torch.zeros((B, 3 * plane), dtype=torch.bool)
    for pl in range(3):
        m3[:, pl * plane:pl * plane + span] = wmask
    g_w3 = fp.Guarded((B, 3 * plane), torch.bfloat16, dev, ld=3 * plane + 8, mask=m3)
    inputs = [S, ids, bias, nb] + ([mem_id, mem_bias] if M else [])

    def run(pattern):
        for g in (g_lse, g_st, g_w, g_w3):
            g.rearm(pattern)
        with fp.frozen(*inputs):
            ops.npair_mixed_stats(S, ids, B, neg_col, mem_col, mem_id, bias, nb, mem_bias, t, symmetric, g_lse.view, g_st.view, ws)
            lse = g_lse.view.clone()                                        # (W reads lse: from a plain copy)
            full = torch.zeros(2 * B, dtype=torch.float32, device=dev)
            full[:n_lse] = lse
            ops.npair_mixed_grad_f32(S, ids, B, neg_col, mem_col, mem_id, bias, nb, mem_bias, t, symmetric, full, g_w.view)
            ops.npair_mixed_grad_x3(S, ids, B, neg_col, mem_col, mem_id, bias, nb, mem_bias, t, symmetric, full, g_w3.view, plane)
            torch.cuda.synchronize()
        for g, name in ((g_lse, "lse"), (g_st, "stats"), (g_w, "W fp32"), (g_w3, "W planes")):
            g.assert_guards_intact(name)
        return {"lse": g_lse.payload(), "stats": g_st.payload(), "W": g_w.payload(), "W3": g_w3.payload()}

    got = fp.assert_fully_written(run)
    assert bool(torch.isfinite(got["lse"]).all()) and bool(torch.isfinite(got["stats"]).all())
    W = got["W"].view(B, -1)
    W3 = got["W3"].view(B, 3, -1).float().sum(1)
    assert bool(torch.isfinite(W).all()) and (W - W3).abs().max().item() <= 1e-6 * W.abs().max().item() + 1e-12
    assert W[4, B + 9].item() == 0 and (W[:, B:2 * B] != 0).float().mean().item() > 0.99
