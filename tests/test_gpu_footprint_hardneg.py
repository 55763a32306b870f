"""Write footprint of the listed sampler's launches (include/cdml_hardneg.h) with tests/footprint.py's poisoned, guarded
buffers: idx_out, kind_out, x_out and x_ki are written in full under two poison patterns -- a row of x_out through its whole
out_stride, columns >= F zeroed, as cdml.h defines for every gather -- nothing beyond them is (the per-step padding of
idx_out and kind_out, rows past the batch, the guard bands), and pairs, lists and the table come back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import hardneg_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
N_ROWS, L, LDL, H = 1000, 8, 12, 0.75


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.engine_bf16, ns.ops, ns.dev = engine, engine_bf16, ops, gpu
    return ns


def _inputs(cd, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_ROWS, size=333)
    pairs = np.stack([a, (a + 1 + rng.integers(0, N_ROWS - 1, size=333)) % N_ROWS], 1).astype(np.int32)
    lists = rng.integers(0, N_ROWS, size=(N_ROWS, LDL)).astype(np.int32)
    lists[rng.random((N_ROWS, LDL)) < 0.3] = -1
    return pairs, lists, torch.from_numpy(pairs).to(cd.dev), torch.from_numpy(lists).to(cd.dev)


def _check(cd, fmt, batch, F, n_steps, extra_rows=0):
    """One listed launch of row format ``fmt`` into guarded buffers, under both poisons; returns the second run's payloads."""
    ops, dev = cd.ops, cd.dev
    pairs_np, lists_np, pairs, lists_full = _inputs(cd, batch + F)
    lists = lists_full[:, :L]
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
            cols, ld, xdt = 3 * plane, 3 * plane, torch.bfloat16       # (a row IS its three planes: no row gap in this form)
    # every step's rows in ONE guarded buffer: [n_steps * (R + extra_rows), ld]; rows past the batch are masked out
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
        with fp.frozen(pairs, lists_full, table.data, names=["pairs", "lists", "table"]):
            ops.sample_gather_listed(pairs, 5, 2, batch, table.data, F, lists, H, idx[0] if one else idx,
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
    want_idx = np.concatenate([ref.listed_triplets(pairs_np, N_ROWS, 5, 2 + s, batch, lists_np, L, H)[0].reshape(-1)
                               for s in range(n_steps)])
    want_kind = np.concatenate([ref.listed_triplets(pairs_np, N_ROWS, 5, 2 + s, batch, lists_np, L, H)[1]
                                for s in range(n_steps)])
    assert np.array_equal(got["idx"].cpu().numpy(), want_idx) and np.array_equal(got["kind"].cpu().numpy(), want_kind)
    assert 0 < want_kind.sum() < want_kind.size
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
    pairs_np, lists_np, pairs, lists_full = _inputs(cd, 1)
    for batch in (37, 256):
        gi = fp.Guarded((3 * batch,), torch.int32, dev)
        gk = fp.Guarded((batch,), torch.int32, dev)

        def run(pattern):
            gi.rearm(pattern), gk.rearm(pattern)
            with fp.frozen(pairs, lists_full, names=["pairs", "lists"]):
                ops.sample_listed(pairs, N_ROWS, 5, 2, batch, lists_full[:, :L], H, gi.view, kind_out=gk.view)
                torch.cuda.synchronize()
            gi.assert_guards_intact("idx_out"), gk.assert_guards_intact("kind_out")
            return {"idx": gi.payload(), "kind": gk.payload()}

        got = fp.assert_fully_written(run)
        want, kind = ref.listed_triplets(pairs_np, N_ROWS, 5, 2, batch, lists_np, L, H)
        assert np.array_equal(got["idx"].cpu().numpy(), want.reshape(-1)) and np.array_equal(got["kind"].cpu().numpy(), kind)
