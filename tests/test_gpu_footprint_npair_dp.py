"""Write footprints of the data-parallel N-pair launches (include/cdml_npair_dp.h) under the poisoned-output / guard-band
helpers of tests/footprint.py: every element the contract says is written is written (two runs under two poison patterns,
bit-identical, no poison left), nothing outside the payload is touched -- leading-dimension padding, plane gaps, the
workspace's back guard, rows 2i of de -- and the inputs come back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import npair_dp_ref  # noqa: E402

pytestmark = pytest.mark.gpu
f32, bf16, i32 = torch.float32, torch.bfloat16, torch.int32
T = 0.1
# (world, B, rank): the f32x3 shape of the simulated-rank test as rank 0 and as rank 1, the f32 shape (G = 192) as every rank
SHAPES = [(2, 256, 0), (2, 256, 1), (3, 64, 0), (3, 64, 1), (3, 64, 2)]


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.ops, ns.dev = ops, gpu
    return ns


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_DATA = {}


def _data(W, B, D=64):
    """the global batch and its fp64 three-phase model, computed once per shape"""
    if (W, B) not in _DATA:
        G = W * B
        rng = np.random.default_rng(W * 1000 + B)
        A = _unit(rng.standard_normal((G, D)))
        P = _unit(A + 0.5 * rng.standard_normal((G, D)))
        ids = rng.choice(50 * G, size=2 * G, replace=False).astype(np.int32)
        ids[2 * (B + 2) + 1] = ids[2 * 2 + 1]              # a positive on rank 1 that duplicates one on rank 0
        ids[2 * 4 + 1] = ids[2 * 11 + 1]
        for r in range(W):                                 # every rank: an anchor that is a positive of the next rank --
            ids[2 * (r * B + 9)] = ids[2 * (((r + 1) % W) * B + 5) + 1]    # an entry neither rule counts, in its rows
        _DATA[(W, B)] = (A, P, ids, npair_dp_ref.npair_dp(A, P, ids, W, T, True))
    return _DATA[(W, B)]


def _t(x, dev, dtype=f32):
    return torch.as_tensor(np.asarray(x)).to(device=dev, dtype=dtype)


def _S(cd, W, B, rank, pad=8):
    A, P, ids, ref = _data(W, B)
    G = W * B
    S = fp.Guarded((B, G), f32, cd.dev, ld=G + pad)
    S.fill_from(_t(A[rank * B:(rank + 1) * B] @ P.T, cd.dev))
    return S, _t(ids, cd.dev, i32), ref, G


@pytest.mark.parametrize("W,B,rank", SHAPES)
def test_footprint_local_stats(cd, W, B, rank):
    S, ids, ref, G = _S(cd, W, B, rank)
    lse, cp = fp.Guarded((B,), f32, cd.dev), fp.Guarded((G, 2), f32, cd.dev)
    w = fp.Guarded((cd.ops.npair_dp_workspace(B, G) // 4,), f32, cd.dev)      # exactly the queried size, the guard right behind

    def run(pattern):
        for g in (lse, cp, w):
            g.rearm(pattern)
        with fp.frozen(S.view, ids):
            cd.ops.npair_dp_local_stats(S.view, ids, B, G, rank * B, T, True, lse.view, cp.view, w.view)
            torch.cuda.synchronize()
        for name, g in (("lse_row", lse), ("colpart", cp), ("workspace", w), ("S", S)):
            g.assert_guards_intact(name)
        return {"lse_row": lse.payload(), "colpart": cp.payload(), "part": w.payload()[:4 * B]}
    out = fp.assert_fully_written(run)
    assert np.abs(out["lse_row"].double().cpu().numpy() - ref["lse_row"][rank]).max() < 1e-5
    got = out["colpart"].double().cpu().numpy()
    want = ref["colpart"][rank]
    lse_of = lambda c: c[:, 0] + np.log(c[:, 1])
    assert np.isfinite(got).all() and np.abs(lse_of(got) - lse_of(want)).max() < 1e-5
    # the asymmetric loss writes no column partials: colpart keeps its poison
    cp.rearm(0), lse.rearm(0), w.rearm(0)
    cd.ops.npair_dp_local_stats(S.view, ids, B, G, rank * B, T, False, lse.view, cp.view, w.view)
    torch.cuda.synchronize()
    assert bool((fp.bits_of(cp.payload()) == fp.poison_scalar(f32, 0)).all())
    for name, g in (("lse_row", lse), ("colpart", cp), ("workspace", w)):
        g.assert_guards_intact(name)


@pytest.mark.parametrize("W,B,rank", SHAPES)
def test_footprint_col_fold_and_stats(cd, W, B, rank):
    S, ids, ref, G = _S(cd, W, B, rank)
    cpa = _t(np.stack(ref["colpart"]), cd.dev)
    lse_col = fp.Guarded((G,), f32, cd.dev)

    def run_fold(pattern):
        lse_col.rearm(pattern)
        with fp.frozen(cpa):
            cd.ops.npair_dp_col_fold(cpa, lse_col.view)
            torch.cuda.synchronize()
        lse_col.assert_guards_intact("lse_col")
        return lse_col.payload()
    lc = fp.assert_fully_written(run_fold)["out"]
    assert np.abs(lc.double().cpu().numpy() - ref["lse_col"]).max() < 1e-5
    # the stats launch reads the row partials the local pass left in the workspace
    n = cd.ops.npair_dp_workspace(B, G) // 4
    w = fp.Guarded((n,), f32, cd.dev)
    scratch = [torch.zeros(k, dtype=f32, device=cd.dev) for k in (B, 2 * G)]
    cd.ops.npair_dp_local_stats(S.view, ids, B, G, rank * B, T, True, scratch[0], scratch[1].view(G, 2), w.view)
    stats = fp.Guarded((4,), f32, cd.dev)

    def run_stats(pattern):
        stats.rearm(pattern)
        with fp.frozen(S.view, lc, w.view):
            cd.ops.npair_dp_stats(S.view, B, G, rank * B, T, True, lc, stats.view, w.view)
            torch.cuda.synchronize()
        for name, g in (("stats", stats), ("workspace", w), ("S", S)):
            g.assert_guards_intact(name)
        return stats.payload()
    st = fp.assert_fully_written(run_stats)["out"]
    assert np.abs(st.double().cpu().numpy() - ref["stats"][rank]).max() < 1e-5


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("W,B,rank", SHAPES)
def test_footprint_grad(cd, W, B, rank, x3):
    S, ids, ref, G = _S(cd, W, B, rank)
    lr, lc = _t(ref["lse_row"][rank], cd.dev), _t(ref["lse_col"], cd.dev)
    plane = G + 8
    if x3:                                              # three planes, a gap of 8 columns after each: not payload
        mask = torch.zeros((B, 3 * plane), dtype=torch.bool)
        for p in range(3):
            mask[:, p * plane:p * plane + G] = True
        Wg = fp.Guarded((B, 3 * plane), bf16, cd.dev, ld=3 * plane + 8, mask=mask)
    else:
        Wg = fp.Guarded((B, G), f32, cd.dev, ld=G + 12)

    def run(pattern):
        Wg.rearm(pattern)
        with fp.frozen(S.view, ids, lr, lc):
            if x3:
                cd.ops.npair_dp_grad_x3(S.view, ids, B, G, rank * B, T, True, lr, lc, Wg.view, plane)
            else:
                cd.ops.npair_dp_grad_f32(S.view, ids, B, G, rank * B, T, True, lr, lc, Wg.view)
            torch.cuda.synchronize()
        Wg.assert_guards_intact("W")
        S.assert_guards_intact("S")
        return Wg.payload()
    fp.assert_fully_written(run)
    v = Wg.view
    got = sum(v[:, p * plane:p * plane + G].double() for p in range(3)) if x3 else v.double()
    want = _t(ref["W"][rank], cd.dev, torch.float64)
    assert ((got - want).norm() / want.norm()).item() < 1e-4
    assert int((want == 0).sum()) > 0 and bool((got[want == 0] == 0).all()), "entries no rule counts are exactly 0"


@pytest.mark.parametrize("W,B,rank", [(2, 256, 1), (3, 64, 0)])
def test_footprint_pos_fold(cd, W, B, rank):
    D, ldr = 64, 72
    rng = np.random.default_rng(9)
    recv = fp.Guarded((W * B, D), f32, cd.dev, ld=ldr)
    recv.fill_from(torch.as_tensor(rng.standard_normal((W * B, D)).astype(np.float32)))
    odd = torch.zeros((2 * B, D), dtype=torch.bool)
    odd[1::2] = True                                   # the positives' rows are the payload; rows 2i keep the poison
    de = fp.Guarded((2 * B, D), f32, cd.dev, ld=D + 4, mask=odd)
    rv = recv.flat.view(W, B, ldr)[:, :, :D]

    def run(pattern):
        de.rearm(pattern)
        with fp.frozen(recv.view):
            cd.ops.npair_dp_pos_fold(rv, B, D, de.view)
            torch.cuda.synchronize()
        de.assert_guards_intact("de")
        recv.assert_guards_intact("recv")
        return de.payload()
    out = fp.assert_fully_written(run)["out"].cpu().numpy().reshape(B, D)
    r = recv.view.cpu().numpy().reshape(W, B, D)
    want = r[0].copy()
    for s in range(1, W):
        want = (want + r[s]).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
