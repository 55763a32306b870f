"""Write footprints of the config-4 N-pair launches (include/cdml_npair_bf16.h) under the poisoned-output / guard-band helpers
of tests/footprint.py: every element the contract says is written is written (two runs under two poison patterns,
bit-identical, no poison left), nothing outside the payload is touched -- leading-dimension padding, rows and columns past
B / D, the in-batch block beside the memory block, the ring's other slots -- and the inputs come back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402

pytestmark = pytest.mark.gpu
f32, bf16, i32 = torch.float32, torch.bfloat16, torch.int32
T = 0.1


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


def _mask(rows, cols, r, c, c0=0):
    m = torch.zeros((rows, cols), dtype=torch.bool)
    m[:r, c0:c0 + c] = True
    return m


def _bits(t):
    return t.contiguous().view(torch.int16)


# B = 200, D = 72: partial last tiles in both directions, several blocks; buffers larger than the payload on every side
@pytest.mark.parametrize("B,D", [(200, 72), (256, 64)])
def test_footprint_operands(cd, B, D):
    rng = np.random.default_rng(B)
    Bbuf, Dq = 256, 128
    e = fp.Guarded((2 * B, D), f32, cd.dev, ld=D + 4)
    e.fill_from(torch.as_tensor(rng.standard_normal((2 * B, D)).astype(np.float32)))
    A = fp.Guarded((Bbuf, Dq), bf16, cd.dev, ld=Dq + 8, mask=_mask(Bbuf, Dq, B, D))
    P = fp.Guarded((Bbuf, Dq), bf16, cd.dev, ld=Dq + 16, mask=_mask(Bbuf, Dq, B, D))
    PT = fp.Guarded((Dq, Bbuf), bf16, cd.dev, ld=Bbuf + 8, mask=_mask(Dq, Bbuf, D, B))

    def run(pattern):
        for g in (A, P, PT):
            g.rearm(pattern)
        with fp.frozen(e.view):
            cd.ops.npair_operands_bf16(e.view, B, D, A.view, P.view, PT.view)
            torch.cuda.synchronize()
        for name, g in (("A", A), ("P", P), ("PT", PT), ("e", e)):
            g.assert_guards_intact(name)
        return {"A": A.payload(), "P": P.payload(), "PT": PT.payload()}
    fp.assert_fully_written(run)
    assert torch.equal(_bits(A.view[:B, :D]), _bits(e.view[0::2].to(bf16)))
    assert torch.equal(_bits(P.view[:B, :D]), _bits(e.view[1::2].to(bf16)))
    assert torch.equal(_bits(PT.view[:D, :B]), _bits(e.view[1::2].to(bf16).T))


def _scores(cd, B, M, pad=8):
    """S [B][B + M] in a guarded buffer, ids with duplicates, a ring's ids with empty slots, lse from the fp32 statistics"""
    rng = np.random.default_rng(B + M)
    D = 32
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.5 * rng.standard_normal((B, D)))
    mem = _unit(rng.standard_normal((max(M, 1), D)))
    ids = rng.choice(50 * B, size=2 * B, replace=False).astype(np.int32)
    ids[2 * 4 + 1] = ids[2 * 11 + 1]
    ids[2 * 9] = ids[2 * 5 + 1]
    q = rng.choice(np.arange(50 * B, 50 * B + 2 * max(M, 4)), size=max(M, 4), replace=False).astype(np.int32)
    q[::5] = -1
    q[3] = ids[2 * 7]
    K = B + M
    S = fp.Guarded((B, K), f32, cd.dev, ld=K + pad)
    full = np.concatenate([A @ P.T, A @ mem[:M].T], 1) if M else A @ P.T
    S.fill_from(torch.as_tensor(full, dtype=f32))
    t = lambda x, dt: torch.as_tensor(x).to(device=cd.dev, dtype=dt)
    rows, mem_id = t(ids, i32), t(q[:M], i32) if M else None
    bias, mem_bias = t(rng.normal(-6, 1, 2 * B), f32), t(rng.normal(-6, 1, max(M, 1)), f32)[:M] if M else None
    return S, rows, mem_id, bias, mem_bias


@pytest.mark.parametrize("logq", [False, True])
@pytest.mark.parametrize("B", [256, 200])
def test_footprint_grad(cd, B, logq):
    """the in-batch W: columns < B of rows < B; B = 200: a scalar tail is not taken (B a multiple of 4), 50 lanes of one block"""
    S, rows, _, bias, _ = _scores(cd, B, 0)
    lse, stats = torch.zeros(2 * B, dtype=f32, device=cd.dev), torch.zeros(4, dtype=f32, device=cd.dev)
    w = torch.zeros(cd.ops.npair_workspace(B) // 4, dtype=f32, device=cd.dev)
    if logq:
        cd.ops.npair_logq_stats(S.view, rows, B, bias, T, True, lse, stats, w)
    else:
        cd.ops.npair_stats(S.view, rows, B, T, True, lse, stats, w)
    Wf = torch.zeros((B, B), dtype=f32, device=cd.dev)
    (cd.ops.npair_logq_grad_f32(S.view, rows, B, bias, T, True, lse, Wf) if logq else
     cd.ops.npair_grad_f32(S.view, rows, B, T, True, lse, Wf))
    Wg = fp.Guarded((B + 8, B + 24), bf16, cd.dev, ld=B + 36, mask=_mask(B + 8, B + 24, B, B))

    def run(pattern):
        Wg.rearm(pattern)
        ins = (S.view, rows, lse) + ((bias,) if logq else ())
        with fp.frozen(*ins):
            cd.ops.npair_grad_bf16(S.view, rows, B, T, True, lse, Wg.view, bias=bias if logq else None)
            torch.cuda.synchronize()
        Wg.assert_guards_intact("W")
        S.assert_guards_intact("S")
        return Wg.payload()
    fp.assert_fully_written(run)
    assert torch.equal(_bits(Wg.view[:B, :B]), _bits(Wf.to(bf16)))
    assert int((Wf == 0).sum()) > 0


@pytest.mark.parametrize("logq", [False, True])
@pytest.mark.parametrize("B,M", [(256, 512), (64, 1100)])
def test_footprint_memory_grad(cd, B, M, logq):
    """the memory block: columns mem_col .. mem_col + M - 1 only -- the in-batch block beside it keeps its poison; M = 1100:
    more than one block of 1024 slots, the last one partial"""
    S, rows, mem_id, bias, mem_bias = _scores(cd, B, M)
    lse, stats = torch.zeros(2 * B, dtype=f32, device=cd.dev), torch.zeros(4, dtype=f32, device=cd.dev)
    w = torch.zeros(cd.ops.npair_memory_workspace(B, M) // 4, dtype=f32, device=cd.dev)
    if logq:
        cd.ops.npair_memory_logq_stats(S.view, rows, B, bias, B, mem_id, mem_bias, T, True, lse, stats, w)
    else:
        cd.ops.npair_memory_stats(S.view, rows, B, B, mem_id, T, True, lse, stats, w)
    K = B + M
    Wf = torch.zeros((B, K), dtype=f32, device=cd.dev)
    (cd.ops.npair_memory_logq_grad_f32(S.view, rows, B, B, mem_id, mem_bias, T, True, lse, Wf) if logq else
     cd.ops.npair_memory_grad_f32(S.view, rows, B, B, mem_id, T, True, lse, Wf))
    Wg = fp.Guarded((B + 8, K + 8), bf16, cd.dev, ld=K + 20, mask=_mask(B + 8, K + 8, B, M, c0=B))

    def run(pattern):
        Wg.rearm(pattern)
        ins = (S.view, rows, lse, mem_id) + ((mem_bias,) if logq else ())
        with fp.frozen(*ins):
            cd.ops.npair_memory_grad_bf16(S.view, rows, B, B, mem_id, T, True, lse, Wg.view, mem_bias=mem_bias if logq else None)
            torch.cuda.synchronize()
        Wg.assert_guards_intact("W")
        S.assert_guards_intact("S")
        return Wg.payload()
    fp.assert_fully_written(run)
    got = Wg.view[:B, B:K]
    assert torch.equal(_bits(got), _bits(Wf[:, B:].to(bf16)))
    assert bool((_bits(got)[:, (mem_id < 0)] == 0).all()) and int((mem_id < 0).sum()) > 0


@pytest.mark.parametrize("B,D,step", [(200, 72, 1), (64, 64, 5)])
def test_footprint_memory_push(cd, B, D, step):
    """slots s .. s + B - 1 of the ring's fp32 rows, ids and both images, columns < D: the other slots keep their poison"""
    M, start, Dq = 3 * B, 1, 128
    s = ((step - start) % (M // B)) * B
    rng = np.random.default_rng(B + step)
    P = fp.Guarded((B, D), f32, cd.dev, ld=2 * (D + 4))                 # (the positives: every other row of e)
    P.fill_from(torch.as_tensor(rng.standard_normal((B, D)).astype(np.float32)))
    rows = torch.as_tensor(rng.choice(10 ** 6, 2 * B, replace=False).astype(np.int32)).to(cd.dev)
    slot = torch.zeros((M, 1), dtype=torch.bool)
    slot[s:s + B] = True
    mem = fp.Guarded((M, Dq), f32, cd.dev, ld=Dq + 4, mask=slot & _mask(M, Dq, M, D))
    ids = fp.Guarded((M,), i32, cd.dev, mask=slot.reshape(1, M))
    R = fp.Guarded((M, Dq), bf16, cd.dev, ld=Dq + 8, mask=slot & _mask(M, Dq, M, D))
    Tt = fp.Guarded((Dq, M + 8), bf16, cd.dev, ld=M + 24, mask=_mask(Dq, M + 8, D, B, c0=s))
    step_dev = torch.tensor([step - 1], dtype=torch.int64, device=cd.dev)

    def run(pattern):
        for g in (mem, ids, R, Tt):
            g.rearm(pattern)
        with fp.frozen(P.view, rows, step_dev):
            cd.ops.npair_memory_push_bf16(P.view, rows, B, D, 1, step_dev, start, mem.view, ids.view, R.view, Tt.view[:, :M])
            torch.cuda.synchronize()
        for name, g in (("mem", mem), ("mem_id", ids), ("R", R), ("T", Tt), ("P", P)):
            g.assert_guards_intact(name)
        return {"mem": mem.payload(), "mem_id": ids.payload(), "R": R.payload(), "T": Tt.payload()}
    fp.assert_fully_written(run)
    img = P.view.to(bf16)
    assert torch.equal(mem.view[s:s + B, :D], P.view) and torch.equal(ids.view[s:s + B], rows[1::2])
    assert torch.equal(_bits(R.view[s:s + B, :D]), _bits(img)) and torch.equal(_bits(Tt.view[:D, s:s + B]), _bits(img.T))
    # a step before `start` pushes nothing at all
    for g in (mem, ids, R, Tt):
        g.rearm(0)
    cd.ops.npair_memory_push_bf16(P.view, rows, B, D, 0, None, start, mem.view, ids.view, R.view, Tt.view[:, :M])
    torch.cuda.synchronize()
    for name, g in (("mem", mem), ("mem_id", ids), ("R", R), ("T", Tt)):
        assert bool((fp.bits_of(g.flat) == fp.poison_scalar(g.dtype, 0)).all()), name
        g.assert_guards_intact(name)
