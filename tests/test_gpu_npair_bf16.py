"""The N-pair loss on the config-4 precision (fp16 catalogue, bf16 MFMA) on the MI355X: csrc/npair_bf16.hip, the one-plane
gradient weights of csrc/npair.hip, ops.npair_loss(precision="bf16") and TrainStep(mode="npair", precision="bf16").

What is exact is tested as an equality (the operand images, W against the rounded fp32 W, the ring).  The chain is held to
two models: the fp64 loss of the ROUNDED rows (only fp32 accumulation separates the device from it: test_gpu_npair.py's own
bars) and the fp64 loss of the rows as given (the project's bf16 gradient gate, 1e-2, and a loss bound from the rounding:
RNE moves a unit row by <= 2^-9 of its norm, so a score by <= 2^-8 + 2^-18, and a log-sum-exp and the diagonal are each
1-Lipschitz in the logits: |loss - ref| <= 2 (2^-8 + 2^-18) / t, + 1e-5 for the fp32 arithmetic)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_logq_ref  # noqa: E402
import npair_memory_ref  # noqa: E402
import npair_ref  # noqa: E402
from oracle import synth as osynth, tower as otower  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
f32, bf16, i32 = torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, ops, train
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.engine_bf16, ns.ops, ns.train, ns.dev = engine, engine_bf16, ops, train, gpu
    return ns


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _batch(B, D, seed):
    """Unit anchor / positive rows (positives near their anchors) and video ids with planted duplicates
    (tests/test_gpu_npair.py's helper)."""
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.7 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    ids = rng.choice(50 * B, size=2 * B, replace=False).astype(np.int32)
    for k in range(0, B - 8, max(1, B // 16)):
        ids[2 * k + 1] = ids[2 * (k + 3) + 1]          # two positives of one video
        ids[2 * (k + 5)] = ids[2 * k + 1]              # an anchor that is another pair's positive
    ids[6] = ids[7]                                    # a pair whose rows are one video
    return A, P, ids


def _rounded(x):
    """the fp32 rows the device holds, rounded to bf16 (nearest even), as float64"""
    return torch.as_tensor(np.asarray(x, np.float32)).to(bf16).double().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ref_torch(A, P, ids, t, symmetric, dev):
    """npair_ref.npair in float64 on the device (B = 8192 on the host is gigabytes of fp64 temporaries)."""
    A, P = (torch.as_tensor(x, dtype=torch.float64, device=dev) for x in (A, P))
    B = A.shape[0]
    idt = torch.as_tensor(ids, device=dev).view(B, 2).long()
    a, p = idt[:, 0], idt[:, 1]
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    S0 = A @ P.T
    S = S0 / t
    lr = torch.logsumexp(S.masked_fill(~m, -float("inf")), 1)
    d = torch.diagonal(S)
    loss = (lr - d).mean()
    lc = None
    if symmetric:
        lc = torch.logsumexp(S.masked_fill(~mc, -float("inf")), 0)
        loss = 0.5 * (loss + (lc - d).mean())
    return {"loss": loss.item(), "lse_row": lr, "lse_col": lc, "m": m, "mc": mc,
            "stat1": (2 - 2 * torch.diagonal(S0)).mean().item()}


# ---- 1. the operand images --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 192, 256])
@pytest.mark.parametrize("B,Bbuf", [(256, 256), (320, 512)])
def test_operand_images_are_exact(cd, B, Bbuf, D):
    rng = np.random.default_rng(B + D)
    lde, Dq = D + 12, 256
    x = rng.standard_normal((2 * Bbuf, lde)).astype(np.float32)
    # ties of the rounding (an odd and an even bf16 neighbour below), a subnormal, signed zeros, large values
    x[0, :8] = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1e-40, -0.0, 0.0, 3e38, -65504.0]
    x[1, :4] = [1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, 2.0 ** -126, 255.5]
    e = torch.as_tensor(x).to(cd.dev)
    A = torch.zeros((Bbuf, Dq), dtype=bf16, device=cd.dev)
    P, PT = torch.zeros_like(A), torch.zeros((Dq, Bbuf), dtype=bf16, device=cd.dev)
    cd.ops.npair_operands_bf16(e[:, :D], B, D, A, P, PT)
    torch.cuda.synchronize()
    wantA, wantP = e[0:2 * B:2, :D].to(bf16), e[1:2 * B:2, :D].to(bf16)
    assert torch.equal(_bits(A[:B, :D]), _bits(wantA)) and torch.equal(_bits(P[:B, :D]), _bits(wantP))
    assert torch.equal(_bits(PT[:D, :B]), _bits(P[:B, :D].T))
    for name, img, r, c in (("A", A, B, D), ("P", P, B, D), ("PT", PT, D, B)):
        pad = _bits(img).clone()
        pad[:r, :c] = 0
        assert not bool(pad.any()), "%s: padding written" % name


# ---- 2. W is the rounded fp32 W -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("logq", [False, True])
@pytest.mark.parametrize("Mx", [0, 1, 2])
@pytest.mark.parametrize("t", [0.05, 1.0])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("B", [256, 1024])
def test_w_is_the_rounded_fp32_w(cd, B, symmetric, t, Mx, logq):
    ops, dev = cd.ops, cd.dev
    M, D = Mx * B, 64
    K = B + M
    A, P, ids = _batch(B, D, seed=B + Mx)
    rng = np.random.default_rng(7 * B + Mx)
    rows = torch.as_tensor(ids, dtype=i32, device=dev)
    S = torch.zeros((B, K), dtype=f32, device=dev)
    S[:, :B] = torch.as_tensor(A @ P.T, dtype=f32)
    bias = torch.as_tensor(rng.normal(-6, 1, 2 * B), dtype=f32, device=dev) if logq else None
    mem_id = mem_bias = None
    if M:
        mem = _unit(A[rng.integers(0, B, M)] + 1.5 * rng.standard_normal((M, D)) / np.sqrt(D) * 4)
        S[:, B:] = torch.as_tensor(A @ mem.T, dtype=f32)
        q = rng.choice(np.arange(50 * B, 60 * B), size=M, replace=False).astype(np.int32)
        q[rng.choice(M, M // 8, replace=False)] = -1                       # empty slots
        for k in range(0, M, max(1, M // 32)):
            q[k] = ids[(7 * k) % (2 * B)]                                  # a slot of an anchor's / positive's video
        mem_id = torch.as_tensor(q, device=dev)
        mem_bias = torch.as_tensor(rng.normal(-6, 1, M), dtype=f32, device=dev) if logq else None
    lse, stats = torch.zeros(2 * B, dtype=f32, device=dev), torch.zeros(4, dtype=f32, device=dev)
    w = torch.zeros(ops.npair_workspace(B) // 4, dtype=f32, device=dev)
    if M and logq:
        ops.npair_memory_logq_stats(S, rows, B, bias, B, mem_id, mem_bias, t, symmetric, lse, stats, w)
    elif M:
        ops.npair_memory_stats(S, rows, B, B, mem_id, t, symmetric, lse, stats, w)
    elif logq:
        ops.npair_logq_stats(S, rows, B, bias, t, symmetric, lse, stats, w)
    else:
        ops.npair_stats(S, rows, B, t, symmetric, lse, stats, w)
    Wf = torch.zeros((B, K), dtype=f32, device=dev)
    Wb = torch.zeros((B, K), dtype=bf16, device=dev)
    if logq:
        ops.npair_logq_grad_f32(S, rows, B, bias, t, symmetric, lse, Wf)
    else:
        ops.npair_grad_f32(S, rows, B, t, symmetric, lse, Wf)
    ops.npair_grad_bf16(S, rows, B, t, symmetric, lse, Wb, bias=bias)
    if M and logq:
        ops.npair_memory_logq_grad_f32(S, rows, B, B, mem_id, mem_bias, t, symmetric, lse, Wf)
    elif M:
        ops.npair_memory_grad_f32(S, rows, B, B, mem_id, t, symmetric, lse, Wf)
    if M:
        ops.npair_memory_grad_bf16(S, rows, B, B, mem_id, t, symmetric, lse, Wb, mem_bias=mem_bias)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Wf).all()) and int((Wf != 0).sum()) > B * B // 2
    assert torch.equal(_bits(Wb), _bits(Wf.to(bf16)))
    if M:
        dead = (mem_id < 0)[None, :].expand(B, M)
        assert int(dead.sum()) > 0 and bool((_bits(Wb[:, B:])[dead] == 0).all())


# ---- 3. / 4. the chain ---------------------------------------------------------------------------------------------------
_RUNS = {}


def _chain(cd, B, D, symmetric, t):
    """one device run per case and its references, shared by the two chain tests"""
    key = (B, D, symmetric, t)
    if key in _RUNS:
        return _RUNS[key]
    A, P, ids = _batch(B, D, seed=B + D)
    e = torch.zeros((2 * B, D), dtype=f32, device=cd.dev)
    e[0::2] = torch.as_tensor(A, dtype=f32, device=cd.dev)
    e[1::2] = torch.as_tensor(P, dtype=f32, device=cd.dev)
    rows = torch.as_tensor(ids, dtype=i32, device=cd.dev)
    de = torch.zeros_like(e)
    ws = cd.ops.NPairWorkspace(B, D, "bf16", cd.dev)
    stats, lse = cd.ops.npair_loss(e, rows, B, D, t, symmetric, "bf16", de=de, ws=ws)
    torch.cuda.synchronize()
    out = {"A": A, "P": P, "ids": ids, "Ah": e[0::2].to(bf16).double(), "Ph": e[1::2].to(bf16).double(),
           "stats": stats.clone(), "lse": lse.clone(), "de": de, "W": ws.W()[:B, :B].clone()}
    if B <= 1024:                                      # (a few MB each; the B = 8192 case is used once)
        _RUNS[key] = out
    return out


CHAIN_CASES = [(B, D, s, t) for B in (256, 1024) for D in (64, 256) for s in (True, False) for t in (0.05, 1.0)]


@pytest.mark.parametrize("B,D,symmetric,t", CHAIN_CASES + [(8192, 256, True, 0.05)])
def test_chain_against_the_rounded_operand_model(cd, B, D, symmetric, t):
    r = _chain(cd, B, D, symmetric, t)
    stats, lse, de, W, ids = r["stats"], r["lse"], r["de"], r["W"], r["ids"]
    if B <= 1024:
        ref = npair_ref.npair(r["Ah"].cpu().numpy(), r["Ph"].cpu().numpy(), ids, t, symmetric)
        tt = lambda x: None if x is None else torch.as_tensor(x, device=cd.dev)
        ref = {"loss": ref["loss"], "lse_row": tt(ref["lse_row"]), "lse_col": tt(ref["lse_col"]), "m": tt(ref["m"]),
               "mc": tt(ref["mc"]), "stat1": ref["stats"][1]}
    else:
        ref = _ref_torch(r["Ah"], r["Ph"], ids, t, symmetric, cd.dev)
    d_loss = abs(stats[0].item() - ref["loss"])
    d_lse = (lse[:B].double() - ref["lse_row"]).abs().max().item()
    d_col = (lse[B:2 * B].double() - ref["lse_col"]).abs().max().item() if symmetric else 0.0
    # the existing chain gate: the products of the device's own W with the rounded rows, in fp64
    g = torch.empty((2 * B, D), dtype=torch.float64, device=cd.dev)
    g[0::2], g[1::2] = W.double() @ r["Ph"], W.double().T @ r["Ah"]
    rel = ((de.double() - g).norm() / g.norm()).item()
    print("bf16 chain B %d D %d sym %d t %g: |loss - ref| %.3g, lse %.3g / %.3g, de rel %.3g"
          % (B, D, symmetric, t, d_loss, d_lse, d_col, rel))
    assert np.isfinite(stats[0].item())
    assert d_loss < TOL and d_lse < TOL and d_col < TOL
    assert rel < 1e-4, rel
    dead = (~ref["m"] & ~ref["mc"]) if symmetric else ~ref["m"]
    assert int(dead.sum()) > 0
    assert (W[dead] == 0).all()
    assert (W[~dead] != 0).float().mean().item() > 0.99
    # stats [1] the positives' mean squared distance 2 - 2 S_ii (of the rounded rows, which S is the product of), [3] the
    # counted fraction of the row term's off-diagonal entries
    m = ref["m"]
    assert abs(stats[1].item() - ref["stat1"]) < 1e-5
    assert abs(stats[3].item() - (int(m.sum()) - B) / (B * (B - 1))) < 1e-6


@pytest.mark.parametrize("t", [0.05, 0.1, 1.0])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("B", [256, 1024])
def test_end_to_end_against_fp64_of_the_fp32_rows(cd, B, D, symmetric, t):
    r = _chain(cd, B, D, symmetric, t)
    # (the rows as the device holds them: fp32)
    A32, P32 = (np.asarray(x, np.float32).astype(np.float64) for x in (r["A"], r["P"]))
    ref = npair_ref.npair(A32, P32, r["ids"], t, symmetric)
    g = torch.as_tensor(npair_ref.interleave(ref["dA"], ref["dP"]), device=cd.dev)
    rel = ((r["de"].double() - g).norm() / g.norm()).item()
    d_loss = abs(r["stats"][0].item() - ref["loss"])
    bound = 2 * (2.0 ** -8 + 2.0 ** -18) / t + 1e-5
    print("bf16 end to end B %d D %d sym %d t %g: de rel %.3g (bar 1e-2), |loss - ref| %.3g (bound %.3g)"
          % (B, D, symmetric, t, rel, d_loss, bound))
    assert rel < 1e-2, rel
    assert d_loss <= bound, (d_loss, bound)


# ---- 5. memory and logQ ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("with_logq", [False, True])
def test_memory_and_logq_steps(cd, with_logq, symmetric):
    ops, dev = cd.ops, cd.dev
    B, M, D, t, start, steps = 256, 512, 64, 0.1, 1, 4
    rng = np.random.default_rng(3)
    table = rng.normal(-6, 1, 60 * B)
    logq = ops.LogQTable(torch.as_tensor(table, dtype=f32), dev) if with_logq else None
    tab32 = np.asarray(table, np.float32).astype(np.float64)
    ws = ops.NPairWorkspace(B, D, "bf16", dev, in_batch=False)
    mem = ops.NPairMemory(M, B, D, "bf16", dev, start=start)
    wf = ops.NPairWorkspace(B, D, "f32", dev, in_batch=False)        # the f32 chain beside it: the same pushes
    mf = ops.NPairMemory(M, B, D, "f32", dev, start=start)
    pos, pid = [], []
    for step in range(steps):
        A, P, ids = _batch(B, D, seed=100 + step)
        if step == 2:
            ids[2 * 9 + 1] = pid[1][4]                 # a positive whose video sits in the ring: its slot is masked
        e = torch.zeros((2 * B, D), dtype=f32, device=dev)
        e[0::2], e[1::2] = torch.as_tensor(A, dtype=f32), torch.as_tensor(P, dtype=f32)
        rows = torch.as_tensor(ids, dtype=i32, device=dev)
        ring, ring_id = npair_memory_ref.ring_after(step, start, M, pos, pid) if step else (np.zeros((M, D)), np.full(M, -1))
        de = torch.zeros_like(e)
        stats, lse = ops.npair_loss(e, rows, B, D, t, symmetric, "bf16", de=de, ws=ws, memory=mem, step=step, logq=logq)
        ops.npair_loss(e, rows, B, D, t, symmetric, "f32", de=torch.zeros_like(e), ws=wf, memory=mf, step=step, logq=logq)
        torch.cuda.synchronize()
        Ah, Ph, Rh = _rounded(A), _rounded(P), _rounded(ring)
        if with_logq:
            mb = np.where(ring_id >= 0, tab32[np.maximum(ring_id, 0)], 0.0)
            ref = npair_logq_ref.npair_logq(Ah, Ph, ids, tab32[ids], t, symmetric, mem=Rh, mem_id=ring_id, mem_bias=mb)
        else:
            ref = npair_memory_ref.npair_memory(Ah, Ph, ids, Rh, ring_id, t, symmetric)
        d_loss = abs(stats[0].item() - ref["loss"])
        d_lse = np.abs(lse[:B].double().cpu().numpy() - ref["lse_row"]).max()
        d_col = np.abs(lse[B:2 * B].double().cpu().numpy() - ref["lse_col"]).max() if symmetric else 0.0
        W = mem.W().double().cpu().numpy()
        g = npair_ref.interleave(W[:, :B] @ Ph + W[:, B:] @ Rh, W[:, :B].T @ Ah)
        rel = np.linalg.norm(de.double().cpu().numpy() - g) / np.linalg.norm(g)
        print("bf16 memory%s step %d: |loss - ref| %.3g, lse %.3g / %.3g, de rel %.3g"
              % (" + logQ" if with_logq else "", step, d_loss, d_lse, d_col, rel))
        assert d_loss < TOL and d_lse < TOL and d_col < TOL and rel < 1e-4
        cm = npair_memory_ref.mem_mask(ids, ring_id, B)
        assert (W[:, B:][~cm] == 0).all()
        if cm.any():
            assert (W[:, B:][cm] != 0).mean() > 0.99
        assert abs(stats[1].item() - ref["stats"][1]) < 1e-5 and abs(stats[3].item() - ref["stats"][3]) < 1e-6
        pos.append(np.asarray(P, np.float32).astype(np.float64))
        pid.append(ids[1::2].copy())
        # the ring after this step's push: the host model, the f32 chain's ring bit for bit, and the images
        want_rows, want_ids = npair_memory_ref.ring_after(step + 1, start, M, pos, pid)
        assert np.array_equal(mem.ids.cpu().numpy(), want_ids) and np.array_equal(mem.rows.double().cpu().numpy(), want_rows)
        assert torch.equal(mem.rows, mf.rows) and torch.equal(mem.ids, mf.ids)
        img = mem.rows.to(bf16)
        assert torch.equal(_bits(mem.PM16[B:, :D]), _bits(img)) and torch.equal(_bits(mem.PMT16[:D, B:]), _bits(img.T))
        assert not bool(_bits(mem.PM16[:, D:]).any()) and not bool(_bits(mem.PMT16[D:]).any())
    assert int((mem.ids >= 0).sum()) == M               # (steps 1 .. 3 pushed: the ring of two batches wrapped)


# ---- 6. TrainStep -----------------------------------------------------------------------------------------------------------
def _step(cd, use_graph=False, precision="bf16", **kw):
    N, F = 2000, 64
    table = cd.engine_bf16.FeatureTableF16.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0), dtype=i32).to(cd.dev)
    return cd.train.TrainStep(table, pairs, 256, hidden_size=256, output_size=64, mode="npair", optimizer="adam",
                              base_learning_rate=0.01, device=cd.dev, precision=precision, use_graph=use_graph, **kw)


def test_train_step_loss_is_the_op_level_loss_and_runs_repeat(cd):
    runs = []
    for _ in range(2):
        ts = _step(cd)
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone()))
    assert ts.precision == "bf16" and ts.npair_memory is None
    assert np.isfinite(ts.loss())
    Dp = ts.layout.Dp
    stats, _ = cd.ops.npair_loss(ts.ws.e, ts.idx, 256, Dp, ts.temperature, ts.symmetric, "bf16",
                                 ws=cd.ops.NPairWorkspace(256, Dp, "bf16", cd.dev))
    torch.cuda.synchronize()
    assert stats[0].item() == ts.loss()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    assert _step(cd, precision="auto").precision == "bf16"


def test_train_step_graph_replay_is_eager(cd):
    runs = []
    for use_graph in (False, True):
        ts = _step(cd, use_graph=use_graph, memory_size=512, logq="stream")
        for _ in range(4):                                 # the ring of two batches wraps; the estimator moves every step
            ts.step()
        torch.cuda.synchronize()
        m, q = ts.npair_memory, ts.npair_logq
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone(), m.rows.clone(), m.ids.clone(), m.W().clone(),
                     _bits(m.PM16).clone(), _bits(m.PMT16).clone(), q.last.clone(), q.gap.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert (runs[0][3] >= 0).all() and np.isfinite(runs[0][1].cpu().numpy()).all()
    assert int((runs[0][7] >= 0).sum()) > 0


def test_train_step_resume_is_bit_exact(cd):
    kw = dict(memory_size=512, logq="stream")
    straight = _step(cd, **kw)
    for _ in range(6):
        straight.step()
    first = _step(cd, **kw)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    state = first.state_dict()
    assert state["npair_memory"]["rows"].dtype == f32 and state["npair_memory"]["rows"].shape == (512, first.layout.Dp)
    resumed = _step(cd, **kw)
    resumed.load_state_dict(state)
    m = resumed.npair_memory
    assert torch.equal(_bits(m.PM16[256:]), _bits(first.npair_memory.PM16[256:]))      # the images re-derived on load
    assert torch.equal(_bits(m.PMT16[:, 256:]), _bits(first.npair_memory.PMT16[:, 256:]))
    for _ in range(3):
        resumed.step()
    torch.cuda.synchronize()
    assert torch.equal(straight.params.flat, resumed.params.flat)
    assert torch.equal(straight.npair_memory.rows, resumed.npair_memory.rows)
    assert torch.equal(straight.npair_memory.ids, resumed.npair_memory.ids)
    assert torch.equal(straight.stats[:4], resumed.stats[:4])
    assert torch.equal(straight.npair_logq.gap, resumed.npair_logq.gap)


def test_train_step_refusals(cd):
    with pytest.raises(ValueError, match="uniform_negatives"):
        _step(cd, uniform_negatives=True)
    with pytest.raises(ValueError, match="npair_sync"):
        _step(cd, npair_sync=type("Sync", (), {"world": 1, "rank": 0})())
    with pytest.raises(ValueError, match="train_table"):
        _step(cd, train_table=True)
    with pytest.raises(ValueError, match="FeatureTableF16"):            # an fp32 table does not take "bf16" ...
        table = cd.engine.FeatureTable.synthetic(2000, 64, 0, cd.dev)
        pairs = torch.as_tensor(osynth.cowatch_pairs(2000, 300, 0), dtype=i32).to(cd.dev)
        cd.train.TrainStep(table, pairs, 256, hidden_size=256, output_size=64, mode="npair", device=cd.dev, precision="bf16")
    with pytest.raises(ValueError, match="FeatureTableF16"):            # ... nor an fp16 one the fp32 precisions
        _step(cd, precision="f32x3")
    with pytest.raises(ValueError, match="multiple of 256"):
        N = 2000
        table = cd.engine_bf16.FeatureTableF16.synthetic(N, 64, 0, cd.dev)
        pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0), dtype=i32).to(cd.dev)
        cd.train.TrainStep(table, pairs, 320, hidden_size=256, output_size=64, mode="npair", device=cd.dev)


# ---- 7. training works --------------------------------------------------------------------------------------------------------
def test_npair_bf16_training_raises_recall(cd):
    """tests/test_gpu_npair.py's test_npair_training_raises_recall on an fp16 copy of its catalogue: a few hundred N-pair
    steps on within-cluster co-watch pairs raise recall@10 of held-out within-cluster pairs."""
    from cdml_amd.evaluate import Evaluation
    rng = np.random.default_rng(21)
    K, per, F = 512, 8, 96
    N = K * per
    cid = np.repeat(np.arange(K), per)
    feats = (rng.standard_normal((K, F))[cid] + 1.2 * rng.standard_normal((N, F))).astype(np.float32)
    draw = lambda n: np.array([(a, rng.choice(np.flatnonzero(cid == cid[a]))) for a in rng.integers(0, N, n)])
    train_pairs = draw(20000)
    train_pairs = train_pairs[train_pairs[:, 0] != train_pairs[:, 1]].astype(np.int32)
    held = draw(3000)
    held = held[held[:, 0] != held[:, 1]]
    feats = feats.astype(np.float16).astype(np.float32)        # the catalogue as the fp16 table holds it
    table = cd.engine_bf16.FeatureTableF16.from_numpy(feats, cd.dev)
    ts = cd.train.TrainStep(table, torch.as_tensor(train_pairs).to(cd.dev), 256, hidden_size=512, output_size=64,
                            mode="npair", optimizer="adam", base_learning_rate=0.003, device=cd.dev)
    assert ts.precision == "bf16"                      # "auto" on an fp16 catalogue
    ev = Evaluation(None, [], device=cd.dev)

    def recall():
        W = [w.detach().cpu().numpy().astype(np.float64) for w in ts.params.unpadded()]
        emb = otower.vnet_forward(feats.astype(np.float64), *W, dtype=np.float64)["l2_norm"].astype(np.float32)
        return ev.retrieval_metrics(emb, held, ks=(10,))["recall@10"]

    r0 = recall()
    for _ in range(300):
        ts.step()
    loss = ts.loss()
    r1 = recall()
    print("npair bf16 learning: recall@10 %.4f -> %.4f, loss %.4f" % (r0, r1, loss))
    assert np.isfinite(loss)
    assert r1 > 0.9 and r1 > r0 + 0.5, (r0, r1)
