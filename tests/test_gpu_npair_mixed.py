"""Mixed negative sampling of the N-pair loss on the MI355X (csrc/npair_mixed.hip cdml_npair_mixed_*, ops.NPairMixed,
ops.npair_mixed_loss, TrainStep(mode="npair", uniform_negatives=True)) against the fp64 reference of
tests/npair_mixed_ref.py.  The gates are tests/test_gpu_npair_memory.py's: 1e-5 on the loss and every lse, relative L2
< 1e-4 on de over all 3B rows, 1e-5 on stats[1], 1e-6 on stats[3]."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import npair_logq_ref as lref  # noqa: E402
import npair_mixed_ref as xref  # noqa: E402
from oracle import sampler as osampler, synth as osynth, tower as otower  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, ops, train
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.ops, ns.train, ns.dev = engine, ops, train, gpu
    return ns


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(B, M, D, seed):
    """A batch of triplets with planted duplicates -- in-batch ones as test_gpu_npair_memory._case plants them, uniform
    negatives that are another row's anchor / positive, uniform negatives equal to some p_k -- and a ring with empty slots
    and slots of the batch's own videos.  ids3 int32 [3B]; the video ids lie in [0, 60 B)."""
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.7 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    N = _unit(A[rng.integers(0, B, B)] + 1.5 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    ids3 = rng.choice(50 * B, size=3 * B, replace=False).astype(np.int32).reshape(B, 3)
    for k in range(0, B - 8, max(1, B // 16)):
        ids3[k, 1] = ids3[k + 3, 1]                                         # in-batch duplicates
        ids3[k + 5, 0] = ids3[k, 1]
        ids3[k + 1, 2] = ids3[k + 6, 0]                                     # n is another row's anchor
        ids3[k + 2, 2] = ids3[k + 7, 1]                                     # n equals a p_k
        ids3[k + 4, 2] = ids3[k + 2, 2]                                     # the same video drawn twice
    mem = mem_id = None
    if M:
        mem = _unit(A[rng.integers(0, B, M)] + 1.5 * rng.standard_normal((M, D)) / np.sqrt(D) * 4)
        mem = mem.astype(np.float32).astype(np.float64)                     # the fp32 values the chain holds
        mem_id = rng.choice(np.arange(50 * B, 60 * B), size=M, replace=False).astype(np.int32)
        mem_id[rng.choice(M, M // 8, replace=False)] = -1                   # empty slots
        for k in range(0, M, max(1, M // 32)):
            mem_id[k] = ids3.reshape(-1)[(7 * k) % (3 * B)]                 # a slot of a video of the batch
    return A, P, N, ids3.reshape(-1), mem, mem_id


def _ref_torch(A, P, N, ids3, mem, mem_id, t, symmetric, bias, lq_u, mem_bias, dev):
    """npair_mixed_ref.npair_mixed in float64 on the device."""
    A, P, N = (torch.as_tensor(x, dtype=torch.float64, device=dev) for x in (A, P, N))
    B = A.shape[0]
    idt = torch.as_tensor(ids3, device=dev).view(B, 3).long()
    a, p, n = idt[:, 0], idt[:, 1], idt[:, 2]
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    cn = (n[None, :] != a[:, None]) & (n[None, :] != p[:, None])
    b = torch.zeros((B, 2), dtype=torch.float64, device=dev) if bias is None else \
        torch.as_tensor(bias, dtype=torch.float64, device=dev).view(B, 2)
    lq_u = float(lq_u) if bias is not None else 0.0
    ninf = -float("inf")
    S, U = A @ P.T / t, A @ N.T / t
    X, Xu = S - b[None, :, 1], U - lq_u
    cols, M, cm = [X.masked_fill(~m, ninf), Xu.masked_fill(~cn, ninf)], 0, None
    if mem is not None:
        mem = torch.as_tensor(mem, dtype=torch.float64, device=dev)
        M = mem.shape[0]
        q = torch.as_tensor(mem_id, device=dev).long()
        cm = (q[None, :] >= 0) & (q[None, :] != a[:, None]) & (q[None, :] != p[:, None])
        Xm = A @ mem.T / t
        if bias is not None:
            Xm = Xm - torch.as_tensor(mem_bias, dtype=torch.float64, device=dev)[None, :]
        cols.append(Xm.masked_fill(~cm, ninf))
    lr = torch.logsumexp(torch.cat(cols, 1), 1)
    d = torch.diagonal(S)
    loss = (lr - (d - b[:, 1])).mean()
    z = torch.zeros_like(S)
    W = torch.where(m, torch.exp(X - lr[:, None]), z) - eye.double()
    Wn = torch.where(cn, torch.exp(Xu - lr[:, None]), z)
    Wm = torch.where(cm, torch.exp(Xm - lr[:, None]), torch.zeros_like(Xm)) if mem is not None else None
    lc = None
    if symmetric:
        Xc = S - b[:, 0:1]
        lc = torch.logsumexp(Xc.masked_fill(~mc, ninf), 0)
        loss = 0.5 * (loss + (lc - (d - b[:, 0])).mean())
        W = 0.5 * (W + torch.where(mc, torch.exp(Xc - lc[None, :]), z) - eye.double())
        Wn = 0.5 * Wn
        Wm = None if Wm is None else 0.5 * Wm
    W, Wn = W / (B * t), Wn / (B * t)
    dA = W @ P + Wn @ N
    cnt = (m & ~eye).sum() + cn.sum()
    if Wm is not None:
        dA = dA + (Wm / (B * t)) @ mem
        cnt = cnt + cm.sum()
    return {"loss": loss.item(), "lse_row": lr, "lse_col": lc, "dA": dA, "dP": W.T @ A, "dN": Wn.T @ A, "m": m, "mc": mc,
            "cn": cn, "cm": cm, "frac": cnt.item() / (B * (B - 1) + B * B + B * M)}


def _e3(cd, A, P, N):
    B, D = A.shape
    e = torch.zeros((3 * B, D), dtype=torch.float32, device=cd.dev)
    for k, x in enumerate((A, P, N)):
        e[k::3] = torch.as_tensor(x, dtype=torch.float32, device=cd.dev)
    return e


def _logq_source(cd, kind, n_videos, B, seed):
    """(source, lq per video fp64 [n_videos], lq_u): a fixed table, or an estimator holding a state as after many steps."""
    rng = np.random.default_rng(seed)
    if kind == "fixed":
        lq = rng.normal(-8.0, 1.5, n_videos).astype(np.float32)
        src = cd.ops.LogQTable(torch.as_tensor(lq), cd.dev)
        return src, lq.astype(np.float64), cd.ops.uniform_logq(src)
    src = cd.ops.LogQEstimator(n_videos, B, alpha=0.05, device=cd.dev)
    gap = rng.uniform(1.0, 400.0, n_videos).astype(np.float32)
    last = rng.integers(-1, 50, n_videos).astype(np.int32)
    src.load({"last": torch.as_tensor(last), "gap": torch.as_tensor(gap), "alpha": 0.05, "init_gap": src.init_gap})
    return src, -np.log(gap.astype(np.float64)), cd.ops.uniform_logq(src)


def _run(cd, case, t, symmetric, precision, logq=None, lq_u=0.0, with_de=True, step=0):
    A, P, N, ids3, mem, mem_id = case
    B, D = A.shape
    e = _e3(cd, A, P, N)
    rows3 = torch.as_tensor(ids3, dtype=torch.int32, device=cd.dev)
    de = torch.zeros_like(e) if with_de else None
    ws = cd.ops.NPairMixed(B, D, precision, cd.dev, memory_size=0 if mem is None else mem.shape[0])
    if mem is not None:
        ws.ring.load(torch.as_tensor(mem, dtype=torch.float32), torch.as_tensor(mem_id))
    stats, lse = cd.ops.npair_mixed_loss(e, rows3, B, D, t, symmetric, precision, de=de, ws=ws, step=step, logq=logq, lq_u=lq_u)
    torch.cuda.synchronize()
    return e, stats, lse, de, ws


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("logq", ["off", "fixed", "stream"])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("B,M,D,t", [(256, 0, 64, 0.05), (1024, 2048, 256, 1.0), (8192, 16384, 256, 0.1)])
def test_chain_against_fp64(cd, B, M, D, t, symmetric, logq, precision):
    case = _case(B, M, D, seed=B + M + D)
    A, P, N, ids3, mem, mem_id = case
    src, bias, mem_bias, lq_u = None, None, None, 0.0
    if logq != "off":
        src, lq, lq_u = _logq_source(cd, logq, 60 * B, B, seed=B)
        bias = lq[ids3.reshape(B, 3)[:, :2].reshape(-1)]
        mem_bias = None if mem is None else np.where(mem_id >= 0, lq[np.maximum(mem_id, 0)], 0.0)
    _, stats, lse, de, ws = _run(cd, case, t, symmetric, precision, logq=src, lq_u=lq_u)
    ref = _ref_torch(A, P, N, ids3, mem, mem_id, t, symmetric, bias, lq_u, mem_bias, cd.dev)
    err = {"loss": abs(stats[0].item() - ref["loss"]), "lse": (lse[:B].double() - ref["lse_row"]).abs().max().item()}
    g = torch.empty((3 * B, D), dtype=torch.float64, device=cd.dev)
    g[0::3], g[1::3], g[2::3] = ref["dA"], ref["dP"], ref["dN"]
    err["de"] = ((de.double() - g).norm() / g.norm()).item()
    err["stats1"] = abs(stats[1].item() - np.mean(np.sum((A - P) ** 2, 1)))
    err["stats3"] = abs(stats[3].item() - ref["frac"])
    print("mixed chain B %d M %d D %d t %g sym %d logq %s %s: %s" % (B, M, D, t, symmetric, logq, precision, err))
    assert np.isfinite(stats[0].item())
    assert err["loss"] < TOL and err["lse"] < TOL
    if symmetric:
        assert (lse[B:2 * B].double() - ref["lse_col"]).abs().max().item() < TOL
    assert err["de"] < 1e-4, err
    assert de[2::3].abs().max().item() > 0                                 # the uniform negatives get a gradient
    assert err["stats1"] < 1e-5 and err["stats3"] < 1e-6
    # conditions on the inputs: an uncounted entry in every block; W exactly 0 there, and non-zero where a rule counts
    W = ws.W()
    dead = (~ref["m"] & ~ref["mc"]) if symmetric else ~ref["m"]
    blocks = [(W[:, :B], dead), (W[:, B:2 * B], ~ref["cn"])]
    if M:
        blocks.append((W[:, 2 * B:], ~ref["cm"]))
    for Wb, off in blocks:
        assert int(off.sum()) > 0 and (Wb[off] == 0).all()
        assert (Wb[~off] != 0).float().mean().item() > 0.99
    if M:                                                                  # the push: positives only, slots 0 .. B-1 at step 0
        assert torch.equal(ws.ring.rows[:B], torch.as_tensor(P, dtype=torch.float32, device=cd.dev))
        assert torch.equal(ws.ring.ids[:B].cpu(), torch.as_tensor(ids3.reshape(B, 3)[:, 1].copy()))
        assert torch.equal(ws.ring.rows[B:].cpu(), torch.as_tensor(mem[B:], dtype=torch.float32))
    if logq == "stream":                                                   # the estimator was fed by the positives only
        pos = ids3.reshape(B, 3)[:, 1]
        others = np.setdiff1d(ids3.reshape(B, 3)[:, [0, 2]].reshape(-1), pos)
        last = src.last.cpu().numpy()
        assert (last[pos] == 0).all() and (last[others] != 0).any()


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_masked_uniform_column_moves_nothing(cd, precision):
    B, D, t = 256, 256, 0.05
    A, P, N, ids3, _, _ = _case(B, 0, D, seed=11)
    i, k = 10, 40
    ids3 = ids3.copy()
    ids3[3 * k + 2] = ids3[3 * i + 1]                  # n_k is positive i's video: masked in row i
    _, st0, lse0, de0, ws0 = _run(cd, (A, P, N, ids3, None, None), t, False, precision)
    assert de0[2::3].abs().max().item() > 0            # dN is not zero
    s0, l0 = ws0.S[i, B + k].item(), lse0[i].item()
    W0 = ws0.W().clone()
    assert W0[i, B + k].item() == 0
    N2 = N.copy()
    N2[k] = A[i]                                       # the masked column as close to anchor i as a unit row goes
    _, st1, lse1, de1, ws1 = _run(cd, (A, P, N2, ids3, None, None), t, False, precision)
    assert abs(ws1.S[i, B + k].item() - s0) > 0.5      # the masked entry's score changed ...
    assert abs(lse1[i].item() - l0) < 1e-6             # ... and the anchor's lse did not, nor row i of W, nor its gradient
    assert torch.equal(ws1.W()[i], W0[i]) and torch.equal(de1[3 * i], de0[3 * i])
    ids3[3 * k + 2] = 10 ** 8                          # the same column as another video: it counts, and the lse moves
    _, _, lse2, _, _ = _run(cd, (A, P, N2, ids3, None, None), t, False, precision)
    assert lse2[i].item() - l0 > 0.5


def _config0(cd, precision, optimizer, **kw):
    N, F = 10000, 1500
    feats = osynth.features_numpy(N, F, seed=0).astype(np.float32)
    pairs = osynth.cowatch_pairs(N, 3000, 0)
    table = cd.engine.FeatureTable.from_numpy(feats, cd.dev)
    lr = 0.01 if optimizer == "adam" else 1.0
    ts = cd.train.TrainStep(table, torch.as_tensor(pairs, dtype=torch.int32).to(cd.dev), 256, optimizer=optimizer,
                            base_learning_rate=lr, device=cd.dev, precision=precision, **kw)
    return feats, pairs, ts, lr


@pytest.mark.parametrize("precision", ["f32", "f32x3"])
@pytest.mark.parametrize("optimizer", ["adam", "lars"])
def test_train_steps_config0_shape(cd, precision, optimizer):
    """test_gpu_npair.test_train_steps_config0_shape with uniform negatives: sampler (the mode "uniform" one) -> tower ->
    the mixed reference -> tower backward in fp64, from the device's own weights, step by step."""
    feats, pairs, ts, lr = _config0(cd, precision, optimizer, mode="npair", uniform_negatives=True)
    _, _, tu, _ = _config0(cd, precision, optimizer, mode="uniform")
    B, D, N = 256, 256, feats.shape[0]
    f64 = feats.astype(np.float64)
    host = lambda ts_: [x.detach().cpu().numpy().copy() for x in ts_]
    for step in range(3):
        W = host(ts.params.unpadded())
        slots = [host(ts.params._views(ts.m)), host(ts.params._views(ts.v))] if optimizer == "adam" else \
            [host(ts.params._views(ts.acc))]
        ts.step()
        tu.step()
        idx = osampler.device_triplets_vec(pairs, N, 1234, step, B).reshape(-1)
        assert np.array_equal(ts.idx.cpu().numpy(), idx)
        assert torch.equal(ts.idx, tu.idx)                                 # the mode "uniform" sampler's triplets, n ids included
        Wd = [w.astype(np.float64) for w in W]
        fwd = otower.vnet_forward(f64[idx], *Wd, dtype=np.float64)
        E = fwd["l2_norm"]
        ref = xref.npair_mixed(E[0::3], E[1::3], E[2::3], idx, 0.1, True)
        grads = otower.vnet_backward(fwd, Wd[2], xref.interleave3(ref["dA"], ref["dP"], ref["dN"]), np.float64)
        e = ts.ws.e[:, :D].cpu().numpy()
        assert np.abs(e - E).max() < TOL, f"embeddings step {step}"
        assert abs(ts.loss() - ref["loss"]) < TOL, f"loss step {step}"
        G = host(ts.params.unpadded(grads=True))
        for got, k in zip(G, ("dW1", "db1", "dW2", "db2")):
            scale = max(np.abs(grads[k]).max(), 1e-30)
            assert np.abs(got - grads[k]).max() < max(TOL, 5e-2 * scale), f"{k} step {step}"
        L = ts.layout
        sl = ((slice(0, L.F), slice(0, L.H)), (slice(0, L.H),), (slice(0, L.H), slice(0, L.D)), (slice(0, L.D),))
        for i, got in enumerate(host(ts.params.unpadded())):
            if optimizer == "adam":
                w, _, _ = otower.adam_step(W[i], G[i], slots[0][i][sl[i]], slots[1][i][sl[i]], step + 1, lr, dtype=np.float32)
            else:
                w, _ = otower.lars_step(W[i], G[i], slots[0][i][sl[i]], lr, dtype=np.float32)
            assert np.abs(got - w).max() < 1e-6, f"optimizer var {i} step {step}"
    s = ts.summaries()
    assert s["variance"] is None and 0.5 < s["active_triplets"] <= 1.0


def _step(cd, precision, optimizer="adam", use_graph=False, N=4000, F=200, **kw):
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 500, 0), dtype=torch.int32).to(cd.dev)
    B = 256 if precision == "f32x3" else 64
    return cd.train.TrainStep(table, pairs, B, hidden_size=512, output_size=64, mode="npair", optimizer=optimizer,
                              base_learning_rate=0.01 if optimizer == "adam" else 1.0, device=cd.dev, precision=precision,
                              use_graph=use_graph, **kw)


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_deterministic_and_graph_replay_across_a_wrap(cd, precision):
    B = 256 if precision == "f32x3" else 64
    runs = []
    for use_graph in (False, False, True):
        ts = _step(cd, precision, optimizer="adam" if precision == "f32x3" else "momentum", use_graph=use_graph,
                   uniform_negatives=True, memory_size=2 * B, memory_start=1, logq="stream")
        for _ in range(6):                             # steps 1 .. 5 push: the ring of 2 batches wraps twice
            ts.step()
        torch.cuda.synchronize()
        m, q = ts.npair_memory, ts.npair_logq
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone(), m.rows.clone(), m.ids.clone(), ts.npair_mixed.W().clone(),
                     q.last.clone(), q.gap.clone()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    assert (runs[0][3] >= 0).all() and np.isfinite(runs[0][1].cpu().numpy()).all()


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_resume_is_bit_exact(cd, precision):
    M = 2 * (256 if precision == "f32x3" else 64)
    kw = dict(uniform_negatives=True, memory_size=M, logq="stream")
    straight = _step(cd, precision, **kw)
    for _ in range(7):
        straight.step()
    first = _step(cd, precision, **kw)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    state = first.state_dict()
    assert state["npair_memory"]["rows"].shape == (M, first.layout.Dp) and "npair_logq" in state
    resumed = _step(cd, precision, **kw)
    resumed.load_state_dict(state)
    for _ in range(4):
        resumed.step()
    torch.cuda.synchronize()
    assert torch.equal(straight.params.flat, resumed.params.flat)
    assert torch.equal(straight.npair_memory.rows, resumed.npair_memory.rows)
    assert torch.equal(straight.npair_memory.ids, resumed.npair_memory.ids)
    assert torch.equal(straight.npair_logq.gap, resumed.npair_logq.gap)
    assert torch.equal(straight.stats[:4], resumed.stats[:4])


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_false_and_memory_zero_equivalences(cd, precision):
    """uniform_negatives=False is the step built without the argument, bit for bit (with and without a memory + logQ); with
    True, memory_size=0 is the step built without a memory_size."""
    B = 256 if precision == "f32x3" else 64
    for base in ({}, {"memory_size": 2 * B, "logq": "stream"}):
        runs = []
        for kw in (base, dict(base, uniform_negatives=False, uniform_logq=None)):
            ts = _step(cd, precision, **kw)
            assert ts.npair_mixed is None and ts.R == 2 * B
            for _ in range(3):
                ts.step()
            torch.cuda.synchronize()
            runs.append((ts.params.flat.clone(), ts.stats[:4].clone(), ts.idx.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
    runs = []
    for kw in ({"uniform_negatives": True}, {"uniform_negatives": True, "memory_size": 0, "memory_start": 0}):
        ts = _step(cd, precision, **kw)
        assert ts.npair_memory is None and ts.R == 3 * B
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- write footprints: poisoned outputs, guard bands, padded leading dimensions; one case per new entry point ----
def _fp_inputs(cd, B=256, M=512, D=64, pad=8):
    A, P, N, ids3, mem, mem_id = _case(B, M, D, seed=7)
    K = 2 * B + M
    g = torch.Generator().manual_seed(3)
    S = fp.Guarded((B, K), torch.float32, cd.dev, ld=K + pad)
    S.fill_from(torch.as_tensor(np.concatenate([A @ P.T, A @ N.T, A @ mem.T], 1)))
    ids = torch.as_tensor(ids3, dtype=torch.int32, device=cd.dev)
    mid = torch.as_tensor(mem_id, dtype=torch.int32, device=cd.dev)
    bias = torch.randn(2 * B, generator=g).to(cd.dev) - 6
    mb = torch.randn(M, generator=g).to(cd.dev) - 6
    return B, M, D, K, S, ids, mid, bias, mb, (A, P, N)


def _lse_of(cd, B, M, K, S, ids, mid, bias, mb):
    lse = torch.zeros(2 * B, dtype=torch.float32, device=cd.dev)
    st = torch.zeros(4, dtype=torch.float32, device=cd.dev)
    w = torch.zeros(cd.ops.npair_mixed_workspace(B, M) // 4, dtype=torch.float32, device=cd.dev)
    cd.ops.npair_mixed_stats(S.view, ids, B, B, 2 * B, mid, bias, -3.0, mb, 0.1, True, lse, st, w)
    return lse


def test_footprint_stats(cd):
    B, M, D, K, S, ids, mid, bias, mb, _ = _fp_inputs(cd)
    lse, st = fp.Guarded((2 * B,), torch.float32, cd.dev), fp.Guarded((4,), torch.float32, cd.dev)
    n = cd.ops.npair_mixed_workspace(B, M) // 4
    w = fp.Guarded((n,), torch.float32, cd.dev)

    def run(pattern):
        for gbuf in (lse, st, w):
            gbuf.rearm(pattern)
        with fp.frozen(S.view, ids, mid, bias, mb):
            cd.ops.npair_mixed_stats(S.view, ids, B, B, 2 * B, mid, bias, -3.0, mb, 0.1, True, lse.view, st.view, w.view)
            torch.cuda.synchronize()
        for name, gbuf in (("lse", lse), ("stats", st), ("workspace", w), ("S", S)):
            gbuf.assert_guards_intact(name)
        return {"lse": lse.payload(), "stats": st.payload()}
    out = fp.assert_fully_written(run)
    assert torch.isfinite(out["lse"]).all() and torch.isfinite(out["stats"]).all()


@pytest.mark.parametrize("x3", [True, False])
def test_footprint_grad(cd, x3):
    B, M, D, K, S, ids, mid, bias, mb, _ = _fp_inputs(cd)
    lse = _lse_of(cd, B, M, K, S, ids, mid, bias, mb)
    plane = K + 8
    if x3:                                              # three planes, a gap of 8 columns after each: not payload
        mask = torch.zeros((B, 3 * plane), dtype=torch.bool)
        for p in range(3):
            mask[:, p * plane:p * plane + K] = True
        W = fp.Guarded((B, 3 * plane), torch.bfloat16, cd.dev, ld=3 * plane + 8, mask=mask)
    else:
        W = fp.Guarded((B, K), torch.float32, cd.dev, ld=K + 12)

    def run(pattern):
        W.rearm(pattern)
        with fp.frozen(S.view, ids, mid, bias, mb, lse):
            if x3:
                cd.ops.npair_mixed_grad_x3(S.view, ids, B, B, 2 * B, mid, bias, -3.0, mb, 0.1, True, lse, W.view, plane)
            else:
                cd.ops.npair_mixed_grad_f32(S.view, ids, B, B, 2 * B, mid, bias, -3.0, mb, 0.1, True, lse, W.view)
            torch.cuda.synchronize()
        W.assert_guards_intact("W")
        return W.payload()
    out = fp.assert_fully_written(run)["out"]
    assert torch.isfinite(out.float()).all()


def test_footprint_split(cd):
    B, M, D, K, _, _, _, _, _, (A, P, N) = _fp_inputs(cd)
    e = fp.Guarded((3 * B, D), torch.float32, cd.dev, ld=D + 4)
    e.fill_from(_e3(cd, A, P, N))
    pa, pt = D + 8, K + 8

    def planes(rows, width, plane, live_rows, live_cols, ld_pad):
        mask = torch.zeros((rows, 3 * plane), dtype=torch.bool)
        for p in range(3):
            mask[live_rows, p * plane + live_cols.start:p * plane + live_cols.stop] = True
        return fp.Guarded((rows, 3 * plane), torch.bfloat16, cd.dev, ld=3 * plane + ld_pad, mask=mask)
    A3 = planes(B, D, pa, slice(0, B), slice(0, D), 4)
    R3 = planes(K, D, pa, slice(0, 2 * B), slice(0, D), 4)            # the ring's rows 2B .. are the push's, not the split's
    T3 = planes(D, K, pt, slice(0, D), slice(0, 2 * B), 8)

    def run(pattern):
        for gbuf in (A3, R3, T3):
            gbuf.rearm(pattern)
        with fp.frozen(e.view):
            cd.ops.npair_mixed_split_x3(e.view, B, D, A3.view, pa, R3.view, pa, T3.view, pt, B)
            torch.cuda.synchronize()
        for name, gbuf in (("A3", A3), ("R3", R3), ("T3", T3), ("e", e)):
            gbuf.assert_guards_intact(name)
        return {"A3": A3.payload(), "R3": R3.payload(), "T3": T3.payload()}
    fp.assert_fully_written(run)
    # the planes are cdml_split_f32_bf16x3's: hi + mid + lo is the fp32 value, in both images
    ev = e.view
    for img, src in ((A3.view[:, :D], ev[0::3]), (R3.view[:B, :D], ev[1::3]), (R3.view[B:2 * B, :D], ev[2::3])):
        hi = src.to(torch.bfloat16)
        assert torch.equal(img, hi)
    rows = R3.view[:2 * B]
    tot = rows[:, :D].float() + rows[:, pa:pa + D].float() + rows[:, 2 * pa:2 * pa + D].float()
    assert torch.equal(tot, torch.cat([ev[1::3], ev[2::3]]))
    tt = T3.view[:, :2 * B].float() + T3.view[:, pt:pt + 2 * B].float() + T3.view[:, 2 * pt:2 * pt + 2 * B].float()
    assert torch.equal(tt, tot.T)


def test_npair_loss_module_with_negatives(cd):
    from cdml_amd import losses
    B, D = 256, 64
    A, P, N, ids3, _, _ = _case(B, 0, D, seed=5)
    pairs = torch.stack([torch.as_tensor(A), torch.as_tensor(P)], 1).float().to(cd.dev).requires_grad_(True)
    negs = torch.as_tensor(N).float().to(cd.dev).requires_grad_(True)
    idt = torch.as_tensor(ids3.reshape(B, 3))
    out = losses.NPairLoss().calculate_loss(pairs, 0.1, True, ids=idt[:, :2], negatives=negs, negative_ids=idt[:, 2])
    out["npair_loss"].backward()
    ref = xref.npair_mixed(A, P, N, ids3, 0.1, True)
    assert abs(out["npair_loss"].item() - ref["loss"]) < TOL and out["negatives"].shape == (B, 1, D)
    g = np.stack([ref["dA"], ref["dP"]], 1)
    assert np.linalg.norm(pairs.grad.double().cpu().numpy() - g) / np.linalg.norm(g) < 1e-4
    assert np.linalg.norm(negs.grad.double().cpu().numpy() - ref["dN"]) / np.linalg.norm(ref["dN"]) < 1e-4


def test_mixed_training_raises_recall(cd):
    """test_gpu_npair_memory.test_memory_training_raises_recall's catalogue and thresholds with uniform negatives."""
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
    table = cd.engine.FeatureTable.from_numpy(feats, cd.dev)
    ts = cd.train.TrainStep(table, torch.as_tensor(train_pairs).to(cd.dev), 256, hidden_size=512, output_size=64,
                            mode="npair", optimizer="adam", base_learning_rate=0.003, device=cd.dev, memory_size=1024,
                            uniform_negatives=True)
    assert ts.precision == "f32x3"
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
    s = ts.summaries()
    print("npair + memory + uniform negatives: recall@10 %.4f -> %.4f, loss %.4f, counted fraction %.4f"
          % (r0, r1, loss, s["active_triplets"]))
    assert np.isfinite(loss)
    assert r1 > 0.9 and r1 > r0 + 0.5, (r0, r1)
    assert 0.5 < s["active_triplets"] <= 1.0
