"""The N-pair loss's sampling-bias (logQ) correction on the MI355X (csrc/npair.hip's BIAS passes, csrc/npair_logq.hip,
ops.LogQTable / ops.LogQEstimator, ops.npair_loss(logq=...), TrainStep(mode="npair", logq=...), losses.NPairLoss(logq=...))
against the fp64 reference and the estimator's host model of tests/npair_logq_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_logq_ref as lref  # noqa: E402
from oracle import synth as osynth, tower as otower  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, losses, ops, train, utils
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.losses, ns.ops, ns.train, ns.utils, ns.dev = engine, losses, ops, train, utils, gpu
    return ns


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(B, M, D, seed, n_videos):
    """A batch with planted duplicate ids (in the batch and in the ring), a ring with empty slots, and a random lq table
    in [-12, 0] over n_videos."""
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.7 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    ids = rng.choice(n_videos // 2, size=2 * B, replace=False).astype(np.int32)
    for k in range(0, B - 8, max(1, B // 16)):
        ids[2 * k + 1] = ids[2 * (k + 3) + 1]
        ids[2 * (k + 5)] = ids[2 * k + 1]
    table = rng.uniform(-12.0, 0.0, n_videos).astype(np.float32)
    mem = mem_id = None
    if M:
        mem = _unit(A[rng.integers(0, B, M)] + 1.5 * rng.standard_normal((M, D)) / np.sqrt(D) * 4)
        mem = mem.astype(np.float32).astype(np.float64)
        mem_id = rng.choice(np.arange(n_videos // 2, n_videos), size=M, replace=False).astype(np.int32)
        mem_id[rng.choice(M, M // 8, replace=False)] = -1
        for k in range(0, M, max(1, M // 32)):
            mem_id[k] = ids[(7 * k) % (2 * B)]
    return A, P, ids, table, mem, mem_id


def _ref_torch(A, P, ids, bias, t, symmetric, dev, mem=None, mem_id=None, mem_bias=None):
    """npair_logq_ref.npair_logq in float64 on the device (B = 8192 with a ring is slow on the host)."""
    A, P = (torch.as_tensor(x, dtype=torch.float64, device=dev) for x in (A, P))
    B = A.shape[0]
    idt = torch.as_tensor(ids, device=dev).view(B, 2).long()
    b = torch.as_tensor(bias, dtype=torch.float64, device=dev).view(B, 2)
    a, p = idt[:, 0], idt[:, 1]
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    S = A @ P.T / t
    X = S - b[:, 1][None, :]
    Xs = X.masked_fill(~m, -float("inf"))
    if mem is not None:
        memt = torch.as_tensor(mem, dtype=torch.float64, device=dev)
        q = torch.as_tensor(mem_id, device=dev).long()
        cm = (q[None, :] >= 0) & (q[None, :] != a[:, None]) & (q[None, :] != p[:, None])
        Xm = A @ memt.T / t - torch.as_tensor(mem_bias, dtype=torch.float64, device=dev)[None, :]
        lr = torch.logsumexp(torch.cat([Xs, Xm.masked_fill(~cm, -float("inf"))], 1), 1)
    else:
        lr = torch.logsumexp(Xs, 1)
    d = torch.diagonal(S)
    loss = (lr - (d - b[:, 1])).mean()
    W = torch.where(m, torch.exp(X - lr[:, None]), torch.zeros_like(S)) - eye.double()
    Wm = torch.where(cm, torch.exp(Xm - lr[:, None]), torch.zeros_like(Xm)) if mem is not None else None
    lc = None
    if symmetric:
        Xc = S - b[:, 0][:, None]
        lc = torch.logsumexp(Xc.masked_fill(~mc, -float("inf")), 0)
        loss = 0.5 * (loss + (lc - (d - b[:, 0])).mean())
        W = 0.5 * (W + torch.where(mc, torch.exp(Xc - lc[None, :]), torch.zeros_like(S)) - eye.double())
        if Wm is not None:
            Wm = 0.5 * Wm
    W = W / (B * t)
    dA = W @ P
    if Wm is not None:
        dA = dA + (Wm / (B * t)) @ memt
    return {"loss": loss.item(), "lse_row": lr, "lse_col": lc, "dA": dA, "dP": W.T @ A}


def _run(cd, A, P, ids, t, symmetric, precision, logq, mem=None, mem_id=None, with_de=True):
    B, D = A.shape
    e = torch.zeros((2 * B, D), dtype=torch.float32, device=cd.dev)
    e[0::2] = torch.as_tensor(A, dtype=torch.float32, device=cd.dev)
    e[1::2] = torch.as_tensor(P, dtype=torch.float32, device=cd.dev)
    rows = torch.as_tensor(ids, dtype=torch.int32, device=cd.dev)
    de = torch.zeros_like(e) if with_de else None
    memory = None
    if mem is not None:
        memory = cd.ops.NPairMemory(mem.shape[0], B, D, precision, cd.dev)
        memory.load(torch.as_tensor(mem, dtype=torch.float32), torch.as_tensor(mem_id))
    ws = cd.ops.NPairWorkspace(B, D, precision, cd.dev, in_batch=memory is None)
    stats, lse = cd.ops.npair_loss(e, rows, B, D, t, symmetric, precision, de=de, ws=ws, memory=memory, logq=logq)
    torch.cuda.synchronize()
    return stats.clone(), lse.clone(), de, ws, memory


@pytest.mark.parametrize("M_per_B", [0, 2])
@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("B,D,t", [(256, 64, 0.05), (1024, 256, 1.0), (8192, 256, 0.05), (8192, 64, 1.0)])
def test_chain_against_fp64(cd, B, D, t, symmetric, precision, M_per_B):
    """1. Random lq in [-12, 0] through a fixed table, planted duplicate ids: loss, both lse vectors, dA and dP against
    fp64 within the uncorrected chain tests' bounds; the bias vectors are the table's entries of the slots' ids."""
    M = M_per_B * B
    n_videos = 8 * B + 2 * M
    A, P, ids, table, mem, mem_id = _case(B, M, D, B + D + M + int(symmetric), n_videos)
    src = cd.ops.LogQTable(torch.as_tensor(table), cd.dev)
    stats, lse, de, ws, memory = _run(cd, A, P, ids, t, symmetric, precision, src, mem, mem_id)
    bias = table[ids].astype(np.float64)
    mem_bias = None
    if M:
        mem_bias = np.where(mem_id >= 0, table[np.maximum(mem_id, 0)], 0.0)
        assert np.array_equal(memory.bias.cpu().numpy(), mem_bias.astype(np.float32))
    assert np.array_equal(ws.bias[:2 * B].cpu().numpy(), table[ids])
    ref = _ref_torch(A, P, ids, bias, t, symmetric, cd.dev, mem, mem_id, mem_bias)
    assert np.isfinite(stats[0].item())
    assert abs(stats[0].item() - ref["loss"]) < TOL, (stats[0].item(), ref["loss"])
    assert (lse[:B].double() - ref["lse_row"]).abs().max().item() < TOL
    if symmetric:
        assert (lse[B:2 * B].double() - ref["lse_col"]).abs().max().item() < TOL
    g = torch.empty((2 * B, D), dtype=torch.float64, device=cd.dev)
    g[0::2], g[1::2] = ref["dA"], ref["dP"]
    rel = ((de.double() - g).norm() / g.norm()).item()
    assert rel < 1e-4, rel
    assert abs(stats[1].item() - np.mean(np.sum((A - P) ** 2, 1))) < 1e-5


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("M_per_B", [0, 2])
def test_constant_table_and_fresh_estimator_match_the_uncorrected_chain(cd, precision, M_per_B):
    """2. A constant table and a fresh estimator (every gap g0) shift every logit alike: the corrected chain sits within
    the chain tests' tolerance of the uncorrected one (and the step-0 estimator is exactly that constant)."""
    B, D, t = 1024, 256, 0.1
    M = M_per_B * B
    n_videos = 16 * B
    A, P, ids, _, mem, mem_id = _case(B, M, D, 99 + M, n_videos)
    s0, l0, de0, _, _ = _run(cd, A, P, ids, t, True, precision, None, mem, mem_id)
    est = cd.ops.LogQEstimator(n_videos, B, 0.01, None, cd.dev)
    assert est.init_gap == 16.0
    for src in (cd.ops.LogQTable(torch.full((n_videos,), -3.5), cd.dev), est):
        s1, l1, de1, _, _ = _run(cd, A, P, ids, t, True, precision, src, mem, mem_id)
        assert abs(s1[0].item() - s0[0].item()) < TOL
        assert torch.equal(s1[1:4], s0[1:4])                      # distances and counts: untouched by the bias
        rel = ((de1 - de0).double().norm() / de0.double().norm()).item()
        assert rel < 1e-5, rel
    # the estimator ran one training step: its positives now have last = 0 and (first sightings) gap g0
    pos = np.unique(ids[1::2])
    assert (est.last[torch.as_tensor(pos, device=cd.dev).long()] == 0).all()
    assert (est.gap == 16.0).all()


_OMIT = object()


def _step(cd, precision, N=600, memory_size=0, use_graph=False, optimizer="adam", **kw):
    """a small catalogue, so that batches repeat ids within and across steps (logq "stream" unless given; _OMIT: the
    argument is not passed at all)"""
    table = cd.engine.FeatureTable.synthetic(N, 128, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 120, 0), dtype=torch.int32).to(cd.dev)
    B = 256 if precision == "f32x3" else 64
    kw.setdefault("logq", "stream")
    if kw["logq"] is _OMIT:
        del kw["logq"]
    return cd.train.TrainStep(table, pairs, B, hidden_size=256, output_size=64, mode="npair", optimizer=optimizer,
                              base_learning_rate=0.01 if optimizer == "adam" else 1.0, device=cd.dev, precision=precision,
                              memory_size=memory_size, use_graph=use_graph, **kw)


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_estimator_state_against_the_host_model(cd, precision):
    """3. After T = 24 training steps whose batches repeat ids within and across steps, last and gap are bit-equal to the
    host model, sampling_logq() is -log(gap), and hipGraph replay leaves the same bits as eager steps."""
    T, N, alpha = 24, 600, 0.3
    runs = []
    for use_graph in (False, True):
        ts = _step(cd, precision, N=N, logq_alpha=alpha, use_graph=use_graph)
        est = ts.npair_logq
        assert isinstance(est, cd.ops.LogQEstimator) and est.init_gap == max(1.0, N / ts.B)
        pos = []
        for _ in range(T):
            ts.step()
            torch.cuda.synchronize()
            pos.append(ts.idx[1::2].cpu().numpy())
        runs.append((est.last.clone(), est.gap.clone(), ts.params.flat.clone(), ts.stats[:4].clone()))
        if not use_graph:
            p = np.concatenate(pos)
            assert len(np.unique(pos[0])) < len(pos[0])                       # duplicates within a batch
            assert len(np.intersect1d(pos[0], pos[1])) > 0                    # and across steps
            last, gap = lref.estimator_after(pos, N, ts.B, alpha)
            assert np.array_equal(est.last.cpu().numpy(), last)
            assert np.array_equal(est.gap.cpu().numpy(), gap)
            assert (gap != np.float32(est.init_gap)).sum() > N // 4 and (last == -1).sum() < N
            assert len(np.unique(p)) > N // 2
        lq = ts.sampling_logq()
        ref = -torch.log(est.gap.double())
        ulp = torch.abs(torch.nextafter(lq, torch.full_like(lq, float("inf"))) - lq).double()
        assert ((lq.double() - ref).abs() <= 2 * ulp).all()
        assert np.isfinite(ts.loss())
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_deterministic_and_resume_is_bit_exact(cd, precision):
    """4. Two runs are bit-identical; save at step 3 and resume to step 7: weights, ring and estimator are bit-exact
    against the uninterrupted run (with a memory)."""
    M = 2 * (256 if precision == "f32x3" else 64)
    straight = [_step(cd, precision, memory_size=M, logq_alpha=0.05) for _ in range(2)]
    for ts in straight:
        for _ in range(7):
            ts.step()
    torch.cuda.synchronize()
    a, b = straight
    assert torch.equal(a.params.flat, b.params.flat) and torch.equal(a.npair_logq.gap, b.npair_logq.gap)
    first = _step(cd, precision, memory_size=M, logq_alpha=0.05)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    state = first.state_dict()
    assert set(state["npair_logq"]) == {"last", "gap", "alpha", "init_gap"} and state["npair_logq"]["alpha"] == 0.05
    resumed = _step(cd, precision, memory_size=M)                    # (alpha comes back from the checkpoint)
    resumed.load_state_dict(state)
    assert resumed.npair_logq.alpha == 0.05
    for _ in range(4):
        resumed.step()
    torch.cuda.synchronize()
    assert torch.equal(a.params.flat, resumed.params.flat)
    assert torch.equal(a.npair_memory.rows, resumed.npair_memory.rows)
    assert torch.equal(a.npair_memory.ids, resumed.npair_memory.ids)
    assert torch.equal(a.npair_logq.last, resumed.npair_logq.last)
    assert torch.equal(a.npair_logq.gap, resumed.npair_logq.gap)
    assert torch.equal(a.stats[:4], resumed.stats[:4])
    # a checkpoint without an estimator loads as a fresh one
    resumed.load_state_dict({k: v for k, v in state.items() if k != "npair_logq"})
    assert (resumed.npair_logq.last == -1).all() and (resumed.npair_logq.gap == resumed.npair_logq.init_gap).all()


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("memory_size", [0, 512])
def test_logq_none_is_the_uncorrected_step(cd, precision, memory_size):
    """5. logq=None is bit-identical to a step built without the argument."""
    runs = []
    for kw in ({"logq": _OMIT}, {"logq": None, "logq_alpha": 0.5}):
        ts = _step(cd, precision, memory_size=memory_size, **kw)
        assert ts.npair_logq is None
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_facade_matches_fp64(cd):
    """6. NPairLoss(logq=...) at an unpadded batch (300 pairs) against fp64 on the loss and pairs.grad."""
    cls = cd.utils.find_class_by_name("NPairLoss", [cd.losses])
    B, D, t = 300, 48, 0.1
    rng = np.random.default_rng(6)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.3 * rng.standard_normal((B, D)))
    ids = rng.choice(4 * B, size=2 * B, replace=False)
    ids[3] = ids[10]
    lq = rng.uniform(-12.0, 0.0, 2 * B)
    for symmetric, with_ids in ((True, True), (False, False)):
        pairs = torch.tensor(np.stack([A, P], 1), dtype=torch.float32, device=cd.dev, requires_grad=True)
        idt = torch.as_tensor(ids.reshape(B, 2), device=cd.dev) if with_ids else None
        out = cls().calculate_loss(pairs, temperature=t, symmetric=symmetric, ids=idt,
                                   logq=torch.as_tensor(lq.reshape(B, 2), dtype=torch.float32, device=cd.dev))
        out["npair_loss"].backward()
        r = lref.npair_logq(A, P, ids if with_ids else None, lq.astype(np.float32), t, symmetric)
        assert abs(out["npair_loss"].item() - r["loss"]) < TOL
        g = np.stack([r["dA"], r["dP"]], 1)
        rel = np.linalg.norm(pairs.grad.double().cpu().numpy() - g) / np.linalg.norm(g)
        assert rel < 1e-4, rel
    with pytest.raises(ValueError, match="logq"):
        cls().calculate_loss(pairs, logq=torch.zeros(B, 3, device=cd.dev))


def _clustered(rng):
    K, per, F = 512, 8, 96
    N = K * per
    cid = np.repeat(np.arange(K), per)
    feats = (rng.standard_normal((K, F))[cid] + 1.2 * rng.standard_normal((N, F))).astype(np.float32)
    return N, cid, feats


def _recall_fn(cd, ts, feats, held):
    from cdml_amd.evaluate import Evaluation
    ev = Evaluation(None, [], device=cd.dev)

    def recall():
        W = [w.detach().cpu().numpy().astype(np.float64) for w in ts.params.unpadded()]
        emb = otower.vnet_forward(feats.astype(np.float64), *W, dtype=np.float64)["l2_norm"].astype(np.float32)
        return ev.retrieval_metrics(emb, held, ks=(10,))["recall@10"]
    return recall


def test_logq_training_raises_recall(cd):
    """7a. test_gpu_npair.test_npair_training_raises_recall's clustered catalogue, trained with logq="stream"."""
    rng = np.random.default_rng(21)
    N, cid, feats = _clustered(rng)
    draw = lambda n: np.array([(a, rng.choice(np.flatnonzero(cid == cid[a]))) for a in rng.integers(0, N, n)])
    train_pairs = draw(20000)
    train_pairs = train_pairs[train_pairs[:, 0] != train_pairs[:, 1]].astype(np.int32)
    held = draw(3000)
    held = held[held[:, 0] != held[:, 1]]
    table = cd.engine.FeatureTable.from_numpy(feats, cd.dev)
    ts = cd.train.TrainStep(table, torch.as_tensor(train_pairs).to(cd.dev), 256, hidden_size=512, output_size=64,
                            mode="npair", optimizer="adam", base_learning_rate=0.003, device=cd.dev, logq="stream")
    recall = _recall_fn(cd, ts, feats, held)
    r0 = recall()
    for _ in range(300):
        ts.step()
    loss, r1 = ts.loss(), recall()
    print("npair + logQ learning: recall@10 %.4f -> %.4f, loss %.4f" % (r0, r1, loss))
    assert np.isfinite(loss)
    assert r1 > 0.9 and r1 > r0 + 0.5, (r0, r1)


def test_zipf_skewed_training_stays_finite_and_learns(cd):
    """7b. Zipf-drawn anchors (exponent 1.1) over the clustered catalogue, logq="stream": finite, and recall@10 of
    held-out pairs rises by at least 0.3."""
    rng = np.random.default_rng(22)
    N, cid, feats = _clustered(rng)
    pop = 1.0 / np.arange(1, N + 1) ** 1.1
    perm = rng.permutation(N)
    prob = np.empty(N)
    prob[perm] = pop / pop.sum()
    draw = lambda n: np.array([(a, rng.choice(np.flatnonzero(cid == cid[a]))) for a in rng.choice(N, n, p=prob)])
    train_pairs = draw(20000)
    train_pairs = train_pairs[train_pairs[:, 0] != train_pairs[:, 1]].astype(np.int32)
    held = np.array([(a, rng.choice(np.flatnonzero(cid == cid[a]))) for a in rng.integers(0, N, 3000)])
    held = held[held[:, 0] != held[:, 1]]
    table = cd.engine.FeatureTable.from_numpy(feats, cd.dev)
    ts = cd.train.TrainStep(table, torch.as_tensor(train_pairs).to(cd.dev), 256, hidden_size=512, output_size=64,
                            mode="npair", optimizer="adam", base_learning_rate=0.003, device=cd.dev, logq="stream")
    recall = _recall_fn(cd, ts, feats, held)
    r0 = recall()
    for _ in range(300):
        ts.step()
    loss, r1 = ts.loss(), recall()
    lq = ts.sampling_logq()
    print("npair + logQ, Zipf anchors: recall@10 %.4f -> %.4f, loss %.4f, lq range [%.3f, %.3f]"
          % (r0, r1, loss, lq.min().item(), lq.max().item()))
    assert np.isfinite(loss) and bool(torch.isfinite(lq).all())
    assert r1 >= r0 + 0.3, (r0, r1)                   # (a recorded run: 0.2191 -> 0.8472)


def test_refusals(cd):
    """8. TrainStep's logq refusals, and ids outside [0, n_videos) in the gather and update launches."""
    N, F = 2000, 64
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0), dtype=torch.int32).to(cd.dev)
    mk = lambda B=256, **kw: cd.train.TrainStep(table, pairs, B, hidden_size=256, output_size=64, device=cd.dev, **kw)
    for mode in ("uniform", "inbatch", "semihard"):
        with pytest.raises(ValueError, match="mode 'npair'"):
            mk(mode=mode, logq="stream")
    with pytest.raises(ValueError, match="one entry per catalogue row"):
        mk(mode="npair", logq=torch.zeros(N - 1))
    bad = torch.zeros(N)
    bad[7] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        mk(mode="npair", logq=bad)
    bad[7] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        mk(mode="npair", logq=bad)
    with pytest.raises(ValueError, match="None, 'stream'"):
        mk(mode="npair", logq="batch")
    for a in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="logq_alpha"):
            mk(mode="npair", logq="stream", logq_alpha=a)
    for g in (0.5, 0.0, float("inf")):
        with pytest.raises(ValueError, match="logq_init_gap"):
            mk(mode="npair", logq="stream", logq_init_gap=g)
    ts = mk(mode="npair", logq=torch.linspace(-5.0, -1.0, N))
    assert isinstance(ts.npair_logq, cd.ops.LogQTable) and "npair_logq" not in ts.state_dict()
    assert torch.equal(ts.sampling_logq().cpu(), torch.linspace(-5.0, -1.0, N))
    with pytest.raises(ValueError, match="no logQ"):
        mk(mode="npair").sampling_logq()
    from cdml_amd.config import TrainConfig
    with pytest.raises(ValueError, match="mode 'npair'"):
        TrainConfig(mode="inbatch", logq="stream", batch_size=256, hidden_size=256, output_size=64).train_step(
            table, pairs, device=cd.dev)
    ts = TrainConfig(mode="npair", logq="stream", logq_alpha=0.2, batch_size=256, hidden_size=256,
                     output_size=64).train_step(table, pairs, device=cd.dev)
    assert isinstance(ts.npair_logq, cd.ops.LogQEstimator) and ts.npair_logq.alpha == 0.2
    e = torch.zeros((512, ts.layout.Dp), dtype=torch.float32, device=cd.dev)
    with pytest.raises(ValueError, match="video ids"):
        cd.ops.npair_loss(e, None, 256, ts.layout.Dp, logq=ts.npair_logq)
    # ids outside [0, n_videos): bias 0, never read, never written (the state past n is a guard band the launches
    # must leave alone)
    n, B, M = 100, 8, 8
    dev = cd.dev
    est = cd.ops.LogQEstimator(n + 16, B, 0.5, 4.0, dev)
    full_last, full_gap = est.last, est.gap
    est.last, est.gap = full_last[:n], full_gap[:n]                   # the launches see n_videos = n
    rows = torch.tensor([3, 5, -1, 100, 7, 105, 2 ** 31 - 1, -7, 5, 5, 9, 115, 0, 99, 1, 2], dtype=torch.int32,
                        device=dev)
    mem_id = torch.tensor([-1, 100, 4, 2 ** 30, 5, -5, 99, 110], dtype=torch.int32, device=dev)
    bias = torch.full((2 * B,), 7.0, device=dev)
    mem_bias = torch.full((M,), 7.0, device=dev)
    est.gather(rows, B, mem_id, bias, mem_bias)
    est.update(rows, B, 3, None)
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    inr = (r >= 0) & (r < n)
    assert (bias.cpu().numpy()[~inr] == 0).all() and np.allclose(bias.cpu().numpy()[inr], -np.log(4.0))
    q = mem_id.cpu().numpy()
    assert (mem_bias.cpu().numpy()[(q < 0) | (q >= n)] == 0).all()
    pos = r[1::2]
    seen = np.unique(pos[(pos >= 0) & (pos < n)])
    last = est.last.cpu().numpy()
    assert (last[seen] == 3).all() and (np.delete(last, seen) == -1).all()
    assert (full_last[n:] == -1).all() and (full_gap[n:] == 4.0).all()
    tab = cd.ops.LogQTable(torch.linspace(-3.0, -1.0, n), dev)
    tab.gather(rows, B, mem_id, bias, mem_bias)
    torch.cuda.synchronize()
    assert (bias.cpu().numpy()[~inr] == 0).all()
    assert np.array_equal(bias.cpu().numpy()[inr], tab.table.cpu().numpy()[r[inr]])
