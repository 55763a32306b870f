"""The N-pair loss's cross-batch memory on the MI355X (csrc/npair.hip cdml_npair_memory_*, ops.NPairMemory,
ops.npair_loss(memory=...), TrainStep(mode="npair", memory_size=...)) against the fp64 reference of
tests/npair_memory_ref.py and a host model of the ring."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_memory_ref as mref  # noqa: E402
from oracle import synth as osynth, tower as otower  # noqa: E402

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
    """A batch with planted in-batch duplicates and a ring with empty slots and slots of the batch's own videos."""
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.7 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    ids = rng.choice(50 * B, size=2 * B, replace=False).astype(np.int32)
    for k in range(0, B - 8, max(1, B // 16)):
        ids[2 * k + 1] = ids[2 * (k + 3) + 1]
        ids[2 * (k + 5)] = ids[2 * k + 1]
    mem = _unit(A[rng.integers(0, B, M)] + 1.5 * rng.standard_normal((M, D)) / np.sqrt(D) * 4)   # hard-ish negatives
    mem_id = rng.choice(np.arange(50 * B, 60 * B), size=M, replace=False).astype(np.int32)
    mem_id[rng.choice(M, M // 8, replace=False)] = -1                       # empty slots
    for k in range(0, M, max(1, M // 32)):
        mem_id[k] = ids[(7 * k) % (2 * B)]                                  # a slot of an anchor's / positive's video
    return A, P, ids, mem, mem_id


def _ref_torch(A, P, ids, mem, mem_id, t, symmetric, dev):
    """npair_memory_ref.npair_memory in float64 on the device."""
    A, P, mem = (torch.as_tensor(x, dtype=torch.float64, device=dev) for x in (A, P, mem))
    B = A.shape[0]
    idt = torch.as_tensor(ids, device=dev).view(B, 2).long()
    q = torch.as_tensor(mem_id, device=dev).long()
    a, p = idt[:, 0], idt[:, 1]
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    cm = (q[None, :] >= 0) & (q[None, :] != a[:, None]) & (q[None, :] != p[:, None])
    S, Sm = A @ P.T / t, A @ mem.T / t
    lr = torch.logsumexp(torch.cat([S.masked_fill(~m, -float("inf")), Sm.masked_fill(~cm, -float("inf"))], 1), 1)
    d = torch.diagonal(S)
    loss = (lr - d).mean()
    W = torch.where(m, torch.exp(S - lr[:, None]), torch.zeros_like(S)) - eye.double()
    Wm = torch.where(cm, torch.exp(Sm - lr[:, None]), torch.zeros_like(Sm))
    lc = None
    if symmetric:
        lc = torch.logsumexp(S.masked_fill(~mc, -float("inf")), 0)
        loss = 0.5 * (loss + (lc - d).mean())
        W = 0.5 * (W + torch.where(mc, torch.exp(S - lc[None, :]), torch.zeros_like(S)) - eye.double())
        Wm = 0.5 * Wm
    W, Wm = W / (B * t), Wm / (B * t)
    n = (m & ~eye).sum() + cm.sum()
    return {"loss": loss.item(), "lse_row": lr, "lse_col": lc, "dA": W @ P + Wm @ mem, "dP": W.T @ A, "m": m, "mc": mc,
            "cm": cm, "frac": n.item() / (B * (B - 1) + B * mem.shape[0])}


def _run(cd, A, P, ids, mem, mem_id, t, symmetric, precision, with_de=True, step=0):
    B, D = A.shape
    e = torch.zeros((2 * B, D), dtype=torch.float32, device=cd.dev)
    e[0::2] = torch.as_tensor(A, dtype=torch.float32, device=cd.dev)
    e[1::2] = torch.as_tensor(P, dtype=torch.float32, device=cd.dev)
    rows = torch.as_tensor(ids, dtype=torch.int32, device=cd.dev)
    de = torch.zeros_like(e) if with_de else None
    ws = cd.ops.NPairWorkspace(B, D, precision, cd.dev, in_batch=False)
    memory = cd.ops.NPairMemory(mem.shape[0], B, D, precision, cd.dev)
    memory.load(torch.as_tensor(mem, dtype=torch.float32), torch.as_tensor(mem_id))
    stats, lse = cd.ops.npair_loss(e, rows, B, D, t, symmetric, precision, de=de, ws=ws, memory=memory, step=step)
    torch.cuda.synchronize()
    return e, stats, lse, de, memory


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("B,M,D,t", [(256, 256, 64, 0.05), (1024, 2048, 256, 1.0), (8192, 32768, 256, 0.1)])
def test_chain_against_fp64(cd, B, M, D, t, symmetric, precision):
    A, P, ids, mem, mem_id = _case(B, M, D, seed=B + M + D)
    # (the ring's rows as the fp32 values the chain holds)
    mem = mem.astype(np.float32).astype(np.float64)
    _, stats, lse, de, memory = _run(cd, A, P, ids, mem, mem_id, t, symmetric, precision)
    ref = _ref_torch(A, P, ids, mem, mem_id, t, symmetric, cd.dev)
    assert np.isfinite(stats[0].item())
    assert abs(stats[0].item() - ref["loss"]) < TOL
    assert (lse[:B].double() - ref["lse_row"]).abs().max().item() < TOL
    if symmetric:
        assert (lse[B:2 * B].double() - ref["lse_col"]).abs().max().item() < TOL
    g = torch.empty((2 * B, D), dtype=torch.float64, device=cd.dev)
    g[0::2], g[1::2] = ref["dA"], ref["dP"]
    rel = ((de.double() - g).norm() / g.norm()).item()
    assert rel < 1e-4, rel
    Wm = memory.W()[:, B:]
    cm = ref["cm"]
    assert int((~cm).sum()) > 0 and (Wm[~cm] == 0).all()                  # empty / same-video slots: exactly zero
    assert (Wm[cm] != 0).float().mean().item() > 0.99
    assert abs(stats[1].item() - np.mean(np.sum((A - P) ** 2, 1))) < 1e-5
    assert abs(stats[3].item() - ref["frac"]) < 1e-6
    # after the products: the push took the batch's positives into slots 0 .. B-1 (step 0), rows and ids
    assert torch.equal(memory.rows[:B], torch.as_tensor(P, dtype=torch.float32, device=cd.dev))
    assert torch.equal(memory.ids[:B].cpu(), torch.as_tensor(ids[1::2]))
    assert torch.equal(memory.rows[B:].cpu(), torch.as_tensor(mem[B:], dtype=torch.float32))


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_duplicate_slot_does_not_move_the_lse(cd, precision):
    B, M, D, t = 256, 512, 256, 0.05
    A, P, ids, mem, mem_id = _case(B, M, D, seed=11)
    i, k = 10, 40
    mem_id[k] = ids[2 * i + 1]                         # slot k holds positive i's video: masked in row i
    _, _, lse0, _, m0 = _run(cd, A, P, ids, mem, mem_id, t, False, precision, with_de=False)
    s0, l0 = m0.S[i, B + k].item(), lse0[i].item()
    mem2 = mem.copy()
    mem2[k] = A[i]                                    # the slot as close to anchor i as a unit row goes
    _, _, lse1, _, m1 = _run(cd, A, P, ids, mem2, mem_id, t, False, precision, with_de=False)
    assert abs(m1.S[i, B + k].item() - s0) > 0.5      # the masked slot's score changed ...
    assert abs(lse1[i].item() - l0) < 1e-6            # ... and the anchor's lse did not
    mem_id[k] = 10 ** 8                               # the same slot as another video: it counts, and the lse moves
    _, _, lse2, _, _ = _run(cd, A, P, ids, mem2, mem_id, t, False, precision, with_de=False)
    assert lse2[i].item() - l0 > 0.5


def _step(cd, precision, memory_size=0, memory_start=0, optimizer="adam", use_graph=False, N=4000, F=200):
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 500, 0), dtype=torch.int32).to(cd.dev)
    B = 256 if precision == "f32x3" else 64
    kw = dict(memory_size=memory_size, memory_start=memory_start) if memory_size or memory_start else {}
    return cd.train.TrainStep(table, pairs, B, hidden_size=512, output_size=64, mode="npair", optimizer=optimizer,
                              base_learning_rate=0.01 if optimizer == "adam" else 1.0, device=cd.dev, precision=precision,
                              use_graph=use_graph, **kw)


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_memory_size_zero_is_the_in_batch_step(cd, precision):
    runs = []
    for kw in ({}, {"memory_size": 0, "memory_start": 0}):
        ts = _step(cd, precision, **kw)
        assert ts.npair_memory is None
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def _planes(x):
    """bf16 planes of fp32 x as cdml_split_f32_bf16x3 writes them (host model: round to nearest even, three times)."""
    h = x.to(torch.bfloat16)
    r = x - h.float()
    m = r.to(torch.bfloat16)
    lo = (r - m.float()).to(torch.bfloat16)
    return h, m, lo


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_ring_follows_the_push_rule(cd, precision):
    """memory_start 2, M = 3 B, 8 steps: the ring after every step against the host model (two wraps), and on f32x3 the
    operand images of the ring (row and transposed planes) against the split of its fp32 rows."""
    B = 256 if precision == "f32x3" else 64
    ts = _step(cd, precision, memory_size=3 * B, memory_start=2)
    mem, D = ts.npair_memory, ts.layout.Dp
    pos, pid = [], []
    for t in range(8):
        ts.step()
        torch.cuda.synchronize()
        pos.append(ts.ws.e[1::2, :D].double().cpu().numpy())
        pid.append(ts.idx[1::2].cpu().numpy())
        rows, ids = mref.ring_after(t + 1, 2, 3 * B, pos, pid)
        assert np.array_equal(mem.ids.cpu().numpy(), ids), t
        assert np.array_equal(mem.rows.double().cpu().numpy(), rows), t
    if precision == "f32x3":
        K, Dq = mem.K, mem.Dq
        h, m, lo = _planes(mem.rows)
        for p, x in enumerate((h, m, lo)):
            assert torch.equal(mem.PM3[B:, p * Dq:p * Dq + D], x)
            assert torch.equal(mem.PMT3[:D, p * K + B:(p + 1) * K], x.T)
    assert np.isfinite(ts.loss())


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_deterministic_and_graph_replay_across_a_wrap(cd, precision):
    runs = []
    for use_graph in (False, False, True):
        ts = _step(cd, precision, memory_size=(2 * 256 if precision == "f32x3" else 2 * 64), memory_start=1,
                   optimizer="adam" if precision == "f32x3" else "momentum", use_graph=use_graph)
        for _ in range(6):                             # steps 1 .. 5 push: the ring of 2 batches wraps twice
            ts.step()
        torch.cuda.synchronize()
        m = ts.npair_memory
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone(), m.rows.clone(), m.ids.clone(), m.W().clone()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    assert (runs[0][3] >= 0).all() and np.isfinite(runs[0][1].cpu().numpy()).all()


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_resume_is_bit_exact(cd, precision):
    M = 2 * (256 if precision == "f32x3" else 64)
    straight = _step(cd, precision, memory_size=M)
    for _ in range(7):
        straight.step()
    first = _step(cd, precision, memory_size=M)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    state = first.state_dict()
    assert state["npair_memory"]["rows"].shape == (M, first.layout.Dp) and state["npair_memory"]["size"] == M
    resumed = _step(cd, precision, memory_size=M)
    resumed.load_state_dict(state)
    for _ in range(4):
        resumed.step()
    torch.cuda.synchronize()
    assert torch.equal(straight.params.flat, resumed.params.flat)
    assert torch.equal(straight.npair_memory.rows, resumed.npair_memory.rows)
    assert torch.equal(straight.npair_memory.ids, resumed.npair_memory.ids)
    assert torch.equal(straight.stats[:4], resumed.stats[:4])
    # a checkpoint without a ring loads into an empty ring; a ring of another size is refused
    plain = {k: v for k, v in state.items() if k != "npair_memory"}
    resumed.load_state_dict(plain)
    assert (resumed.npair_memory.ids == -1).all() and (resumed.npair_memory.rows == 0).all()
    with pytest.raises(ValueError, match="cross-batch memory"):
        _step(cd, precision, memory_size=2 * M).load_state_dict(state)
    with pytest.raises(ValueError, match="cross-batch memory"):
        _step(cd, precision).load_state_dict(state)


def test_memory_training_raises_recall(cd):
    """test_gpu_npair.test_npair_training_raises_recall's clustered catalogue with a memory of 4 batches."""
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
                            mode="npair", optimizer="adam", base_learning_rate=0.003, device=cd.dev, memory_size=1024)
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
    print("npair + memory learning: recall@10 %.4f -> %.4f, loss %.4f, counted fraction %.4f" % (r0, r1, loss,
                                                                                              s["active_triplets"]))
    assert np.isfinite(loss)
    assert r1 > 0.9 and r1 > r0 + 0.5, (r0, r1)
    assert 0.5 < s["active_triplets"] <= 1.0          # the memory's negatives are counted (M = 4 B: 4/5 of them)


def test_refusals(cd):
    N, F = 2000, 64
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0), dtype=torch.int32).to(cd.dev)
    mk = lambda B=256, **kw: cd.train.TrainStep(table, pairs, B, hidden_size=256, output_size=64, device=cd.dev, **kw)
    for mode in ("uniform", "inbatch", "semihard"):
        with pytest.raises(ValueError, match="mode 'npair'"):
            mk(mode=mode, memory_size=256)
    with pytest.raises(ValueError, match="multiple of the batch"):
        mk(mode="npair", memory_size=384)
    with pytest.raises(ValueError, match="multiple of the batch"):
        mk(B=64, mode="npair", precision="f32", memory_size=96)
    with pytest.raises(ValueError, match=">= 0"):
        mk(mode="npair", memory_size=-256)
    with pytest.raises(ValueError, match=">= 0"):
        mk(mode="npair", memory_size=256, memory_start=-1)
    with pytest.raises(ValueError, match="multiple of the batch"):
        cd.ops.NPairMemory(96, 32, 64, "f32", cd.dev)                   # a multiple of the batch, not of the f32 tile
    from cdml_amd.config import TrainConfig
    with pytest.raises(ValueError, match="mode 'npair'"):
        TrainConfig(mode="inbatch", memory_size=256, batch_size=256, hidden_size=256, output_size=64).train_step(
            table, pairs, device=cd.dev)
    ts = TrainConfig(mode="npair", memory_size=512, memory_start=3, batch_size=256, hidden_size=256,
                     output_size=64).train_step(table, pairs, device=cd.dev)
    assert ts.npair_memory.M == 512 and ts.npair_memory.start == 3
    Dp = ts.layout.Dp
    e = torch.zeros((512, Dp), dtype=torch.float32, device=cd.dev)
    ws = cd.ops.NPairWorkspace(256, Dp, "f32x3", cd.dev, in_batch=False)
    with pytest.raises(ValueError, match="video ids"):
        cd.ops.npair_loss(e, None, 256, Dp, ws=ws, memory=ts.npair_memory)
    with pytest.raises(ValueError, match="in_batch=False"):
        cd.ops.npair_loss(e, None, 256, Dp, ws=ws)
