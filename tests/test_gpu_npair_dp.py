"""The data-parallel N-pair loss on the MI355X (csrc/npair_dp.hip, ops.npair_dp_loss, dist.NPairSync, TrainStep(npair_sync=))
against the fp64 single-batch N-pair loss at the GLOBAL batch: W ranks of B pairs must compute what one rank computes on
G = W B pairs.  Rank r's expected values are its rows [rB, (r+1)B) of that result; its gradients carry the local mean's
scale, W x the global mean's (the gradient average over the ranks divides it out)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_dp_ref  # noqa: E402

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


def _batch(G, D, W, seed):
    """Unit anchor / positive rows of the GLOBAL batch and video ids with planted duplicates, inside one rank and across
    ranks (rank r owns pairs [r B, (r+1) B))."""
    rng = np.random.default_rng(seed)
    B = G // W
    A = _unit(rng.standard_normal((G, D)))
    P = _unit(A + 0.7 * rng.standard_normal((G, D)) / np.sqrt(D) * 4)
    ids = rng.choice(50 * G, size=2 * G, replace=False).astype(np.int32)
    for k in range(0, G - 8, max(1, G // 16)):
        ids[2 * k + 1] = ids[2 * (k + 3) + 1]          # two positives of one video
        ids[2 * (k + 5)] = ids[2 * k + 1]              # an anchor that is another pair's positive
    ids[6] = ids[7]                                    # a pair whose rows are one video
    if W > 1:
        ids[2 * (B + 2) + 1] = ids[2 * 2 + 1]          # a positive on rank 1 that duplicates one on rank 0
        ids[2 * 9] = ids[2 * (G - 3) + 1]              # an anchor on rank 0 that is a positive on rank W - 1
    return A, P, ids


def _ref_torch(A, P, ids, t, symmetric, dev):
    """tests/npair_ref.npair in float64 on the device, at the global batch."""
    A, P = (torch.as_tensor(x, dtype=torch.float64, device=dev) for x in (A, P))
    B = A.shape[0]
    idt = torch.as_tensor(ids, device=dev).view(B, 2).long()
    a, p = idt[:, 0], idt[:, 1]
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    S = A @ P.T / t
    lr = torch.logsumexp(S.masked_fill(~m, -float("inf")), 1)
    d = torch.diagonal(S)
    loss = (lr - d).mean()
    W = torch.where(m, torch.exp(S - lr[:, None]), torch.zeros_like(S)) - eye.double()
    lc = None
    if symmetric:
        lc = torch.logsumexp(S.masked_fill(~mc, -float("inf")), 0)
        loss = 0.5 * (loss + (lc - d).mean())
        W = 0.5 * (W + torch.where(mc, torch.exp(S - lc[None, :]), torch.zeros_like(S)) - eye.double())
    W = W / (B * t)
    return {"loss": loss.item(), "lse_row": lr, "lse_col": lc, "dA": W @ P, "dP": W.T @ A, "m": m, "mc": mc}


def _rank_inputs(cd, A, P, ids, r, B):
    D = A.shape[1]
    e = torch.zeros((2 * B, D), dtype=torch.float32, device=cd.dev)
    e[0::2] = torch.as_tensor(A[r * B:(r + 1) * B], dtype=torch.float32, device=cd.dev)
    e[1::2] = torch.as_tensor(P[r * B:(r + 1) * B], dtype=torch.float32, device=cd.dev)
    rows = torch.as_tensor(ids[2 * r * B:2 * (r + 1) * B], dtype=torch.int32, device=cd.dev)
    return e, rows


def _simulate(cd, A, P, ids, W, t, symmetric, precision):
    """All W ranks in one process: the phase functions in turn, the collectives between them as plain tensor copies."""
    ops = cd.ops
    G, D = A.shape
    B = G // W
    wss = [ops.NPairDP(B, G, D, precision, cd.dev) for _ in range(W)]
    inp = [_rank_inputs(cd, A, P, ids, r, B) for r in range(W)]
    des = [torch.zeros_like(e) for e, _ in inp]
    stats = [torch.zeros(4, dtype=torch.float32, device=cd.dev) for _ in range(W)]
    for r in range(W):
        ops.npair_dp_pack(inp[r][0], inp[r][1], wss[r])
    wire = torch.cat([ws.send for ws in wss])                              # the all-gather of the positives
    for r in range(W):
        wss[r].wire.copy_(wire)
        ops.npair_dp_phase1(inp[r][0], r, wss[r], t, symmetric)
    cpa = torch.stack([ws.colpart for ws in wss])                          # the all-gather of the column partials
    for r in range(W):
        wss[r].colpart_all.copy_(cpa)
        ops.npair_dp_phase2(inp[r][0], r, wss[r], t, symmetric, de=des[r], stats=stats[r])
    for r in range(W):                                                     # the all-to-all of the partial dP blocks
        wss[r].recv.copy_(torch.stack([wss[s].dP_part[r * B:(r + 1) * B] for s in range(W)]))
        ops.npair_dp_phase3(wss[r], des[r])
    torch.cuda.synchronize()
    return wss, des, stats


CASES = [("f32x3", 2, 256, 64, 0.1, True), ("f32x3", 2, 256, 256, 0.1, True), ("f32x3", 2, 256, 64, 0.1, False),
         ("f32", 3, 64, 64, 0.1, True)]
CASES += [("f32", 4, 64, 64, t, s) for t in (0.05, 1.0) for s in (True, False)]


@pytest.mark.parametrize("precision,W,B,D,t,symmetric", CASES)
def test_simulated_ranks_against_fp64_at_global_batch(cd, precision, W, B, D, t, symmetric):
    G = W * B
    A, P, ids = _batch(G, D, W, seed=G + D)
    ref = _ref_torch(A, P, ids, t, symmetric, cd.dev)
    wss, des, stats = _simulate(cd, A, P, ids, W, t, symmetric, precision)
    dead = (~ref["m"] & ~ref["mc"]) if symmetric else ~ref["m"]
    assert int(dead.sum()) > 0
    assert int(dead[:B, B:].sum()) > 0                 # (dead entries ACROSS ranks too: rank 0's rows, another rank's columns)
    losses = []
    for r in range(W):
        sl = slice(r * B, (r + 1) * B)
        ws = wss[r]
        assert (ws.lse_row.double() - ref["lse_row"][sl]).abs().max().item() < TOL
        if symmetric:
            assert (ws.lse_col.double() - ref["lse_col"]).abs().max().item() < TOL
            assert torch.equal(ws.lse_col, wss[0].lse_col), "lse_col differs between the ranks"
        g = torch.empty((2 * B, D), dtype=torch.float64, device=cd.dev)
        g[0::2], g[1::2] = W * ref["dA"][sl], W * ref["dP"][sl]           # the local mean's scale
        rel = ((des[r].double() - g).norm() / g.norm()).item()
        assert rel < 1e-4, (r, rel)
        Wr = ws.W()
        assert (Wr[dead[sl]] == 0).all()
        assert (Wr[~dead[sl]] != 0).float().mean().item() > 0.99
        m = ref["m"][sl].cpu().numpy()
        assert abs(stats[r][1].item() - np.mean(np.sum((A[sl] - P[sl]) ** 2, 1))) < 1e-5
        assert abs(stats[r][3].item() - (m.sum() - B) / (B * (G - 1))) < 1e-6
        assert np.isfinite(stats[r][0].item())
        losses.append(stats[r][0].item())
    assert abs(np.mean(losses) - ref["loss"]) < TOL


@pytest.mark.parametrize("precision,B", [("f32x3", 256), ("f32", 64)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_world_of_one_is_the_single_gpu_chain(cd, precision, B, symmetric):
    D, t = 64, 0.1
    A, P, ids = _batch(B, D, 1, seed=17)
    wss, des, stats = _simulate(cd, A, P, ids, 1, t, symmetric, precision)
    e, rows = _rank_inputs(cd, A, P, ids, 0, B)
    de = torch.zeros_like(e)
    st, lse = cd.ops.npair_loss(e, rows, B, D, t, symmetric, precision, de=de)
    torch.cuda.synchronize()
    assert abs(stats[0][0].item() - st[0].item()) < TOL
    assert (stats[0][1:4] - st[1:4]).abs().max().item() < 1e-5
    assert (wss[0].lse_row - lse[:B]).abs().max().item() < TOL
    if symmetric:
        assert (wss[0].lse_col - lse[B:2 * B]).abs().max().item() < TOL
    rel = ((des[0] - de).double().norm() / de.double().norm()).item()
    assert rel < 1e-4, rel


def test_column_fold_alone(cd):
    W, G = 3, 64
    rng = np.random.default_rng(4)
    cp = np.stack([rng.uniform(-5, 5, (W, G)), rng.uniform(1, 50, (W, G))], 2).astype(np.float32)
    empty = lambda r, j: cp.__setitem__((r, j), (-np.inf, 0.0))
    empty(0, 3)                                        # an empty partial in the first ...
    empty(1, 7)                                        # ... a middle ...
    empty(2, 11)                                       # ... and the last rank position
    empty(0, 20), empty(1, 20)                         # columns where only one rank counts anything: the last,
    empty(1, 21), empty(2, 21)                         # the first,
    empty(0, 22), empty(2, 22)                         # the middle one
    empty(0, 30), empty(1, 30), empty(2, 30)           # nobody counts: -inf, not a NaN
    cpa = torch.as_tensor(cp, device=cd.dev)
    out = []
    for _ in range(2):
        lse = torch.full((G,), 123.0, dtype=torch.float32, device=cd.dev)
        cd.ops.npair_dp_col_fold(cpa, lse)
        torch.cuda.synchronize()
        out.append(lse)
    assert torch.equal(out[0], out[1])
    got = out[0].double().cpu().numpy()
    want = npair_dp_ref.fold(cp)
    counted = np.isfinite(cp[:, :, 0]).any(0)
    assert counted.sum() == G - 1 and np.isfinite(got[counted]).all()
    assert not np.isnan(got).any() and got[30] == -np.inf
    assert np.abs(got[counted] - want[counted]).max() < TOL


def test_positive_gradient_fold_alone(cd):
    W, B, D = 3, 64, 64
    rng = np.random.default_rng(5)
    recv = (rng.standard_normal((W, B, D)) * (10.0 ** np.arange(W))[:, None, None]).astype(np.float32)
    de0 = rng.standard_normal((2 * B, D)).astype(np.float32)
    de = torch.as_tensor(de0, device=cd.dev).clone()
    cd.ops.npair_dp_pos_fold(torch.as_tensor(recv, device=cd.dev), B, D, de)
    torch.cuda.synchronize()
    want = recv[0].copy()
    for r in range(1, W):
        want = (want + recv[r]).astype(np.float32)     # fp32, rank order
    got = de.cpu().numpy()
    assert np.array_equal(got[1::2].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[0::2].view(np.uint32), de0[0::2].view(np.uint32)), "rows 2i were touched"


# ---- two real ranks on one card (gloo, host-staged collectives) against one rank at the global batch ----------------------
CFG_F32 = dict(n_rows=3000, F=200, H=300, D=64, B=64, steps=2, precision="f32")
CFG_X3 = dict(CFG_F32, F=250, H=500, D=256, B=256, precision="f32x3")


def _make(dev, rank, world, c, exchange=None, grad_sync=None, npair_sync=None):
    from cdml_amd import dist as cdist, engine, train
    from oracle import synth as osynth
    pairs = torch.from_numpy(osynth.cowatch_pairs(c["n_rows"], 400, 0)).to(dev)
    if world == 1:
        table = engine.FeatureTable.synthetic(c["n_rows"], c["F"], 0, dev)
        B, slot0 = 2 * c["B"], 0
    else:
        lo, hi, _ = cdist.shard_bounds(c["n_rows"], world, rank)
        table = engine.FeatureTable.synthetic(hi - lo, c["F"], 0, dev, row0=lo, n_rows_global=c["n_rows"])
        B, slot0 = c["B"], rank * c["B"]
    return train.TrainStep(table, pairs, B, hidden_size=c["H"], output_size=c["D"], mode="npair", device=dev,
                           exchange=exchange, grad_sync=grad_sync, npair_sync=npair_sync, slot0=slot0,
                           batch_global=2 * c["B"], precision=c["precision"])


def _worker(rank, world, port, q, c):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cdml_amd import dist as cdist
        dev = torch.device("cuda:0")
        ts = _make(dev, rank, world, c, cdist.RowExchange(c["n_rows"], group=dist.new_group()), cdist.GradSync(),
                   cdist.NPairSync(group=dist.new_group()))
        idx, g0 = [], None
        for _ in range(c["steps"]):
            ts.step()
            idx.append(ts.idx.cpu().numpy().copy())
            if g0 is None:
                g0 = ts.params.grad.cpu().numpy().copy()                # the averaged gradient of step 0
        torch.cuda.synchronize()
        q.put((rank, "ok", np.stack(idx), ts.params.flat.cpu().numpy(), ts.loss(), g0))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None, None, None, None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("c", [CFG_F32, CFG_X3], ids=["f32", "f32x3"])
def test_two_rank_step_equals_single_rank(gpu, c):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, c)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()                               # this exact child, by handle
    for r in res:
        assert r[1] == "ok", "rank %d: %s" % (r[0], r[1])
    single = _make(gpu, 0, 1, c)
    idx, g0 = [], None
    for _ in range(c["steps"]):
        single.step()
        idx.append(single.idx.cpu().numpy().copy())
        if g0 is None:
            g0 = single.params.grad.cpu().numpy().copy()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.concatenate([r[2] for r in res], axis=1), np.stack(idx))      # the same global pairs
    np.testing.assert_array_equal(res[0][3], res[1][3])                                            # replicas stay identical
    dl = abs(np.mean([r[4] for r in res]) - single.loss())
    rel = np.linalg.norm(res[0][5].astype(np.float64) - g0) / np.linalg.norm(g0.astype(np.float64))
    print("two ranks vs one at the global batch (%s): |loss difference| %.3g, step-0 gradient relative L2 %.3g"
          % (c["precision"], dl, rel))
    assert dl < 1e-4
    # both gradients are held to 1e-4 (relative L2) of the fp64 gradient, hence at most 2e-4 apart
    assert rel < 2e-4, rel


# ---- the hook's RCCL entry points, world size 1 -----------------------------------------------------------------------------
def _nccl_worker(port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        from cdml_amd import dist as cdist, engine, train
        from oracle import synth as osynth
        N, F, B = 3000, 250, 256
        table = engine.FeatureTable.synthetic(N, F, 0, dev)
        pairs = torch.from_numpy(osynth.cowatch_pairs(N, 400, 0)).to(dev)
        kw = dict(hidden_size=500, output_size=256, mode="npair", device=dev, precision="f32x3")
        plain = train.TrainStep(table, pairs, B, **kw)
        sync = cdist.NPairSync(group=dist.new_group(), skip_self=False)     # the collectives run although there is one rank
        dp = train.TrainStep(table, pairs, B, npair_sync=sync, **kw)
        plain.step(), dp.step()                        # the same weights, rows and kernels up to the loss chain
        torch.cuda.synchronize()
        dl = abs(plain.stats[0].item() - dp.stats[0].item())
        rel = ((plain.ws.de - dp.ws.de).double().norm() / plain.ws.de.double().norm()).item()
        same = torch.equal(plain.idx, dp.idx)
        dlse = max((plain.npair_ws.lse[:B] - dp.npair_dp.lse_row).abs().max().item(),
                   (plain.npair_ws.lse[B:2 * B] - dp.npair_dp.lse_col).abs().max().item())      # (G = B: the same columns)
        plain.step(), dp.step()
        torch.cuda.synchronize()
        fin = bool(np.isfinite(dp.stats[0].item())) and torch.equal(plain.idx, dp.idx)
        ok = same and dl < 1e-5 and dlse < 1e-5 and rel < 1e-4 and fin
        q.put("ok" if ok else "loss difference %.3g, lse difference %.3g, de relative L2 %.3g, same ids %s, second step fine %s"
              % (dl, dlse, rel, same, fin))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put(traceback.format_exc()[-3000:])


def _run_worker(target, timeout):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=target, args=(port, q))
    p.start()
    try:
        return q.get(timeout=timeout)
    except Exception:
        return "worker gave no answer within %d s (hung?)" % timeout
    finally:
        p.join(timeout=20)
        if p.is_alive():
            p.kill()                                  # this exact child, by handle
            p.join(timeout=20)


def test_rccl_single_rank_npair_sync(gpu):
    """One GPU, so RCCL runs with world_size 1 -- enough to execute the hook's real all_gather / all_to_all entry points
    (skip_self=False) inside a training step and to compare it with the plain single-GPU N-pair step."""
    msg = _run_worker(_nccl_worker, 200)
    assert msg == "ok", msg


# ---- refusals -----------------------------------------------------------------------------------------------------------------
class _LocalSync:
    """a world of one without torch.distributed: the hook's interface, its collectives plain copies"""
    world, rank, group = 1, 0, None

    def all_gather(self, out, inp):
        out.view(-1).copy_(inp.view(-1))

    all_to_all = all_gather


def test_refusals_and_eager_under_use_graph(cd, caplog):
    from oracle import synth as osynth
    N, F = 2000, 64
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0), dtype=torch.int32).to(cd.dev)
    sync = _LocalSync()
    mk = lambda B=256, mode="npair", **kw: cd.train.TrainStep(table, pairs, B, hidden_size=256, output_size=64, mode=mode,
                                                              device=cd.dev, **kw)
    with pytest.raises(ValueError, match="npair_sync goes with mode 'npair'"):
        mk(mode="uniform", npair_sync=sync)
    for name, kw in (("memory_size", dict(memory_size=256)), ("logq", dict(logq="stream")),
                     ("uniform_negatives", dict(uniform_negatives=True)), ("train_table", dict(train_table=True))):
        with pytest.raises(ValueError, match=name):
            mk(npair_sync=sync, **kw)
    with pytest.raises(ValueError, match="multiple of 256"):
        mk(B=320, npair_sync=sync, precision="f32x3")
    with pytest.raises(ValueError, match="multiple of 64"):
        mk(B=100, npair_sync=sync)
    with pytest.raises(ValueError, match="batch_global"):
        mk(npair_sync=sync, batch_global=512)
    with pytest.raises(ValueError, match="one GPU"):
        mk(exchange=object())
    # the ops layer: a mis-tiled workspace, a padded batch
    with pytest.raises(ValueError, match="multiple of 256"):
        cd.ops.NPairDP(320, 640, 64, "f32x3", cd.dev)
    with pytest.raises(ValueError, match="multiple of the local batch"):
        cd.ops.NPairDP(64, 96, 64, "f32", cd.dev)
    ws = cd.ops.NPairDP(64, 64, 64, "f32", cd.dev)
    with pytest.raises(ValueError, match="unpadded"):
        cd.ops.npair_dp_phase1(torch.zeros((2 * 128, 64), device=cd.dev), 0, ws)
    with pytest.raises(ValueError, match="unpadded"):
        cd.ops.npair_dp_loss(torch.zeros((2 * 128, 64), device=cd.dev), torch.zeros(128, dtype=torch.int32, device=cd.dev), 64,
                             64, ws=ws, precision="f32", sync=sync)
    # use_graph with the hook: the step runs eagerly (with a logged warning) and is the plain step's loss
    import logging
    with caplog.at_level(logging.WARNING, logger="cdml.train"):
        dp = mk(npair_sync=sync, use_graph=True)
    assert dp.use_graph is False and any("npair_sync" in r.getMessage() for r in caplog.records)
    plain = mk()
    dp.step(), plain.step()                            # the same weights and rows: the plain chain's loss
    torch.cuda.synchronize()
    assert torch.equal(dp.idx, plain.idx) and abs(dp.stats[0].item() - plain.stats[0].item()) < TOL
    for _ in range(2):
        dp.step()
    torch.cuda.synchronize()
    assert not dp._graphs and np.isfinite(dp.loss())
