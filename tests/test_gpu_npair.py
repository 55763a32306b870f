"""The multi-class N-pair loss on the MI355X (csrc/npair.hip, ops.npair_loss, TrainStep(mode="npair"), losses.NPairLoss)
against the fp64 reference of tests/npair_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_ref  # noqa: E402
from oracle import sampler as osampler, synth as osynth, tower as otower  # noqa: E402

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


def _batch(B, D, seed):
    """Unit anchor / positive rows (positives near their anchors) and video ids with planted duplicates."""
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.7 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    ids = rng.choice(50 * B, size=2 * B, replace=False).astype(np.int32)
    for k in range(0, B - 8, max(1, B // 16)):
        ids[2 * k + 1] = ids[2 * (k + 3) + 1]          # two positives of one video
        ids[2 * (k + 5)] = ids[2 * k + 1]              # an anchor that is another pair's positive
    ids[6] = ids[7]                                    # a pair whose rows are one video
    return A, P, ids


def _ref_torch(A, P, ids, t, symmetric, dev):
    """npair_ref.npair in float64 on the device (B = 8192 on the host is gigabytes of fp64 temporaries)."""
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


def _run(cd, A, P, ids, t, symmetric, precision, with_de=True):
    B, D = A.shape
    e = torch.zeros((2 * B, D), dtype=torch.float32, device=cd.dev)
    e[0::2] = torch.as_tensor(A, dtype=torch.float32, device=cd.dev)
    e[1::2] = torch.as_tensor(P, dtype=torch.float32, device=cd.dev)
    rows = torch.as_tensor(ids, dtype=torch.int32, device=cd.dev)
    de = torch.zeros_like(e) if with_de else None
    ws = cd.ops.NPairWorkspace(B, D, precision, cd.dev)
    stats, lse = cd.ops.npair_loss(e, rows, B, D, t, symmetric, precision, de=de, ws=ws)
    torch.cuda.synchronize()
    return e, stats, lse, de, ws


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("t", [0.05, 1.0])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("B", [256, 1024, 8192])
def test_chain_against_fp64(cd, B, D, symmetric, t, precision):
    A, P, ids = _batch(B, D, seed=B + D)
    _, stats, lse, de, ws = _run(cd, A, P, ids, t, symmetric, precision)
    ref = _ref_torch(A, P, ids, t, symmetric, cd.dev)
    assert np.isfinite(stats[0].item())
    assert abs(stats[0].item() - ref["loss"]) < TOL
    assert (lse[:B].double() - ref["lse_row"]).abs().max().item() < TOL
    if symmetric:
        assert (lse[B:2 * B].double() - ref["lse_col"]).abs().max().item() < TOL
    g = torch.empty((2 * B, D), dtype=torch.float64, device=cd.dev)
    g[0::2], g[1::2] = ref["dA"], ref["dP"]
    rel = ((de.double() - g).norm() / g.norm()).item()
    assert rel < 1e-4, rel
    dead = (~ref["m"] & ~ref["mc"]) if symmetric else ~ref["m"]
    assert int(dead.sum()) > 0
    W = ws.W()[:B, :B]
    assert (W[dead] == 0).all()
    assert (W[~dead] != 0).float().mean().item() > 0.99        # (not a matrix of zeros)
    # stats: [1] the positives' mean squared distance, [3] the counted fraction of the row term's off-diagonal entries
    m = ref["m"].cpu().numpy()
    assert abs(stats[1].item() - np.mean(np.sum((A - P) ** 2, 1))) < 1e-5
    assert abs(stats[3].item() - (m.sum() - B) / (B * (B - 1))) < 1e-6


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_masked_duplicate_does_not_move_the_lse(cd, precision):
    B, D, t = 256, 256, 0.05
    A, P, ids = _batch(B, D, seed=11)
    i, k = 10, 40
    ids[2 * k + 1] = ids[2 * i + 1]                    # positive k is the same video as positive i: masked in row i
    _, _, lse0, _, ws0 = _run(cd, A, P, ids, t, False, precision, with_de=False)
    s0, l0 = ws0.S[i, k].item(), lse0[i].item()
    P2 = P.copy()
    P2[k] = _unit(-A[i:i + 1])[0]                      # move the duplicate as far from anchor i as a unit row goes
    _, _, lse1, _, ws1 = _run(cd, A, P2, ids, t, False, precision, with_de=False)
    assert abs(ws1.S[i, k].item() - s0) > 0.5          # the masked entry's score changed ...
    assert abs(lse1[i].item() - l0) < 1e-6             # ... and the anchor's lse did not


def _config0(cd, precision, optimizer, **kw):
    N, F = 10000, 1500
    feats = osynth.features_numpy(N, F, seed=0).astype(np.float32)
    pairs = osynth.cowatch_pairs(N, 3000, 0)
    table = cd.engine.FeatureTable.from_numpy(feats, cd.dev)
    lr = 0.01 if optimizer == "adam" else 1.0
    ts = cd.train.TrainStep(table, torch.as_tensor(pairs, dtype=torch.int32).to(cd.dev), 256, mode="npair",
                            optimizer=optimizer, base_learning_rate=lr, device=cd.dev, precision=precision, **kw)
    return feats, pairs, ts, lr


@pytest.mark.parametrize("precision", ["f32", "f32x3"])
@pytest.mark.parametrize("optimizer", ["adam", "lars"])
def test_train_steps_config0_shape(cd, precision, optimizer):
    """Config 0's shape (10 k x 1500, H 5000, D 256) at B = 256, checked per step from the device's own weights as
    test_gpu_parity.test_train_steps_config0 is: sampler -> tower -> N-pair reference -> tower backward in fp64."""
    feats, pairs, ts, lr = _config0(cd, precision, optimizer)
    B, D = 256, 256
    f64 = feats.astype(np.float64)
    host = lambda ts_: [x.detach().cpu().numpy().copy() for x in ts_]
    for step in range(3):
        W = host(ts.params.unpadded())
        slots = [host(ts.params._views(ts.m)), host(ts.params._views(ts.v))] if optimizer == "adam" else \
            [host(ts.params._views(ts.acc))]
        ts.step()
        rows, _, _, _ = osampler.device_inbatch(pairs, 1234, step, B)
        assert np.array_equal(ts.idx.cpu().numpy(), rows)
        Wd = [w.astype(np.float64) for w in W]
        fwd = otower.vnet_forward(f64[rows], *Wd, dtype=np.float64)
        E = fwd["l2_norm"]
        ref = npair_ref.npair(E[0::2], E[1::2], rows, 0.1, True)
        grads = otower.vnet_backward(fwd, Wd[2], npair_ref.interleave(ref["dA"], ref["dP"]), np.float64)
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
    assert s["variance"] is None and 0.0 < s["active_triplets"] <= 1.0 and s["mean_pos_dist"] < s["mean_neg_dist"] + 1.0


def _small_step(cd, precision, optimizer="adam", use_graph=False):
    N, F = 4000, 200
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 500, 0), dtype=torch.int32).to(cd.dev)
    B = 256 if precision == "f32x3" else 64
    return cd.train.TrainStep(table, pairs, B, hidden_size=512, output_size=64, mode="npair", optimizer=optimizer,
                              base_learning_rate=0.01 if optimizer == "adam" else 1.0, device=cd.dev, precision=precision,
                              use_graph=use_graph)


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_deterministic_and_graph_replay_bit_exact(cd, precision):
    runs = []
    for use_graph in (False, False, True):
        ts = _small_step(cd, precision, "adam" if precision == "f32x3" else "momentum", use_graph=use_graph)
        for _ in range(4):
            ts.step()
        torch.cuda.synchronize()
        runs.append((ts.params.flat.clone(), ts.stats[:4].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two eager runs differ"
    assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1], runs[2][1]), "graph replay differs from eager"
    assert np.isfinite(runs[0][1].cpu().numpy()).all()


def test_npair_loss_facade(cd):
    cls = cd.utils.find_class_by_name("NPairLoss", [cd.losses])
    B, D, t = 100, 32, 0.1                             # neither a tile multiple: the facade pads
    A, P, ids = _batch(B, D, seed=5)
    for symmetric, with_ids in ((True, True), (False, False)):
        pairs = torch.tensor(np.stack([A, P], 1), dtype=torch.float32, device=cd.dev, requires_grad=True)
        idt = torch.as_tensor(ids.reshape(B, 2), device=cd.dev) if with_ids else None
        loss_obj = cls()
        out = loss_obj.calculate_loss(pairs, temperature=t, symmetric=symmetric, ids=idt)
        out["npair_loss"].backward()
        assert set(out) == {"npair_loss", "anchors", "positives", "pos_dist", "neg_dist"}
        assert out["pos_dist"].shape == (B, 1) and out["neg_dist"].shape == (B, 1)
        assert set(loss_obj.summary) == {"mean_pos_dist", "mean_neg_dist"}
        ref = torch.tensor(np.stack([A, P], 1), dtype=torch.float64, requires_grad=True)
        a, p = ref[:, 0], ref[:, 1]
        m, mc = (torch.from_numpy(x) for x in npair_ref.masks(ids if with_ids else None, B))
        S = a @ p.T / t
        d = torch.diagonal(S)
        L = (torch.logsumexp(S.masked_fill(~m, -float("inf")), 1) - d).mean()
        if symmetric:
            L = 0.5 * (L + (torch.logsumexp(S.masked_fill(~mc, -float("inf")), 0) - d).mean())
        L.backward()
        assert abs(out["npair_loss"].item() - L.item()) < TOL
        g = pairs.grad.double().cpu()
        assert ((g - ref.grad).norm() / ref.grad.norm()).item() < 1e-4
        np.testing.assert_allclose(out["pos_dist"].cpu().numpy()[:, 0], np.sum((A - P) ** 2, 1), atol=1e-5)


def test_npair_training_raises_recall(cd):
    """Seeded clustered catalogue (512 clusters of 8 rows): a few hundred N-pair steps on within-cluster co-watch pairs
    raise recall@10 of held-out within-cluster pairs (Evaluation.retrieval_metrics)."""
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
                            mode="npair", optimizer="adam", base_learning_rate=0.003, device=cd.dev)
    assert ts.precision == "f32x3"                     # "auto" at B = 256
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
    print("npair learning: recall@10 %.4f -> %.4f, loss %.4f" % (r0, r1, loss))
    assert np.isfinite(loss)
    assert r1 > 0.9 and r1 > r0 + 0.5, (r0, r1)        # (a recorded run: 0.2024 -> 0.9985)


def test_production_shape_f32x3_matches_f32(cd):
    """1 M x 1500 catalogue, B = 8192 on f32x3: the loss is finite, and the same embedded rows through the f32 chain give
    the same loss.  The embedding gradient of this catalogue (iid-uniform features: the embedded rows nearly coincide) is
    a sum of cancelling terms, so both fp32-equivalent chains sit ~1e-4 from the fp64 gradient of the same rows (a
    recorded run: f32x3 1.55e-4, f32 1.56e-4, 2.14e-4 apart): each is held to 5e-4 of fp64, and f32x3 to no worse than
    the fp32-MFMA chain."""
    N, F, B = 1_000_000, 1500, 8192
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    rng = np.random.default_rng(0)
    pairs = rng.integers(0, N, size=(2_000_000, 2))
    pairs = torch.as_tensor(pairs[pairs[:, 0] != pairs[:, 1]], dtype=torch.int32).to(cd.dev)
    ts = cd.train.TrainStep(table, pairs, B, mode="npair", device=cd.dev)
    assert ts.precision == "f32x3"
    ts.step()
    ts.forward_loss()                                  # the step's embeddings and de at the updated weights
    torch.cuda.synchronize()
    loss = ts.stats[0].item()
    assert np.isfinite(loss)
    L = ts.layout
    de = torch.zeros_like(ts.ws.de)
    stats, _ = cd.ops.npair_loss(ts.ws.e, ts.idx, B, L.Dp, 0.1, True, "f32", de=de)
    torch.cuda.synchronize()
    assert abs(stats[0].item() - loss) < TOL
    e = ts.ws.e.double()
    ref = _ref_torch(e[0::2], e[1::2], ts.idx, 0.1, True, cd.dev)
    assert abs(ref["loss"] - loss) < TOL
    g = torch.empty_like(e)
    g[0::2], g[1::2] = ref["dA"], ref["dP"]
    err = lambda x: ((x.double() - g).norm() / g.norm()).item()
    e3, e1, apart = err(ts.ws.de), err(de), ((ts.ws.de - de).double().norm() / g.norm()).item()
    print("production shape: de relative L2 against fp64 -- f32x3 %.3g, f32 %.3g; chains %.3g apart" % (e3, e1, apart))
    assert e1 < 5e-4 and e3 < 5e-4 and e3 <= 1.25 * e1 + 1e-5, (e3, e1)
    del ts, table
    torch.cuda.empty_cache()


def test_refusals(cd):
    N, F = 2000, 64
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs = torch.as_tensor(osynth.cowatch_pairs(N, 300, 0), dtype=torch.int32).to(cd.dev)
    mk = lambda B=256, **kw: cd.train.TrainStep(table, pairs, B, hidden_size=256, output_size=64, mode="npair",
                                               device=cd.dev, **kw)
    for precision in ("bf16", "f16x2"):
        with pytest.raises(ValueError, match="f32x3"):
            mk(precision=precision)
    with pytest.raises(ValueError, match="one GPU"):
        mk(exchange=object())
    with pytest.raises(ValueError, match="one GPU"):
        mk(grad_sync=object())
    with pytest.raises(ValueError, match="train_table"):
        mk(train_table=True)
    with pytest.raises(ValueError, match="multiple of 256"):
        mk(B=320, precision="f32x3")
    with pytest.raises(ValueError, match="multiple of 64"):
        mk(B=100)                                      # "auto" -> f32, whose tiles need a multiple of 64
    with pytest.raises(ValueError, match="temperature"):
        mk(temperature=0.0)
    assert mk(B=320).precision == "f32"                # "auto": f32x3 only when B is a multiple of 256
