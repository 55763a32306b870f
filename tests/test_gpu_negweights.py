"""Weighted negatives on the MI355X: sampler mode 3 (csrc/sampler_gather.hip: cdml_sample_weighted and the fused
cdml_sample_gather_weighted / _x3 / _f16) bit for bit against the host model of tests/negweights_ref.py and against the
un-fused gather; the mixed N-pair chain with a per-negative bias (cdml_npair_mixed_*_nb) against an fp64 restatement and
against the scalar path; TrainStep(negative_weights=...) in both modes."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import negweights_ref as ref  # noqa: E402
from oracle import synth as osynth  # noqa: E402

pytestmark = pytest.mark.gpu
BIG_STEP = 2 ** 32 + 5
TOL = 1e-5


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, negweights, ops, train
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.engine_bf16, ns.negweights, ns.ops, ns.train, ns.dev = engine, engine_bf16, negweights, ops, train, gpu
    return ns


def _pairs(n_rows, n_pairs, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n_rows, size=n_pairs)
    p = (a + 1 + rng.integers(0, n_rows - 1, size=n_pairs)) % n_rows
    return np.stack([a, p], 1).astype(np.int32)


def _weights(kind, n_rows, pairs):
    """(the weight table of a case, its two heavy rows or None); "two": all mass on the two rows of pair 0, which every
    fourth pair then is (both ways)"""
    if kind == "equal":
        return ref.equal_weights(n_rows), None
    if kind == "zipf":
        return ref.zipf_weights(n_rows, 11), None
    if kind == "halfzero":
        return ref.half_zero_weights(n_rows, 12), None
    ra, rp = int(pairs[0, 0]), int(pairs[0, 1])
    pairs[0::8] = (ra, rp)
    pairs[4::8] = (rp, ra)
    third = next(v for v in range(n_rows) if v not in (ra, rp))
    return ref.two_row_weights(n_rows, ra, rp, third), (ra, rp)


# n_rows, weight table, bits, batch, second rank, step, n_steps
SAMPLER_CASES = [
    (3, "equal", 8, 37, False, 0, 1),
    (3, "equal", 16, 256, True, 1, 3),
    (1000, "zipf", 16, 256, False, BIG_STEP, 1),
    (1000, "halfzero", 8, 37, True, BIG_STEP, 3),
    (1000, "two", 16, 256, True, 1, 3),
    (1000, "equal", 8, 37, False, 2, 3),
    (200000, "zipf", 16, 256, True, 1, 1),
    (200000, "halfzero", 16, 37, False, BIG_STEP, 3),
    (200000, "two", 8, 37, True, 0, 1),
    (200000, "equal", 8, 256, False, 2, 1),
]


def _rank(batch, second):
    return (batch, 2 * batch) if second else (0, batch)


def _model(pairs, n_rows, seed, step, batch, start, slot0, bg, n_steps):
    idx = np.empty((n_steps, batch, 3), dtype=np.int32)
    kind = np.empty((n_steps, batch), dtype=np.int32)
    for s in range(n_steps):
        idx[s], kind[s] = ref.weighted_triplets(pairs, n_rows, seed, step + s, batch, start, slot0, bg)
    return idx.reshape(n_steps, -1), kind


@pytest.mark.parametrize("n_rows,table,bits,batch,second,step,n_steps", SAMPLER_CASES)
def test_ids_and_kinds_equal_the_host_model(cd, n_rows, table, bits, batch, second, step, n_steps):
    """1. cdml_sample_weighted and the fused launch (fp32 rows, a narrow table) against the model, bit for bit, with and
    without kind_out and with the step from a device counter; a pair id outside the catalogue raises the fused launch's
    flag and the triplet is still drawn."""
    dev, ops = cd.dev, cd.ops
    slot0, bg = _rank(batch, second)
    n_pairs = 301
    used = np.concatenate([((step + s) * bg + slot0 + np.arange(batch)) % n_pairs for s in range(n_steps)])
    for oob in (False, True):
        pairs = _pairs(n_rows, n_pairs, seed=bits + batch)
        w, heavy = _weights(table, n_rows, pairs)
        if oob:                                            # (in pairs this launch reads: slots 3 and 5 of its first step)
            pairs[used[3], 0] = n_rows + 5
            pairs[used[5], 1] = n_rows
        nw = cd.negweights.NegativeWeights.from_weights(w, bits=bits)
        tables = nw.tables(dev)
        start = ref.as_start(nw.start.numpy())
        want_idx, want_kind = _model(pairs, n_rows, 77, step, batch, start, slot0, bg, n_steps)
        dp = torch.from_numpy(pairs).to(dev)
        for s in range(n_steps):
            idx = torch.full((3 * batch,), -9, dtype=torch.int32, device=dev)
            kind = torch.full((batch,), -9, dtype=torch.int32, device=dev)
            ops.sample_weighted(dp, n_rows, 77, step + s, batch, tables, idx, kind_out=kind, slot0=slot0, batch_global=bg)
            assert np.array_equal(idx.cpu().numpy(), want_idx[s]) and np.array_equal(kind.cpu().numpy(), want_kind[s])
        # the step from a device counter, without kind_out
        sd = torch.tensor([step], dtype=torch.int64, device=dev)
        idx = torch.full((3 * batch,), -9, dtype=torch.int32, device=dev)
        ops.sample_weighted(dp, n_rows, 77, None, batch, tables, idx, slot0=slot0, batch_global=bg, step_dev=sd)
        assert np.array_equal(idx.cpu().numpy(), want_idx[0])
        F = 8
        ftable = cd.engine.FeatureTable.synthetic(n_rows, F, 3, dev)
        R = 3 * batch
        one = n_steps == 1
        for with_kind in (True, False):
            x = torch.zeros((n_steps, R, 8), dtype=torch.float32, device=dev)
            idx = torch.full((n_steps, R), -9, dtype=torch.int32, device=dev)
            kind = torch.full((n_steps, batch), -9, dtype=torch.int32, device=dev) if with_kind else None
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            ops.sample_gather_weighted(dp, 77, step, batch, ftable.data, F, tables, idx[0] if one else idx, x[0] if one else x,
                                       kind_out=None if kind is None else (kind[0] if one else kind), slot0=slot0,
                                       batch_global=bg, n_steps=n_steps, oob_flag=flag)
            assert np.array_equal(idx.cpu().numpy(), want_idx)
            assert kind is None or np.array_equal(kind.cpu().numpy(), want_kind)
            assert int(flag.item()) == (1 if oob else 0)
        ids_ok = want_idx.reshape(n_steps, batch, 3)
        if oob:                                            # ... the ids pass through, and that triplet has its negative
            assert ids_ok[0, 3, 0] == n_rows + 5 and ids_ok[0, 5, 1] == n_rows
        neg = ids_ok[:, :, 2]
        assert ((neg != ids_ok[:, :, 0]) & (neg != ids_ok[:, :, 1])).all() and (neg >= 0).all() and (neg < n_rows).all()
        assert (w[neg[want_kind == 1]] > 0).all()
        if table == "two":                                 # every pair that IS the two heavy rows fell back to the uniform draw
            ra, rp = heavy
            both = ((ids_ok[:, :, 0] == ra) & (ids_ok[:, :, 1] == rp)) | ((ids_ok[:, :, 0] == rp) & (ids_ok[:, :, 1] == ra))
            assert both.sum() >= batch // 8 and not want_kind[both].any() and want_kind[~both].all()
        elif n_rows > 3:
            assert want_kind.mean() > 0.95
        else:
            assert want_kind.any()


FORMATS = ["f32", "x3", "x3k", "f16"]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _buffers(cd, fmt, F, R, n_steps, N=1000):
    """(table, x_out [n_steps, R, ld], x_ki or None) for a row format"""
    dev = cd.dev
    if fmt == "f16":
        table = cd.engine_bf16.FeatureTableF16.synthetic(N, F, 5, dev)
        return table, torch.zeros((n_steps, R, (F + 7) // 8 * 8 + 8), dtype=torch.bfloat16, device=dev), None
    table = cd.engine.FeatureTable.synthetic(N, F, 5, dev)
    if fmt == "f32":
        return table, torch.zeros((n_steps, R, (F + 3) // 4 * 4 + 4), dtype=torch.float32, device=dev), None
    plane = (F + 255) // 256 * 256
    x = torch.zeros((n_steps, R, 3 * plane), dtype=torch.bfloat16, device=dev)
    xk = torch.zeros((n_steps, 3 * R * plane), dtype=torch.bfloat16, device=dev) if fmt == "x3k" else None
    return table, x, xk


@pytest.mark.parametrize("F", [64, 1500])
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_equal_the_unfused_gather(cd, fmt, F):
    """2. Every output row of the four fused forms is what the existing un-fused gather (plus the split / the interleave
    where the format has one) writes for the same ids, bit for bit."""
    ops = cd.ops
    N, batch, n_steps = 1000, 256, 2
    pairs_np = _pairs(N, 400, seed=10)
    nw = cd.negweights.NegativeWeights.from_weights(ref.zipf_weights(N, 13))
    pairs = torch.from_numpy(pairs_np).to(cd.dev)
    table, x, xk = _buffers(cd, fmt, F, 3 * batch, n_steps, N)
    idx = torch.full((n_steps, 3 * batch), -9, dtype=torch.int32, device=cd.dev)
    kind = torch.full((n_steps, batch), -9, dtype=torch.int32, device=cd.dev)
    ops.sample_gather_weighted(pairs, 31, 4, batch, table.data, F, nw.tables(cd.dev), idx, x, kind_out=kind, n_steps=n_steps,
                               x_ki=xk)
    want_idx, want_kind = _model(pairs_np, N, 31, 4, batch, ref.as_start(nw.start.numpy()), 0, batch, n_steps)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kind.cpu().numpy(), want_kind)
    R = 3 * batch
    for s in range(n_steps):
        want = torch.zeros_like(x[s])
        if fmt == "f16":
            ops.gather_rows_f16(table.data, 0, idx[s], F, want)
        elif fmt == "f32":
            ops.gather_rows(table.data, 0, idx[s], F, want)
        else:
            plane = x.shape[2] // 3
            rows = torch.zeros((R, plane), dtype=torch.float32, device=cd.dev)
            ops.gather_rows(table.data, 0, idx[s], F, rows)
            ops.split_f32_bf16x3(rows, want, plane)
            if xk is not None:
                il = torch.zeros(3 * R * plane, dtype=torch.bfloat16, device=cd.dev)
                ops.interleave8_bf16x3(x[s], plane, R, plane, il)
                assert torch.equal(_bits(xk[s]), _bits(il)), s
        assert torch.equal(_bits(x[s]), _bits(want)), s
    assert x.float().abs().sum() > 0


def test_negw_bias_gathers_the_negatives_log_probability(cd):
    N, B = 1000, 256
    nw = cd.negweights.NegativeWeights.from_weights(ref.half_zero_weights(N, 3))
    lq = nw.lq.to(cd.dev)
    rng = np.random.default_rng(0)
    ids = rng.integers(0, N, size=(B, 3)).astype(np.int32)
    ids[7, 2], ids[9, 2] = N, -1                          # outside the catalogue: 0
    out = torch.full((B,), 9.0, dtype=torch.float32, device=cd.dev)
    cd.ops.negw_bias(lq, torch.from_numpy(ids).to(cd.dev).view(-1), B, 0.625, out)
    want = nw.lq.numpy()[np.clip(ids[:, 2], 0, N - 1)] + np.float32(0.625)
    want[[7, 9]] = 0
    assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))


# ---- 4. the mixed chain with a per-negative bias ----
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(B, M, D, seed):
    """Triplets with planted duplicates in every block (an in-batch positive that is another row's, a negative that is
    another row's anchor / positive, the same negative twice) and a ring with empty slots and slots of the batch's videos."""
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.7 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    N = _unit(A[rng.integers(0, B, B)] + 1.5 * rng.standard_normal((B, D)) / np.sqrt(D) * 4)
    ids3 = rng.choice(50 * B, size=3 * B, replace=False).astype(np.int32).reshape(B, 3)
    for k in range(0, B - 8, B // 16):
        ids3[k, 1] = ids3[k + 3, 1]
        ids3[k + 5, 0] = ids3[k, 1]
        ids3[k + 1, 2] = ids3[k + 6, 0]
        ids3[k + 2, 2] = ids3[k + 7, 1]
        ids3[k + 4, 2] = ids3[k + 2, 2]
    mem = mem_id = None
    if M:
        mem = _unit(A[rng.integers(0, B, M)] + 1.5 * rng.standard_normal((M, D)) / np.sqrt(D) * 4)
        mem = mem.astype(np.float32).astype(np.float64)
        mem_id = rng.choice(np.arange(50 * B, 60 * B), size=M, replace=False).astype(np.int32)
        mem_id[rng.choice(M, M // 8, replace=False)] = -1
        for k in range(0, M, M // 32):
            mem_id[k] = ids3.reshape(-1)[(7 * k) % (3 * B)]
    return A, P, N, ids3.reshape(-1), mem, mem_id


def _fp64(A, P, N, ids3, mem, mem_id, t, symmetric, bias, neg_bias, mem_bias, dev):
    """The definition of include/cdml_npair_mixed.h with neg_bias[j] in place of lq_u, in float64 torch; the gradients by
    autograd of the loss."""
    A, P, N = (torch.as_tensor(x, dtype=torch.float64, device=dev).clone().requires_grad_(True) for x in (A, P, N))
    B = A.shape[0]
    idt = torch.as_tensor(ids3, device=dev).view(B, 3).long()
    a, p, n = idt[:, 0], idt[:, 1], idt[:, 2]
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    cn = (n[None, :] != a[:, None]) & (n[None, :] != p[:, None])
    f64 = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev)
    b = torch.zeros((B, 2), dtype=torch.float64, device=dev) if bias is None else f64(bias).view(B, 2)
    nb = torch.zeros(B, dtype=torch.float64, device=dev) if bias is None else f64(neg_bias)
    ninf = -float("inf")
    S, U = A @ P.T / t, A @ N.T / t
    cols = [(S - b[None, :, 1]).masked_fill(~m, ninf), (U - nb[None, :]).masked_fill(~cn, ninf)]
    cm = None
    if mem is not None:
        q = torch.as_tensor(mem_id, device=dev).long()
        cm = (q[None, :] >= 0) & (q[None, :] != a[:, None]) & (q[None, :] != p[:, None])
        Xm = A @ f64(mem).T / t
        if bias is not None:
            Xm = Xm - f64(mem_bias)[None, :]
        cols.append(Xm.masked_fill(~cm, ninf))
    lr = torch.logsumexp(torch.cat(cols, 1), 1)
    d = torch.diagonal(S)
    loss = (lr - (d - b[:, 1])).mean()
    lc = None
    if symmetric:
        lc = torch.logsumexp((S - b[:, 0:1]).masked_fill(~mc, ninf), 0)
        loss = 0.5 * (loss + (lc - (d - b[:, 0])).mean())
    loss.backward()
    g = torch.empty((3 * B, A.shape[1]), dtype=torch.float64, device=dev)
    g[0::3], g[1::3], g[2::3] = A.grad, P.grad, N.grad
    return {"loss": loss.item(), "lse_row": lr.detach(), "lse_col": None if lc is None else lc.detach(), "de": g, "m": m,
            "mc": mc, "cn": cn, "cm": cm}


def _e3(cd, A, P, N):
    B, D = A.shape
    e = torch.zeros((3 * B, D), dtype=torch.float32, device=cd.dev)
    for k, x in enumerate((A, P, N)):
        e[k::3] = torch.as_tensor(x, dtype=torch.float32, device=cd.dev)
    return e


def _chain(cd, case, t, symmetric, precision, row_logq=None, mem_lq=None, lq_u=0.0, neg_bias=None):
    """ops.npair_mixed_loss on a fresh workspace.  The correction comes from a LogQTable over the video ids when the case has
    a ring (mem_lq: lq per video), else from a per-row tensor."""
    A, P, N, ids3, mem, mem_id = case
    B, D = A.shape
    e = _e3(cd, A, P, N)
    rows3 = torch.as_tensor(ids3, dtype=torch.int32, device=cd.dev)
    de = torch.zeros_like(e)
    ws = cd.ops.NPairMixed(B, D, precision, cd.dev, memory_size=0 if mem is None else mem.shape[0])
    logq = None
    if mem is not None:
        ws.ring.load(torch.as_tensor(mem, dtype=torch.float32), torch.as_tensor(mem_id))
        if mem_lq is not None:
            logq = cd.ops.LogQTable(torch.as_tensor(mem_lq), cd.dev)
    elif row_logq is not None:
        logq = torch.as_tensor(row_logq, dtype=torch.float32, device=cd.dev)
    stats, lse = cd.ops.npair_mixed_loss(e, rows3, B, D, t, symmetric, precision, de=de, ws=ws, logq=logq, lq_u=lq_u,
                                         neg_bias=neg_bias)
    torch.cuda.synchronize()
    return stats.clone(), lse.clone(), de, ws


@pytest.mark.parametrize("precision", ["f32x3", "f32"])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("M", [0, 256])
def test_mixed_chain_with_a_per_negative_bias(cd, M, symmetric, precision):
    """4. B = 256, D = 64, a random neg_bias: loss and every lse within 1e-5 of fp64, de within 1e-4 (relative L2), masked
    weights exactly 0 -- the scalar path's bounds (tests/test_gpu_npair_mixed.py); and with neg_bias[j] = c for all j,
    stats, lse and W are bit-equal to the scalar path at lq_u = c."""
    B, D, t = 256, 64, 0.1
    case = _case(B, M, D, seed=B + M + D)
    A, P, N, ids3, mem, mem_id = case
    rng = np.random.default_rng(5)
    lq = rng.normal(-8.0, 1.5, 60 * B).astype(np.float32)                 # one log-probability per video id
    bias = lq[ids3.reshape(B, 3)[:, :2].reshape(-1)]
    mem_bias = None if mem is None else np.where(mem_id >= 0, lq[np.maximum(mem_id, 0)], 0.0)
    nb = rng.normal(-7.0, 2.0, B).astype(np.float32)
    kw = dict(row_logq=bias, mem_lq=lq)
    stats, lse, de, ws = _chain(cd, case, t, symmetric, precision, neg_bias=torch.from_numpy(nb).to(cd.dev), **kw)
    r = _fp64(A, P, N, ids3, mem, mem_id, t, symmetric, bias.astype(np.float64), nb.astype(np.float64), mem_bias, cd.dev)
    err = {"loss": abs(stats[0].item() - r["loss"]), "lse": (lse[:B].double() - r["lse_row"]).abs().max().item(),
           "de": ((de.double() - r["de"]).norm() / r["de"].norm()).item()}
    if symmetric:
        err["lse_col"] = (lse[B:2 * B].double() - r["lse_col"]).abs().max().item()
    print("mixed chain with neg_bias, M %d sym %d %s: %s" % (M, symmetric, precision, err))
    assert np.isfinite(stats[0].item())
    assert err["loss"] <= TOL and err["lse"] <= TOL and err.get("lse_col", 0.0) <= TOL
    assert err["de"] <= 1e-4
    assert de[2::3].abs().max().item() > 0
    W = ws.W()
    dead = (~r["m"] & ~r["mc"]) if symmetric else ~r["m"]
    blocks = [(W[:, :B], dead), (W[:, B:2 * B], ~r["cn"])]
    if M:
        blocks.append((W[:, 2 * B:], ~r["cm"]))
    for Wb, off in blocks:
        assert int(off.sum()) > 0 and (Wb[off] == 0).all()
        assert (Wb[~off] != 0).float().mean().item() > 0.99
    # the vector must matter: the scalar path at the vector's mean is another loss
    c = float(np.float32(nb.mean()))
    s_stats, s_lse, s_de, s_ws = _chain(cd, case, t, symmetric, precision, lq_u=c, **kw)
    assert abs(s_stats[0].item() - stats[0].item()) > 1e-3
    # ... and a constant vector IS the scalar path, bit for bit
    const = torch.full((B,), c, dtype=torch.float32, device=cd.dev)
    v_stats, v_lse, v_de, v_ws = _chain(cd, case, t, symmetric, precision, neg_bias=const, **kw)
    n_lse = 2 * B if symmetric else B
    assert torch.equal(v_stats, s_stats) and torch.equal(v_lse[:n_lse], s_lse[:n_lse])
    assert torch.equal(v_ws.W(), s_ws.W()) and torch.equal(v_de, s_de)
    # without a correction the vector is not read
    u_stats, _, _, _ = _chain(cd, case, t, symmetric, precision)
    n_stats, _, _, _ = _chain(cd, case, t, symmetric, precision, neg_bias=torch.from_numpy(nb).to(cd.dev))
    assert torch.equal(u_stats, n_stats)


def test_npair_loss_facade_takes_a_per_negative_logq(cd):
    """losses.NPairLoss.calculate_loss(negative_logq=<tensor [batch]>) runs the vector path: loss and the gradients of
    pairs and negatives against fp64, test 4's bounds; a one-element value still means the scalar."""
    from cdml_amd import losses
    B, D = 256, 64
    A, P, N, ids3, _, _ = _case(B, 0, D, seed=9)
    rng = np.random.default_rng(10)
    logq = rng.normal(-8.0, 1.5, (B, 2)).astype(np.float32)
    nb = rng.normal(-7.0, 2.0, B).astype(np.float32)
    pairs = torch.stack([torch.as_tensor(A), torch.as_tensor(P)], 1).float().to(cd.dev).requires_grad_(True)
    negs = torch.as_tensor(N).float().to(cd.dev).requires_grad_(True)
    idt = torch.as_tensor(ids3.reshape(B, 3))
    out = losses.NPairLoss().calculate_loss(pairs, 0.1, True, ids=idt[:, :2], logq=torch.from_numpy(logq), negatives=negs,
                                            negative_ids=idt[:, 2], negative_logq=torch.from_numpy(nb))
    out["npair_loss"].backward()
    r = _fp64(A, P, N, ids3, None, None, 0.1, True, logq.reshape(-1).astype(np.float64), nb.astype(np.float64), None, cd.dev)
    assert abs(out["npair_loss"].item() - r["loss"]) <= TOL
    g = torch.empty((3 * B, D), dtype=torch.float64, device=cd.dev)
    g[0::3], g[1::3], g[2::3] = pairs.grad[:, 0].double(), pairs.grad[:, 1].double(), negs.grad.double()
    assert ((g - r["de"]).norm() / r["de"].norm()).item() <= 1e-4
    with pytest.raises(ValueError, match="negative_logq tensor"):
        losses.NPairLoss().calculate_loss(pairs, 0.1, True, ids=idt[:, :2], logq=torch.from_numpy(logq), negatives=negs,
                                          negative_ids=idt[:, 2], negative_logq=torch.zeros(B - 1))


# ---- 5. / 6. TrainStep ----
N_ROWS, F, H, D, B = 4000, 200, 512, 64, 256


def _step(cd, f16, weights, use_graph=False, mode="uniform", **kw):
    mk = cd.engine_bf16.FeatureTableF16 if f16 else cd.engine.FeatureTable
    table = mk.synthetic(N_ROWS, F, 0, cd.dev)
    pairs_np = osynth.cowatch_pairs(N_ROWS, 500, 0)
    pairs = torch.as_tensor(pairs_np, dtype=torch.int32).to(cd.dev)
    ts = cd.train.TrainStep(table, pairs, B, hidden_size=H, output_size=D, mode=mode, optimizer="adam",
                            base_learning_rate=0.01, device=cd.dev, use_graph=use_graph, negative_weights=weights, **kw)
    return ts, pairs_np


@pytest.mark.parametrize("f16", [False, True])
def test_train_step_uniform_mode_with_weights(cd, f16):
    """5. mode "uniform" with weights: the model's negatives and weighted share every step, eager == eager == graph replay
    across an in-place set_negative_weights (one captured graph), resume after 3 of 6 steps bit-exact, the refusals of a
    mismatched checkpoint."""
    NW = cd.negweights.NegativeWeights
    wa, wb = ref.zipf_weights(N_ROWS, 1), ref.half_zero_weights(N_ROWS, 2)
    sa, sb = (ref.as_start(NW.from_weights(w).start.numpy()) for w in (wa, wb))
    runs = []
    for use_graph in (False, False, True):
        ts, pairs_np = _step(cd, f16, torch.from_numpy(wa), use_graph=use_graph)
        assert ts.gather_ahead == 1 and ts.precision == ("bf16" if f16 else "f32x3")
        seen = []
        for t in range(6):
            if t == 3:
                ts.set_negative_weights(torch.from_numpy(wb))            # in place: the captured graph keeps reading it
            ts.step()
            want, kind = ref.weighted_triplets(pairs_np, N_ROWS, 1234, t, B, sa if t < 3 else sb)
            assert np.array_equal(ts.idx.cpu().numpy(), want.reshape(-1))
            assert ts.weighted_share() == kind.mean() and kind.mean() > 0.95
            if t >= 3:
                assert (wb[want[:, 2]] > 0).all()
            seen.append(ts.stats[:4].clone())
        torch.cuda.synchronize()
        if use_graph:
            assert len(ts._graphs) == 1                                   # nothing was re-captured
        runs.append((ts.params.flat.clone(), torch.stack(seen)))
        assert np.isfinite(ts.loss())
    for r in runs[1:]:
        assert torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1])
    # resume: 3 steps, checkpoint (the quanta ride in it), 3 more in a step built with OTHER weights
    first, _ = _step(cd, f16, torch.from_numpy(wa))
    for _ in range(3):
        first.step()
    first.set_negative_weights(NW.from_weights(wb))
    torch.cuda.synchronize()
    state = first.state_dict()
    assert torch.equal(state["negative_quanta"], NW.from_weights(wb).quanta) and state["negative_bits"] == 16
    resumed, _ = _step(cd, f16, torch.ones(N_ROWS))
    resumed.load_state_dict(state)
    for _ in range(3):
        resumed.step()
    torch.cuda.synchronize()
    assert torch.equal(resumed.params.flat, runs[0][0]) and torch.equal(resumed.stats[:4], runs[0][1][-1])
    plain, _ = _step(cd, f16, None)
    with pytest.raises(ValueError, match="negative weights"):
        plain.load_state_dict(state)
    with pytest.raises(ValueError, match="negative weights"):
        resumed.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="no negative weights"):
        plain.weighted_share()
    with pytest.raises(ValueError, match="no negative weights"):
        plain.set_negative_weights(torch.ones(N_ROWS))
    with pytest.raises(ValueError, match="one weight per catalogue row"):
        resumed.set_negative_weights(torch.ones(N_ROWS + 1))
    with pytest.raises(ValueError, match="must stay at bits"):
        resumed.set_negative_weights(NW.from_weights(wa, bits=12))


@pytest.mark.parametrize("with_memory", [False, True])
@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_npair_mixed_with_weights_against_fp64(cd, precision, with_memory):
    """6. mode "npair" with uniform_negatives, a logq table and weights: the N block is corrected by lq[n_j] of the
    sampler's own tables -- loss and de of a step against fp64 on the device's own idx and embedded rows, to test 4's
    bounds; with equal weights the loss agrees with the scalar lq_u path fed the same rows and ids to 1e-6."""
    NW = cd.negweights.NegativeWeights
    rng = np.random.default_rng(8)
    logq = torch.from_numpy(rng.normal(-8.0, 1.0, N_ROWS).astype(np.float32))
    kw = dict(memory_size=256) if with_memory else {}
    for which in ("zipf", "equal"):
        w = ref.zipf_weights(N_ROWS, 4) if which == "zipf" else ref.equal_weights(N_ROWS)
        nw = NW.from_weights(w)
        ts, pairs_np = _step(cd, False, nw, mode="npair", precision=precision, uniform_negatives=True, logq=logq, **kw)
        assert ts.neg_bias is not None and ts.uniform_lq == 0.0 and abs(ts.neg_bias_offset) < 1e-12
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        mem = mem_id = ring_rows = None
        if with_memory:
            ring_rows = ts.npair_memory.rows.clone()                       # (the ring as the step below reads it: before its push)
            mem = ts.npair_memory.rows[:, :D].double().cpu().numpy()
            mem_id = ts.npair_memory.ids.cpu().numpy().copy()
            assert (mem_id >= 0).all()
        ts.fetch()
        ts.forward_loss()
        torch.cuda.synchronize()
        idx = ts.idx.cpu().numpy()
        want, kind = ref.weighted_triplets(pairs_np, N_ROWS, 1234, 3, B, ref.as_start(nw.start.numpy()))
        assert np.array_equal(idx, want.reshape(-1)) and ts.weighted_share() == kind.mean() > 0.95
        E = ts.ws.e[:, :D].double().cpu().numpy()
        lq = logq.double().numpy()
        bias = lq[idx.reshape(B, 3)[:, :2].reshape(-1)]
        mem_bias = lq[mem_id] if with_memory else None
        nb = nw.lq.double().numpy()[idx[2::3]]                             # (offset 0: a logq table)
        assert np.array_equal(ts.neg_bias.cpu().numpy(), nw.lq.numpy()[idx[2::3]])
        r = _fp64(E[0::3], E[1::3], E[2::3], idx, mem, mem_id, 0.1, True, bias, nb, mem_bias, cd.dev)
        loss = float(ts.stats[0].item())
        rel = ((ts.ws.de[:, :D].double() - r["de"]).norm() / r["de"].norm()).item()
        print("npair mixed + %s weights (%s, memory %s): loss %.6f (fp64 %.6f), de relative L2 %.2e"
              % (which, precision, with_memory, loss, r["loss"], rel))
        assert abs(loss - r["loss"]) <= TOL
        assert rel <= 1e-4
        assert r["de"][2::3].abs().max().item() > 0                        # the weighted negatives receive a gradient
        if which == "equal":
            # the scalar path on the same rows, ids, ring and table: lq_u = -log(n_rows), today's correction
            mixed = cd.ops.NPairMixed(B, ts.layout.Dp, precision, cd.dev, memory_size=256 if with_memory else 0)
            if with_memory:
                mixed.ring.load(ring_rows, torch.from_numpy(mem_id))
            src = cd.ops.LogQTable(logq, cd.dev)
            lq_u = cd.ops.uniform_logq(src)
            assert lq_u == -math.log(N_ROWS)
            s_stats, _ = cd.ops.npair_mixed_loss(ts.ws.e, ts.idx, B, ts.layout.Dp, 0.1, True, precision, ws=mixed, logq=src,
                                                 lq_u=lq_u)
            scalar = float(s_stats[0].item())
            print("   equal weights: vector path %.7f, scalar lq_u path %.7f, difference %.2e" % (loss, scalar, abs(loss - scalar)))
            assert abs(loss - scalar) <= 1e-6


@pytest.mark.parametrize("logq", [None, "stream"])
def test_npair_mixed_with_weights_other_corrections(cd, logq):
    """Without ``logq`` the weighted negatives are the N block and nothing is corrected (no bias vector at all); with
    logq="stream" the vector is lq[n_j] + the estimator's scale -log(g0) + log(n_rows)."""
    nw = cd.negweights.NegativeWeights.from_weights(ref.zipf_weights(N_ROWS, 4))
    ts, pairs_np = _step(cd, False, nw, mode="npair", uniform_negatives=True, logq=logq)
    for _ in range(2):
        ts.step()
    ts.fetch()
    ts.forward_loss()
    torch.cuda.synchronize()
    idx = ts.idx.cpu().numpy()
    want, kind = ref.weighted_triplets(pairs_np, N_ROWS, 1234, 2, B, ref.as_start(nw.start.numpy()))
    assert np.array_equal(idx, want.reshape(-1)) and ts.weighted_share() == kind.mean()
    if logq is None:
        assert ts.neg_bias is None and ts.uniform_lq == 0.0
        E = ts.ws.e[:, :D].double().cpu().numpy()
        r = _fp64(E[0::3], E[1::3], E[2::3], idx, None, None, 0.1, True, None, None, None, cd.dev)
        assert abs(float(ts.stats[0].item()) - r["loss"]) <= TOL
    else:
        g0 = ts.npair_logq.init_gap
        assert ts.uniform_lq == 0.0 and ts.neg_bias_offset == -math.log(g0) + math.log(N_ROWS)
        want_nb = nw.lq.numpy()[idx[2::3]] + np.float32(ts.neg_bias_offset)
        assert np.array_equal(ts.neg_bias.cpu().numpy(), want_nb.astype(np.float32))
        assert np.isfinite(ts.loss())

