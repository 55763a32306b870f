"""Hard negatives on the MI355X: the listed sampler (csrc/sampler_gather.hip mode 2: cdml_sample_listed and the fused
cdml_sample_gather_listed / _x3 / _f16) bit for bit against the host model of tests/hardneg_ref.py, against the mode-0
launch where the draw must fall through, and against the un-fused gather; TrainStep(negative_lists=...) in both modes;
hardneg.mine_lists against the fp64 brute force; and training with refreshed lists."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hardneg_ref as ref  # noqa: E402
import npair_mixed_ref as xref  # noqa: E402
from oracle import sampler as osampler, synth as osynth, tower as otower  # noqa: E402

pytestmark = pytest.mark.gpu
BIG_STEP = 2 ** 32 + 5


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, hardneg, ops, train
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.engine, ns.engine_bf16, ns.hardneg, ns.ops, ns.train, ns.dev = engine, engine_bf16, hardneg, ops, train, gpu
    return ns


def _planted(n_rows, L, ldl, n_pairs, seed, oob_at=None):
    """(pairs [n_pairs, 2], lists [n_rows, ldl]): random lists with, over the anchors of the pair stream in turn, an empty
    row, a row holding only {a, p}, a row of ids >= n_rows, a row of one duplicated id, and ordinary rows with holes; the
    columns >= L hold a sentinel no draw may return.  oob_at = (i, j): the anchor of pair i and the positive of pair j lie
    outside the catalogue."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n_rows, size=n_pairs)
    p = (a + 1 + rng.integers(0, n_rows - 1, size=n_pairs)) % n_rows
    pairs = np.stack([a, p], 1).astype(np.int32)
    lists = np.full((n_rows, ldl), 7, dtype=np.int32)                     # (7: a valid id, so a read past L would show)
    anchors = np.unique(a)
    lists[anchors, :L] = rng.integers(0, n_rows, size=(len(anchors), L))
    holes = rng.random((len(anchors), L)) < 0.2
    lists[anchors, :L] = np.where(holes, -1, lists[anchors, :L])
    for k, (ai, pi) in enumerate(pairs):
        kind = k % 6
        if kind == 0:
            lists[ai, :L] = -1
        elif kind == 1:
            lists[ai, :L] = np.where(np.arange(L) % 2 == 0, ai, pi)
        elif kind == 2:
            lists[ai, :L] = n_rows + np.arange(L)
        elif kind == 3:
            lists[ai, :L] = (ai + pi + 11) % n_rows
    if oob_at is not None:
        pairs[oob_at[0], 0] = n_rows + 5
        pairs[oob_at[1], 1] = n_rows
    return pairs, lists


# n_rows, L, ldl, h, batch, second rank, step, n_steps
SAMPLER_CASES = [
    (1000, 1, 3, 1.0, 37, False, 0, 1),
    (1000, 4, 8, 0.5, 256, True, 1, 3),
    (1000, 32, 40, 1.0, 256, False, BIG_STEP, 1),
    (1000, 128, 132, 0.5, 37, True, BIG_STEP, 3),
    (1000, 32, 33, 0.0, 256, True, 1, 3),
    (1000, 4, 5, 1.0, 37, False, 2, 3),
    (1000000, 4, 5, 1.0, 256, True, 1, 1),
    (1000000, 32, 33, 0.5, 37, False, BIG_STEP, 3),
    (1000000, 1, 2, 0.0, 37, True, 0, 1),
]


def _rank(batch, second):
    return (batch, 2 * batch) if second else (0, batch)


def _model(pairs, n_rows, seed, step, batch, lists, L, h, slot0, bg, n_steps):
    idx = np.empty((n_steps, batch, 3), dtype=np.int32)
    kind = np.empty((n_steps, batch), dtype=np.int32)
    for s in range(n_steps):
        idx[s], kind[s] = ref.listed_triplets(pairs, n_rows, seed, step + s, batch, lists, L, h, slot0, bg)
    return idx.reshape(n_steps, -1), kind


@pytest.mark.parametrize("n_rows,L,ldl,h,batch,second,step,n_steps", SAMPLER_CASES)
def test_ids_and_kinds_equal_the_host_model(cd, n_rows, L, ldl, h, batch, second, step, n_steps):
    """1. cdml_sample_listed and the fused launch (fp32 rows, a narrow table) against the model, bit for bit; a pair id
    outside the catalogue raises the fused launch's flag and leaves that triplet to the uniform draw."""
    dev, ops = cd.dev, cd.ops
    slot0, bg = _rank(batch, second)
    used = np.concatenate([((step + s) * bg + slot0 + np.arange(batch)) % 301 for s in range(n_steps)])
    for oob in (False, True):
        # (the out-of-catalogue ids sit in pairs this launch reads: slots 3 and 5 of its first step)
        pairs, lists = _planted(n_rows, L, ldl, 301, seed=L + batch, oob_at=(used[3], used[5]) if oob else None)
        want_idx, want_kind = _model(pairs, n_rows, 77, step, batch, lists, L, h, slot0, bg, n_steps)
        dp = torch.from_numpy(pairs).to(dev)
        dl = torch.from_numpy(lists).to(dev)[:, :L]                        # a strided view: ldl > L
        for s in range(n_steps):
            idx = torch.full((3 * batch,), -9, dtype=torch.int32, device=dev)
            kind = torch.full((batch,), -9, dtype=torch.int32, device=dev)
            ops.sample_listed(dp, n_rows, 77, step + s, batch, dl, h, idx, kind_out=kind, slot0=slot0, batch_global=bg)
            assert np.array_equal(idx.cpu().numpy(), want_idx[s]) and np.array_equal(kind.cpu().numpy(), want_kind[s])
        # the step from a device counter, without kind_out
        sd = torch.tensor([step], dtype=torch.int64, device=dev)
        idx = torch.full((3 * batch,), -9, dtype=torch.int32, device=dev)
        ops.sample_listed(dp, n_rows, 77, None, batch, dl, h, idx, slot0=slot0, batch_global=bg, step_dev=sd)
        assert np.array_equal(idx.cpu().numpy(), want_idx[0])
        F = 8
        table = cd.engine.FeatureTable.synthetic(n_rows, F, 3, dev)
        R = 3 * batch
        x = torch.zeros((n_steps, R, 8), dtype=torch.float32, device=dev)
        idx = torch.full((n_steps, R), -9, dtype=torch.int32, device=dev)
        kind = torch.full((n_steps, batch), -9, dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        one = n_steps == 1
        ops.sample_gather_listed(dp, 77, step, batch, table.data, F, dl, h, idx[0] if one else idx, x[0] if one else x,
                                 kind_out=kind[0] if one else kind, slot0=slot0, batch_global=bg, n_steps=n_steps,
                                 oob_flag=flag)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kind.cpu().numpy(), want_kind)
        assert int(flag.item()) == (1 if oob else 0)
        if oob:                                                            # ... and that triplet's negative is the uniform draw
            assert want_kind[0, 3] == 0 and want_idx[0, 9] == n_rows + 5 and want_idx[0, 3 * 5 + 1] == n_rows
        if h > 0:
            assert 0 < want_kind.sum() and (h == 1.0 or want_kind.sum() < want_kind.size)
        else:
            assert not want_kind.any()
        ids_ok = want_idx.reshape(n_steps, batch, 3)
        assert ((ids_ok[:, :, 2] != ids_ok[:, :, 0]) & (ids_ok[:, :, 2] != ids_ok[:, :, 1])).all()
        assert (ids_ok[:, :, 2] >= 0).all() and (ids_ok[:, :, 2] < n_rows).all()


FORMATS = ["f32", "x3", "x3k", "f16"]


def _buffers(cd, fmt, F, R, n_steps):
    """(table, x_out [n_steps, R, ld], x_ki or None) for a row format"""
    dev = cd.dev
    N = 1000
    if fmt == "f16":
        table = cd.engine_bf16.FeatureTableF16.synthetic(N, F, 5, dev)
        ld = (F + 7) // 8 * 8 + 8
        return table, torch.zeros((n_steps, R, ld), dtype=torch.bfloat16, device=dev), None
    table = cd.engine.FeatureTable.synthetic(N, F, 5, dev)
    if fmt == "f32":
        return table, torch.zeros((n_steps, R, (F + 3) // 4 * 4 + 4), dtype=torch.float32, device=dev), None
    plane = (F + 255) // 256 * 256
    x = torch.zeros((n_steps, R, 3 * plane), dtype=torch.bfloat16, device=dev)
    xk = torch.zeros((n_steps, 3 * R * plane), dtype=torch.bfloat16, device=dev) if fmt == "x3k" else None
    return table, x, xk


def _launch(cd, fmt, F, batch, n_steps, pairs, lists, h, listed=True, step=4):
    table, x, xk = _buffers(cd, fmt, F, 3 * batch, n_steps)
    idx = torch.full((n_steps, 3 * batch), -9, dtype=torch.int32, device=cd.dev)
    kind = torch.full((n_steps, batch), -9, dtype=torch.int32, device=cd.dev)
    one = n_steps == 1
    pick = lambda t: None if t is None else (t[0] if one else t)
    if listed:
        cd.ops.sample_gather_listed(pairs, 31, step, batch, table.data, F, lists, h, pick(idx), pick(x), kind_out=pick(kind),
                                    n_steps=n_steps, x_ki=pick(xk))
    else:
        shift = torch.zeros(n_steps, dtype=torch.int32, device=cd.dev)
        cd.ops.sample_gather(0, pairs, 31, step, batch, table.data, F, pick(idx), pick(x), shift_out=shift, n_steps=n_steps,
                             x_ki=pick(xk))
    return table, idx, x, xk, kind


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("F", [64, 1500])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fall_through_is_the_mode0_launch_bit_for_bit(cd, fmt, F):
    """2. With h = 0, and with all-empty lists at h = 1, idx_out, x_out and x_ki are the mode-0 launch's."""
    batch, n_steps, L = 256, 2, 8
    pairs_np, lists_np = _planted(1000, L, L + 4, 400, seed=9)
    pairs = torch.from_numpy(pairs_np).to(cd.dev)
    full = torch.from_numpy(lists_np).to(cd.dev)[:, :L]
    empty = torch.full((1000, L), -1, dtype=torch.int32, device=cd.dev)
    _, idx0, x0, xk0, _ = _launch(cd, fmt, F, batch, n_steps, pairs, None, 0.0, listed=False)
    for lists, h in ((full, 0.0), (empty, 1.0)):
        _, idx, x, xk, kind = _launch(cd, fmt, F, batch, n_steps, pairs, lists, h)
        assert torch.equal(idx, idx0) and torch.equal(_bits(x), _bits(x0)) and not kind.any()
        if xk is not None:
            assert torch.equal(_bits(xk), _bits(xk0))
    assert x0.float().abs().sum() > 0


@pytest.mark.parametrize("F", [64, 1500])
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_equal_the_unfused_gather(cd, fmt, F):
    """3. h = 1: every output row is what the existing un-fused gather writes for the same ids; x_ki is the interleave of
    the row-major planes."""
    ops = cd.ops
    batch, n_steps, L = 256, 2, 8
    pairs_np, lists_np = _planted(1000, L, L + 4, 400, seed=10)
    pairs = torch.from_numpy(pairs_np).to(cd.dev)
    lists = torch.from_numpy(lists_np).to(cd.dev)[:, :L]
    table, idx, x, xk, kind = _launch(cd, fmt, F, batch, n_steps, pairs, lists, 1.0)
    want_idx, want_kind = _model(pairs_np, 1000, 31, 4, batch, lists_np, L, 1.0, 0, batch, n_steps)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(kind.cpu().numpy(), want_kind)
    assert 0 < want_kind.sum() < want_kind.size
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


def _uniform_step(cd, f16, lists=None, h=1.0, use_graph=False, N=4000, F=200, **kw):
    mk = cd.engine_bf16.FeatureTableF16 if f16 else cd.engine.FeatureTable
    table = mk.synthetic(N, F, 0, cd.dev)
    pairs_np = osynth.cowatch_pairs(N, 500, 0)
    pairs = torch.as_tensor(pairs_np, dtype=torch.int32).to(cd.dev)
    ts = cd.train.TrainStep(table, pairs, 256, hidden_size=512, output_size=64, mode="uniform", optimizer="adam",
                            base_learning_rate=0.01, device=cd.dev, use_graph=use_graph, negative_lists=lists,
                            hard_fraction=h, **kw)
    return ts, pairs_np


def _random_lists(N, L, seed):
    rng = np.random.default_rng(seed)
    lists = rng.integers(0, N, size=(N, L)).astype(np.int32)
    lists[rng.random((N, L)) < 0.3] = -1
    return lists


@pytest.mark.parametrize("f16", [False, True])
def test_train_step_uniform_mode_with_lists(cd, f16):
    """4. mode "uniform" with lists at B = 256: deterministic, the model's negatives and hard share, graph replay == eager
    across an in-place set_negative_lists, resume after 3 of 6 steps bit-exact."""
    N, L, h = 4000, 8, 0.75
    la, lb = _random_lists(N, L, 1), _random_lists(N, L, 2)
    runs = []
    for use_graph in (False, False, True):
        ts, pairs_np = _uniform_step(cd, f16, torch.from_numpy(la), h, use_graph=use_graph)
        assert ts.gather_ahead == 1 and ts.precision == ("bf16" if f16 else "f32x3")
        seen = []
        for t in range(6):
            if t == 3:
                ts.set_negative_lists(torch.from_numpy(lb))               # in place: the captured graph keeps reading it
            ts.step()
            want, kind = ref.listed_triplets(pairs_np, N, 1234, t, 256, la if t < 3 else lb, L, h)
            assert np.array_equal(ts.idx.cpu().numpy()[2::3], want[:, 2])
            assert np.array_equal(ts.idx.cpu().numpy(), want.reshape(-1))
            assert ts.hard_share() == kind.mean() and 0.5 < kind.mean() < 1.0
            seen.append(ts.stats[:4].clone())
        torch.cuda.synchronize()
        if use_graph:
            assert len(ts._graphs) == 1                                   # nothing was re-captured
        runs.append((ts.params.flat.clone(), torch.stack(seen)))
        assert np.isfinite(ts.loss())
    for r in runs[1:]:
        assert torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1])
    # resume: 3 steps, checkpoint (the lists and hard_fraction ride in it), 3 more in a step built with OTHER lists
    first, _ = _uniform_step(cd, f16, torch.from_numpy(la), h)
    for _ in range(3):
        first.step()
    first.set_negative_lists(torch.from_numpy(lb))
    torch.cuda.synchronize()
    state = first.state_dict()
    assert torch.equal(state["negative_lists"], torch.from_numpy(lb)) and state["hard_fraction"] == h
    resumed, _ = _uniform_step(cd, f16, torch.from_numpy(la), 0.1)
    resumed.load_state_dict(state)
    for _ in range(3):
        resumed.step()
    torch.cuda.synchronize()
    assert torch.equal(resumed.params.flat, runs[0][0]) and torch.equal(resumed.stats[:4], runs[0][1][-1])
    plain, _ = _uniform_step(cd, f16)
    with pytest.raises(ValueError, match="negative lists"):
        plain.load_state_dict(state)
    with pytest.raises(ValueError, match="no negative lists"):
        plain.hard_share()
    with pytest.raises(ValueError, match="must stay"):
        resumed.set_negative_lists(torch.zeros((N, L + 4), dtype=torch.int32))


@pytest.mark.parametrize("with_memory", [False, True])
@pytest.mark.parametrize("precision", ["f32x3", "f32"])
def test_npair_mixed_with_lists_against_fp64(cd, precision, with_memory):
    """5. mode "npair" with uniform_negatives and lists: the N block is the drawn negatives -- the device's own idx and
    embedded rows through tests/npair_mixed_ref.py give the loss within 1e-5 and de within 1e-4 (relative L2), that
    file's users' bounds; with memory_size=512 and logq="stream" the ring and the estimate are those from before the step."""
    N, F, B, L = 4000, 200, 256, 8
    lists = _random_lists(N, L, 3)
    table = cd.engine.FeatureTable.synthetic(N, F, 0, cd.dev)
    pairs_np = osynth.cowatch_pairs(N, 500, 0)
    pairs = torch.as_tensor(pairs_np, dtype=torch.int32).to(cd.dev)
    kw = dict(memory_size=512, logq="stream") if with_memory else {}
    ts = cd.train.TrainStep(table, pairs, B, hidden_size=512, output_size=64, mode="npair", optimizer="adam",
                            base_learning_rate=0.01, device=cd.dev, precision=precision, uniform_negatives=True,
                            negative_lists=torch.from_numpy(lists), hard_fraction=1.0, **kw)
    for _ in range(3):
        ts.step()
    torch.cuda.synchronize()
    mem = mem_id = lq = None
    if with_memory:
        mem = ts.npair_memory.rows[:, :64].double().cpu().numpy()
        mem_id = ts.npair_memory.ids.cpu().numpy().copy()
        lq = ts.sampling_logq().double().cpu().numpy()
        assert (mem_id >= 0).all()
    ts.fetch()
    ts.forward_loss()
    torch.cuda.synchronize()
    idx = ts.idx.cpu().numpy()
    want, kind = ref.listed_triplets(pairs_np, N, 1234, 3, B, lists, L, 1.0)
    assert np.array_equal(idx, want.reshape(-1)) and ts.hard_share() == kind.mean() > 0.9
    E = ts.ws.e[:, :64].double().cpu().numpy()
    bias = mem_bias = None
    if with_memory:
        bias = lq[idx.reshape(B, 3)[:, :2].reshape(-1)]
        mem_bias = lq[mem_id]
    r = xref.npair_mixed(E[0::3], E[1::3], E[2::3], idx, 0.1, True, mem, mem_id, bias, ts.uniform_lq, mem_bias)
    de = ts.ws.de[:, :64].double().cpu().numpy()
    want_de = xref.interleave3(r["dA"], r["dP"], r["dN"])
    loss = float(ts.stats[0].item())
    rel = np.linalg.norm(de - want_de) / np.linalg.norm(want_de)
    print("npair mixed + lists (%s, memory %s): loss %.6f (fp64 %.6f), de relative L2 %.2e" % (precision, with_memory, loss,
                                                                                                r["loss"], rel))
    assert abs(loss - r["loss"]) < 1e-5
    assert rel < 1e-4
    assert np.abs(want_de[2::3]).max() > 0                               # the listed negatives receive a gradient


def _clustered(seed, n, D, n_clusters, spread):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_clusters, D))
    return (c[rng.integers(0, n_clusters, size=n)] + spread * rng.standard_normal((n, D))).astype(np.float32)


MINE_N, MINE_D, MINE_K = 2048, 64, 16


@pytest.fixture(scope="module")
def mined():
    """the seeded clustered catalogue and its fp64 neighbours (computed once)"""
    emb = _clustered(12, MINE_N, MINE_D, 64, 0.35)
    ids, d = ref.neighbours(emb, MINE_K + 2 + 2)                          # k + skip_top + 2 at skip_top = 2
    rng = np.random.default_rng(13)
    a = rng.integers(0, MINE_N, size=3000)
    pairs = np.stack([a, ids[a, rng.integers(1, 8, size=3000)]], 1).astype(np.int32)   # partners ARE near neighbours
    return emb, ids, d, pairs


def test_mined_catalogue_has_few_near_ties(mined):
    """(CPU arithmetic) rows with two adjacent fp64 distances closer than 1e-6 among their first k + skip_top + 2
    neighbours may take test 6's set comparison: at most 1 % of the rows; the seeded input has 9 such rows of 2048 (at
    skip_top = 2; smallest gap 3.9e-8)."""
    _, _, d, _ = mined
    near = (np.diff(d, axis=1) < 1e-6).any(1)
    print("rows with a near-tie:", int(near.sum()))
    assert near.sum() <= 0.01 * MINE_N
    assert int(near.sum()) == 9


@pytest.mark.parametrize("with_pairs", [False, True])
@pytest.mark.parametrize("skip_top", [0, 2])
def test_mine_lists_equals_the_brute_force(cd, mined, skip_top, with_pairs):
    """6. hardneg.mine_lists == the fp64 brute force row for row; a row with a near-tie (see above) compares as an id set
    with distances within 1e-5."""
    emb, ids, d, pairs = mined
    k = MINE_K
    want = ref.mine_lists(emb, k, skip_top, pairs if with_pairs else None)
    got = cd.hardneg.mine_lists(emb, k, skip_top=skip_top, pairs=torch.from_numpy(pairs) if with_pairs else None,
                                device=cd.dev)
    assert got.dtype == torch.int32 and tuple(got.shape) == (MINE_N, 16) and got.is_cuda
    got = got.cpu().numpy()
    w = k + skip_top + 2
    near = (np.diff(d[:, :w], axis=1) < 1e-6).any(1)
    assert near.sum() <= 0.01 * MINE_N
    x = emb.astype(np.float64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    for i in range(MINE_N):
        if not near[i]:
            assert np.array_equal(got[i], want[i]), i
        else:
            g, t = got[i][got[i] >= 0], want[i][want[i] >= 0]
            dist = lambda c: np.sort(2 - 2 * x[c] @ x[i])
            assert len(g) == len(t) and len(set(g)) == len(g) and np.abs(dist(g) - dist(t)).max() < 1e-5, i
    if with_pairs:
        assert (want[:, :k] == -1).sum() > 1000                          # the partner filter had work to do
    else:
        assert (want[:, :k] >= 0).all()                                  # without partners every list is full


def test_training_with_refreshed_lists(cd):
    """7. On test_npair_training_raises_recall's clustered catalogue (fp32): after 200 uniform steps the share of active
    hinges at those weights is strictly greater under freshly mined lists (k = 16, h = 1, partners dropped) than under
    the uniform draws of the same step; 300 more steps with refresh_negatives_every=100 raise recall@10 of the held-out
    pairs above its value at the switch.

    The training half runs as one would run it on this catalogue: every video has 7 cluster mates, which the held-out
    pairs count as positives and of which the training pairs name only a part, so a row's 7 nearest neighbours are
    expected false negatives -- negative_skip_top = 7 is the guard made for that -- and half the negatives stay uniform
    (hard_fraction = 0.5), the usual ANCE-style mix.  Both settings follow from the catalogue's construction (per = 8),
    not from a run."""
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
    pairs = torch.as_tensor(train_pairs).to(cd.dev)
    mk = lambda **kw: cd.train.TrainStep(table, pairs, 256, hidden_size=512, output_size=64, mode="uniform", optimizer="adam",
                                         base_learning_rate=0.003, device=cd.dev, **kw)
    uni = mk()
    for _ in range(200):
        uni.step()
    torch.cuda.synchronize()
    state = uni.state_dict()
    ev = Evaluation(None, [], device=cd.dev)

    def recall(ts):
        W = [w.detach().cpu().numpy().astype(np.float64) for w in ts.params.unpadded()]
        emb = otower.vnet_forward(feats.astype(np.float64), *W, dtype=np.float64)["l2_norm"].astype(np.float32)
        return ev.retrieval_metrics(emb, held, ks=(10,))["recall@10"]

    hard = mk(negative_lists=cd.hardneg.empty_lists(N, 16), hard_fraction=1.0)
    state_h = dict(state, negative_lists=cd.hardneg.empty_lists(N, 16), hard_fraction=1.0)
    hard.load_state_dict(state_h)
    lists = hard.refresh_negative_lists(16)
    assert tuple(lists.shape) == (N, 16) and (lists >= 0).float().mean().item() > 0.5
    # step 200 at the same weights, forward + loss only: the share of triplets with an active hinge
    active = []
    for ts in (uni, hard):
        ts.fetch()
        ts.forward_loss()
        active.append(float((ts.hinge > 0).float().mean().item()))
    assert torch.equal(uni.idx.view(-1, 3)[:, :2], hard.idx.view(-1, 3)[:, :2])       # the same pairs
    share = hard.hard_share()
    r_switch = recall(hard)
    print("active hinges at step 200: uniform %.4f, listed %.4f (hard share %.4f); recall@10 at the switch %.4f"
          % (active[0], active[1], share, r_switch))
    assert active[1] > active[0]
    assert share > 0.9
    mixed = mk(negative_lists=cd.hardneg.empty_lists(N, 16), hard_fraction=0.5)
    mixed.load_state_dict(dict(state_h, hard_fraction=0.5))                # the switch: step 200's weights and optimizer
    assert mixed.global_step == 200 and mixed.hard_fraction == 0.5 and recall(mixed) == r_switch
    tr = cd.train.Trainer(mixed, num_epochs=100, n_pairs=len(train_pairs), refresh_negatives_every=100, negative_k=16,
                          negative_skip_top=per - 1)
    before = mixed.neg_lists.clone()
    tr.run(max_steps=500)
    assert mixed.global_step == 500 and not torch.equal(before, mixed.neg_lists)
    r_end = recall(mixed)
    print("recall@10 after 300 steps with refreshed lists (h = 0.5, skip_top = 7): %.4f, hard share of the last step %.4f"
          % (r_end, mixed.hard_share()))
    assert np.isfinite(mixed.loss()) and r_end > r_switch
