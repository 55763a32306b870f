"""Write footprint of the two launches of the fp16 IVF lists (include/cdml_ivf_f16.h) with tests/footprint.py's poisoned,
guarded buffers, under both poison patterns: the fp16 scan stores every score of every slot row and nothing else -- not the
pad floats [len, ld) of a score row, not the gaps between the lists' blocks, nothing for an empty list; the re-rank writes
all 128 entries of both outputs of every query; every input comes back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import footprint as fp  # noqa: E402
import ivf_f16_ref as f16  # noqa: E402
import ivf_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = (0, 1, 127, 130, 5, 300, 0)
NQ, NPROBE, D = 300, 3, 64
GAP = 8                                  # floats between the score blocks of two lists
R, K = 40, 8


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import knn, ops
    cdml_amd.load_library()
    assert ops.knn_list_capacity() == xs.LIST

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.dev = knn, ops, gpu
    return ns


@pytest.fixture(scope="module")
def case(cd):
    rng = np.random.RandomState(4)
    nlist, n = len(LENS), sum(LENS)
    x = rng.randn(n, D)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = rng.randn(NQ, D)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    assign = np.repeat(np.arange(nlist), LENS)
    rng.shuffle(assign)
    ids, start = ref.lists_from_assign(assign, nlist)
    probe = np.stack([rng.choice(nlist, size=NPROBE, replace=False) for _ in range(NQ)])
    for r in range(200):                                                  # two slot tiles on the 300-row list
        probe[r] = [5] + list(rng.choice([c for c in range(nlist) if c != 5], size=2, replace=False))
    probe[3] = -1
    probe[10:20, 2] = -1
    dev = cd.dev
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    tb = cd.knn.ivf_tables(t(probe, torch.int32), t(np.asarray(LENS), torch.int64))
    slot_list = np.repeat(np.arange(nlist), np.diff(tb["slot_start"].cpu().numpy()))
    slot_off = tb["slot_off"].cpu().numpy() + GAP * slot_list              # a gap in front of every list's block
    total = int(tb["n_floats"]) + GAP * nlist
    mask = np.zeros(total, dtype=bool)
    lens = np.asarray(LENS)
    for s, c in enumerate(slot_list):
        mask[slot_off[s]:slot_off[s] + lens[c]] = True
    # the re-rank's candidate table: ids in any order, empty entries inside and behind r, one query with none
    cand = np.stack([rng.permutation(n)[:xs.LIST] for _ in range(NQ)]).astype(np.int64)
    cand[:, 9] = xs.NO_ID
    cand[5, :] = xs.NO_ID
    cand[6, 20:] = xs.NO_ID

    class NS:
        pass
    c = NS()
    c.nlist, c.n, c.x, c.q, c.assign, c.ids, c.start, c.probe, c.tb = nlist, n, x, q, assign, ids, start, probe, tb
    c.slot_list, c.total, c.mask, c.cand = slot_list, total, mask, cand
    c.Qh, c.rows_h = t(q, torch.float16), t(x[ids], torch.float16)
    c.Q, c.X = t(q, torch.float32), t(x, torch.float32)
    c.start_d = t(start, torch.int32)
    c.slot_off = t(slot_off, torch.int64)
    c.cand_d = t(cand, torch.int32)
    return c


def test_scan_f16_footprint(cd, case):
    c = case
    tb = c.tb
    gs = fp.Guarded((c.total,), torch.float32, cd.dev, mask=c.mask)
    inputs = (c.Qh, tb["slot_query"], tb["slot_start"], c.slot_off, c.rows_h, c.start_d, tb["tiles"])

    def run(pattern):
        gs.rearm(pattern)
        with fp.frozen(*inputs, names=["Q", "slot_query", "slot_start", "slot_off", "rows", "list_start", "tiles"]):
            cd.ops.ivf_scan_f16(c.Qh, tb["slot_query"], tb["slot_start"], c.slot_off, c.rows_h, c.start_d, tb["tiles"], gs.view)
            torch.cuda.synchronize()
        gs.assert_guards_intact("scores")                                 # pad floats, gaps and guards keep the poison
        return {"scores": gs.payload()}

    got = fp.assert_fully_written(run)["scores"].cpu().double().numpy()
    assert len(got) == int(c.mask.sum()) > 0
    sq = tb["slot_query"].cpu().numpy()
    qh, xh = f16.quantise(c.q).astype(np.float64), f16.quantise(c.x).astype(np.float64)
    want = np.concatenate([qh[sq[s]] @ xh[c.ids[c.start[l]:c.start[l + 1]]].T for s, l in enumerate(c.slot_list)])
    # fp16 x fp16 products are exact in fp32; D accumulation steps, sum |q~_k x~_k| <= (1 + 2^-11)^2
    assert np.abs(got - want).max() <= D * 2.0 ** -24 * (1 + 2.0 ** -11) ** 2


def test_refine_footprint(cd, case):
    c = case
    cap = xs.LIST
    gd = fp.Guarded((NQ, cap), torch.float32, cd.dev)
    gi = fp.Guarded((NQ, cap), torch.int32, cd.dev)

    def run(pattern):
        gd.rearm(pattern), gi.rearm(pattern)
        with fp.frozen(c.Q, c.X, c.cand_d, names=["Q", "base", "cand"]):
            cd.ops.ivf_refine(c.Q, c.X, c.cand_d, R, K, gd.view, gi.view)
            torch.cuda.synchronize()
        gd.assert_guards_intact("best_d"), gi.assert_guards_intact("best_i")
        return {"best_d": gd.payload(), "best_i": gi.payload()}

    got = fp.assert_fully_written(run)
    bd, bi = got["best_d"].cpu().numpy(), got["best_i"].cpu().numpy().astype(np.int64)
    # the whole list: the valid ones of the first R candidates ascending, then +inf / 0x7fffffff
    Dr, Ir = f16.refine(c.q, c.x, c.cand, R, cap)
    Ir = np.where(Ir < 0, xs.NO_ID, Ir)
    finite = np.isfinite(Dr)
    assert finite[0].sum() == R - 1 and finite[5].sum() == 0 and finite[6].sum() == 19
    assert np.array_equal(np.isfinite(bd), finite) and np.array_equal(bi[~finite], Ir[~finite])
    assert (bi[5] == xs.NO_ID).all() and np.isinf(bd[5]).all()
    assert np.abs(bd[finite] - Dr[finite]).max() <= 1e-5
    assert (bi == Ir).mean() > 0.99
    xs.assert_list_ascending(got["best_d"], got["best_i"], "refined list")
    # every id written is one of the query's first R candidates, each once
    for i in range(NQ):
        v = bi[i][bi[i] != xs.NO_ID]
        assert len(set(v)) == len(v) and set(v) <= set(c.cand[i, :R].tolist())
