"""Write footprint of the IVF launches (include/cdml_ivf.h) with tests/footprint.py's poisoned, guarded buffers, under both
poison patterns: the scan stores every score of every slot row and nothing else -- not the pad floats [len, ld) of a score
row, not the gaps between the lists' blocks, nothing for an empty list; the centroid launch leaves the rows of empty lists
(and the columns >= D) untouched; the merge writes every query's full list and does not depend on the pad floats; every input
comes back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import ivf_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = (0, 1, 127, 130, 5, 300, 0)
NQ, NPROBE, D, K = 300, 3, 64, 51
GAP = 8                                  # floats between the score blocks of two lists


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import knn, ops
    cdml_amd.load_library()

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

    class NS:
        pass
    c = NS()
    c.nlist, c.n, c.x, c.q, c.assign, c.ids, c.start, c.probe, c.tb = nlist, n, x, q, assign, ids, start, probe, tb
    c.slot_list, c.slot_off_np, c.total, c.mask = slot_list, slot_off, total, mask
    c.Q, c.rows = t(q, torch.float32), t(x[ids], torch.float32)
    c.X = t(x, torch.float32)
    c.ids_d, c.start_d = t(ids, torch.int32), t(start, torch.int32)
    c.slot_off = t(slot_off, torch.int64)
    c.probe_d = t(probe, torch.int32)
    c.r_sq = torch.zeros(n, dtype=torch.float32, device=dev)
    c.q_sq = torch.zeros(NQ, dtype=torch.float32, device=dev)
    cd.ops.row_sqnorm(c.rows, D, c.r_sq)
    cd.ops.row_sqnorm(c.Q, D, c.q_sq)
    return c


def _scan(cd, c, gs):
    tb = c.tb
    cd.ops.ivf_scan_f32(c.Q, tb["slot_query"], tb["slot_start"], c.slot_off, c.rows, c.start_d, tb["tiles"], gs.view)


def test_scan_footprint(cd, case):
    c = case
    tb = c.tb
    gs = fp.Guarded((c.total,), torch.float32, cd.dev, mask=c.mask)
    inputs = (c.Q, tb["slot_query"], tb["slot_start"], c.slot_off, c.rows, c.start_d, tb["tiles"])

    def run(pattern):
        gs.rearm(pattern)
        with fp.frozen(*inputs, names=["Q", "slot_query", "slot_start", "slot_off", "rows", "list_start", "tiles"]):
            _scan(cd, c, gs)
            torch.cuda.synchronize()
        gs.assert_guards_intact("scores")                                 # pad floats, gaps and guards keep the poison
        return {"scores": gs.payload()}

    got = fp.assert_fully_written(run)["scores"].cpu().double().numpy()
    assert len(got) == int(c.mask.sum()) > 0
    sq = tb["slot_query"].cpu().numpy()
    want = np.concatenate([c.q[sq[s]].astype(np.float64) @ c.x[c.ids[c.start[l]:c.start[l + 1]]].astype(np.float64).T
                           for s, l in enumerate(c.slot_list)])
    assert np.abs(got - want).max() <= D * 2.0 ** -24                     # unit rows: sum |q_k x_k| <= 1, D fused steps


def test_centroid_footprint(cd, case):
    c = case
    mask = torch.zeros((c.nlist, D), dtype=torch.bool)
    mask[np.asarray(LENS) > 0] = True
    gc = fp.Guarded((c.nlist, D), torch.float32, cd.dev, ld=D + 4, mask=mask)

    def run(pattern):
        gc.rearm(pattern)
        with fp.frozen(c.X, c.ids_d, c.start_d, names=["x", "order", "list_start"]):
            cd.ops.ivf_centroid_sums(c.X, c.ids_d, c.start_d, gc.view, D)
            torch.cuda.synchronize()
        gc.assert_guards_intact("centroids")                              # the rows of empty lists and the row gaps untouched
        return {"centroids": gc.payload()}

    got = fp.assert_fully_written(run)["centroids"].cpu().double().numpy()
    want = ref.column_means(c.x, c.assign, c.nlist)
    want = want[np.asarray(LENS) > 0].reshape(-1)
    assert np.abs(got - want).max() <= max(LENS) * 2.0 ** -24


def test_merge_footprint(cd, case):
    c = case
    tb = c.tb
    cap = cd.ops.knn_list_capacity()
    gs = fp.Guarded((c.total,), torch.float32, cd.dev, mask=c.mask)
    gd = fp.Guarded((NQ, cap), torch.float32, cd.dev)
    gi = fp.Guarded((NQ, cap), torch.int32, cd.dev)
    inputs = (c.slot_off, tb["slot_of"], c.probe_d, c.start_d, c.ids_d, c.r_sq, c.q_sq)

    def run(pattern):
        gs.rearm(pattern), gd.rearm(pattern), gi.rearm(pattern)
        _scan(cd, c, gs)                                                  # the pad floats and gaps hold this pattern's poison
        with fp.frozen(gs.raw, *inputs, names=["scores", "slot_off", "slot_of", "probe", "list_start", "ids", "r_sq", "q_sq"]):
            cd.ops.ivf_merge(gs.view, c.slot_off, tb["slot_of"], c.probe_d, c.start_d, c.ids_d, c.r_sq, c.q_sq, K, gd.view, gi.view)
            torch.cuda.synchronize()
        gd.assert_guards_intact("best_d"), gi.assert_guards_intact("best_i")
        return {"best_d": gd.payload(), "best_i": gi.payload()}

    got = fp.assert_fully_written(run)
    bd, bi = got["best_d"].cpu().numpy(), got["best_i"].cpu().numpy().astype(np.int64)
    # the first K entries are the query's K best (what lies behind them is written, sorted, and unspecified: cdml_knn_merge's rule)
    Dr, Ir = ref.search(ref.fp64_dist(c.q, c.x, l2_norm=False), c.assign, c.nlist, c.probe, K)
    Ir = np.where(Ir < 0, 0x7FFFFFFF, Ir)
    finite = np.isfinite(Dr)
    assert np.array_equal(np.isfinite(bd[:, :K]), finite) and np.array_equal(bi[:, :K][~finite], Ir[~finite])
    assert (bi[3] == 0x7FFFFFFF).all() and np.isinf(bd[3]).all()           # every probe -1: an empty list, written in full
    assert np.abs(bd[:, :K][finite] - Dr[finite]).max() <= 1e-5
    assert (bi[:, :K] == Ir).mean() > 0.99
    # the whole list ascends in (d, id)
    asc = (bd[:, 1:] > bd[:, :-1]) | ((bd[:, 1:] == bd[:, :-1]) & (bi[:, 1:] >= bi[:, :-1]))
    assert asc.all()
