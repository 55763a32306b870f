"""Write footprint of the three launches of residual product quantisation (include/cdml_ivf_pqr.h) with tests/footprint.py's
poisoned, guarded buffers, under both poison patterns: the residual encoder writes M bytes per row and nothing of the gap
bytes [M, ldc), its distances only when asked (a row with an assign of -1 included: codes 0, dist +inf); the slot scalars are
exactly n_slots floats; the scan stores every score of every slot row and nothing else -- not the pad floats [len, ld) of a
score row, not the gaps between the lists' blocks, nothing for an empty list or a -1 probe; every input comes back
bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_pqr_ref as pqr  # noqa: E402
import ivf_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
M, D = 16, 64                            # dsub = 4; S = 4 slots, R = 1024 rows
LENS = (0, 1, 127, 1030, 5, 300, 0)      # one list longer than R
NQ, NPROBE = 40, 3
GAP = 8                                  # floats between the score blocks of two lists
UNLISTED = (11, 900)                     # rows handed to the encoder with an assign of -1


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
    x = rng.randn(n, D).astype(np.float32)
    q = rng.randn(NQ, D).astype(np.float32)
    cent = (0.5 * rng.randn(nlist, D)).astype(np.float32)
    cb = rng.randn(M, 256, D // M).astype(np.float32)
    assign = np.repeat(np.arange(nlist), LENS)
    rng.shuffle(assign)
    ids, start = ref.lists_from_assign(assign, nlist)
    probe = np.stack([rng.choice(nlist, size=NPROBE, replace=False) for _ in range(NQ)])
    for r in range(30):                                                   # more than S slots on the lists 3 and 5
        probe[r] = [5, 3] + [int(rng.choice([0, 1, 2, 4, 6]))]
    probe[3] = -1
    probe[10:20, 2] = -1
    S, R = cd.ops.ivf_pq_tile(M)
    assert max(LENS) > R and (probe == 5).sum() > S and (probe == -1).any()
    dev = cd.dev
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    tb = cd.knn.ivf_tables(t(probe, torch.int32), t(np.asarray(LENS), torch.int64), tile_slots=S, tile_rows=R)
    slot_list = np.repeat(np.arange(nlist), np.diff(tb["slot_start"].cpu().numpy()))
    slot_off = tb["slot_off"].cpu().numpy() + GAP * slot_list              # a gap in front of every list's block
    total = int(tb["n_floats"]) + GAP * nlist
    mask = np.zeros(total, dtype=bool)
    lens = np.asarray(LENS)
    for s, c in enumerate(slot_list):
        mask[slot_off[s]:slot_off[s] + lens[c]] = True
    e = x - cent[assign]                                                  # fp32: the kernel's subtract
    codes, dist = pq.encode(e, cb)

    class NS:
        pass
    c = NS()
    c.nlist, c.n, c.x, c.q, c.cb, c.cent, c.ids, c.start, c.tb, c.slot_list, c.total, c.mask = \
        nlist, n, x, q, cb, cent, ids, start, tb, slot_list, total, mask
    c.e, c.codes, c.dist, c.assign = e, codes, dist, assign
    c.X, c.Q, c.CB, c.CEN = t(x, torch.float32), t(q, torch.float32), t(cb, torch.float32), t(cent, torch.float32)
    c.codes_d = t(codes[ids], torch.uint8)
    c.start_d = t(start, torch.int32)
    c.slot_off = t(slot_off, torch.int64)
    a_enc = assign.copy()
    a_enc[list(UNLISTED)] = -1
    c.A = t(a_enc, torch.int64)
    return c


@pytest.mark.parametrize("with_dist", [False, True])
def test_residual_encode_footprint(cd, case, with_dist):
    c = case
    gc = fp.Guarded((c.n, M), torch.uint8, cd.dev, ld=M + 8)
    gd = fp.Guarded((c.n, M), torch.float32, cd.dev, ld=M + 4)

    def run(pattern):
        gc.rearm(pattern), gd.rearm(pattern)
        with fp.frozen(c.X, c.CEN, c.A, c.CB, names=["x", "centroids", "assign", "codebooks"]):
            cd.ops.pqr_encode(c.X, c.CEN, c.A, c.CB, gc.view, gd.view if with_dist else None)
            torch.cuda.synchronize()
        gc.assert_guards_intact("codes")                                  # the gap bytes [M, ldc) keep the poison
        if with_dist:
            gd.assert_guards_intact("dist")
            return {"codes": gc.payload(), "dist": gd.payload()}
        assert bool((fp.bits_of(gd.flat) == fp.poison_scalar(torch.float32, pattern)).all()), "dist written without being given"
        return {"codes": gc.payload()}

    got = fp.assert_fully_written(run)
    codes = got["codes"].cpu().numpy().astype(np.int64)
    un = np.zeros(c.n, dtype=bool)
    un[list(UNLISTED)] = True
    assert (codes[un] == 0).all()
    d = pq.sub_dist(c.e, c.cb)
    chosen = np.take_along_axis(d, codes[:, :, None], 2)[:, :, 0]
    assert (codes[~un] == c.codes[~un]).mean() > 0.999
    assert (chosen[~un] - d.min(2)[~un] <= 2 * pq.encode_bound(D // M) * chosen[~un]).all()
    if with_dist:
        dist = got["dist"].cpu().double().numpy()
        assert np.isposinf(dist[un]).all() and np.abs(dist[~un] - chosen[~un]).max() <= 1e-5


def test_slot_dots_footprint(cd, case):
    c = case
    tb = c.tb
    n_slots = int(tb["n_slots"])
    gb = fp.Guarded((n_slots,), torch.float32, cd.dev)
    inputs = (c.Q, c.CEN, tb["slot_query"], tb["slot_start"])

    def run(pattern):
        gb.rearm(pattern)
        with fp.frozen(*inputs, names=["Q", "centroids", "slot_query", "slot_start"]):
            cd.ops.ivf_slot_dots(c.Q, c.CEN, tb["slot_query"], tb["slot_start"], gb.view)
            torch.cuda.synchronize()
        gb.assert_guards_intact("slot_base")
        return {"slot_base": gb.payload()}

    got = fp.assert_fully_written(run)["slot_base"].cpu().double().numpy()
    sq = tb["slot_query"].cpu().numpy()
    assert len(got) == n_slots == len(c.slot_list) > 0
    assert np.abs(got - pqr.slot_dot(c.q, c.cent)[sq, c.slot_list]).max() <= 1e-5


def test_scan_pqr_footprint(cd, case):
    c = case
    tb = c.tb
    lut = torch.empty((NQ, M, 256), dtype=torch.float32, device=cd.dev)
    cd.ops.pq_lut(c.Q, c.CB, lut)
    slot_base = torch.empty(int(tb["n_slots"]), dtype=torch.float32, device=cd.dev)
    cd.ops.ivf_slot_dots(c.Q, c.CEN, tb["slot_query"], tb["slot_start"], slot_base)
    gs = fp.Guarded((c.total,), torch.float32, cd.dev, mask=c.mask)
    inputs = (lut, tb["slot_query"], tb["slot_start"], c.slot_off, slot_base, c.codes_d, c.start_d, tb["tiles"])

    def run(pattern):
        gs.rearm(pattern)
        with fp.frozen(*inputs, names=["lut", "slot_query", "slot_start", "slot_off", "slot_base", "codes", "list_start", "tiles"]):
            cd.ops.ivf_scan_pqr(lut, tb["slot_query"], tb["slot_start"], c.slot_off, slot_base, c.codes_d, c.start_d, tb["tiles"],
                                gs.view)
            torch.cuda.synchronize()
        gs.assert_guards_intact("scores")                                 # pad floats, gaps and guards keep the poison
        return {"scores": gs.payload()}

    got = fp.assert_fully_written(run)["scores"].cpu().numpy()
    assert len(got) == int(c.mask.sum()) > 0
    sq = tb["slot_query"].cpu().numpy()
    table, sb = lut.cpu().numpy(), slot_base.cpu().numpy()
    want = []
    for s, l in enumerate(c.slot_list):
        rows = c.codes[c.ids[c.start[l]:c.start[l + 1]]]
        want.append(pqr.adc(table[sq[s]:sq[s] + 1], rows, np.full((1, len(rows)), sb[s], dtype=np.float32))[0])
    want = np.concatenate(want)
    assert got.dtype == np.float32 and np.array_equal(got, want)           # fp32 adds in ascending m from the base: bit for bit
