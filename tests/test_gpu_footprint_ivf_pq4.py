"""Write footprint of the three launches of the 4-bit product-quantised IVF lists (include/cdml_ivf_pq4.h) with
tests/footprint.py's poisoned, guarded buffers, under both poison patterns: the encoder writes M whole bytes per row and nothing
of the gap bytes [M, ldc), its 2 M distances only when asked; the lookup tables are exactly nq 2 M 16 floats; the scan stores
every score of every slot row and nothing else -- not the pad floats [len, ld) of a score row, not the gaps between the lists'
blocks, nothing for an empty list or a -1 probe; every input comes back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import ivf_pq4_ref as p4  # noqa: E402
import ivf_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
M, D = 16, 64                            # Ms = 32 subspaces, dsub = 2; S = 16 slots, R = 1024 rows
MS = 2 * M
LENS = (0, 1, 127, 1030, 5, 300, 0)      # one list longer than R
NQ, NPROBE = 40, 3
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
    x = rng.randn(n, D).astype(np.float32)
    q = rng.randn(NQ, D).astype(np.float32)
    cb = rng.randn(MS, 16, D // MS).astype(np.float32)
    assign = np.repeat(np.arange(nlist), LENS)
    rng.shuffle(assign)
    ids, start = ref.lists_from_assign(assign, nlist)
    probe = np.stack([rng.choice(nlist, size=NPROBE, replace=False) for _ in range(NQ)])
    for r in range(30):                                                   # more than S slots on the lists 3 and 5
        probe[r] = [5, 3] + [int(rng.choice([0, 1, 2, 4, 6]))]
    probe[3] = -1
    probe[10:20, 2] = -1
    S, R = cd.ops.ivf_pq4_tile(M)
    assert (S, R) == (16, 1024) and max(LENS) > R and (probe == 5).sum() > S and (probe == -1).any()
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
    codes, dist = p4.encode(x, cb)                                        # unpacked [n, Ms]

    class NS:
        pass
    c = NS()
    c.nlist, c.n, c.x, c.q, c.cb, c.ids, c.start, c.tb, c.slot_list, c.total, c.mask = nlist, n, x, q, cb, ids, start, tb, slot_list, total, mask
    c.codes, c.dist = codes, dist
    c.X, c.Q, c.CB = t(x, torch.float32), t(q, torch.float32), t(cb, torch.float32)
    c.codes_d = t(p4.pack(codes)[ids], torch.uint8)
    c.start_d = t(start, torch.int32)
    c.slot_off = t(slot_off, torch.int64)
    return c


@pytest.mark.parametrize("with_dist", [False, True])
def test_encode_footprint(cd, case, with_dist):
    c = case
    gc = fp.Guarded((c.n, M), torch.uint8, cd.dev, ld=M + 8)
    gd = fp.Guarded((c.n, MS), torch.float32, cd.dev, ld=MS + 4)

    def run(pattern):
        gc.rearm(pattern), gd.rearm(pattern)
        with fp.frozen(c.X, c.CB, names=["x", "codebooks"]):
            cd.ops.pq4_encode(c.X, c.CB, gc.view, gd.view if with_dist else None)
            torch.cuda.synchronize()
        gc.assert_guards_intact("codes")                                  # the gap bytes [M, ldc) keep the poison
        if with_dist:
            gd.assert_guards_intact("dist")
            return {"codes": gc.payload(), "dist": gd.payload()}
        assert bool((fp.bits_of(gd.flat) == fp.poison_scalar(torch.float32, pattern)).all()), "dist written without being given"
        return {"codes": gc.payload()}

    got = fp.assert_fully_written(run)
    codes = p4.unpack(got["codes"].cpu().numpy())
    d = p4.sub_dist(c.x, c.cb)
    chosen = np.take_along_axis(d, codes[:, :, None], 2)[:, :, 0]
    assert (codes == c.codes).mean() > 0.999 and (chosen - d.min(2) <= 2 * p4.encode_bound(D // MS) * chosen).all()
    if with_dist:
        assert np.abs(got["dist"].cpu().double().numpy() - chosen).max() <= 1e-5


def test_lut_footprint(cd, case):
    c = case
    gl = fp.Guarded((NQ * MS * 16,), torch.float32, cd.dev)

    def run(pattern):
        gl.rearm(pattern)
        with fp.frozen(c.Q, c.CB, names=["Q", "codebooks"]):
            cd.ops.pq4_lut(c.Q, c.CB, gl.view)
            torch.cuda.synchronize()
        gl.assert_guards_intact("lut")
        return {"lut": gl.payload()}

    got = fp.assert_fully_written(run)["lut"].cpu().double().numpy().reshape(NQ, MS, 16)
    assert np.abs(got - p4.lut(c.q, c.cb)).max() <= 1e-5


def test_scan_pq4_footprint(cd, case):
    c = case
    tb = c.tb
    lut = torch.empty((NQ, MS, 16), dtype=torch.float32, device=cd.dev)
    cd.ops.pq4_lut(c.Q, c.CB, lut)
    gs = fp.Guarded((c.total,), torch.float32, cd.dev, mask=c.mask)
    inputs = (lut, tb["slot_query"], tb["slot_start"], c.slot_off, c.codes_d, c.start_d, tb["tiles"])

    def run(pattern):
        gs.rearm(pattern)
        with fp.frozen(*inputs, names=["lut", "slot_query", "slot_start", "slot_off", "codes", "list_start", "tiles"]):
            cd.ops.ivf_scan_pq4(lut, tb["slot_query"], tb["slot_start"], c.slot_off, c.codes_d, c.start_d, tb["tiles"], gs.view)
            torch.cuda.synchronize()
        gs.assert_guards_intact("scores")                                 # pad floats, gaps and guards keep the poison
        return {"scores": gs.payload()}

    got = fp.assert_fully_written(run)["scores"].cpu().numpy()
    assert len(got) == int(c.mask.sum()) > 0
    sq = tb["slot_query"].cpu().numpy()
    table = lut.cpu().numpy()
    want = np.concatenate([p4.adc4(table[sq[s]:sq[s] + 1], c.codes[c.ids[c.start[l]:c.start[l + 1]]])[0]
                           for s, l in enumerate(c.slot_list)])
    assert got.dtype == np.float32 and np.array_equal(got, want)           # the pair first, then ascending bytes: bit for bit
