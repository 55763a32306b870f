"""The IVF index on the MI355X (include/cdml_ivf.h, csrc/ivf.hip, cdml_amd.knn.IVFIndex): the probed scan bit for bit against
the int64 model of tests/ivf_ref.py on exact grids, within the project's fp32-MFMA bound against the fp64 model on Gaussian
rows, position independence, the invariants of the k-means build, recall and pruning on a clustered catalogue, and mining
through the index."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_ref as ref  # noqa: E402
from test_gpu_knn import TOL, check  # noqa: E402

pytestmark = pytest.mark.gpu

G_N, G_D, G_NLIST, G_NPROBE, G_K, G_NQ = 20000, 256, 64, 8, 51, 400
G_NAN_ROW = 1234


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import hardneg, knn, ops, train, engine
    cdml_amd.load_library()
    assert ops.knn_list_capacity() == xs.LIST

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.hardneg, ns.train, ns.engine, ns.dev = knn, ops, hardneg, train, engine, gpu
    return ns


def _unit64(x):
    x = np.asarray(x, np.float32).astype(np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-6)


# ---- 1. exact grid, zero tolerance (and 3. nprobe = nlist on the grid) -------------------------------------------------------
@pytest.mark.parametrize("D", ref.GRID_DIMS)
def test_grid_search_is_the_int64_model_bit_for_bit(cd, D):
    c = ref.grid_case(D)
    assert c["safe"] < 2.0 ** 24                                          # assert_select_exact_safe, recorded by the case
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    idx = cd.knn.IVFIndex.from_assignment(x, torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]), l2_norm=False, device=cd.dev)
    ids, start = ref.lists_from_assign(c["assign"], c["nlist"])
    assert idx.n_unlisted == 1 and int(idx.assign[c["nan_row"]]) == -1
    assert torch.equal(idx.ids.cpu().long(), torch.from_numpy(ids)) and torch.equal(idx.list_start.cpu().long(), torch.from_numpy(start))
    assert tuple(idx.rows.shape) == (len(ids), (D + 31) // 32 * 32) and torch.equal(idx.rows[:, :D].cpu(), x[ids])
    assert torch.equal(idx.probes(q, ref.GRID_NPROBE).cpu(), torch.from_numpy(c["probe"]))
    hand = torch.from_numpy(c["probe_hand"])
    for k in ref.GRID_KS:
        Dg, Ig = idx.search(q, k, ref.GRID_NPROBE)
        Dw, Iw = ref.grid_want(c, k)
        assert Dg.dtype == torch.float32 and Ig.dtype == torch.int64 and tuple(Dg.shape) == (ref.GRID_NQ, k)
        assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
        # a hand-made probe table: finite queries with -1 probes
        Dg, Ig = idx.search(q, k, ref.GRID_NPROBE, probe=hand)
        Dw, Iw = ref.grid_want(c, k, probe=c["probe_hand"])
        assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
    # nprobe = nlist: knn_search's neighbours (the NaN row nobody's neighbour, the NaN query empty), bit for bit
    for k in ref.GRID_KS:
        De, Ie = cd.knn.knn_search(x, q, k, l2_norm=False, device=cd.dev)
        Dg, Ig = idx.search(q, k, c["nlist"])
        assert torch.equal(Ig, Ie) and torch.equal(Dg, De)
    # the clamp: |x|^2 lowered for three rows (the merge only reads it), raw distances negative
    idx.r_sq.copy_(torch.from_numpy(c["r_low"])[ids].to(cd.dev))
    for k in ref.GRID_KS:
        Dg, Ig = idx.search(q, k, ref.GRID_NPROBE)
        Dw, Iw = ref.grid_want(c, k, low=True)
        assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)


# ---- the Gaussian index: tests 2 - 5 share it ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss(cd):
    rng = np.random.RandomState(11)
    base = rng.randn(G_N, G_D).astype(np.float32)
    base[G_NAN_ROW, 7] = np.nan
    q = np.concatenate([rng.randn(G_NQ - 3, G_D).astype(np.float32), base[[0, 5000, G_N - 1]]])
    tb, tq = torch.from_numpy(base).to(cd.dev), torch.from_numpy(q).to(cd.dev)
    idx = cd.knn.IVFIndex.build(tb, G_NLIST, device=cd.dev)
    stats = {}
    Dg, Ig = idx.search(tq, G_K, G_NPROBE, stats=stats)
    probe = idx.probes(tq, G_NPROBE)
    torch.cuda.synchronize()
    b64 = _unit64(base)
    d = ref.fp64_dist(q, base)                                            # [nq, n] unclamped; NaN in the NaN row's column

    class NS:
        pass
    g = NS()
    g.base, g.q, g.tb, g.tq, g.idx, g.D, g.I, g.probe, g.stats, g.b64, g.d = base, q, tb, tq, idx, Dg, Ig, probe, stats, b64, d
    g.dfull = np.maximum(np.nan_to_num(d, nan=np.inf), 0.0)
    g.assign = idx.assign.cpu().numpy()
    return g


def test_gaussian_search_matches_the_fp64_model_on_the_device_probes(cd, gauss):
    g = gauss
    probe = g.probe.cpu().numpy()
    assert np.array_equal(g.stats["probe"].cpu().numpy(), probe)
    Dr, Ir = ref.search(g.d, g.assign, G_NLIST, probe, G_K)
    check(g.D.cpu().numpy(), g.I.cpu().numpy(), Dr, Ir, g.dfull)
    assert (g.I[-3:, 0].cpu().numpy() == [0, 5000, G_N - 1]).all()          # a catalogue row finds itself
    # the probe table against fp64: where a probe set differs, the centroids in question lie within 2 TOL of the nprobe-th distance
    C = g.idx.centroids.cpu().double().numpy()
    qn = _unit64(g.q)
    dc = (qn * qn).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * qn @ C.T
    want = ref.probes(dc, G_NPROBE)
    for r in range(G_NQ):
        diff = set(probe[r]) ^ set(want[r])
        kth = np.sort(dc[r])[G_NPROBE - 1]
        assert all(abs(dc[r, c] - kth) <= 2 * TOL for c in diff), (r, diff)


def test_nprobe_nlist_returns_the_exact_neighbours(cd, gauss):
    g = gauss
    allp = np.tile(np.arange(G_NLIST), (G_NQ, 1))
    Dr, Ir = ref.search(g.d, g.assign, G_NLIST, allp, G_K)                 # the exact kNN over the listed (finite) rows
    Dg, Ig = g.idx.search(g.tq, G_K, G_NLIST)
    check(Dg.cpu().numpy(), Ig.cpu().numpy(), Dr, Ir, g.dfull)
    De, Ie = cd.knn.knn_search(g.tb, g.tq, G_K, device=cd.dev)
    check(De.cpu().numpy(), Ie.cpu().numpy(), Dr, Ir, g.dfull)
    assert (Ig == Ie).float().mean().item() > 0.99                        # (swaps only among near-ties of the two arithmetics)


def test_position_independence(cd, gauss):
    g = gauss
    costs_total = 4 * g.stats["n_floats"]
    assert len(g.stats["chunks"]) == 1
    st = {}
    D2, I2 = g.idx.search(g.tq, G_K, G_NPROBE, score_bytes=costs_total // 3 - 4096, stats=st)
    assert len(st["chunks"]) >= 3 and st["n_floats"] == g.stats["n_floats"]
    assert torch.equal(D2, g.D) and torch.equal(I2, g.I)
    perm = torch.from_numpy(np.random.RandomState(5).permutation(G_NQ)).to(cd.dev)
    D3, I3 = g.idx.search(g.tq[perm], G_K, G_NPROBE, score_bytes=costs_total // 2)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(G_NQ, device=cd.dev)
    assert torch.equal(D3[inv], g.D) and torch.equal(I3[inv], g.I)


def test_build_invariants(cd, gauss):
    g, idx = gauss, gauss.idx
    n = G_N
    finite = np.setdiff1d(np.arange(n), [G_NAN_ROW])
    ids, start = idx.ids.cpu().numpy(), idx.list_start.cpu().numpy()
    assert idx.n_unlisted == 1 and g.assign[G_NAN_ROW] == -1 and G_NAN_ROW not in ids
    assert np.array_equal(np.sort(ids), finite)                           # every finite row in exactly one list
    assert np.array_equal(g.assign[ids], np.repeat(np.arange(G_NLIST), np.diff(start)))
    inner = np.ones(len(ids) - 1, dtype=bool)
    inner[start[1:-1][(start[1:-1] > 0) & (start[1:-1] < len(ids))] - 1] = False
    assert (np.diff(ids)[inner] > 0).all()                                # ids ascend inside a list
    assert torch.equal(idx.probes(g.tb, 1)[:, 0], idx.assign)
    obj = idx.objective.numpy()
    assert obj.dtype == np.float64 and len(obj) == 10 and (obj[1:] <= obj[:-1] + n * TOL).all()
    assert len(idx.init_rows) == G_NLIST and len(idx.train_ids) == min(n - 1, 256 * G_NLIST)
    # two builds from the same seed are bit-identical; a reload re-derives the lists bit for bit
    again = cd.knn.IVFIndex.build(g.tb, G_NLIST, device=cd.dev)
    for name in ("centroids", "assign", "ids", "list_start", "rows", "r_sq"):
        assert torch.equal(getattr(again, name), getattr(idx, name)), name
    assert torch.equal(again.objective, idx.objective) and torch.equal(again.init_rows, idx.init_rows)
    back = cd.knn.IVFIndex.load_state_dict(idx.state_dict(), g.tb, device=cd.dev)
    for name in ("centroids", "assign", "ids", "list_start", "rows", "r_sq"):
        assert torch.equal(getattr(back, name), getattr(idx, name)), name
    # the centroids are the means of the LAST update's lists: the assignment of a build with one iteration less, on the
    # training rows.  |c - fp64 mean| <= L 2^-24 mean|x| per column: the worst case of an L-term fp32 sum in any order
    # plus the division; computed here, not fixed
    prev = cd.knn.IVFIndex.build(g.tb, G_NLIST, iters=9, device=cd.dev)
    assert torch.equal(prev.train_ids, idx.train_ids)
    tr = idx.train_ids.numpy()
    a_prev = prev.assign.cpu().numpy()[tr]
    X = torch.zeros((n, G_D), dtype=torch.float32, device=cd.dev)
    X[torch.from_numpy(ids).long().to(cd.dev)] = idx.rows[:, :G_D]        # the normalised rows the build worked on
    xt = X.cpu().double().numpy()[tr]
    C, Cprev = idx.centroids.cpu().numpy(), prev.centroids.cpu().numpy()
    seen = 0
    for c in range(G_NLIST):
        m = a_prev == c
        L = int(m.sum())
        if L == 0:
            assert np.array_equal(C[c], Cprev[c])                         # an empty list keeps its centroid
            continue
        bound = L * 2.0 ** -24 * np.abs(xt[m]).mean(0)
        assert (np.abs(C[c].astype(np.float64) - xt[m].mean(0)) <= bound).all(), c
        seen += 1
    assert seen >= G_NLIST // 2


def test_centroid_means_are_bit_exact_on_the_grid(cd):
    rng = np.random.RandomState(8)
    lens = [1, 2, 0, 64, 256, 8, 0]                                       # powers of two (and empty lists)
    n, D = sum(lens), 80
    xi = xs.grid_rows(n, D, rng)
    assign = np.repeat(np.arange(len(lens)), lens)
    rng.shuffle(assign)
    ids, start = ref.lists_from_assign(assign, len(lens))
    x = torch.zeros((n, 96), dtype=torch.float32, device=cd.dev)
    x[:, :D] = torch.from_numpy(xi * xs.PIPE_UNIT).float().to(cd.dev)
    cent = torch.full((len(lens), 96), 7.0, dtype=torch.float32, device=cd.dev)
    cd.ops.ivf_centroid_sums(x, torch.from_numpy(ids).to(torch.int32).to(cd.dev), torch.from_numpy(start).to(torch.int32).to(cd.dev),
                             cent, D)
    want = ref.column_means(xi * xs.PIPE_UNIT, assign, len(lens), keep=np.full((len(lens), D), 7.0))
    assert np.array_equal(cent[:, :D].cpu().double().numpy(), want)
    assert bool((cent[:, D:] == 7.0).all())                               # columns >= D are not written


# ---- 6. it finds neighbours and it prunes ---------------------------------------------------------------------------------------
def test_recall_and_pruning_on_a_clustered_catalogue(cd):
    """512 centres x 8 rows, noise 0.05, D = 64, shuffled; nlist = 64, iters = 10, nprobe = 4, k = 8.  Measured on an MI355X:
    recall@8 1.0000 on the device and 1.0000 for the numpy Lloyd model from the same init_rows, scanned share 1.153 x nprobe /
    nlist, max / mean list 2.00, no empty list."""
    rng = np.random.RandomState(6)
    K, per, D, nlist, nprobe, k = 512, 8, 64, 64, 4, 8
    centres = rng.randn(K, D)
    x = (np.repeat(centres, per, axis=0) + 0.05 * rng.randn(K * per, D)).astype(np.float32)
    x = x[rng.permutation(len(x))]
    tx = torch.from_numpy(x).to(cd.dev)
    idx = cd.knn.IVFIndex.build(tx, nlist, iters=10, device=cd.dev)
    st = {}
    _, Ig = idx.search(tx, k, nprobe, stats=st)
    _, Ie = cd.knn.knn_search(tx, tx, k, device=cd.dev)
    Ie = Ie.cpu().numpy()
    got = ref.recall(Ig.cpu().numpy(), Ie)
    # the numpy Lloyd model from the same init_rows (fp64), its probes and its search
    xn = _unit64(x)
    C, a, _ = ref.lloyd(xn, idx.init_rows.numpy(), 10)
    dc = (xn * xn).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * xn @ C.T
    _, Im = ref.search(ref.fp64_dist(x, x), a, nlist, ref.probes(dc, nprobe), k)
    model = ref.recall(Im, Ie)
    share = idx.scanned_share(st["probe"])
    lens = np.diff(idx.list_start.cpu().numpy())
    print("recall@%d: device %.4f, numpy Lloyd model %.4f; scanned share %.3f x nprobe / nlist; max / mean list %.2f; empty lists %d"
          % (k, got, model, share * nlist / nprobe, lens.max() / lens.mean(), int((lens == 0).sum())))
    assert got >= model - 0.01
    assert share <= 1.5 * nprobe / nlist                                  # a condition: a degenerate clustering passes everything else


# ---- 7. mining ----------------------------------------------------------------------------------------------------------------
def test_mining_through_the_index(cd):
    rng = np.random.RandomState(9)
    n, D, k, skip, nlist, nprobe = 3000, 64, 16, 2, 16, 4
    e = torch.from_numpy(rng.randn(n, D).astype(np.float32)).to(cd.dev)
    a = rng.randint(0, n, size=500)
    pairs = torch.from_numpy(np.stack([a, (a + 1 + rng.randint(0, n - 1, size=500)) % n], 1).astype(np.int32))
    lists = cd.hardneg.mine_lists(e, k, skip, pairs, device=cd.dev, nlist=nlist, nprobe=nprobe)
    idx = cd.knn.IVFIndex.build(e, nlist, iters=10, seed=0, device=cd.dev)
    _, I = idx.search(e, k + skip + 1, nprobe)
    assert torch.equal(lists, cd.hardneg.filter_lists(I, k, skip, pairs))
    assert tuple(lists.shape) == (n, 16) and lists.dtype == torch.int32 and (lists >= 0).float().mean().item() > 0.9
    # on the grid (unit rows: the normalisation returns them bit for bit) at nprobe = nlist: the exact lists
    c = xs.unit_rows_case()
    b = torch.from_numpy(c["b"]).to(cd.dev)
    exact = cd.hardneg.mine_lists(b, 20, 3, None, device=cd.dev)
    assert torch.equal(cd.hardneg.mine_lists(b, 20, 3, None, device=cd.dev, nlist=8, nprobe=8), exact)


def test_train_step_refreshes_its_lists_through_the_index(cd):
    rng = np.random.default_rng(21)
    K, per, F = 250, 8, 96
    N = K * per
    cid = np.repeat(np.arange(K), per)
    feats = (rng.standard_normal((K, F))[cid] + 1.2 * rng.standard_normal((N, F))).astype(np.float32)
    a = rng.integers(0, N, 4000)
    p = (a // per) * per + rng.integers(0, per, 4000)
    pairs = np.stack([a, p], 1)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]].astype(np.int32)
    table = cd.engine.FeatureTable.from_numpy(feats, cd.dev)
    ts = cd.train.TrainStep(table, torch.as_tensor(pairs).to(cd.dev), 256, hidden_size=512, output_size=64, mode="uniform",
                            optimizer="adam", base_learning_rate=0.003, device=cd.dev,
                            negative_lists=cd.hardneg.empty_lists(N, 16), hard_fraction=1.0)
    ts.step()
    assert ts.hard_share() == 0.0                                         # empty lists: every draw falls through
    lists = ts.refresh_negative_lists(16, nlist=16, nprobe=4)
    assert tuple(lists.shape) == (N, 16) and (lists >= 0).float().mean().item() > 0.5
    ts.step()
    torch.cuda.synchronize()
    assert ts.hard_share() > 0 and np.isfinite(ts.loss())
