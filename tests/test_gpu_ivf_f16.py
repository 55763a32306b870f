"""The fp16 lists of the IVF index on the MI355X (include/cdml_ivf_f16.h, csrc/ivf_f16.hip, cdml_amd.knn.IVFIndex(storage="f16")):
the scan on the fp16 MFMA bit for bit against the int64 model on exact grids (where rounding is the identity) and within the
project's bound against the fp64 model ON THE ROUNDED VALUES on unit Gaussian rows; the fp32 re-rank bit for bit on the grids
and within the bound against the fp64 direct form, both over the device's own candidate table; a tie below fp16 resolution
that only the re-rank can order; position independence; overflowing rows and queries; the derived condition under which the
re-rank recovers the probed-exact answer; mining through the index.

The Gaussian and the clustered rows are l2-normalised HERE and indexed with l2_norm=False, so that the fp32 values the index
rounds are bit for bit the ones the host model rounds (a second normalisation on the device could move a value across a
rounding boundary: one fp16 ulp, far above TOL)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_f16_ref as f16  # noqa: E402
import ivf_ref as ref  # noqa: E402
from test_gpu_knn import TOL, check  # noqa: E402

pytestmark = pytest.mark.gpu

G_N, G_D, G_NLIST, G_NPROBE, G_K, G_NQ, G_R = 2000, 64, 16, 4, 51, 203, 128


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, hardneg, knn, ops, train
    cdml_amd.load_library()
    assert ops.knn_list_capacity() == xs.LIST

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.hardneg, ns.train, ns.engine, ns.dev = knn, ops, hardneg, train, engine, gpu
    return ns


def _unit32(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- exact grids: the scan and the re-rank, zero tolerance ----------------------------------------------------------------------
@pytest.mark.parametrize("D", ref.GRID_DIMS)
def test_grid_scan_and_rerank_are_the_int64_models_bit_for_bit(cd, D):
    c = ref.grid_case(D)
    assert c["safe"] < 2.0 ** 24
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    assert np.array_equal(f16.quantise(c["x"]).astype(np.float32), c["x"], equal_nan=True)      # rounding is the identity here
    idx = cd.knn.IVFIndex.from_assignment(x, torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]), l2_norm=False, device=cd.dev,
                                          storage="f16")
    ids, start = ref.lists_from_assign(c["assign"], c["nlist"])
    Dp = (D + 31) // 32 * 32
    assert idx.storage == "f16" and idx.rows.dtype == torch.float16 and tuple(idx.rows.shape) == (len(ids), Dp)
    assert idx.n_unlisted == 1 and int(idx.assign[c["nan_row"]]) == -1
    assert torch.equal(idx.ids.cpu().long(), torch.from_numpy(ids)) and torch.equal(idx.list_start.cpu().long(), torch.from_numpy(start))
    assert torch.equal(idx.rows[:, :D].float().cpu(), x[ids]) and bool((idx.rows[:, D:] == 0).all())
    assert torch.equal(idx.r_sq.cpu(), (x[ids].double() ** 2).sum(1).float())
    assert torch.equal(idx.probes(q, ref.GRID_NPROBE).cpu(), torch.from_numpy(c["probe"]))
    base = idx.prepare(x)
    assert tuple(base.shape) == (c["n"], Dp) and base.dtype == torch.float32
    for k in ref.GRID_KS:
        Dw, Iw = ref.grid_want(c, k)
        Dg, Ig = idx.search(q, k, ref.GRID_NPROBE)
        assert Dg.dtype == torch.float32 and Ig.dtype == torch.int64 and tuple(Dg.shape) == (ref.GRID_NQ, k)
        assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
        Dh, Ih = idx.search(q, k, ref.GRID_NPROBE, probe=torch.from_numpy(c["probe_hand"]))
        Dwh, Iwh = ref.grid_want(c, k, probe=c["probe_hand"])
        assert torch.equal(Ih.cpu(), Iwh) and torch.equal(Dh.cpu(), Dwh)
        # the re-rank over the device's own candidate table: integer-exact direct distances
        st = {}
        Dr, Ir = idx.search(q, k, ref.GRID_NPROBE, refine=xs.LIST, base=base, stats=st)
        cand = st["candidates"].cpu().numpy().astype(np.int64)
        assert cand.shape == (ref.GRID_NQ, xs.LIST) and c["nan_row"] not in cand and (cand[ref.GRID_NAN_QUERY] == xs.NO_ID).all()
        Dm, Im = f16.refine(c["qi"], c["xi"], cand, xs.LIST, k)
        assert torch.equal(Ir.cpu(), torch.from_numpy(Im)) and torch.equal(Dr.cpu(), xs.from_units(Dm, c["unit"]))
        # (on the grid d~ = d, and the 128 candidates hold the k best: the refined answer is the scan's)
        assert torch.equal(Ir.cpu(), Iw) and torch.equal(Dr.cpu(), Dw)
    # nprobe = nlist: the exact search's neighbours, bit for bit
    De, Ie = cd.knn.knn_search(x, q, 51, l2_norm=False, device=cd.dev)
    Dg, Ig = idx.search(q, 51, c["nlist"])
    assert torch.equal(Ig, Ie) and torch.equal(Dg, De)


def test_rerank_orders_a_tie_below_fp16_resolution(cd):
    D = 32
    x = np.full((6, D), 0.5, dtype=np.float32)
    x[0, 4] = 0.5 + 2.0 ** -13                                            # the farther row has the lower id
    x[2:] += np.arange(1, 5, dtype=np.float32)[:, None] * 0.25            # four rows far away
    q = np.full((1, D), 0.5, dtype=np.float32)
    assert np.array_equal(f16.quantise(x[0]), f16.quantise(x[1])) and x[0, 4] != x[1, 4]
    idx = cd.knn.IVFIndex.from_assignment(torch.from_numpy(x), torch.zeros(1, D), torch.zeros(6, dtype=torch.int64), l2_norm=False,
                                          device=cd.dev, storage="f16")
    tq = torch.from_numpy(q)
    D0, I0 = idx.search(tq, 2, 1)
    assert I0.cpu().tolist() == [[0, 1]] and D0.cpu().tolist() == [[0.0, 0.0]]            # tied on d~: id order
    base = idx.prepare(torch.from_numpy(x))
    for r in (2, 3, 128):
        Dr, Ir = idx.search(tq, 2, 1, refine=r, base=base)
        assert Ir.cpu().tolist() == [[1, 0]] and Dr.cpu().tolist() == [[0.0, 2.0 ** -26]], r
    Dr, Ir = idx.search(tq, 1, 1, refine=1, base=base)                    # r = 1 keeps the scan's first candidate only
    assert Ir.cpu().tolist() == [[0]] and Dr.cpu().tolist() == [[2.0 ** -26]]


# ---- unit Gaussian rows: the fp64 models on the rounded values / the direct form -------------------------------------------------
@pytest.fixture(scope="module")
def gauss(cd):
    rng = np.random.RandomState(13)
    x = _unit32(rng.randn(G_N, G_D))
    q = np.concatenate([_unit32(rng.randn(G_NQ - 3, G_D)), x[[0, 777, G_N - 1]]])
    tx, tq = torch.from_numpy(x).to(cd.dev), torch.from_numpy(q).to(cd.dev)
    idx = cd.knn.IVFIndex.build(tx, G_NLIST, l2_norm=False, device=cd.dev, storage="f16")
    base = idx.prepare(tx)
    s0, s1 = {}, {}
    D0, I0 = idx.search(tq, G_K, G_NPROBE, stats=s0)
    D1, I1 = idx.search(tq, G_K, G_NPROBE, refine=G_R, base=base, stats=s1)
    torch.cuda.synchronize()

    class NS:
        pass
    g = NS()
    g.x, g.q, g.tx, g.tq, g.idx, g.base, g.s0, g.s1, g.D0, g.I0, g.D1, g.I1 = x, q, tx, tq, idx, base, s0, s1, D0, I0, D1, I1
    g.assign = idx.assign.cpu().numpy()
    g.probe = s0["probe"].cpu().numpy().astype(np.int64)
    g.bytes3 = 4 * s0["n_floats"] // 3 - 4096
    return g


def test_f16_lists_share_the_fp32_index_and_take_half_the_bytes(cd, gauss):
    g = gauss
    f32 = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev)
    assert f32.storage == "f32" and f32.rows.dtype == torch.float32
    for name in ("centroids", "assign", "ids", "list_start"):
        assert torch.equal(getattr(f32, name), getattr(g.idx, name)), name
    assert torch.equal(f32.probes(g.tq, G_NPROBE), g.idx.probes(g.tq, G_NPROBE))
    assert torch.equal(g.idx.probes(g.tq, G_NPROBE).cpu(), torch.from_numpy(g.probe))
    assert g.idx.rows.numel() * g.idx.rows.element_size() * 2 == f32.rows.numel() * f32.rows.element_size()
    assert torch.equal(g.idx.rows, f32.rows.to(torch.float16))
    assert list(f32.state_dict()) == ["centroids", "assign", "l2_norm", "precision", "init_rows", "objective"]
    st = g.idx.state_dict()
    assert st["storage"] == "f16"
    back = cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev)
    assert back.storage == "f16"
    for name in ("centroids", "assign", "ids", "list_start", "rows", "r_sq"):
        assert torch.equal(getattr(back, name), getattr(g.idx, name)), name
    del st["storage"]
    assert cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev).storage == "f32"


def test_gaussian_scan_matches_the_fp64_model_on_the_rounded_values(cd, gauss):
    g = gauss
    st = {}
    Dg, Ig = g.idx.search(g.tq, G_K, G_NPROBE, score_bytes=g.bytes3, stats=st)
    assert len(st["chunks"]) >= 3
    Dr, Ir = f16.scan_search(g.q, g.x, g.assign, G_NLIST, g.probe, G_K)
    dfull = np.maximum(f16.rounded_dist(g.q, g.x), 0.0)
    err = np.abs(Dg.cpu().numpy()[np.isfinite(Dr)] - Dr[np.isfinite(Dr)]).max()
    print("f16 scan: max |d - fp64 model on the rounded values| = %.3g (TOL %.0e)" % (err, TOL))
    check(Dg.cpu().numpy(), Ig.cpu().numpy(), Dr, Ir, dfull)
    assert (Ig[-3:, 0].cpu().numpy() == [0, 777, G_N - 1]).all()           # a catalogue row finds itself


def test_gaussian_rerank_matches_the_fp64_direct_form_on_the_device_candidates(cd, gauss):
    g = gauss
    cand = g.s1["candidates"].cpu().numpy().astype(np.int64)
    assert cand.shape == (G_NQ, G_R)
    # the candidate table is the scan's own list: its first k entries are the refine = 0 answer
    assert np.array_equal(np.where(cand[:, :G_K] == xs.NO_ID, -1, cand[:, :G_K]), g.I0.cpu().numpy())
    table = np.full((G_NQ, xs.LIST), xs.NO_ID, dtype=np.int64)
    table[:, :G_R] = cand
    Dr, Ir = f16.refine(g.q, g.x, table, G_R, G_K)
    dfull = np.maximum(ref.fp64_dist(g.q, g.x, l2_norm=False), 0.0)
    err = np.abs(g.D1.cpu().numpy()[np.isfinite(Dr)] - Dr[np.isfinite(Dr)]).max()
    print("re-rank: max |d - fp64 direct form| = %.3g (TOL %.0e)" % (err, TOL))
    check(g.D1.cpu().numpy(), g.I1.cpu().numpy(), Dr, Ir, dfull)
    assert (g.D1[-3:, 0] == 0).all() and (g.I1[-3:, 0].cpu().numpy() == [0, 777, G_N - 1]).all()


@pytest.mark.parametrize("refine", [0, G_R])
def test_position_independence(cd, gauss, refine):
    g = gauss
    kw = dict(refine=refine, base=g.base) if refine else {}
    want_d, want_i = (g.D1, g.I1) if refine else (g.D0, g.I0)
    assert len(g.s0["chunks"]) == 1 and len(g.s1["chunks"]) == 1
    st = {}
    D2, I2 = g.idx.search(g.tq, G_K, G_NPROBE, score_bytes=g.bytes3, stats=st, **kw)
    assert len(st["chunks"]) >= 3 and st["n_floats"] == g.s0["n_floats"]
    assert torch.equal(D2, want_d) and torch.equal(I2, want_i)
    perm = torch.from_numpy(np.random.RandomState(5).permutation(G_NQ)).to(cd.dev)
    D3, I3 = g.idx.search(g.tq[perm], G_K, G_NPROBE, score_bytes=4 * g.s0["n_floats"] // 2, **kw)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(G_NQ, device=cd.dev)
    assert torch.equal(D3[inv], want_d) and torch.equal(I3[inv], want_i)


def test_overflowing_row_and_query(cd):
    rng = np.random.RandomState(17)
    n, D, nlist, nq, k = 400, 32, 4, 20, 10
    x, q = _unit32(rng.randn(n, D)), _unit32(rng.randn(nq, D))
    cent = _unit32(rng.randn(nlist, D))
    assign = rng.randint(0, nlist, size=n)
    probe = np.stack([rng.permutation(nlist)[:2] for _ in range(nq)])
    mk = lambda rows: cd.knn.IVFIndex.from_assignment(torch.from_numpy(rows), torch.from_numpy(cent), torch.from_numpy(assign),
                                                      l2_norm=False, device=cd.dev, storage="f16")
    clean = mk(x)
    Dc, Ic = clean.search(torch.from_numpy(q), k, 2, probe=torch.from_numpy(probe))
    big = int(Ic[0, 0])                                                   # query 0's nearest row overflows ...
    x2, q2 = x.copy(), q.copy()
    x2[big, 5] = 1e5
    q2[7, 2] = 1e5                                                        # ... and so does query 7
    hit = mk(x2)
    assert clean.n_unlisted == 0 and hit.n_unlisted == 1 and int(hit.assign[big]) == -1 and hit.n_listed == n - 1
    f32 = cd.knn.IVFIndex.from_assignment(torch.from_numpy(x2), torch.from_numpy(cent), torch.from_numpy(assign), l2_norm=False,
                                          device=cd.dev)
    assert f32.n_unlisted == 0                                            # (finite in fp32: listed there)
    assert bool(torch.isfinite(hit.rows).all())
    st = {}
    Dh, Ih = hit.search(torch.from_numpy(q2), k, 2, probe=torch.from_numpy(probe), stats=st)
    assert (Ih[7] == -1).all() and bool(torch.isinf(Dh[7]).all()) and (st["probe"][7] == -1).all()
    assert big not in Ih.cpu().numpy()
    Dr, Ir = f16.scan_search(q2, x2, assign, nlist, probe, k)
    assert (Ir[7] == -1).all() and big not in Ir
    dfull = np.maximum(np.nan_to_num(f16.rounded_dist(q2, x2), nan=np.inf), 0.0)
    check(Dh.cpu().numpy(), Ih.cpu().numpy(), Dr, Ir, dfull)
    # the neighbours are unaffected: every other query that did not have the row keeps its answer bit for bit
    keep = [i for i in range(nq) if i != 7 and big not in Ic[i].cpu().numpy()]
    assert len(keep) >= nq // 2 and torch.equal(Ih[keep], Ic[keep]) and torch.equal(Dh[keep], Dc[keep])
    # and with the re-rank: the lost query still finds nothing, the unlisted row is still nobody's neighbour
    base = hit.prepare(torch.from_numpy(x2))
    D2, I2 = hit.search(torch.from_numpy(q2), k, 2, probe=torch.from_numpy(probe), refine=32, base=base)
    assert (I2[7] == -1).all() and bool(torch.isinf(D2[7]).all()) and big not in I2.cpu().numpy()
    # the default probes of such a query are real lists (the coarse search is fp32): the fp16 scan is what drops it
    assert (hit.probes(torch.from_numpy(q2), 2)[7] >= 0).all()
    D3, I3 = hit.search(torch.from_numpy(q2), k, 2)
    assert (I3[7] == -1).all() and bool(torch.isinf(D3[7]).all())


# ---- recovery of the probed-exact answer under the derived condition ------------------------------------------------------------
def test_rerank_recovers_the_exact_answer_where_the_gap_allows(cd):
    """64 clusters x 16 unit rows, D = 32, within-cluster noise 0.02; nlist = 16, nprobe = 4, k = 8, r = 32.  E = 2^-8 + 2^-20
    (ivf_f16_ref.rounding_bound).  A query whose (r + 1)-th true probed distance exceeds its k-th by more than 2 E + 4 TOL has
    its whole true top k among the r candidates: a row of the true top k has d~ <= d_k + E (+ TOL on the device), a row
    outside the true top r has d~ >= d_(r+1) - E (- TOL), so at most r - k rows can come before it.  Then the refined ids
    are the fp64 probed-exact ids, up to near-ties of the fp32 direct form (``check``).  Measured on an MI355X: every query
    meets the condition; the ids are the probed-exact ones for 0.785 of the queries at refine = 0 and for all at refine = 32."""
    x, q = f16.recovery_fixture()
    nlist, nprobe, k, r = 16, 4, 8, 32
    tx, tq = torch.from_numpy(x).to(cd.dev), torch.from_numpy(q).to(cd.dev)
    idx = cd.knn.IVFIndex.build(tx, nlist, l2_norm=False, device=cd.dev, storage="f16")
    st = {}
    Dg, Ig = idx.search(tq, k, nprobe, refine=r, base=idx.prepare(tx), stats=st)
    D0, I0 = idx.search(tq, k, nprobe)
    probe = st["probe"].cpu().numpy().astype(np.int64)
    assign = idx.assign.cpu().numpy()
    d_true = f16.direct_dist(q, x)
    ok = f16.recoverable(d_true, probe, assign, nlist, k, r, TOL)
    Dr, Ir = ref.search(d_true, assign, nlist, probe, k)
    Dg, Ig, I0 = Dg.cpu().numpy(), Ig.cpu().numpy(), I0.cpu().numpy()
    print("recoverable share %.4f; ids equal to the probed-exact ones: refine=0 %.4f, refine=%d %.4f"
          % (ok.mean(), (I0 == Ir).all(1).mean(), r, (Ig == Ir).all(1).mean()))
    assert ok.mean() >= 0.9
    check(Dg[ok], Ig[ok], Dr[ok], Ir[ok], d_true[ok])


# ---- mining ----------------------------------------------------------------------------------------------------------------------
def test_mining_through_the_f16_index(cd):
    rng = np.random.RandomState(9)
    n, D, k, skip, nlist, nprobe, r = 3000, 64, 16, 2, 16, 4, 64
    e = torch.from_numpy(rng.randn(n, D).astype(np.float32)).to(cd.dev)
    a = rng.randint(0, n, size=500)
    pairs = torch.from_numpy(np.stack([a, (a + 1 + rng.randint(0, n - 1, size=500)) % n], 1).astype(np.int32))
    for refine in (0, r):
        lists = cd.hardneg.mine_lists(e, k, skip, pairs, device=cd.dev, nlist=nlist, nprobe=nprobe, storage="f16", refine=refine)
        idx = cd.knn.IVFIndex.build(e, nlist, iters=10, seed=0, device=cd.dev, storage="f16")
        _, I = idx.search(e, k + skip + 1, nprobe, refine=refine, base=idx.prepare(e) if refine else None)
        assert torch.equal(lists, cd.hardneg.filter_lists(I, k, skip, pairs))
        assert tuple(lists.shape) == (n, 16) and lists.dtype == torch.int32 and (lists >= 0).float().mean().item() > 0.9
        L = lists.cpu().numpy().astype(np.int64)
        rows = np.arange(n)[:, None]
        assert (L != rows).all()                                          # the row itself is dropped ...
        partner = set(map(tuple, pairs.numpy().tolist())) | set((b_, a_) for a_, b_ in pairs.numpy().tolist())
        ii, jj = np.nonzero(L >= 0)
        assert not set(zip(ii.tolist(), L[ii, jj].tolist())) & partner    # ... and its partners
        valid = L >= 0
        assert (valid[:, :-1] | ~valid[:, 1:]).all()                      # left-packed
        assert all(len(set(row[row >= 0])) == (row >= 0).sum() for row in L)
        # skip_top: with the re-rank the self row is first (d = 0 exactly), and the skip nearest behind it are not listed
        if refine:
            assert (I[:, 0].cpu().numpy() == np.arange(n)).all()
            assert not (L[:, :, None] == I[:, 1:1 + skip].cpu().numpy()[:, None, :]).any()


def test_train_step_refreshes_its_lists_through_the_f16_index(cd):
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
    lists = ts.refresh_negative_lists(16, nlist=16, nprobe=4, storage="f16", refine=32)
    assert tuple(lists.shape) == (N, 16) and (lists >= 0).float().mean().item() > 0.5
    L = lists.cpu().numpy()
    assert (L != np.arange(N)[:, None]).all()
    ts.step()
    torch.cuda.synchronize()
    assert ts.hard_share() > 0 and np.isfinite(ts.loss())
