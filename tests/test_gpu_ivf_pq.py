"""The product-quantised lists of the IVF index on the MI355X (include/cdml_ivf_pq.h, csrc/ivf_pq.hip,
cdml_amd.knn.IVFIndex(storage="pq")): the encoder, the lookup tables and the ADC scan bit for bit against the int64 models on
exact grids (lossless rows: the f32 index's search and the exact search; lossy rows with planted encode ties: the model on the
decoded rows, the re-rank over the device's own candidates), the scan's tile edges, unit Gaussian rows against the fp64
models, position independence, the deterministic training, the derived recovery condition, the refusals from the device-side
call sites, ``ivf_knn`` and ``export``.

The Gaussian rows are l2-normalised HERE and indexed with l2_norm=False, so that the fp32 values the index encodes are bit
for bit the ones the host model encodes."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402
import ivf_f16_ref as f16  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_ref as ref  # noqa: E402
from test_gpu_knn import TOL, check  # noqa: E402

pytestmark = pytest.mark.gpu

G_N, G_D, G_NLIST, G_NPROBE, G_K, G_NQ, G_R = 2000, 64, 16, 4, 51, 203, 128
LOSSLESS = ((48, 8), (48, 32), (256, 32), (256, 64))
LOSSY = ((48, 8), (256, 64))


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import hardneg, knn, ops
    cdml_amd.load_library()
    assert ops.knn_list_capacity() == xs.LIST

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.hardneg, ns.dev = knn, ops, hardneg, gpu
    return ns


def _unit32(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _index(cd, c, storage="pq"):
    kw = {"codebooks": torch.from_numpy(c["cb"])} if storage == "pq" else {}
    return cd.knn.IVFIndex.from_assignment(torch.from_numpy(c["x"]), torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]),
                                           l2_norm=False, device=cd.dev, storage=storage, **kw)


def _check_lists(c, idx):
    ids, start = ref.lists_from_assign(c["assign"], c["nlist"])
    assert idx.storage == "pq" and idx.pq_m == c["M"] and not hasattr(idx, "rows")
    assert idx.codes.dtype == torch.uint8 and tuple(idx.codes.shape) == (len(ids), c["M"]) and idx.codes.is_contiguous()
    assert idx.n_unlisted == 1 and int(idx.assign[c["nan_row"]]) == -1
    assert torch.equal(idx.ids.cpu().long(), torch.from_numpy(ids)) and torch.equal(idx.list_start.cpu().long(), torch.from_numpy(start))
    assert torch.equal(idx.codes.cpu().long(), torch.from_numpy(c["codes"][ids]))                  # the model's codes, bit for bit
    dec = idx.decode(torch.arange(len(ids)))
    assert dec.dtype == torch.float32 and tuple(dec.shape) == (len(ids), c["Dp"])
    assert torch.equal(dec.cpu(), torch.from_numpy((c["xhi"][ids] * xs.PIPE_UNIT).astype(np.float32)))
    assert torch.equal(idx.r_sq.cpu(), torch.from_numpy(((c["xhi"][ids] ** 2).sum(1) * c["unit"]).astype(np.float32)))
    return ids


# ---- exact grids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", LOSSLESS)
def test_lossless_grid_is_the_f32_index_bit_for_bit(cd, D, M):
    c = pq.lossless_case(D, M)
    assert c["safe"] < 2.0 ** 24
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    idx = _index(cd, c)
    ids = _check_lists(c, idx)
    assert torch.equal(idx.decode(torch.arange(len(ids)))[:, :D].cpu(), x[ids])                    # decode equals the rows
    f32 = _index(cd, c, "f32")
    assert torch.equal(idx.probes(q, ref.GRID_NPROBE).cpu(), torch.from_numpy(c["probe"]))
    base = idx.prepare(x)
    hand = torch.from_numpy(c["probe_hand"])
    for k in ref.GRID_KS:
        for probe, pk in ((c["probe_hand"], dict(probe=hand)), (None, {})):
            Dw, Iw = pq.grid_want(c, k, probe=probe)
            Dm, Im = ref.search(c["d"], c["assign"], c["nlist"], c["probe"] if probe is None else probe, k, bad_queries=c["bad_queries"])
            assert torch.equal(Iw, torch.from_numpy(Im))                                           # (lossless: the models agree)
            Dg, Ig = idx.search(q, k, ref.GRID_NPROBE, **pk)
            assert Dg.dtype == torch.float32 and Ig.dtype == torch.int64 and tuple(Dg.shape) == (ref.GRID_NQ, k)
            assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
            Df, If = f32.search(q, k, ref.GRID_NPROBE, **pk)
            assert torch.equal(Ig, If) and torch.equal(Dg, Df)
            Dr, Ir = idx.search(q, k, ref.GRID_NPROBE, refine=xs.LIST, base=base, **pk)
            assert torch.equal(Ir.cpu(), Iw) and torch.equal(Dr.cpu(), Dw)
    De, Ie = cd.knn.knn_search(x, q, 51, l2_norm=False, device=cd.dev)
    Dg, Ig = idx.search(q, 51, c["nlist"])
    assert torch.equal(Ig, Ie) and torch.equal(Dg, De)


@pytest.mark.parametrize("D,M", LOSSY)
def test_lossy_grid_codes_search_and_rerank_bit_for_bit(cd, D, M):
    c = pq.lossy_case(D, M)
    assert c["safe"] < 2.0 ** 24 and len(c["tie_rows"]) == pq.LOSSY_TIES
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    idx = _index(cd, c)
    ids = _check_lists(c, idx)
    pos = {int(r): i for i, r in enumerate(ids)}
    for r, m, lo, hi in c["tie_rows"]:                                    # the planted ties went to the lower code
        assert int(idx.codes[pos[r], m]) == c["codes"][r, m] <= lo < hi
    base = idx.prepare(x)
    for k in ref.GRID_KS:
        Dw, Iw = pq.grid_want(c, k)
        Dg, Ig = idx.search(q, k, ref.GRID_NPROBE)
        assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
        Dh, Ih = idx.search(q, k, ref.GRID_NPROBE, probe=torch.from_numpy(c["probe_hand"]))
        Dwh, Iwh = pq.grid_want(c, k, probe=c["probe_hand"])
        assert torch.equal(Ih.cpu(), Iwh) and torch.equal(Dh.cpu(), Dwh)
        st = {}
        Dr, Ir = idx.search(q, k, ref.GRID_NPROBE, refine=xs.LIST, base=base, stats=st)
        cand = st["candidates"].cpu().numpy().astype(np.int64)
        assert cand.shape == (ref.GRID_NQ, xs.LIST) and c["nan_row"] not in cand and (cand[ref.GRID_NAN_QUERY] == xs.NO_ID).all()
        assert np.array_equal(np.where(cand[:, :k] == xs.NO_ID, -1, cand[:, :k]), Iw.numpy())
        Dm, Im = f16.refine(c["qi"], c["xi"], cand, xs.LIST, k)
        assert torch.equal(Ir.cpu(), torch.from_numpy(Im)) and torch.equal(Dr.cpu(), xs.from_units(Dm, c["unit"]))
    Iw = pq.grid_want(c, 51)[1]
    assert not torch.equal(Iw, ref.grid_want(ref.grid_case(D), 51)[1])                             # (lossy indeed)


# ---- tile edges ----------------------------------------------------------------------------------------------------------------------
# every instance of the scan (M / 8 = 1..8); D = lcm(2 M, 32): M (8 bits) and 2 M (4 bits) divide the padded width, dsub is 1, 2 or 4
TILE_MS = list(range(8, 72, 8))


def tile_dim(M):
    return math.lcm(2 * M, 32)


@pytest.mark.parametrize("M", TILE_MS)
def test_tile_edges(cd, M):
    """list lengths 0, 1, R - 1, R, R + 1, 2 R + 5 and lists probed by S - 1, S and S + 1 queries, against the int64 model"""
    S, R = cd.ops.ivf_pq_tile(M)
    assert (S, R) == (64 // M, 1024)
    D = tile_dim(M)
    dsub = D // M
    lens = (0, 1, R - 1, R, R + 1, 2 * R + 5)
    nlist, n = len(lens), sum(lens)
    rng = xg.case_rng("ivfpq-tiles", M)
    assign = np.repeat(np.arange(nlist), lens)
    rng.shuffle(assign)
    xi = xs.grid_rows(n, D, rng)
    cbi = np.stack([pq._distinct_codewords(rng, dsub, dsub)[0] for _ in range(M)])
    codes, _ = pq.encode(xi, cbi)
    xh = pq.decode(codes, cbi)
    # queries: list 5 (three row tiles) is probed by S + 1 of them, list 4 by S, list 3 by S - 1, the others by a few
    # and one first query that probes lists 1 and 5 (list 5: S + 2 with it, S + 1 without)
    groups = [(5, S + 1), (4, S), (3, S - 1), (2, 3), (1, 2), (0, 2)]
    probe = [[1, 5]] + [[a, -1] for a, cnt in groups for _ in range(cnt)]
    probe[-1] = [0, 2]
    probe = np.asarray(probe, dtype=np.int64)
    nq = len(probe)
    qi = xs.grid_rows(nq, D, rng)
    u = xs.PIPE_UNIT
    unit = u * u
    q, xd = qi * u, xh * u
    assert xs.assert_select_exact_safe((q * q).sum(1), (xd * xd).sum(1), unit, [q], [xd], xg.PAIRS1) < 2.0 ** 24
    cent = np.zeros((nlist, D), dtype=np.float32)
    idx = cd.knn.IVFIndex.from_assignment(torch.from_numpy((xi * u).astype(np.float32)), torch.from_numpy(cent),
                                          torch.from_numpy(assign), l2_norm=False, device=cd.dev, storage="pq",
                                          codebooks=torch.from_numpy((cbi * u).astype(np.float32)))
    ids, _ = ref.lists_from_assign(assign, nlist)
    assert torch.equal(idx.codes.cpu().long(), torch.from_numpy(codes[ids]))
    d = xs.grid_dist(qi, xh)
    tq = torch.from_numpy(q.astype(np.float32))
    for k in (51, 128):
        Dm, Im = ref.search(d, assign, nlist, probe, k)
        st = {}
        Dg, Ig = idx.search(tq, k, 2, probe=torch.from_numpy(probe), stats=st)
        assert torch.equal(Ig.cpu(), torch.from_numpy(Im)) and torch.equal(Dg.cpu(), xs.from_units(Dm, unit))
    cnt = np.bincount(probe[probe >= 0], minlength=nlist)
    assert cnt[4] == S and cnt[3] == S - 1 and cnt[5] == S + 2
    want_tiles = sum(-(-int(cnt[c]) // S) * -(-lens[c] // R) for c in range(nlist))
    assert st["n_tiles"] == want_tiles
    # S + 1 exactly: the same search without the first query
    Dm, Im = ref.search(d[1:], assign, nlist, probe[1:], 51)
    Dg, Ig = idx.search(tq[1:], 51, 2, probe=torch.from_numpy(probe[1:]))
    assert np.bincount(probe[1:][probe[1:] >= 0], minlength=nlist)[5] == S + 1
    assert torch.equal(Ig.cpu(), torch.from_numpy(Im)) and torch.equal(Dg.cpu(), xs.from_units(Dm, unit))


# ---- unit Gaussian rows --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 16])
def gauss(cd, request):
    M = request.param
    rng = np.random.RandomState(13)
    x = _unit32(rng.randn(G_N, G_D))
    q = np.concatenate([_unit32(rng.randn(G_NQ - 3, G_D)), x[[0, 777, G_N - 1]]])
    tx, tq = torch.from_numpy(x).to(cd.dev), torch.from_numpy(q).to(cd.dev)
    idx = cd.knn.IVFIndex.build(tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=M)
    base = idx.prepare(tx)
    s0, s1 = {}, {}
    D0, I0 = idx.search(tq, G_K, G_NPROBE, stats=s0)
    D1, I1 = idx.search(tq, G_K, G_NPROBE, refine=G_R, base=base, stats=s1)
    torch.cuda.synchronize()

    class NS:
        pass
    g = NS()
    g.M, g.x, g.q, g.tx, g.tq, g.idx, g.base, g.s0, g.s1, g.D0, g.I0, g.D1, g.I1 = M, x, q, tx, tq, idx, base, s0, s1, D0, I0, D1, I1
    g.assign = idx.assign.cpu().numpy()
    g.probe = s0["probe"].cpu().numpy().astype(np.int64)
    g.floats = s0["n_floats"] + G_NQ * 256 * M                            # the scores and the tables of all queries
    g.bytes3 = 4 * g.floats // 3 - 4096
    g.cb = idx.codebooks.cpu().numpy()
    pos = np.empty(G_N, dtype=np.int64)
    pos[idx.ids.cpu().numpy()] = np.arange(G_N)
    g.codes = idx.codes.cpu().numpy().astype(np.int64)[pos]               # in catalogue order
    return g


def test_gaussian_codes_are_nearest_within_the_fp32_bound(cd, gauss):
    g = gauss
    dsub = G_D // g.M
    assert g.cb.shape == (g.M, 256, dsub) and g.idx.n_unlisted == 0
    d = pq.sub_dist(g.x, g.cb)                                            # fp64 [n, M, 256]
    chosen = np.take_along_axis(d, g.codes[:, :, None], 2)[:, :, 0]
    dmin = d.min(2)
    slack = chosen - dmin
    print("pq encode M=%d: %.4f of the codes are the fp64 argmin; max (d(chosen) - d_min) / d(chosen) = %.3g (bound %.3g)"
          % (g.M, (g.codes == d.argmin(2)).mean(), (slack / np.maximum(chosen, 1e-300)).max(), 2 * pq.encode_bound(dsub)))
    assert (slack <= 2 * pq.encode_bound(dsub) * chosen).all()
    # r_sq is the decoded rows' norm
    xh = pq.decode(g.codes, g.cb).astype(np.float64)
    ids = g.idx.ids.cpu().numpy()
    assert np.abs(g.idx.r_sq.cpu().numpy() - (xh[ids] ** 2).sum(1)).max() <= 1e-6


def test_gaussian_search_matches_the_fp64_model_on_the_decoded_rows(cd, gauss):
    g = gauss
    st = {}
    Dg, Ig = g.idx.search(g.tq, G_K, G_NPROBE, score_bytes=g.bytes3, stats=st)
    assert len(st["chunks"]) >= 3
    xh = pq.decode(g.codes, g.cb)
    d = pq.direct_dist(g.q, xh)
    Dr, Ir = ref.search(d, g.assign, G_NLIST, g.probe, G_K)
    err = np.abs(Dg.cpu().numpy()[np.isfinite(Dr)] - Dr[np.isfinite(Dr)]).max()
    print("pq scan M=%d: max |d - fp64 model on the decoded rows| = %.3g (TOL %.0e)" % (g.M, err, TOL))
    check(Dg.cpu().numpy(), Ig.cpu().numpy(), Dr, Ir, np.maximum(d, 0.0))
    # the re-rank: fp32 distances of the fp32 rows over the device's own candidates
    cand = g.s1["candidates"].cpu().numpy().astype(np.int64)
    table = np.full((G_NQ, xs.LIST), xs.NO_ID, dtype=np.int64)
    table[:, :G_R] = cand
    Dr, Ir = f16.refine(g.q, g.x, table, G_R, G_K)
    check(g.D1.cpu().numpy(), g.I1.cpu().numpy(), Dr, Ir, np.maximum(ref.fp64_dist(g.q, g.x, l2_norm=False), 0.0))
    assert (g.D1[-3:, 0] == 0).all() and (g.I1[-3:, 0].cpu().numpy() == [0, 777, G_N - 1]).all()


def _raw_scores(cd, idx, Q, probe):
    """every slot row's raw scores as {(query, list): tensor}, through the launches themselves"""
    S, R = cd.ops.ivf_pq_tile(idx.pq_m)
    tb = cd.knn.ivf_tables(probe, idx.list_len, tile_slots=S, tile_rows=R)
    lut = torch.empty((Q.shape[0], idx.pq_m, 256), dtype=torch.float32, device=Q.device)
    cd.ops.pq_lut(Q, idx.codebooks, lut)
    scores = torch.full((max(tb["n_floats"], 4),), float("nan"), dtype=torch.float32, device=Q.device)
    cd.ops.ivf_scan_pq(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], idx.codes, idx.list_start, tb["tiles"], scores)
    out = {}
    sq, off = tb["slot_query"].cpu().numpy(), tb["slot_off"].cpu().numpy()
    lists = np.repeat(np.arange(idx.nlist), np.diff(tb["slot_start"].cpu().numpy()))
    lens = idx.list_len.cpu().numpy()
    sc = scores.cpu()
    for s in range(len(sq)):
        out[(int(sq[s]), int(lists[s]))] = sc[off[s]:off[s] + lens[lists[s]]]
    return out


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
    D3, I3 = g.idx.search(g.tq[perm], G_K, G_NPROBE, score_bytes=4 * g.floats // 2, **kw)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(G_NQ, device=cd.dev)
    assert torch.equal(D3[inv], want_d) and torch.equal(I3[inv], want_i)
    if refine:
        return
    # the raw scores: a query in the crowd, permuted, and probing alone
    Q = g.tq.contiguous()
    pr = g.s0["probe"]
    crowd = _raw_scores(cd, g.idx, Q, pr)
    shuffled = _raw_scores(cd, g.idx, Q[perm].contiguous(), pr[perm].contiguous())
    p = perm.cpu().numpy()
    for (qs, c), v in shuffled.items():
        assert torch.equal(v, crowd[(int(p[qs]), c)])
    for qi in (0, 101, G_NQ - 1):
        alone = _raw_scores(cd, g.idx, Q[qi:qi + 1].contiguous(), pr[qi:qi + 1].contiguous())
        assert len(alone) == G_NPROBE
        for (_, c), v in alone.items():
            assert torch.equal(v, crowd[(qi, c)]) and not bool(torch.isnan(v).any())


# ---- training --------------------------------------------------------------------------------------------------------------------------
def test_training_is_deterministic_and_shares_the_coarse_index(cd, gauss):
    g = gauss
    again = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=g.M)
    for name in ("codebooks", "codes", "r_sq", "centroids", "assign", "ids", "list_start"):
        assert torch.equal(getattr(again, name), getattr(g.idx, name)), name
    assert torch.equal(again.pq_objective, g.idx.pq_objective) and torch.equal(again.objective, g.idx.objective)
    obj = g.idx.pq_objective
    assert obj.dtype == torch.float64 and tuple(obj.shape) == (g.M, 10) and obj.device.type == "cpu"
    assert bool((obj[:, 1:] <= obj[:, :-1] + G_N * TOL).all())            # (the slack of the coarse k-means test)
    assert bool((obj[:, -1] < obj[:, 0]).all())
    cb, o2 = cd.knn.pq_train(g.base, g.M)
    assert torch.equal(cb, g.idx.codebooks) and torch.equal(o2, obj)
    f32 = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev)
    for name in ("centroids", "assign", "ids", "list_start"):
        assert torch.equal(getattr(f32, name), getattr(g.idx, name)), name
    assert torch.equal(f32.probes(g.tq, G_NPROBE), g.idx.probes(g.tq, G_NPROBE))
    assert g.idx.codes.numel() * 4 * G_D == f32.rows.numel() * f32.rows.element_size() * g.M       # M bytes against 4 Dp
    other = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=g.M, pq_seed=1, pq_iters=2)
    assert not torch.equal(other.codebooks, g.idx.codebooks) and tuple(other.pq_objective.shape) == (g.M, 2)
    assert torch.equal(other.assign, g.idx.assign)
    st = g.idx.state_dict()
    assert list(st)[-3:] == ["storage", "pq_m", "codebooks"] and st["storage"] == "pq" and st["pq_m"] == g.M
    back = cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev)
    assert back.storage == "pq" and back.pq_m == g.M
    for name in ("centroids", "assign", "ids", "list_start", "codebooks", "codes", "r_sq"):
        assert torch.equal(getattr(back, name), getattr(g.idx, name)), name
    D2, I2 = back.search(g.tq, G_K, G_NPROBE)
    assert torch.equal(D2, g.D0) and torch.equal(I2, g.I0)
    assert cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev, storage="f32").storage == "f32"


# ---- recovery ----------------------------------------------------------------------------------------------------------------------------
def test_rerank_recovers_the_exact_answer_where_the_gap_allows(cd):
    """RandomState(7), D = 64, M = 8: rows = codeword picks + 0.05 randn, queries = rows + 0.1 randn, scaled by 2^-3; k = 10, r =
    128, all lists probed, the generating codebooks.  With e_q = max |d~ - d| over the probed rows and d_k the k-th true
    distance, a query with #{rows: d~ <= d_k + e_q + 4 TOL} <= r has its whole true top k among the r candidates
    (ivf_pq_ref.recoverable).  The fp64 model gives 200 of 200 such queries and a PQ-only recall@10 of 0.925."""
    x, q, cb = pq.recovery_fixture()
    k, r, nlist = pq.REC_K, pq.REC_R, pq.REC_NLIST
    assign = np.arange(pq.REC_N) % nlist
    tx, tq = torch.from_numpy(x).to(cd.dev), torch.from_numpy(q).to(cd.dev)
    idx = cd.knn.IVFIndex.from_assignment(tx, torch.zeros(nlist, pq.REC_D), torch.from_numpy(assign), l2_norm=False, device=cd.dev,
                                          storage="pq", codebooks=torch.from_numpy(cb))
    probe = torch.arange(nlist).repeat(pq.REC_NQ, 1)
    Dg, Ig = idx.search(tq, k, nlist, probe=probe, refine=r, base=idx.prepare(tx))
    D0, I0 = idx.search(tq, k, nlist, probe=probe)
    pos = np.empty(pq.REC_N, dtype=np.int64)
    pos[idx.ids.cpu().numpy()] = np.arange(pq.REC_N)
    codes = idx.codes.cpu().numpy().astype(np.int64)[pos]                 # the DEVICE's codes
    d_true = pq.direct_dist(q, x)
    d_pq = pq.direct_dist(q, pq.decode(codes, cb))
    ok = pq.recoverable(d_true, d_pq, k, r, TOL)
    Dr, Ir = ref.search(d_true, assign, nlist, probe.numpy(), k)
    Dg, Ig, I0 = Dg.cpu().numpy(), Ig.cpu().numpy(), I0.cpu().numpy()
    print("recoverable share %.4f; recall@%d against the probed-exact ids: refine=0 %.4f, refine=%d %.4f"
          % (ok.mean(), k, ref.recall(I0, Ir), r, ref.recall(Ig, Ir)))
    assert ok.mean() >= 0.9
    check(Dg[ok], Ig[ok], Dr[ok], Ir[ok], np.maximum(d_true, 0.0)[ok])


# ---- refusals, ivf_knn, export ----------------------------------------------------------------------------------------------------------
def test_refusals_from_the_device_side_call_sites(cd, gauss):
    g = gauss
    with pytest.raises(ValueError, match="9f.2"):
        g.idx.search(g.tq, 5, 2, scan="filter")
    with pytest.raises(ValueError, match="needs pq_m"):
        cd.knn.ivf_knn(g.tx, None, 5, nlist=4, nprobe=2, storage="pq")
    with pytest.raises(ValueError, match="needs pq_m"):                   # the miner is not taught pq_m
        cd.hardneg.mine_lists(g.tx, 4, nlist=4, nprobe=2, storage="pq")
    with pytest.raises(ValueError, match="at least 256 finite rows"):
        cd.knn.IVFIndex.build(g.tx[:200], 4, l2_norm=False, device=cd.dev, storage="pq", pq_m=8)
    with pytest.raises(ValueError, match="does not divide"):
        cd.knn.pq_train(g.base, 24)
    with pytest.raises(ValueError, match="codebooks must be"):
        cd.knn.IVFIndex.from_assignment(g.tx, g.idx.centroids, g.idx.assign, l2_norm=False, device=cd.dev, storage="pq",
                                        codebooks=g.idx.codebooks[:, :, :2])
    st = g.idx.state_dict()
    del st["codebooks"]
    with pytest.raises(ValueError, match="holds no codebooks"):
        cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev)


def test_ivf_knn_and_export_run_on_pq_lists(cd, tmp_path):
    rng = np.random.RandomState(31)
    n, D, F = 600, 64, 96
    emb = torch.from_numpy(rng.randn(n, D).astype(np.float32))
    feats = torch.from_numpy(rng.randn(n, F).astype(np.float32))
    Dk, Ik = cd.knn.ivf_knn(emb, None, 10, nlist=8, nprobe=4, storage="pq", pq_m=8, refine=128, device=cd.dev)
    idx = cd.knn.IVFIndex.build(emb, 8, device=cd.dev, storage="pq", pq_m=8)
    Dw, Iw = idx.search(emb, 10, 4, refine=128, base=idx.prepare(emb))
    assert torch.equal(Dk, Dw) and torch.equal(Ik, Iw) and (Ik[:, 0].cpu().numpy() == np.arange(n)).all()
    st = {}
    D, I_desim = cd.knn.export(emb, feats, list("g%04d" % i for i in range(n)), str(tmp_path), doc_location=0, nearest_num=10,
                               desim_nearest_num=5, nlist=8, nprobe=4, feature_nlist=8, feature_nprobe=4, storage="pq", pq_m=8,
                               feature_pq_m=16, refine=64, device=cd.dev, stats=st)
    assert st["embedding_knn"]["ivf"]["n_tiles"] > 0
    idx = cd.knn.IVFIndex.build(emb, 8, device=cd.dev, storage="pq", pq_m=8)
    Dw, Iw = idx.search(emb, 10, 4, refine=64, base=idx.prepare(emb))
    assert torch.equal(D, Dw)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "strictI.npy")), Iw.cpu().numpy())
    fidx = cd.knn.IVFIndex.build(feats, 8, device=cd.dev, storage="pq", pq_m=16)
    fD, fI = fidx.search(feats, 5, 4, refine=64, base=fidx.prepare(feats))
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "fI.npy")), fI.cpu().numpy())
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "fD.npy")), fD.cpu().numpy())
    assert torch.equal(I_desim, cd.knn.desim(Iw, fI, fD, device=cd.dev))
    assert os.path.exists(os.path.join(str(tmp_path), "strict_knn0"))
