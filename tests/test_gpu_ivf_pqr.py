"""Residual product quantisation on the IVF index on the MI355X (include/cdml_ivf_pqr.h, csrc/ivf_pqr.hip,
cdml_amd.knn.IVFIndex(storage="pq", pq_residual=True)): the fused residual encoder, the slot scalars and the scan that starts
from them bit for bit against the int64 models on exact grids (lossless rows: the f32 index on the same (centroids, assign);
lossy rows with planted residual encode ties: the model on the decoded rows, the re-rank over the device's own candidates), a
dsub outside the template set, the scan's tile edges, unit Gaussian rows against the fp64 models, position independence, the
deterministic training, the clustered fixture with the model's codebooks, the defaults, the refusals from the device-side
call sites.

The float rows are l2-normalised HERE and indexed with l2_norm=False, so that the fp32 values the index encodes are bit for
bit the ones the host model encodes."""
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
import ivf_pqr_ref as pqr  # noqa: E402
import ivf_ref as ref  # noqa: E402
from test_gpu_knn import TOL, check  # noqa: E402

pytestmark = pytest.mark.gpu

G_N, G_D, G_NLIST, G_NPROBE, G_K, G_NQ, G_R = 2000, 64, 16, 4, 51, 203, 128
LOSSLESS = ((48, 8), (48, 32), (256, 64))
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


def _index(cd, c, storage="pq", residual=True):
    kw = {"codebooks": torch.from_numpy(c["cb"]), "pq_residual": residual} if storage == "pq" else {}
    return cd.knn.IVFIndex.from_assignment(torch.from_numpy(c["x"]), torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]),
                                           l2_norm=False, device=cd.dev, storage=storage, **kw)


def _check_lists(c, idx):
    ids, start = ref.lists_from_assign(c["assign"], c["nlist"])
    assert idx.storage == "pq" and idx.pq_residual and idx.pq_m == c["M"] and not hasattr(idx, "rows")
    assert idx.codes.dtype == torch.uint8 and tuple(idx.codes.shape) == (len(ids), c["M"]) and idx.codes.is_contiguous()
    assert idx.n_unlisted == 1 and int(idx.assign[c["nan_row"]]) == -1
    assert torch.equal(idx.ids.cpu().long(), torch.from_numpy(ids)) and torch.equal(idx.list_start.cpu().long(), torch.from_numpy(start))
    assert torch.equal(idx.codes.cpu().long(), torch.from_numpy(c["codes"][ids]))                  # the model's codes, bit for bit
    dec = idx.decode(torch.arange(len(ids)))
    assert dec.dtype == torch.float32 and tuple(dec.shape) == (len(ids), c["Dp"])
    assert torch.equal(dec.cpu(), torch.from_numpy((c["xhi"][ids] * xs.PIPE_UNIT).astype(np.float32)))     # centroid + codewords
    some = torch.tensor([len(ids) - 1, 0, 131, 131, 5])
    assert torch.equal(idx.decode(some), dec[some.to(dec.device)])
    assert torch.equal(idx.r_sq.cpu(), torch.from_numpy(((c["xhi"][ids] ** 2).sum(1) * c["unit"]).astype(np.float32)))
    return ids


# ---- exact grids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", LOSSLESS)
def test_lossless_grid_is_the_f32_index_bit_for_bit(cd, D, M):
    c = pqr.lossless_case(D, M)
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
            Dw, Iw = pqr.grid_want(c, k, probe=probe)
            Dg, Ig = idx.search(q, k, ref.GRID_NPROBE, **pk)
            assert Dg.dtype == torch.float32 and Ig.dtype == torch.int64 and tuple(Dg.shape) == (ref.GRID_NQ, k)
            assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
            Df, If = f32.search(q, k, ref.GRID_NPROBE, **pk)
            assert torch.equal(Ig, If) and torch.equal(Dg, Df)
            Dr, Ir = idx.search(q, k, ref.GRID_NPROBE, refine=xs.LIST, base=base, **pk)
            assert torch.equal(Ir.cpu(), Iw) and torch.equal(Dr.cpu(), Dw)


@pytest.mark.parametrize("D,M", LOSSY)
def test_lossy_grid_codes_search_and_rerank_bit_for_bit(cd, D, M):
    c = pqr.lossy_case(D, M)
    assert c["safe"] < 2.0 ** 24 and len(c["tie_rows"]) == pq.LOSSY_TIES
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    idx = _index(cd, c)
    ids = _check_lists(c, idx)
    pos = {int(r): i for i, r in enumerate(ids)}
    for r, m, lo, hi in c["tie_rows"]:                                    # the planted residual ties went to the lower code
        assert int(idx.codes[pos[r], m]) == c["codes"][r, m] <= lo < hi
    plain = _index(cd, c, residual=False)                                 # the same codebooks on the rows themselves: other codes
    assert not torch.equal(plain.codes, idx.codes)
    base = idx.prepare(x)
    for k in ref.GRID_KS:
        Dw, Iw = pqr.grid_want(c, k)
        Dg, Ig = idx.search(q, k, ref.GRID_NPROBE)
        assert torch.equal(Ig.cpu(), Iw) and torch.equal(Dg.cpu(), Dw)
        Dh, Ih = idx.search(q, k, ref.GRID_NPROBE, probe=torch.from_numpy(c["probe_hand"]))
        Dwh, Iwh = pqr.grid_want(c, k, probe=c["probe_hand"])
        assert torch.equal(Ih.cpu(), Iwh) and torch.equal(Dh.cpu(), Dwh)
        st = {}
        Dr, Ir = idx.search(q, k, ref.GRID_NPROBE, refine=xs.LIST, base=base, stats=st)
        cand = st["candidates"].cpu().numpy().astype(np.int64)
        assert cand.shape == (ref.GRID_NQ, xs.LIST) and c["nan_row"] not in cand and (cand[ref.GRID_NAN_QUERY] == xs.NO_ID).all()
        assert np.array_equal(np.where(cand[:, :k] == xs.NO_ID, -1, cand[:, :k]), Iw.numpy())
        Dm, Im = f16.refine(c["qi"], c["xi"], cand, xs.LIST, k)
        assert torch.equal(Ir.cpu(), torch.from_numpy(Im)) and torch.equal(Dr.cpu(), xs.from_units(Dm, c["unit"]))
    Iw = pqr.grid_want(c, 51)[1]
    Dm, Im = ref.search(c["d"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    assert not torch.equal(Iw, torch.from_numpy(Im))                      # (lossy indeed)


def _int_case(D, M, lens, nq, rng):
    """integer rows in lists of ``lens`` (shuffled ids) on random small integer centroids, residual codebooks of distinct grid
    codewords; the int64 model's codes, decoded rows and distances"""
    dsub = D // M
    nlist, n = len(lens), sum(lens)
    assign = np.repeat(np.arange(nlist), lens)
    rng.shuffle(assign)
    xi = xs.grid_rows(n, D, rng)
    ci = rng.randint(-2, 3, size=(nlist, D)).astype(np.int64)
    cbi = np.stack([pq._distinct_codewords(rng, dsub, dsub)[0] for _ in range(M)])
    codes, _ = pqr.encode(xi, ci, assign, cbi)
    xh = pqr.decode(codes, ci, assign, cbi)
    qi = xs.grid_rows(nq, D, rng)
    u = xs.PIPE_UNIT
    q, xd = qi * u, xh * u
    assert xs.assert_select_exact_safe((q * q).sum(1), (xd * xd).sum(1), u * u, [q], [xd], xg.PAIRS1) < 2.0 ** 24
    assert float(np.abs(pqr.slot_dot(qi, ci)).max() + np.abs(pq.lut(qi, cbi)).max(2).sum(1).max()) < 2.0 ** 24
    return dict(assign=assign, xi=xi, ci=ci, cbi=cbi, codes=codes, xh=xh, qi=qi, d=xs.grid_dist(qi, xh), nlist=nlist, n=n, unit=u * u)


def _int_index(cd, c, x=None, assign=None):
    u = xs.PIPE_UNIT
    x = (c["xi"] * u).astype(np.float32) if x is None else x
    return cd.knn.IVFIndex.from_assignment(torch.from_numpy(x), torch.from_numpy((c["ci"] * u).astype(np.float32)),
                                           torch.from_numpy(c["assign"] if assign is None else assign), l2_norm=False,
                                           device=cd.dev, storage="pq", codebooks=torch.from_numpy((c["cbi"] * u).astype(np.float32)),
                                           pq_residual=True)


def test_a_dsub_outside_the_template_set(cd):
    """D = 96, M = 8: dsub 12 takes k_pqr_encode_any (and k_pq_lut_any); the same sums in the same order"""
    rng = xg.case_rng("ivfpqr-dsub12")
    lens = (150, 0, 301, 77)
    c = _int_case(96, 8, lens, 60, rng)
    idx = _int_index(cd, c)
    assert idx.codebooks.shape[2] == 12
    ids, _ = ref.lists_from_assign(c["assign"], c["nlist"])
    assert torch.equal(idx.codes.cpu().long(), torch.from_numpy(c["codes"][ids]))
    assert torch.equal(idx.decode(torch.arange(len(ids))).cpu(), torch.from_numpy((c["xh"][ids] * xs.PIPE_UNIT).astype(np.float32)))
    probe = np.stack([rng.permutation(c["nlist"])[:2] for _ in range(60)]).astype(np.int64)
    tq = torch.from_numpy((c["qi"] * xs.PIPE_UNIT).astype(np.float32))
    for k in (51, 128):
        Dm, Im = ref.search(c["d"], c["assign"], c["nlist"], probe, k)
        Dg, Ig = idx.search(tq, k, 2, probe=torch.from_numpy(probe))
        assert torch.equal(Ig.cpu(), torch.from_numpy(Im)) and torch.equal(Dg.cpu(), xs.from_units(Dm, c["unit"]))


# ---- tile edges ----------------------------------------------------------------------------------------------------------------------
# every instance of the scan (M / 8 = 1..8); D = lcm(2 M, 32): M (8 bits) and 2 M (4 bits) divide the padded width, dsub is 1, 2 or 4
TILE_MS = list(range(8, 72, 8))


def tile_dim(M):
    return math.lcm(2 * M, 32)


@pytest.mark.parametrize("M", TILE_MS)
def test_tile_edges(cd, M):
    """list lengths 0, 1, R - 1, R, R + 1, 2 R + 5 and lists probed by S - 1, S, S + 1 and S + 2 queries, -1 probes, a NaN query,
    a NaN row and an assign of -1 handed to the encoder, against the int64 model"""
    S, R = cd.ops.ivf_pq_tile(M)
    assert (S, R) == (64 // M, 1024)
    D = tile_dim(M)
    lens = (0, 1, R - 1, R, R + 1, 2 * R + 5)
    rng = xg.case_rng("ivfpqr-tiles", M)
    groups = [(5, S + 1), (4, S), (3, S - 1), (2, 3), (1, 2), (0, 2)]
    probe = [[1, 5]] + [[a, -1] for a, cnt in groups for _ in range(cnt)]
    probe[-1] = [0, 2]
    probe.append([-1, -1])                                                # the NaN query: what the coarse search gives it
    probe = np.asarray(probe, dtype=np.int64)
    nq = len(probe)
    c = _int_case(D, M, lens, nq, rng)
    nlist, n, assign = c["nlist"], c["n"], c["assign"]
    # one more row, NaN, claimed for list 5: it is unlisted, and the encoder is handed its assign of -1
    u = xs.PIPE_UNIT
    x = np.concatenate([(c["xi"] * u).astype(np.float32), np.full((1, D), np.nan, dtype=np.float32)])
    assign_x = np.concatenate([assign, [5]])
    idx = _int_index(cd, c, x=x, assign=assign_x)
    assert idx.n_unlisted == 1 and int(idx.assign[n]) == -1 and idx.list_len.cpu().tolist() == list(lens)
    ids, _ = ref.lists_from_assign(assign, nlist)
    assert torch.equal(idx.codes.cpu().long(), torch.from_numpy(c["codes"][ids]))
    # the encoder itself on (x, assign with a -1): codes 0 and dist +inf for that row, the model's codes elsewhere
    a_dev = torch.from_numpy(np.concatenate([assign, [-1]])).to(cd.dev)
    codes = torch.full((n + 1, M), 255, dtype=torch.uint8, device=cd.dev)
    dist = torch.zeros((n + 1, M), dtype=torch.float32, device=cd.dev)
    cd.ops.pqr_encode(torch.from_numpy(x).to(cd.dev), idx._C, a_dev, idx.codebooks, codes, dist)
    assert bool((codes[n] == 0).all()) and bool(torch.isinf(dist[n]).all()) and bool((dist[n] > 0).all())
    assert torch.equal(codes[:n].cpu().long(), torch.from_numpy(c["codes"]))
    want_dist = np.take_along_axis(pq.sub_dist(pqr.residual(c["xi"], c["ci"], assign), c["cbi"]), c["codes"][:, :, None], 2)[:, :, 0]
    assert torch.equal(dist[:n].cpu(), xs.from_units(want_dist, c["unit"]))
    tq = torch.from_numpy((c["qi"] * u).astype(np.float32))
    tq[nq - 1, 7] = float("nan")
    bad = (nq - 1,)
    for k in (51, 128):
        Dm, Im = ref.search(c["d"], assign, nlist, probe, k, bad_queries=bad)
        st = {}
        Dg, Ig = idx.search(tq, k, 2, probe=torch.from_numpy(probe), stats=st)
        assert torch.equal(Ig.cpu(), torch.from_numpy(Im)) and torch.equal(Dg.cpu(), xs.from_units(Dm, c["unit"]))
        assert bool((Ig[nq - 1] == -1).all()) and n not in Ig.cpu().numpy()
    cnt = np.bincount(probe[probe >= 0], minlength=nlist)
    assert cnt[4] == S and cnt[3] == S - 1 and cnt[5] == S + 2
    want_tiles = sum(-(-int(cnt[l]) // S) * -(-lens[l] // R) for l in range(nlist))
    assert st["n_tiles"] == want_tiles
    # S + 1 exactly: the same search without the first query
    Dm, Im = ref.search(c["d"][1:], assign, nlist, probe[1:], 51, bad_queries=(nq - 2,))
    Dg, Ig = idx.search(tq[1:], 51, 2, probe=torch.from_numpy(probe[1:]))
    assert np.bincount(probe[1:][probe[1:] >= 0], minlength=nlist)[5] == S + 1
    assert torch.equal(Ig.cpu(), torch.from_numpy(Im)) and torch.equal(Dg.cpu(), xs.from_units(Dm, c["unit"]))


# ---- unit Gaussian rows --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 16])
def gauss(cd, request):
    M = request.param
    rng = np.random.RandomState(13)
    x = _unit32(rng.randn(G_N, G_D))
    q = np.concatenate([_unit32(rng.randn(G_NQ - 3, G_D)), x[[0, 777, G_N - 1]]])
    tx, tq = torch.from_numpy(x).to(cd.dev), torch.from_numpy(q).to(cd.dev)
    idx = cd.knn.IVFIndex.build(tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=M, pq_residual=True)
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
    g.floats = s0["n_floats"] + G_NQ * (256 * M + G_NPROBE)               # the scores, tables and slot scalars of all queries
    g.bytes3 = 4 * g.floats // 3 - 4096
    g.cb = idx.codebooks.cpu().numpy()
    g.cent = idx._C.cpu().numpy()
    pos = np.empty(G_N, dtype=np.int64)
    pos[idx.ids.cpu().numpy()] = np.arange(G_N)
    g.pos = pos
    g.codes = idx.codes.cpu().numpy().astype(np.int64)[pos]               # in catalogue order
    g.xh = idx.decode(torch.arange(G_N)).cpu().numpy()[pos]               # the DEVICE's decoded rows, in catalogue order
    return g


def test_gaussian_codes_are_nearest_to_the_residual_within_the_fp32_bound(cd, gauss):
    g = gauss
    dsub = G_D // g.M
    assert g.cb.shape == (g.M, 256, dsub) and g.idx.n_unlisted == 0 and g.cent.shape == (G_NLIST, G_D)
    e = g.x - g.cent[g.assign]                                            # the fp32 residual: the kernel's own subtract
    assert e.dtype == np.float32
    d = pq.sub_dist(e, g.cb)                                              # fp64 [n, M, 256]
    chosen = np.take_along_axis(d, g.codes[:, :, None], 2)[:, :, 0]
    slack = chosen - d.min(2)
    print("pqr encode M=%d: %.4f of the codes are the fp64 argmin; max (d(chosen) - d_min) / d(chosen) = %.3g (bound %.3g)"
          % (g.M, (g.codes == d.argmin(2)).mean(), (slack / np.maximum(chosen, 1e-300)).max(), 2 * pq.encode_bound(dsub)))
    assert (slack <= 2 * pq.encode_bound(dsub) * chosen).all()
    # the decoded rows are centroid + codewords in fp32 (one add), r_sq their norm
    assert np.array_equal(g.xh, g.cent[g.assign] + pq.decode(g.codes, g.cb))
    ids = g.idx.ids.cpu().numpy()
    assert np.abs(g.idx.r_sq.cpu().numpy() - (g.xh[ids].astype(np.float64) ** 2).sum(1)).max() <= 1e-6


def _launches(cd, idx, Q, probe, poison=float("nan")):
    """(tables, lut, slot_base, scores) of one chunk through the launches themselves"""
    S, R = cd.ops.ivf_pq_tile(idx.pq_m)
    tb = cd.knn.ivf_tables(probe, idx.list_len, tile_slots=S, tile_rows=R)
    lut = torch.empty((Q.shape[0], idx.pq_m, 256), dtype=torch.float32, device=Q.device)
    cd.ops.pq_lut(Q, idx.codebooks, lut)
    slot_base = torch.full((tb["n_slots"],), poison, dtype=torch.float32, device=Q.device)
    cd.ops.ivf_slot_dots(Q, idx._C, tb["slot_query"], tb["slot_start"], slot_base)
    scores = torch.full((max(tb["n_floats"], 4),), poison, dtype=torch.float32, device=Q.device)
    cd.ops.ivf_scan_pqr(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], slot_base, idx.codes, idx.list_start, tb["tiles"],
                        scores)
    return tb, lut, slot_base, scores


def _raw(cd, idx, Q, probe):
    """every slot's base and raw score row as {(query, list): (base, tensor)}"""
    tb, _, slot_base, scores = _launches(cd, idx, Q, probe)
    out = {}
    sq, off = tb["slot_query"].cpu().numpy(), tb["slot_off"].cpu().numpy()
    lists = np.repeat(np.arange(idx.nlist), np.diff(tb["slot_start"].cpu().numpy()))
    lens = idx.list_len.cpu().numpy()
    sc, sb = scores.cpu(), slot_base.cpu()
    for s in range(len(sq)):
        out[(int(sq[s]), int(lists[s]))] = (sb[s], sc[off[s]:off[s] + lens[lists[s]]])
    return out


def test_gaussian_slot_scalars_and_search_match_the_fp64_models(cd, gauss):
    g = gauss
    raw = _raw(cd, g.idx, g.tq.contiguous(), g.s0["probe"])
    assert len(raw) == G_NQ * G_NPROBE
    b64 = pqr.slot_dot(g.q, g.cent)
    err = max(abs(float(b) - b64[qi, c]) for (qi, c), (b, _) in raw.items())
    print("slot scalars M=%d: max |b - fp64| = %.3g (TOL %.0e)" % (g.M, err, TOL))
    assert err <= TOL
    st = {}
    Dg, Ig = g.idx.search(g.tq, G_K, G_NPROBE, score_bytes=g.bytes3, stats=st)
    assert len(st["chunks"]) >= 3
    d = pq.direct_dist(g.q, g.xh)                                         # fp64, on the device's decoded rows
    Dr, Ir = ref.search(d, g.assign, G_NLIST, g.probe, G_K)
    err = np.abs(Dg.cpu().numpy()[np.isfinite(Dr)] - Dr[np.isfinite(Dr)]).max()
    print("pqr scan M=%d: max |d - fp64 model on the decoded rows| = %.3g (TOL %.0e)" % (g.M, err, TOL))
    check(Dg.cpu().numpy(), Ig.cpu().numpy(), Dr, Ir, np.maximum(d, 0.0))
    # the re-rank: fp32 distances of the fp32 rows over the device's own candidates
    cand = g.s1["candidates"].cpu().numpy().astype(np.int64)
    table = np.full((G_NQ, xs.LIST), xs.NO_ID, dtype=np.int64)
    table[:, :G_R] = cand
    Dr, Ir = f16.refine(g.q, g.x, table, G_R, G_K)
    check(g.D1.cpu().numpy(), g.I1.cpu().numpy(), Dr, Ir, np.maximum(ref.fp64_dist(g.q, g.x, l2_norm=False), 0.0))
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
    D3, I3 = g.idx.search(g.tq[perm], G_K, G_NPROBE, score_bytes=4 * g.floats // 2, **kw)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(G_NQ, device=cd.dev)
    assert torch.equal(D3[inv], want_d) and torch.equal(I3[inv], want_i)
    if refine:
        return
    # the slot scalars and the raw scores: a query in the crowd, permuted, and probing alone
    Q = g.tq.contiguous()
    pr = g.s0["probe"]
    crowd = _raw(cd, g.idx, Q, pr)
    shuffled = _raw(cd, g.idx, Q[perm].contiguous(), pr[perm].contiguous())
    p = perm.cpu().numpy()
    for (qs, c), (b, v) in shuffled.items():
        assert torch.equal(b, crowd[(int(p[qs]), c)][0]) and torch.equal(v, crowd[(int(p[qs]), c)][1])
    for qi in (0, 101, G_NQ - 1):
        alone = _raw(cd, g.idx, Q[qi:qi + 1].contiguous(), pr[qi:qi + 1].contiguous())
        assert len(alone) == G_NPROBE
        for (_, c), (b, v) in alone.items():
            assert torch.equal(b, crowd[(qi, c)][0]) and torch.equal(v, crowd[(qi, c)][1]) and not bool(torch.isnan(v).any())
    # the bits of a score: fp32 adds over ascending m from the slot's base, on the device's own tables
    tb, lut, slot_base, scores = _launches(cd, g.idx, Q[:7].contiguous(), pr[:7].contiguous())
    sq, off = tb["slot_query"].cpu().numpy(), tb["slot_off"].cpu().numpy()
    lists = np.repeat(np.arange(G_NLIST), np.diff(tb["slot_start"].cpu().numpy()))
    start = g.idx.list_start.cpu().numpy()
    codes, table, sb, sc = g.idx.codes.cpu().numpy().astype(np.int64), lut.cpu().numpy(), slot_base.cpu().numpy(), scores.cpu().numpy()
    for s in range(len(sq)):
        rows = codes[start[lists[s]]:start[lists[s] + 1]]
        want = pqr.adc(table[sq[s]:sq[s] + 1], rows, np.full((1, len(rows)), sb[s], dtype=np.float32))[0]
        assert np.array_equal(sc[off[s]:off[s] + len(rows)], want)


# ---- training --------------------------------------------------------------------------------------------------------------------------
def test_training_is_deterministic_and_shares_the_coarse_index(cd, gauss):
    g = gauss
    again = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=g.M, pq_residual=True)
    for name in ("codebooks", "codes", "r_sq", "centroids", "assign", "ids", "list_start"):
        assert torch.equal(getattr(again, name), getattr(g.idx, name)), name
    assert torch.equal(again.pq_objective, g.idx.pq_objective) and torch.equal(again.objective, g.idx.objective)
    obj = g.idx.pq_objective
    assert obj.dtype == torch.float64 and tuple(obj.shape) == (g.M, 10) and obj.device.type == "cpu"
    assert bool((obj[:, 1:] <= obj[:, :-1] + G_N * TOL).all())            # (the slack of the coarse k-means test)
    assert bool((obj[:, -1] < obj[:, 0]).all())
    cb, o2 = cd.knn.pq_train(g.base, g.M, centroids=g.idx._C, assign=g.idx.assign)
    assert torch.equal(cb, g.idx.codebooks) and torch.equal(o2, obj)
    f32 = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev)
    for name in ("centroids", "assign", "ids", "list_start"):
        assert torch.equal(getattr(f32, name), getattr(g.idx, name)), name
    assert torch.equal(f32.probes(g.tq, G_NPROBE), g.idx.probes(g.tq, G_NPROBE))
    st = g.idx.state_dict()
    assert list(st)[-4:] == ["storage", "pq_m", "codebooks", "pq_residual"] and st["pq_residual"] is True and st["pq_m"] == g.M
    back = cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev)
    assert back.storage == "pq" and back.pq_residual and back.pq_m == g.M
    for name in ("centroids", "assign", "ids", "list_start", "codebooks", "codes", "r_sq"):
        assert torch.equal(getattr(back, name), getattr(g.idx, name)), name
    D2, I2 = back.search(g.tq, G_K, G_NPROBE)
    assert torch.equal(D2, g.D0) and torch.equal(I2, g.I0)
    assert cd.knn.IVFIndex.load_state_dict(st, g.tx, device=cd.dev, storage="f32").storage == "f32"


def test_defaults_are_the_plain_index(cd, gauss):
    g = gauss
    a = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=g.M)
    b = cd.knn.IVFIndex.build(g.tx, G_NLIST, l2_norm=False, device=cd.dev, storage="pq", pq_m=g.M, pq_residual=False)
    assert not a.pq_residual and not b.pq_residual and list(a.state_dict())[-3:] == ["storage", "pq_m", "codebooks"]
    for name in ("codebooks", "codes", "r_sq", "assign"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    cb, _ = cd.knn.pq_train(g.base, g.M)
    assert torch.equal(cb, a.codebooks) and not torch.equal(cb, g.idx.codebooks)
    codes = torch.empty((G_N, g.M), dtype=torch.uint8, device=cd.dev)
    cd.ops.pq_encode(g.base, cb, codes)
    assert torch.equal(a.codes, codes[a.ids.long()])
    Da, Ia = a.search(g.tq, G_K, G_NPROBE)
    Db, Ib = cd.knn.ivf_knn(g.tx, g.tq, G_K, nlist=G_NLIST, nprobe=G_NPROBE, l2_norm=False, storage="pq", pq_m=g.M, device=cd.dev)
    assert torch.equal(Da, Db) and torch.equal(Ia, Ib)
    # a zero centroid matrix makes the residual index the plain one: same codes, same (D, I)
    z = cd.knn.IVFIndex.from_assignment(g.tx, torch.zeros(G_NLIST, G_D), a.assign, l2_norm=False, device=cd.dev, storage="pq",
                                        codebooks=cb, pq_residual=True)
    p = cd.knn.IVFIndex.from_assignment(g.tx, torch.zeros(G_NLIST, G_D), a.assign, l2_norm=False, device=cd.dev, storage="pq",
                                        codebooks=cb)
    assert torch.equal(z.codes, p.codes) and torch.equal(z.r_sq, p.r_sq)
    probe = g.s0["probe"]
    Dz, Iz = z.search(g.tq, G_K, G_NPROBE, probe=probe)
    Dp, Ip = p.search(g.tq, G_K, G_NPROBE, probe=probe)
    assert torch.equal(Dz, Dp) and torch.equal(Iz, Ip)                    # (0 + LUT_0 is LUT_0)


# ---- the clustered fixture ---------------------------------------------------------------------------------------------------------------
def _recoverable_probed(d_true, d_pq, assign, probe, k, r, tol):
    """ivf_pq_ref.recoverable restricted to every query's probed rows"""
    ok = np.zeros(len(probe), dtype=bool)
    for qi in range(len(probe)):
        mem = np.nonzero(np.isin(assign, probe[qi]))[0]
        e = np.abs(d_pq[qi, mem] - d_true[qi, mem]).max()
        dk = np.sort(d_true[qi, mem])[k - 1]
        ok[qi] = (d_pq[qi, mem] <= dk + e + 4 * tol).sum() <= r
    return ok


def test_clustered_fixture_with_the_models_codebooks(cd):
    """The float64 model's centroids, assignment and codebooks given through from_assignment: the device's recall@10 of the
    residual codes is the model's to 0.01, and above the plain codes'; re-ranked, both indexes give the same answer wherever
    the recovery condition holds for both."""
    f = pqr.clustered_fixture()
    k, r, nlist, nprobe = pqr.CL_K, 128, pqr.CL_NLIST, pqr.CL_NPROBE
    tx, tq = torch.from_numpy(f["x"]).to(cd.dev), torch.from_numpy(f["q"]).to(cd.dev)
    cent, assign, probe = torch.from_numpy(f["cent"]), torch.from_numpy(f["assign"]), torch.from_numpy(f["probe"])
    res = cd.knn.IVFIndex.from_assignment(tx, cent, assign, l2_norm=False, device=cd.dev, storage="pq",
                                          codebooks=torch.from_numpy(f["cb_res"]), pq_residual=True)
    pln = cd.knn.IVFIndex.from_assignment(tx, cent, assign, l2_norm=False, device=cd.dev, storage="pq",
                                          codebooks=torch.from_numpy(f["cb_plain"]))
    out = {}
    for name, idx in (("res", res), ("plain", pln)):
        _, I0 = idx.search(tq, k, nprobe, probe=probe)
        D1, I1 = idx.search(tq, k, nprobe, probe=probe, refine=r, base=idx.prepare(tx))
        pos = np.empty(pqr.CL_N, dtype=np.int64)
        pos[idx.ids.cpu().numpy()] = np.arange(pqr.CL_N)
        xh = idx.decode(torch.arange(pqr.CL_N)).cpu().numpy()[pos]
        ok = _recoverable_probed(f["d_true"], pq.direct_dist(f["q"], xh), f["assign"], f["probe"], k, r, TOL)
        rec = ref.recall(I0.cpu().numpy(), f["true"])
        print("clustered fixture, %s codes: device recall@%d %.4f (model %.4f); recoverable share %.4f"
              % (name, k, rec, f["recall_" + name], ok.mean()))
        assert rec >= f["recall_" + name] - 0.01
        out[name] = (rec, ok, D1, I1)
    assert out["res"][0] > out["plain"][0]
    both = torch.from_numpy(out["res"][1] & out["plain"][1]).to(cd.dev)
    assert int(both.sum()) >= pqr.CL_NQ // 2
    assert torch.equal(out["res"][2][both], out["plain"][2][both]) and torch.equal(out["res"][3][both], out["plain"][3][both])
    # trained on the device, the residual codebooks end at a lower objective than the plain ones (the same rows, ids and seed)
    a = cd.knn.IVFIndex.build(tx, nlist, l2_norm=False, device=cd.dev, storage="pq", pq_m=pqr.CL_M, pq_residual=True)
    b = cd.knn.IVFIndex.build(tx, nlist, l2_norm=False, device=cd.dev, storage="pq", pq_m=pqr.CL_M)
    print("clustered fixture, device training: final objective residual %.2f, plain %.2f"
          % (float(a.pq_objective[:, -1].sum()), float(b.pq_objective[:, -1].sum())))
    assert float(a.pq_objective[:, -1].sum()) < float(b.pq_objective[:, -1].sum())
    assert torch.equal(a.assign, b.assign) and torch.equal(a.centroids, b.centroids)


# ---- refusals, ivf_knn, export ----------------------------------------------------------------------------------------------------------
def test_refusals_from_the_device_side_call_sites(cd, gauss):
    g = gauss
    with pytest.raises(ValueError, match="9f.2"):
        g.idx.search(g.tq, 5, 2, scan="filter")
    for storage in ("f32", "f16"):
        with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
            cd.knn.ivf_knn(g.tx, None, 5, nlist=4, nprobe=2, storage=storage, pq_residual=True)
        with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
            cd.knn.IVFIndex.build(g.tx, 4, l2_norm=False, device=cd.dev, storage=storage, pq_residual=True)
    with pytest.raises(ValueError, match="centroids and assign together"):
        cd.knn.pq_train(g.base, g.M, centroids=g.idx._C)
    with pytest.raises(ValueError, match="every finite row needs an assign"):
        cd.knn.pq_train(g.base, g.M, centroids=g.idx._C, assign=torch.full((G_N,), -1, dtype=torch.int64))
    with pytest.raises(TypeError):                                        # the miner is not taught pq_residual
        cd.hardneg.mine_lists(g.tx, 4, nlist=4, nprobe=2, storage="pq", pq_residual=True)


def test_ivf_knn_and_export_run_on_residual_lists(cd, tmp_path):
    rng = np.random.RandomState(31)
    n, D, F = 600, 64, 96
    emb = torch.from_numpy(rng.randn(n, D).astype(np.float32))
    feats = torch.from_numpy(rng.randn(n, F).astype(np.float32))
    Dk, Ik = cd.knn.ivf_knn(emb, None, 10, nlist=8, nprobe=4, storage="pq", pq_m=8, pq_residual=True, refine=128, device=cd.dev)
    idx = cd.knn.IVFIndex.build(emb, 8, device=cd.dev, storage="pq", pq_m=8, pq_residual=True)
    Dw, Iw = idx.search(emb, 10, 4, refine=128, base=idx.prepare(emb))
    assert torch.equal(Dk, Dw) and torch.equal(Ik, Iw) and (Ik[:, 0].cpu().numpy() == np.arange(n)).all()
    plain = cd.knn.IVFIndex.build(emb, 8, device=cd.dev, storage="pq", pq_m=8)
    assert not torch.equal(plain.codes, idx.codes)
    with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
        cd.knn.export(emb, feats, list("g%04d" % i for i in range(n)), str(tmp_path), doc_location=0, nearest_num=10,
                      desim_nearest_num=5, nlist=8, nprobe=4, storage="f16", pq_residual=True, device=cd.dev)
    assert not os.listdir(str(tmp_path))
    st = {}
    D, I_desim = cd.knn.export(emb, feats, list("g%04d" % i for i in range(n)), str(tmp_path), doc_location=0, nearest_num=10,
                               desim_nearest_num=5, nlist=8, nprobe=4, feature_nlist=8, feature_nprobe=4, storage="pq", pq_m=8,
                               feature_pq_m=16, pq_residual=True, refine=64, device=cd.dev, stats=st)
    assert st["embedding_knn"]["ivf"]["n_tiles"] > 0
    Dw, Iw = idx.search(emb, 10, 4, refine=64, base=idx.prepare(emb))
    assert torch.equal(D, Dw)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "strictI.npy")), Iw.cpu().numpy())
    fidx = cd.knn.IVFIndex.build(feats, 8, device=cd.dev, storage="pq", pq_m=16, pq_residual=True)
    fD, fI = fidx.search(feats, 5, 4, refine=64, base=fidx.prepare(feats))
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "fI.npy")), fI.cpu().numpy())
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "fD.npy")), fD.cpu().numpy())
    assert torch.equal(I_desim, cd.knn.desim(Iw, fI, fD, device=cd.dev))
