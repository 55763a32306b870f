"""The range search of the IVF index on the MI355X (cdml_amd.knn.IVFIndex.range_search; include/cdml_ivf_range.h,
csrc/ivf_range.hip for product-quantised lists, the filter scans of include/cdml_ivf_filter.h for fp32 / fp16 lists): bit for bit
against the int64 model of tests/ivf_range_ref.py on the exact grids of every storage (a tie AT the radius, a radius inside a
gap), every instance of the two new kernels on the PQ scan's tile edges, against ``search`` itself on unit Gaussian rows, the
second pass (forced, split, impossible), the radius edges, position independence, an index after updates, ``ivf_range``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_pqr_ref as pqr  # noqa: E402
import ivf_range_ref as rr  # noqa: E402
import ivf_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = [("f32", 48, 0), ("f32", 256, 0), ("f16", 48, 0), ("f16", 256, 0),
        ("pq-lossless", 48, 8), ("pq-lossless", 256, 64), ("pq-lossy", 48, 8), ("pq-lossy", 256, 64),
        ("pqr-lossless", 48, 8), ("pqr-lossless", 256, 64), ("pqr-lossy", 48, 8), ("pqr-lossy", 256, 64)]
TILE_MS = list(range(8, 72, 8))           # every instance of the kernels: M / 8 = 1..8
G_N, G_D, G_NLIST, G_NPROBE, G_NQ = 2000, 64, 16, 4, 203
G_KINDS = ("f32", "f16", "pq", "pqr")


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


def _grid(cd, kind, D, M):
    """(case, index, the model's distance matrix) of one exact grid"""
    if kind in ("f32", "f16"):
        c = ref.grid_case(D)
        kw, d = dict(storage=kind), c["d"]                # (grid values are fp16 numbers: the fp16 lists lose nothing)
    else:
        form, loss = kind.split("-")
        c = getattr(pqr if form == "pqr" else pq, loss + "_case")(D, M)
        kw, d = dict(storage="pq", codebooks=torch.from_numpy(c["cb"]), pq_residual=form == "pqr"), c["d_pq"]
    assert c["safe"] < 2.0 ** 24
    idx = cd.knn.IVFIndex.from_assignment(torch.from_numpy(c["x"]), torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]),
                                          l2_norm=False, device=cd.dev, **kw)
    return c, idx, d


def _radius(rad, unit):
    """the model's radii (float64, in units) as the fp32 tensor the index takes; exact"""
    v = np.asarray(rad, np.float64) * unit
    w = v.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), v, equal_nan=True)
    return torch.from_numpy(w)


def _same(got, want):
    for g, w, name in zip(got, want, ("lims", "D", "I")):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), name


def _model(c, d, probe, rad, **rule):
    return rr.as_tensors(rr.range_search(d, c["assign"], c["nlist"], probe, rad, bad_queries=c.get("bad_queries", ()), **rule),
                         c["unit"])


# ---- exact grids ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,M", GRID)
def test_grid_is_the_model_bit_for_bit(cd, kind, D, M):
    c, idx, d = _grid(cd, kind, D, M)
    q = torch.from_numpy(c["q"])
    bad = c["bad_queries"]
    args = (d, c["assign"], c["nlist"])
    for k in ref.GRID_KS:                                 # the k-th distance: a tie AT the radius; the index's own probes
        rad = rr.kth_radius(*args, c["probe"], k, bad_queries=bad)
        want = _model(c, d, c["probe"], rad)
        n = want[0][1:] - want[0][:-1]
        assert int(n[ref.GRID_FEW]) == 6 and int(n[ref.GRID_NAN_QUERY]) == 0 and int((n >= k).sum()) > 250
        lost = _model(c, d, c["probe"], rad, strict=True)[0]
        assert int(((lost[1:] - lost[:-1]) < n).sum()) > 250              # (`<` would lose a row of most queries)
        st = {}
        got = idx.range_search(q, _radius(rad, c["unit"]), ref.GRID_NPROBE, stats=st)
        _same(got, want)
        assert st["n_results"] == int(want[0][-1]) and st["range_cap"] == 256 and c["nan_row"] not in got[2].cpu().numpy()
    # a radius halfway between two distinct model distances, a probe table with -1 entries
    rad = rr.gap_radius(*args, c["probe_hand"], 60, bad_queries=bad)
    for i in range(ref.GRID_NQ):
        dq = np.maximum(d[i, rr.members_of(c["assign"], c["nlist"], c["probe_hand"][i])], 0)
        assert not (dq == rad[i]).any()
    want = _model(c, d, c["probe_hand"], rad)
    assert all(torch.equal(a, b) for a, b in zip(want, _model(c, d, c["probe_hand"], rad, strict=True)))
    got = idx.range_search(q, _radius(rad, c["unit"]), ref.GRID_NPROBE, probe=torch.from_numpy(c["probe_hand"]))
    _same(got, want)
    assert int(want[0][-1]) > 30 * ref.GRID_NQ and int(want[0][26]) == int(want[0][25])   # (query 25 probes nothing)


# ---- every kernel instance on the scan's tile edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("M", TILE_MS)
def test_tile_edges(cd, M, residual):
    """list lengths 0, 1, R - 1, R, R + 1, 2 R + 5; lists probed by S - 1, S, S + 1 and S + 2 queries; -1 probes: against the
    int64 model at a mid-gap radius and at +inf (where the counts are the probed lists' lengths and the second pass runs)"""
    import math
    S, R = cd.ops.ivf_pq_tile(M)
    assert (S, R) == (64 // M, 1024)
    c = rr.tile_case(M, math.lcm(2 * M, 32), S, R, residual)              # (asserts assert_select_exact_safe < 2^24)
    idx = cd.knn.IVFIndex.from_assignment(torch.from_numpy(c["x"]), torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]),
                                          l2_norm=False, device=cd.dev, storage="pq", codebooks=torch.from_numpy(c["cb"]),
                                          pq_residual=residual)
    ids, _ = ref.lists_from_assign(c["assign"], c["nlist"])
    assert torch.equal(idx.codes.cpu().long(), torch.from_numpy(c["codes"][ids])) and idx.list_len.cpu().tolist() == list(c["lens"])
    q, probe = torch.from_numpy(c["q"]), c["probe"]
    lens = np.asarray(c["lens"])
    probed = np.where(probe >= 0, lens[np.maximum(probe, 0)], 0).sum(1)
    for sl in (slice(None), slice(1, None)):                              # list 5 probed by S + 2 queries, and by S + 1
        p = probe[sl]
        rad = rr.gap_radius(c["d"][sl], c["assign"], c["nlist"], p, 40)
        for i in range(len(p)):
            assert not (np.maximum(c["d"][sl][i, rr.members_of(c["assign"], c["nlist"], p[i])], 0) == rad[i]).any()
        for r in (rad, np.full(len(p), np.inf)):
            want = rr.as_tensors(rr.range_search(c["d"][sl], c["assign"], c["nlist"], p, r), c["unit"])
            st = {}
            got = idx.range_search(q[sl], _radius(r, c["unit"]), 2, probe=torch.from_numpy(p), stats=st)
            _same(got, want)
        assert np.array_equal(np.diff(got[0].cpu().numpy()), probed[sl])   # +inf: every probed listed row
        assert st["second_pass"] == int((probed[sl] > 256).sum()) > S and st["second_cap"] == 4096


# ---- against search itself -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss(cd):
    rng = np.random.RandomState(21)
    x = torch.from_numpy(rng.randn(G_N, G_D).astype(np.float32)).to(cd.dev)
    q = torch.cat([torch.from_numpy(rng.randn(G_NQ - 3, G_D).astype(np.float32)).to(cd.dev), x[[0, 777, G_N - 1]]])

    class NS:
        pass
    g = NS()
    g.x, g.q, g.idx = x, q, {}

    def index(kind):
        if kind not in g.idx:
            kw = dict(storage="pq", pq_m=8, pq_residual=kind == "pqr") if kind.startswith("pq") else dict(storage=kind)
            g.idx[kind] = cd.knn.IVFIndex.build(x, G_NLIST, device=cd.dev, **kw)
        return g.idx[kind]
    g.index = index
    return g


def _spans(res):
    lims, D, I = (t.cpu() for t in res)
    return [(D[lims[i]:lims[i + 1]], I[lims[i]:lims[i + 1]]) for i in range(lims.numel() - 1)]


@pytest.mark.parametrize("kind", G_KINDS)
def test_radius_of_the_kth_neighbour_returns_the_search(cd, gauss, kind):
    idx = gauss.index(kind)
    for k in (10, 51):
        st = {}
        Dk, Ik = idx.search(gauss.q, k, G_NPROBE, stats=st)
        res = idx.range_search(gauss.q, Dk[:, k - 1].contiguous(), G_NPROBE, probe=st["probe"])
        assert res[0].dtype == torch.int64 and res[1].dtype == torch.float32 and res[2].dtype == torch.int64
        assert res[0].device.type == "cuda" and int(res[0][0]) == 0 and int(res[0][-1]) == res[1].numel() == res[2].numel()
        Dk, Ik = Dk.cpu(), Ik.cpu()
        for i, (D, I) in enumerate(_spans(res)):
            assert len(D) >= k and torch.equal(D[:k], Dk[i]) and torch.equal(I[:k], Ik[i]), (kind, k, i)
            assert bool((D[k:] == Dk[i, k - 1]).all())                    # what lies behind ties with the k-th


# ---- the second pass -------------------------------------------------------------------------------------------------------------
def test_second_pass_forced_split_and_impossible(cd):
    c, idx, d = _grid(cd, "f32", 48, 0)
    q = torch.from_numpy(c["q"])
    want = _model(c, d, c["probe"], np.inf)
    n = (want[0][1:] - want[0][:-1]).numpy()
    over = int((n > 64).sum())
    assert n[0] >= 300 and 5 in c["probe"][0] and over > 140 and n.max() <= 1024          # query 0 probes the 300-row list
    st = {}
    _same(idx.range_search(q, float("inf"), ref.GRID_NPROBE, range_cap=64, stats=st), want)
    assert st["second_pass"] == over >= 1 and st["second_cap"] == 1024 >= 512 and st["range_cap"] == 64
    assert st["n_results"] == int(n.sum()) and len(st["chunks"]) == 1
    # a budget that splits the second pass (8 KiB a query there) and the first (512 B a query)
    budget = 8 * 1024 * 50
    assert over * 8 * st["second_cap"] > budget
    st2 = {}
    _same(idx.range_search(q, float("inf"), ref.GRID_NPROBE, range_cap=64, result_bytes=budget, stats=st2), want)
    assert st2["second_pass"] == over and st2["second_cap"] == 1024 and st2["n_tiles"] > st["n_tiles"]
    # a budget below one query of the second pass is refused by name
    with pytest.raises(ValueError, match=r"result_bytes = 8191 is less than the 8192 bytes"):
        idx.range_search(q, float("inf"), ref.GRID_NPROBE, range_cap=64, result_bytes=8191)
    # no second pass where the capacity holds every probed row
    assert n.max() <= 1024
    st3 = {}
    _same(idx.range_search(q, float("inf"), ref.GRID_NPROBE, range_cap=1024, stats=st3), want)
    assert st3["second_pass"] == 0 and st3["second_cap"] == 0


# ---- radius edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,M", [("f32", 48, 0), ("f16", 48, 0), ("pq-lossy", 48, 8), ("pqr-lossy", 48, 8)])
def test_radius_edges(cd, kind, D, M):
    c, idx, d = _grid(cd, kind, D, M)
    q = torch.from_numpy(c["q"])
    probe = c["probe_hand"]
    rad = rr.gap_radius(d, c["assign"], c["nlist"], probe, 30, bad_queries=c["bad_queries"])
    rad[[0, 1, 2, 50]] = 0.0
    rad[7], rad[8], rad[9] = -1.0, np.nan, np.inf
    want = _model(c, d, probe, rad)
    n = (want[0][1:] - want[0][:-1]).numpy()
    assert n[7] == 0 and n[8] == 0 and n[25] == 0 and n[ref.GRID_NAN_QUERY] == 0 and n[9] > 100
    got = idx.range_search(q, _radius(rad, c["unit"]), ref.GRID_NPROBE, probe=torch.from_numpy(probe))
    _same(got, want)
    assert c["nan_row"] not in got[2].cpu().numpy()
    # a NaN query with a probe table that names lists, and radius +inf for all: still nothing for it
    probe2 = c["probe"].copy()
    probe2[ref.GRID_NAN_QUERY] = [5, 3, 2]
    got = idx.range_search(q, float("inf"), ref.GRID_NPROBE, probe=torch.from_numpy(probe2))
    want = _model(c, d, probe2, np.inf)                   # (bad_queries: the model gives it nothing)
    _same(got, want)
    assert int(got[0][ref.GRID_NAN_QUERY + 1] - got[0][ref.GRID_NAN_QUERY]) == 0 and c["nan_row"] not in got[2].cpu().numpy()
    # radius 0 finds what ties with the query itself: catalogue rows as queries, each probing its own list (the planted
    # source: itself and its two duplicates in that list, not the two in another one)
    if kind in ("f32", "f16"):
        rows = [c["src"], c["dups"][0], 0, 1]
        probe0 = np.array([[c["assign"][r], -1, -1] for r in rows], dtype=np.int64)
        want = rr.as_tensors(rr.range_search(xs.grid_dist(c["xi"][rows], c["xi"]), c["assign"], c["nlist"], probe0, 0.0), c["unit"])
        assert (want[0][1:] - want[0][:-1]).tolist()[:2] == [3, 3] and bool((want[1] == 0).all()) and c["src"] in want[2][:3].tolist()
        _same(idx.range_search(torch.from_numpy(c["x"][rows]), 0.0, ref.GRID_NPROBE, probe=torch.from_numpy(probe0)), want)
    # scalar radii of every kind
    for r in (-1.0, float("nan")):
        lims, Dg, Ig = idx.range_search(q, r, ref.GRID_NPROBE)
        assert not bool(lims.any()) and Dg.numel() == 0 and Ig.numel() == 0


# ---- position independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G_KINDS)
def test_position_independence(cd, gauss, kind):
    idx = gauss.index(kind)
    Dk, _ = idx.search(gauss.q, 40, G_NPROBE)
    rad = Dk[:, 39].contiguous()
    rad[::7] = Dk[::7, 5]
    s0 = {}
    whole = _spans(idx.range_search(gauss.q, rad, G_NPROBE, stats=s0))
    assert len(s0["chunks"]) == 1
    perm = torch.from_numpy(np.random.RandomState(3).permutation(G_NQ)).to(cd.dev)
    budget = 4 * int(idx.range_costs(G_NQ, G_NPROBE, 64)[0]) * (G_NQ // 4)
    s1 = {}
    parts = _spans(idx.range_search(gauss.q[perm], rad[perm], G_NPROBE, range_cap=64, result_bytes=budget, stats=s1))
    assert len(s1["chunks"]) >= 3 and s1["range_cap"] == 64
    for j, i in enumerate(perm.cpu().tolist()):
        assert torch.equal(parts[j][0], whole[i][0]) and torch.equal(parts[j][1], whole[i][1]), (kind, i)


# ---- after updates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G_KINDS)
def test_after_updates_equals_from_assignment(cd, gauss, kind):
    kw = dict(storage="pq", pq_m=8, pq_residual=kind == "pqr") if kind.startswith("pq") else dict(storage=kind)
    idx = cd.knn.IVFIndex.train(gauss.x[:1000], G_NLIST, device=cd.dev, **kw)
    idx.add(gauss.x[:1500])
    idx.remove(torch.arange(3, 1500, 11))
    idx.add(gauss.x[1500:])
    assert idx.n_rows == G_N and idx.n_listed == G_N - len(range(3, 1500, 11))
    kw2 = dict(l2_norm=idx.l2_norm, precision=idx.precision, storage=idx.storage)
    if idx.storage == "pq":
        kw2.update(codebooks=idx.codebooks, pq_residual=idx.pq_residual)
    twin = cd.knn.IVFIndex.from_assignment(gauss.x, idx.centroids, idx.assign, device=cd.dev, **kw2)
    Dk, _ = twin.search(gauss.q, 30, G_NPROBE)
    rad = Dk[:, 29].contiguous()
    a = idx.range_search(gauss.q, rad, G_NPROBE)
    b = twin.range_search(gauss.q, rad, G_NPROBE)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and int(a[0][-1]) >= 30 * G_NQ
    assert not bool(torch.isin(a[2], torch.arange(3, 1500, 11, device=cd.dev)).any())      # the removed rows are gone


# ---- ivf_range ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "pqr"])
def test_ivf_range_is_build_then_range_search(cd, gauss, kind):
    kw = dict(storage="pq", pq_m=8, pq_residual=True) if kind == "pqr" else dict(storage=kind)
    idx = gauss.index(kind)
    st = {}
    a = cd.knn.ivf_range(gauss.x, None, radius=0.8, nlist=G_NLIST, nprobe=G_NPROBE, device=cd.dev, stats=st, **kw)
    b = idx.range_search(gauss.x, 0.8, G_NPROBE)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and tuple(a[0].shape) == (G_N + 1,) and st["n_results"] == int(a[0][-1])
    if kind == "f32":                                     # the self-search: every row finds itself
        owner = torch.repeat_interleave(torch.arange(G_N, device=cd.dev), a[0][1:] - a[0][:-1])
        assert int((a[2] == owner).sum()) == G_N
    c = cd.knn.ivf_range(gauss.x, gauss.q, radius=0.8, nprobe=G_NPROBE, index=idx)
    assert all(torch.equal(u, v) for u, v in zip(c, idx.range_search(gauss.q, 0.8, G_NPROBE)))
    with pytest.raises(ValueError, match="range_search has no launch for pq_bits=4"):
        cd.knn.IVFIndex.build(gauss.x, G_NLIST, device=cd.dev, storage="pq", pq_m=8, pq_bits=4).range_search(gauss.q, 0.8, G_NPROBE)
