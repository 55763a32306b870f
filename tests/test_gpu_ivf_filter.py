"""The threshold-filter search of the IVF index on the MI355X (include/cdml_ivf_filter.h, csrc/ivf_filter.hip, cdml_amd.knn.
IVFIndex.search(scan="filter")): bit for bit against the int64 model of tests/ivf_filter_ref.py on exact grids and against
scan="buffer" everywhere -- both storages, with and without the re-rank, default and minimal seeds, hand-made probe tables, a
tie at tau, forced overflow (the re-search), overflow impossible by construction (the filter alone serves the search),
position independence, the budget rule, non-finite input and mining."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_f16_ref as f16  # noqa: E402
import ivf_filter_ref as flt  # noqa: E402
import ivf_ref as ref  # noqa: E402
from test_gpu_knn import TOL, check  # noqa: E402

pytestmark = pytest.mark.gpu

G_N, G_D, G_NLIST, G_NPROBE, G_K, G_NQ = 2000, 64, 16, 4, 8, 203
STORAGES = ("f32", "f16")


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


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- exact grids: the int64 model and the buffered search, zero tolerance --------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("D", ref.GRID_DIMS)
def test_grid_filter_is_the_int64_model_and_the_buffered_search_bit_for_bit(cd, D, storage):
    c = ref.grid_case(D)
    assert c["safe"] < 2.0 ** 24
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    idx = cd.knn.IVFIndex.from_assignment(x, torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]), l2_norm=False, device=cd.dev,
                                          storage=storage)
    base = idx.prepare(x) if storage == "f16" else None
    col0 = c["probe_hand"].copy()
    col0[:, 0] = -1                                                        # no seed list at all for seed_probes = 1
    col0[40:60, 1] = -1
    tables = (("own", None, c["probe"]), ("hand", c["probe_hand"], c["probe_hand"]), ("col0", col0, col0))
    taus = []
    for k in ref.GRID_KS:
        assert idx.default_seed_probes(k, ref.GRID_NPROBE) == ref.GRID_NPROBE       # lists of 100 rows: the default seeds every column
        for name, given, table in tables:
            probe = None if given is None else torch.from_numpy(given)
            want = ref.grid_want(c, k, probe=table)
            for refine in ((0, xs.LIST) if storage == "f16" else (0,)):
                kw = dict(probe=probe, refine=refine, base=base) if refine else dict(probe=probe)
                buf = idx.search(q, k, ref.GRID_NPROBE, **kw)
                buf = (buf[0].cpu(), buf[1].cpu())
                assert _same(buf, want)                                    # (on the grid the re-ranked answer is the scan's)
                for s in (None, 1, 2):
                    st = {}
                    got = idx.search(q, k, ref.GRID_NPROBE, scan="filter", seed_probes=s, stats=st, **kw)
                    got = (got[0].cpu(), got[1].cpu())
                    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and tuple(got[0].shape) == (ref.GRID_NQ, k)
                    assert _same(got, want) and _same(got, buf), (k, name, refine, s)
                    keep = refine or k
                    assert st["scan"] == "filter" and st["seed_probes"] == (s or ref.GRID_NPROBE)
                    assert st["filter_cap"] == flt.default_filter_cap(keep)
                    if s is None:
                        assert st["n_appended"] == 0 and st["refiltered"] == 0       # nothing left for the filter pass
                    else:
                        # the model itself, with this seed: its merged list is the answer, and its tau is empty for some queries
                        Dm, Im, tau, cands = flt.search(c["d"], c["assign"], c["nlist"], table, s, keep, bad_queries=c["bad_queries"],
                                                        parts=True)
                        assert torch.equal(got[1], torch.from_numpy(Im[:, :k])) and torch.equal(got[0], xs.from_units(Dm[:, :k], c["unit"]))
                        taus.append(int((tau == xs.INF_I).sum()))
                        # every candidate within tau is counted, dropped ones included: the model's count exactly
                        assert st["n_appended"] == sum(len(v) for v in cands) > 0
    assert min(taus) > 1                                                   # tau = +inf occurs (lists of length 0 and 1)


def test_a_tie_at_tau_is_appended(cd):
    """lists {2, 3} (the seed) and {0, 1}: the seed's 2nd distance 5 is tau, row 0 ties with it and has the lower id"""
    D = 32
    x = np.zeros((4, D), dtype=np.float32)
    x[0, :2], x[1, 0], x[2, 0], x[3, :2] = (1, 2), 3, 1, (2, 1)            # |x|^2 = 5, 9, 1, 5; the query is the origin
    assign, probe = np.array([1, 1, 0, 0]), torch.tensor([[0, 1]])
    for storage in STORAGES:
        idx = cd.knn.IVFIndex.from_assignment(torch.from_numpy(x), torch.zeros(2, D), torch.from_numpy(assign), l2_norm=False,
                                              device=cd.dev, storage=storage)
        st = {}
        Dg, Ig = idx.search(torch.zeros(1, D), 2, 2, probe=probe, scan="filter", seed_probes=1, stats=st)
        assert Ig.cpu().tolist() == [[2, 0]] and Dg.cpu().tolist() == [[1.0, 5.0]]
        assert st["n_appended"] == 1 and st["refiltered"] == 0             # row 0 (d = 5 <= tau = 5), not row 1 (d = 9)
        assert _same((Dg, Ig), idx.search(torch.zeros(1, D), 2, 2, probe=probe))


# ---- forced overflow: the re-search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_forced_overflow_is_searched_again(cd, storage):
    c = ref.grid_case(48)
    x, q = torch.from_numpy(c["x"]), torch.from_numpy(c["q"])
    idx = cd.knn.IVFIndex.from_assignment(x, torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]), l2_norm=False, device=cd.dev,
                                          storage=storage)
    probe = c["probe"].copy()
    forced = list(range(30, 50)) + [ref.GRID_NQ - 2]
    probe[forced] = [1, 5, 3]                                              # seed = the one-row list: tau = +inf; 300 + 128 rows behind it
    assert ref.GRID_LENS[1] == 1 and ref.GRID_LENS[5] + ref.GRID_LENS[3] > 64
    tp = torch.from_numpy(probe)
    for k, refine in ((51, 0), (8, 0)) + (((8, 32),) if storage == "f16" else ()):
        kw = dict(refine=refine, base=idx.prepare(x)) if refine else {}
        st = {}
        got = idx.search(q, k, ref.GRID_NPROBE, probe=tp, scan="filter", filter_cap=64, seed_probes=1, stats=st, **kw)
        assert st["refiltered"] >= len(forced) and st["filter_cap"] == 64 and st["n_appended"] >= (300 + 128) * len(forced)
        assert _same(got, idx.search(q, k, ref.GRID_NPROBE, probe=tp, **kw))
        want = ref.grid_want(c, k, probe=probe)
        assert _same((got[0].cpu(), got[1].cpu()), want)
        # ... and in three chunks: the re-searched queries come from every chunk and land in their own rows
        s3 = {}
        total = 4 * (st["n_floats"] + 2 * 64 * ref.GRID_NQ)
        got3 = idx.search(q, k, ref.GRID_NPROBE, probe=tp, scan="filter", filter_cap=64, seed_probes=1, stats=s3,
                          score_bytes=total // 3 - 4096, **kw)
        assert len(s3["chunks"]) >= 3 and s3["refiltered"] == st["refiltered"] and s3["n_appended"] == st["n_appended"]
        assert _same(got3, got)


# ---- unit Gaussian rows ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss(cd):
    rng = np.random.RandomState(13)
    x = _unit32(rng.randn(G_N, G_D))
    q = np.concatenate([_unit32(rng.randn(G_NQ - 3, G_D)), x[[0, 777, G_N - 1]]])
    tx, tq = torch.from_numpy(x).to(cd.dev), torch.from_numpy(q).to(cd.dev)

    class NS:
        pass
    g = NS()
    g.x, g.q, g.tx, g.tq = x, q, tx, tq
    g.idx = {s: cd.knn.IVFIndex.build(tx, G_NLIST, l2_norm=False, device=cd.dev, storage=s) for s in STORAGES}
    g.base = g.idx["f16"].prepare(tx)
    g.probe = g.idx["f32"].probes(tq, G_NPROBE).cpu().numpy().astype(np.int64)
    g.assign = g.idx["f32"].assign.cpu().numpy()
    lens = np.diff(g.idx["f32"].list_start.cpu().numpy())
    g.behind = int(lens[g.probe[:, 1:]].sum(1).max())                      # the largest sum of non-seed probed list lengths
    g.cap = 64
    while g.cap < g.behind:
        g.cap *= 2
    g.buf = {}
    for s, refine in (("f32", 0), ("f16", 0), ("f16", 32)):
        kw = dict(refine=refine, base=g.base) if refine else {}
        g.buf[s, refine] = g.idx[s].search(tq, G_K, G_NPROBE, **kw)
    torch.cuda.synchronize()
    return g


def _kw(g, refine):
    return dict(refine=refine, base=g.base) if refine else {}


@pytest.mark.parametrize("storage,refine", [("f32", 0), ("f16", 0), ("f16", 32)])
def test_overflow_impossible_by_construction(cd, gauss, storage, refine):
    """A candidate table as long as a query's non-seed lists cannot overflow: the filter pass alone serves the search (a search
    served wholly by the re-search would pass every equality test)."""
    g, idx = gauss, gauss.idx[storage]
    seed = idx.default_seed_probes(refine or G_K, G_NPROBE)               # 1 column for keep = 8, 2 for keep = 32 (125 rows a list)
    assert seed == (2 if refine else 1) and g.cap >= g.behind > 64        # (the lists behind two seed columns are fewer still)
    assert torch.equal(idx.probes(g.tq, G_NPROBE).cpu(), torch.from_numpy(g.probe))
    st = {}
    got = idx.search(g.tq, G_K, G_NPROBE, scan="filter", filter_cap=g.cap, stats=st, **_kw(g, refine))
    assert st["refiltered"] == 0 and st["n_appended"] > 0 and st["seed_probes"] == seed and st["filter_cap"] == g.cap
    assert st["n_appended"] < g.behind * G_NQ // 2                         # ... and tau does filter
    assert _same(got, g.buf[storage, refine])
    Dg, Ig = got[0].cpu().numpy(), got[1].cpu().numpy()
    if storage == "f32":
        d = ref.fp64_dist(g.q, g.x, l2_norm=False)
        Dr, Ir = ref.search(d, g.assign, G_NLIST, g.probe, G_K)
        dfull = np.maximum(d, 0.0)
    elif not refine:
        Dr, Ir = f16.scan_search(g.q, g.x, g.assign, G_NLIST, g.probe, G_K)
        dfull = np.maximum(f16.rounded_dist(g.q, g.x), 0.0)
    else:
        cand = st["candidates"].cpu().numpy().astype(np.int64)
        table = np.full((G_NQ, xs.LIST), xs.NO_ID, dtype=np.int64)
        table[:, :refine] = cand
        Dr, Ir = f16.refine(g.q, g.x, table, refine, G_K)
        dfull = np.maximum(ref.fp64_dist(g.q, g.x, l2_norm=False), 0.0)
    err = np.abs(Dg[np.isfinite(Dr)] - Dr[np.isfinite(Dr)]).max()
    print("filter %s refine=%d: n_appended / query %.1f, max |d - fp64 model| = %.3g (TOL %.0e)"
          % (storage, refine, st["n_appended"] / G_NQ, err, TOL))
    check(Dg, Ig, Dr, Ir, dfull)
    assert (Ig[-3:, 0] == [0, 777, G_N - 1]).all()                         # a catalogue row finds itself


@pytest.mark.parametrize("storage,refine", [("f32", 0), ("f16", 0), ("f16", 32)])
def test_position_independence(cd, gauss, storage, refine):
    g, idx = gauss, gauss.idx[storage]
    want = g.buf[storage, refine]
    for cap in (None, g.cap):                                              # with and without re-searched queries
        s1 = {}
        assert _same(idx.search(g.tq, G_K, G_NPROBE, scan="filter", filter_cap=cap, stats=s1, **_kw(g, refine)), want)
        assert len(s1["chunks"]) == 1
        total = 4 * (s1["n_floats"] + 2 * s1["filter_cap"] * G_NQ)        # the bytes the one chunk was planned with
        st = {}
        got = idx.search(g.tq, G_K, G_NPROBE, scan="filter", filter_cap=cap, score_bytes=total // 3 - 4096, stats=st, **_kw(g, refine))
        assert len(st["chunks"]) >= 3 and st["n_floats"] == s1["n_floats"] and st["n_appended"] == s1["n_appended"]
        assert st["refiltered"] == s1["refiltered"] and (cap is None or st["refiltered"] == 0)
        print("%s refine=%d cap=%d: %d chunks, %d re-searched" % (storage, refine, st["filter_cap"], len(st["chunks"]), st["refiltered"]))
        assert _same(got, want)
        perm = torch.from_numpy(np.random.RandomState(5).permutation(G_NQ)).to(cd.dev)
        D3, I3 = idx.search(g.tq[perm], G_K, G_NPROBE, scan="filter", filter_cap=cap, score_bytes=total // 2, **_kw(g, refine))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(G_NQ, device=cd.dev)
        assert _same((D3[inv], I3[inv]), want)
    for s in (2, 3, G_NPROBE):                                             # any seed width
        assert _same(idx.search(g.tq, G_K, G_NPROBE, scan="filter", seed_probes=s, **_kw(g, refine)), want)


@pytest.mark.parametrize("storage", STORAGES)
def test_budget_accepts_what_the_buffer_refuses(cd, gauss, storage):
    g, idx = gauss, gauss.idx[storage]
    tp = torch.from_numpy(g.probe).to(torch.int32).to(cd.dev)
    budget = 4 * int(idx.filter_costs(tp, 1, 64).max())                   # every query's seed list + 64 slots fit ...
    ld = (np.diff(idx.list_start.cpu().numpy()) + 3) // 4 * 4
    assert 4 * int(ld[g.probe].sum(1).max()) > budget                      # ... some query's four lists do not
    with pytest.raises(ValueError, match="own scores"):
        idx.search(g.tq, G_K, G_NPROBE, score_bytes=budget)
    st = {}
    got = idx.search(g.tq, G_K, G_NPROBE, score_bytes=budget, scan="filter", filter_cap=64, stats=st)
    assert _same(got, g.buf[storage, 0]) and len(st["chunks"]) > G_NQ // 2
    print("budget %d B: %d chunks, %d re-searched of %d" % (budget, len(st["chunks"]), st["refiltered"], G_NQ))


# ---- non-finite input --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_non_finite_rows_and_queries(cd, storage):
    rng = np.random.RandomState(17)
    n, D, nlist, nq, k = 400, 32, 4, 20, 10
    x, q = _unit32(rng.randn(n, D)), _unit32(rng.randn(nq, D))
    cent = _unit32(rng.randn(nlist, D))
    assign = rng.randint(0, nlist, size=n)
    probe = torch.from_numpy(np.stack([rng.permutation(nlist)[:3] for _ in range(nq)]))
    mk = lambda rows: cd.knn.IVFIndex.from_assignment(torch.from_numpy(rows), torch.from_numpy(cent), torch.from_numpy(assign),
                                                      l2_norm=False, device=cd.dev, storage=storage)
    Dc, Ic = mk(x).search(torch.from_numpy(q), k, 3, probe=probe)
    x2, q2 = x.copy(), q.copy()
    nan_row, big_row = int(Ic[0, 0]), int(Ic[1, 0])
    x2[nan_row, 3] = np.nan                                                # unlisted for both storages
    x2[big_row, 5] = 1e5                                                   # listed in fp32, overflows in fp16
    q2[7, 2] = np.nan                                                      # a NaN query WITH real probes (the table is given) ...
    q2[9, 4] = 1e5                                                         # ... and one that overflows in fp16
    idx = mk(x2)
    assert idx.n_unlisted == (2 if storage == "f16" else 1)
    tq = torch.from_numpy(q2)
    for kw in (dict(probe=probe), {}):                                     # the given table, and the index's own probes
        buf = idx.search(tq, k, 3, **kw)
        for cap, s in ((None, None), (64, 1), (1024, 1), (1024, 2)):
            st = {}
            got = idx.search(tq, k, 3, scan="filter", filter_cap=cap, seed_probes=s, stats=st, **kw)
            assert _same(got, buf), (cap, s)
            assert (got[1][7] == -1).all() and bool(torch.isinf(got[0][7]).all())
            assert nan_row not in got[1].cpu().numpy()
            if storage == "f16":
                assert (got[1][9] == -1).all() and big_row not in got[1].cpu().numpy()
            if cap == 1024:
                assert st["refiltered"] == 0 and st["n_appended"] > 0     # the NaN query appended nothing and lost nothing


# ---- mining ----------------------------------------------------------------------------------------------------------------------
def test_mining_with_the_filter_scan(cd):
    rng = np.random.RandomState(9)
    n, D, k, skip, nlist, nprobe = 3000, 64, 16, 2, 16, 4
    e = torch.from_numpy(rng.randn(n, D).astype(np.float32)).to(cd.dev)
    a = rng.randint(0, n, size=500)
    pairs = torch.from_numpy(np.stack([a, (a + 1 + rng.randint(0, n - 1, size=500)) % n], 1).astype(np.int32))
    for kw in ({}, dict(storage="f16", refine=64)):
        want = cd.hardneg.mine_lists(e, k, skip, pairs, device=cd.dev, nlist=nlist, nprobe=nprobe, **kw)
        got = cd.hardneg.mine_lists(e, k, skip, pairs, device=cd.dev, nlist=nlist, nprobe=nprobe, scan="filter", **kw)
        assert torch.equal(got, want) and (got >= 0).float().mean().item() > 0.9
