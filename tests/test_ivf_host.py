"""CPU-side checks of the IVF index (include/cdml_ivf.h, cdml_amd.knn.IVFIndex): the host models of tests/ivf_ref.py against
the exact oracle and against their own mutations, the query-chunk planner and the slot / tile tables (pure host / torch
arithmetic), the refusals of IVFIndex and of the C ABI (before any HIP call), header == binding table == library."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_ref as ref  # noqa: E402
from oracle import knn as oknn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


# ---- the models -------------------------------------------------------------------------------------------------------------
def test_search_model_at_nprobe_nlist_is_calc_knn_exact():
    rng = np.random.RandomState(0)
    n, D, nlist, k = 400, 32, 7, 51
    b, q = rng.randn(n, D).astype(np.float32), rng.randn(30, D).astype(np.float32)
    assign = rng.randint(0, nlist, size=n)
    probe = np.tile(np.arange(nlist), (30, 1))
    Dm, Im = ref.search(ref.fp64_dist(q, b), assign, nlist, probe, k)
    Dr, Ir, _ = oknn.calc_knn_exact(b, q, k)
    assert np.array_equal(Im, Ir) and np.array_equal(Dm, Dr)
    # fewer rows than k: the tail is +inf / -1, as the oracle's
    Dm, Im = ref.search(ref.fp64_dist(q, b[:20]), assign[:20], nlist, probe, k)
    Dr, Ir, _ = oknn.calc_knn_exact(b[:20], q, k)
    assert np.array_equal(Im, Ir) and np.array_equal(Dm, Dr)


def test_lists_and_probes_models():
    assign = np.array([2, 0, -1, 2, 0, 2, 4])
    ids, start = ref.lists_from_assign(assign, 5)
    assert ids.tolist() == [1, 4, 0, 3, 5, 6] and start.tolist() == [0, 2, 2, 5, 5, 6]
    dc = np.array([[3, 1, 1, 0], [5, 5, 5, 5]], dtype=np.int64)
    assert ref.probes(dc, 3).tolist() == [[3, 1, 2], [0, 1, 2]]           # ties to the lower centroid id
    assert ref.probes(dc, 2, bad_queries=(1,)).tolist() == [[3, 1], [-1, -1]]
    dcf = np.array([[0.5, np.nan, 0.25]])
    assert ref.probes(dcf, 3).tolist() == [[2, 0, -1]]                    # a NaN centroid is nobody's nearest


def test_lloyd_model_descends_and_keeps_empty_lists():
    rng = np.random.RandomState(1)
    x = rng.randn(300, 8)
    C, a, obj = ref.lloyd(x, np.arange(6), 8)
    assert (np.diff(obj) <= 1e-9).all() and len(obj) == 8
    a2, _ = ref.nearest(x, C)
    assert np.array_equal(a, a2)
    far = np.concatenate([x, [[1e3] * 8]])                                # a centroid nobody is assigned to keeps its place
    keep = ref.column_means(far[:300], np.zeros(300, dtype=np.int64), 2, keep=far[[0, 300]])
    assert np.array_equal(keep[1], far[300]) and np.allclose(keep[0], x.mean(0))


@pytest.mark.parametrize("D", ref.GRID_DIMS)
def test_grid_case_conditions_and_mutations(D):
    c = ref.grid_case(D)
    assert c["safe"] < 2.0 ** 24
    assert sorted(np.bincount(c["assign"][c["assign"] >= 0], minlength=c["nlist"]).tolist()) == sorted(ref.GRID_LENS)
    assert c["assign"][c["nan_row"]] == -1 and np.isnan(c["x"][c["nan_row"]]).any() and np.isnan(c["q"][ref.GRID_NAN_QUERY]).any()
    # the duplicates tie with their source: below and above its id, in its own list and in another one
    a = c["assign"]
    assert a[c["dups"][0]] == a[c["src"]] == a[c["dups"][1]] and a[c["dups"][2]] == a[c["dups"][3]] != a[c["src"]]
    assert c["dups"][0] < c["src"] < c["dups"][1] and c["dups"][2] < c["src"] < c["dups"][3]
    seen = {m: False for m in ("tie", "clamp", "minus one", "unlisted", "empty")}
    for k in ref.GRID_KS:
        args = (c["assign"], c["nlist"])
        want = ref.search(c["d"], *args, c["probe"], k, bad_queries=c["bad_queries"])
        assert (want[1][ref.GRID_NAN_QUERY] == -1).all() and (want[0][ref.GRID_NAN_QUERY] == xs.INF_I).all()
        if k == 128:
            assert (want[1][ref.GRID_FEW] >= 0).sum() == 6                # fewer rows probed than k
        rows = want[1][want[1] >= 0]
        assert c["nan_row"] not in rows
        seen["tie"] |= _differs(ref.search(c["d"], *args, c["probe"], k, bad_queries=c["bad_queries"], tie_larger=True), want)
        seen["unlisted"] |= _differs(ref.search(c["d"], *args, c["probe"], k, bad_queries=c["bad_queries"], list_unlisted=True), want)
        seen["empty"] |= _differs(ref.search(c["d"], *args, c["probe"], k, bad_queries=c["bad_queries"], empty_borrows=True), want)
        hand = ref.search(c["d"], *args, c["probe_hand"], k, bad_queries=c["bad_queries"])
        assert (hand[1][25] == -1).all()                                  # every probe -1: nothing
        seen["minus one"] |= _differs(ref.search(c["d"], *args, c["probe_hand"], k, bad_queries=c["bad_queries"],
                                                 minus_one_is_last=True), hand)
        low = ref.search(c["d_low"], *args, c["probe"], k, bad_queries=c["bad_queries"])
        assert (low[0] >= 0).all() and (c["d_low"] < 0).any()
        seen["clamp"] |= _differs(ref.search(c["d_low"], *args, c["probe"], k, bad_queries=c["bad_queries"], clamp=False), low)
        # the float32 tensors the GPU test compares with exist (every expected distance is an fp32 number)
        ref.grid_want(c, k)
        ref.grid_want(c, k, low=True)
    assert all(seen.values()), seen


# ---- the planner and the tables ------------------------------------------------------------------------------------------------
def test_chunk_planner_stays_inside_the_budget_and_covers_every_query_once():
    from cdml_amd import knn
    rng = np.random.RandomState(2)
    for trial in range(20):
        costs = rng.randint(0, 5000, size=rng.randint(1, 400))
        budget = int(4 * max(costs.max(), 1) * rng.choice([1, 2, 7.5, 100]))
        chunks = knn.ivf_plan_chunks(costs, budget)
        assert chunks[0][0] == 0 and chunks[-1][1] == len(costs)
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(q0 < q1 for q0, q1 in chunks)
        assert all(4 * costs[q0:q1].sum() <= budget for q0, q1 in chunks)
        # greedy: a chunk ends only where the next query would not fit
        assert all(4 * costs[q0:q1 + 1].sum() > budget for q0, q1 in chunks[:-1])
    assert knn.ivf_plan_chunks([4, 4, 4, 4, 4], 10 ** 9, max_queries=2) == [(0, 2), (2, 4), (4, 5)]
    assert knn.ivf_plan_chunks(np.zeros(5, dtype=np.int64), 16) == [(0, 5)]
    assert knn.ivf_plan_chunks([], 16) == []
    with pytest.raises(ValueError, match="score_bytes"):
        knn.ivf_plan_chunks([10, 300, 10], 4 * 299)
    assert knn.ivf_plan_chunks([10, 300, 10], 4 * 300) == [(0, 1), (1, 2), (2, 3)]


def test_slot_and_tile_tables():
    from cdml_amd import knn
    rng = np.random.RandomState(3)
    nlist, m, nprobe = 9, 310, 3
    lens = np.array([0, 1, 127, 128, 129, 300, 5, 130, 64])
    probe = np.stack([rng.choice(nlist, size=nprobe, replace=False) for _ in range(m)])
    for q in range(200):                                                  # 200+ slots on the 300-row list: two slot tiles
        probe[q] = [5] + list(rng.choice([c for c in range(nlist) if c != 5], size=2, replace=False))
    probe[7] = -1
    probe[9, 1] = -1
    tb = knn.ivf_tables(torch.from_numpy(probe).to(torch.int32), torch.from_numpy(lens))
    valid = probe >= 0
    assert tb["n_slots"] == valid.sum()
    sq, so, sof = tb["slot_query"].numpy(), tb["slot_off"].numpy(), tb["slot_of"].numpy()
    start = tb["slot_start"].numpy()
    ld = (lens + 3) // 4 * 4
    assert (sof[~valid] == -1).all() and sorted(sof[valid].tolist()) == list(range(tb["n_slots"]))
    end = 0
    for c in range(nlist):
        qs = np.nonzero((probe == c).any(1))[0]                           # by query inside a list
        assert sq[start[c]:start[c + 1]].tolist() == qs.tolist()
        for i, q in enumerate(qs):
            s = start[c] + i
            assert sof[q, list(probe[q]).index(c)] == s and so[s] == end + i * ld[c] and so[s] % 4 == 0
        end += len(qs) * ld[c]
    assert tb["n_floats"] == end
    # the tiles cover every (slot, row) of every list with slots and rows exactly once, list by list
    t = tb["tiles"].numpy()
    assert t.shape == (tb["n_tiles"], 4) and (np.diff(t[:, 0]) >= 0).all() and (t[:, 3] == 0).all()
    for c in range(nlist):
        cnt = start[c + 1] - start[c]
        tc = t[t[:, 0] == c]
        want = [(i, j) for i in range(0, cnt, knn.IVF_TILE) for j in range(0, lens[c], knn.IVF_TILE)]
        assert sorted(map(tuple, tc[:, 1:3].tolist())) == want
    # a chunk with nothing to scan
    tb0 = knn.ivf_tables(torch.full((4, 2), -1, dtype=torch.int32), torch.from_numpy(lens))
    assert (tb0["n_slots"], tb0["n_floats"], tb0["n_tiles"]) == (0, 0, 0) and tb0["tiles"].shape == (0, 4)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_index_refusals_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn, ops
    cap = ops.knn_list_capacity()
    x = torch.randn(10, 8)
    x[3, 2] = float("nan")
    with pytest.raises(ValueError, match="nlist"):
        knn.IVFIndex.build(x, 0)
    with pytest.raises(ValueError, match="nlist"):
        knn.IVFIndex.build(x, 10)                                         # nine finite rows
    with pytest.raises(ValueError, match="train_rows"):
        knn.IVFIndex.build(x, 4, train_rows=3)
    with pytest.raises(ValueError, match="iters"):
        knn.IVFIndex.build(x, 4, iters=-1)
    with pytest.raises(ValueError, match="dimension mismatch"):
        knn.IVFIndex.from_assignment(x, torch.zeros(3, 7), torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="assign"):
        knn.IVFIndex.from_assignment(x, torch.zeros(3, 8), torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="assign"):
        knn.IVFIndex.from_assignment(x, torch.zeros(3, 8), torch.full((10,), 3, dtype=torch.int64))
    with pytest.raises(TypeError):
        knn.IVFIndex()
    idx = knn.IVFIndex._blank(6, 8, True, "cuda:0", "f32x3")              # the checks of search / probes come before any device work
    q = torch.randn(5, 8)
    for k in (0, cap + 1):
        with pytest.raises(ValueError, match="k must be"):
            idx.search(q, k, 2)
    for nprobe in (0, 7):
        with pytest.raises(ValueError, match="nprobe"):
            idx.search(q, 5, nprobe)
        with pytest.raises(ValueError, match="nprobe"):
            idx.probes(q, nprobe)
    with pytest.raises(ValueError, match="dimension mismatch"):
        idx.search(torch.randn(5, 9), 5, 2)
    with pytest.raises(ValueError, match="probe"):
        idx.search(q, 5, 2, probe=torch.zeros((5, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="probe ids"):
        idx.search(q, 5, 2, probe=torch.full((5, 2), 6, dtype=torch.int64))
    big = knn.IVFIndex._blank(1000, 8, True, "cuda:0", "f32x3")
    with pytest.raises(ValueError, match="nprobe"):
        big.search(q, 5, cap + 1)
    from cdml_amd import hardneg
    with pytest.raises(ValueError, match="nlist"):
        hardneg.mine_lists(x, 4, nlist=-1)
    with pytest.raises(ValueError, match="nprobe"):
        hardneg.mine_lists(x, 4, nprobe=2)


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cdml_ivf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_table_and_library_agree():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    syms = _header_symbols()
    assert syms == sorted(_lib.SIGNATURES_IVF) and len(syms) == 3
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.SIGNATURES_IVF[s][1]
    assert not set(syms) & set(_lib.SIGNATURES)


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(260)

    def cent(x=p, order=p, start=p, nlist=4, D=64, c=p, ldx=64, ldc=64):
        return lib.cdml_ivf_centroid_sums(x, ldx, order, start, nlist, D, c, ldc, None)

    def scan(Q=p, ldq=64, nq=8, sq=p, ss=p, so=p, rows=p, ldr=64, start=p, Dp=64, tiles=p, n_tiles=1, scores=p):
        return lib.cdml_ivf_scan_f32(Q, ldq, nq, sq, ss, so, rows, ldr, start, Dp, tiles, n_tiles, scores, None)

    def merge(scores=p, so=p, sof=p, probe=p, nq=8, nprobe=4, start=p, ids=p, rsq=p, qsq=p, k=10, bd=p, bi=p):
        return lib.cdml_ivf_merge(scores, so, sof, probe, nq, nprobe, start, ids, rsq, qsq, k, bd, bi, None)

    for fn, kw, word in ((cent, dict(x=None), b"null"), (cent, dict(c=None), b"null"), (cent, dict(nlist=0), b"nlist"), (cent, dict(ldx=32), b"ldx"),
                     (cent, dict(ldc=63), b"ldc"),
                     (scan, dict(Q=None), b"null"), (scan, dict(tiles=None), b"null"), (scan, dict(n_tiles=0), b"bad size"), (scan, dict(Dp=48), b"multiple of 32"),
                     (scan, dict(ldq=66), b"multiples of 4"), (scan, dict(ldr=32), b"multiples of 4"), (scan, dict(rows=odd), b"aligned"),
                     (scan, dict(scores=odd), b"aligned"),
                     (merge, dict(qsq=None), b"null"), (merge, dict(nq=0), b"bad size"), (merge, dict(k=0), b"k must be"), (merge, dict(k=129), b"k must be"),
                     (merge, dict(nprobe=0), b"nprobe"), (merge, dict(nprobe=129), b"nprobe"), (merge, dict(scores=odd), b"aligned")):
        rc = fn(**kw)
        assert rc < 0 and word in lib.cdml_last_error(), (rc, word, lib.cdml_last_error())
