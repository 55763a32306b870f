"""CPU-side checks of the threshold-filter search of the IVF index (include/cdml_ivf_filter.h, cdml_amd.knn.IVFIndex.search(scan=
"filter")): the host model of tests/ivf_filter_ref.py against tests/ivf_ref.py's search and against its own mutations, the
default rules by hand values, the chunk costs, header == binding table == library, the argument errors of the two launches
(before any HIP call), the refusals by name, and the pass-through of ``scan`` down from the Trainer."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_filter_ref as flt  # noqa: E402
import ivf_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ref.GRID_DIMS)
def test_model_equals_the_buffered_model_on_the_grid(D):
    c = ref.grid_case(D)
    for keep in ref.GRID_KS:
        for probe in (c["probe"], c["probe_hand"]):
            want = ref.search(c["d"], c["assign"], c["nlist"], probe, keep, bad_queries=c["bad_queries"])
            for s in (1, 2, ref.GRID_NPROBE):
                got = flt.search(c["d"], c["assign"], c["nlist"], probe, s, keep, bad_queries=c["bad_queries"])
                assert not _differs(got, want), (keep, s)
    # the seed of the query with six rows leaves tau empty for k = 51: everything of its other lists is a candidate
    _, _, tau = flt.seed_tau(c["d"], c["assign"], c["nlist"], c["probe"], 1, 51, c["bad_queries"])
    assert tau[ref.GRID_FEW] == xs.INF_I and (tau == xs.INF_I).sum() > 1 and (tau != xs.INF_I).sum() > 100
    cands = flt.candidates(c["d"], c["assign"], c["nlist"], c["probe"], 1, tau, c["bad_queries"])
    assert len(cands[ref.GRID_FEW]) == sum(ref.GRID_LENS[l] for l in c["probe"][ref.GRID_FEW][1:])
    assert cands[ref.GRID_NAN_QUERY] == []


def _random_case(seed, n=400, nlist=7, nq=40, nprobe=4):
    rng = np.random.RandomState(seed)
    d = rng.randn(nq, n) ** 2 - 0.05                          # a few negative raw distances: the clamp makes ties at 0
    d[:, rng.randint(0, n, size=5)] = np.nan                  # NaN rows pass no compare
    d[rng.randint(0, nq, size=30), rng.randint(0, n, size=30)] = 0.25      # exact ties across lists
    assign = rng.randint(-1, nlist, size=n)
    probe = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    probe[3, 0] = -1
    probe[4] = -1
    probe[5, 1:] = -1
    return d, assign, nlist, probe


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_equals_the_buffered_model_on_random_cases(seed):
    d, assign, nlist, probe = _random_case(seed)
    for keep in (1, 8, 51, 128):
        want = ref.search(d, assign, nlist, probe, keep)
        for s in (1, 2, 3, 4):
            assert not _differs(flt.search(d, assign, nlist, probe, s, keep), want), (keep, s)


def test_each_rule_against_its_mutation():
    # `<` instead of `<=` loses a tie at tau: lists {2, 3} (seed) and {0, 1}; the seed's 2nd distance 5 is tau, row 0 ties with it
    # and has the lower id
    d = np.array([[5.0, 9.0, 1.0, 5.0]])
    assign, probe = np.array([1, 1, 0, 0]), np.array([[0, 1]])
    want = ref.search(d, assign, 2, probe, 2)
    assert want[1].tolist() == [[2, 0]] and want[0].tolist() == [[1.0, 5.0]]
    assert not _differs(flt.search(d, assign, 2, probe, 1, 2), want)
    lost = flt.search(d, assign, 2, probe, 1, 2, strict=True)
    assert lost[1].tolist() == [[2, 3]]
    # (the grid's planted ties do not fall on a query's k-th seed entry: the GPU test runs these four rows for that reason)
    # tau from k instead of keep under a re-rank: the merged list must be right in its first keep = r entries
    d, assign, nlist, probe = _random_case(7)
    k, r = 4, 32
    want = ref.search(d, assign, nlist, probe, r)
    assert not _differs(flt.search(d, assign, nlist, probe, 1, r), want)
    assert _differs(flt.search(d, assign, nlist, probe, 1, r, tau_rank=k), want)
    # seed columns not masked out of the filter pass: a seed row within tau comes twice
    dup = flt.search(d, assign, nlist, probe, 2, 8, mask_seed=False)
    assert _differs(dup, ref.search(d, assign, nlist, probe, 8))
    assert any(len(set(row[row >= 0])) < (row >= 0).sum() for row in dup[1])


# ---- the default rules and the chunk costs ---------------------------------------------------------------------------------------
def _blank(nlist, n_listed, list_len=None, storage="f32"):
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn
    idx = knn.IVFIndex._blank(nlist, 8, True, "cpu", "f32x3", storage)
    idx.n_listed = n_listed
    if list_len is not None:
        idx.list_len = torch.as_tensor(list_len, dtype=torch.int64)
    return idx


def test_default_rules_by_hand():
    from_model = flt.default_seed_probes
    # 343 455 rows in 1024 lists (335 rows a list): 4 x 51 = 204 rows need one list, 4 x 128 = 512 need two
    idx = _blank(1024, 343455)
    assert idx.default_seed_probes(51, 16) == 1 == from_model(51, 16, 1024, 343455)
    assert idx.default_seed_probes(128, 16) == 2 == from_model(128, 16, 1024, 343455)
    assert idx.default_seed_probes(128, 1) == 1                          # never more than nprobe
    # 10 M rows in 16 384 lists (610 rows a list)
    assert _blank(16384, 10_000_000).default_seed_probes(40, 8) == 1
    # short lists: 1 000 rows in 100 lists, keep = 51 -> ceil(20 400 / 1 000) = 21 columns, capped at nprobe
    idx = _blank(100, 1000)
    assert idx.default_seed_probes(51, 32) == 21 and idx.default_seed_probes(51, 8) == 8
    assert idx.default_seed_probes(1, 8) == 1 and _blank(4, 16).default_seed_probes(1, 4) == 1      # exactly 4 keep rows a list
    assert _blank(4, 15).default_seed_probes(1, 4) == 2                  # ... and just under it
    from cdml_amd import knn
    cap = knn.IVFIndex.default_filter_cap
    assert [cap(k) for k in (1, 16, 17, 32, 33, 51, 64, 65, 128)] == [64, 64, 128, 128, 256, 256, 256, 512, 512]
    assert all(cap(k) == flt.default_filter_cap(k) for k in range(1, 129))


def test_chunk_costs_and_the_budget_rule():
    from cdml_amd import knn
    lens = [0, 1, 127, 130, 5, 300, 100000]
    idx = _blank(len(lens), sum(lens), lens)
    probe = torch.tensor([[5, 6, 2], [1, 0, 6], [-1, 6, 3], [3, -1, -1], [-1, -1, -1]], dtype=torch.int32)
    for s in (1, 2, 3):
        for cap in (64, 512):
            got = idx.filter_costs(probe, s, cap)
            assert got.dtype == np.int64 and np.array_equal(got, flt.chunk_costs(probe.numpy(), lens, s, cap))
    assert idx.filter_costs(probe, 1, 64).tolist() == [300 + 128, 4 + 128, 128, 132 + 128, 128]
    assert idx.filter_costs(probe, 2, 64).tolist() == [300 + 100000 + 128, 4 + 0 + 128, 100000 + 128, 132 + 128, 128]
    # the buffered plan refuses query 0 under 64 KiB (its own lists hold 100 428 floats); the filter's plan takes it
    full = flt.chunk_costs(probe.numpy(), lens, 3, 0)
    with pytest.raises(ValueError, match="query 0's own scores"):
        knn.ivf_plan_chunks(full, 1 << 16)
    chunks = knn.ivf_plan_chunks(idx.filter_costs(probe, 1, 64), 1 << 16)
    assert chunks == [(0, 5)]
    assert knn.ivf_plan_chunks(idx.filter_costs(probe, 1, 64), 4 * 600) == [(0, 2), (2, 5)]         # 428 + 132 | 128 + 260 + 128
    assert knn.ivf_plan_chunks(idx.filter_costs(probe, 1, 64), 4 * 500) == [(0, 1), (1, 3), (3, 5)]
    with pytest.raises(ValueError, match="own scores"):                  # ... unless its SEED lists do not fit either
        knn.ivf_plan_chunks(idx.filter_costs(probe, 2, 64), 1 << 16)


# ---- header == table == library ---------------------------------------------------------------------------------------------
def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cdml_ivf_filter.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_table_and_library_agree():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib, ops
    lib = _lib.load_library()
    syms = _header_symbols()
    assert syms == sorted(_lib.SIGNATURES_IVF_FILTER) == ["cdml_ivf_filter_f16", "cdml_ivf_filter_f32"]
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.SIGNATURES_IVF_FILTER[s][1] and len(getattr(lib, s).argtypes) == 19
    assert not set(syms) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_IVF) | set(_lib.SIGNATURES_IVF_F16))
    assert callable(ops.ivf_filter_f32) and callable(ops.ivf_filter_f16)
    # the headers existing tests count stay as they were; the contract is stated in the new one
    for h in ("cdml.h", "cdml_ivf.h", "cdml_ivf_f16.h"):
        assert "ivf_filter" not in open(os.path.join(ROOT, "include", h)).read()
    head = open(os.path.join(ROOT, "include", "cdml_ivf_filter.h")).read()
    assert "bit for bit" in head and "NOT promised" in head
    assert set(g.IVF_FILTER_KERNELS) == {"k_ivf_filter_f32", "k_ivf_filter_f16"}


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16
    odd4 = C.c_void_p(260)                                # 4-B aligned, not 8

    def launch(fn):
        def call(Q=p, ldq=64, nq=8, sq=p, ss=p, q_sq=p, tau=p, cnt=p, rows=p, ldr=64, start=p, r_sq=p, ids=p, Dp=64, tiles=p,
                 n_tiles=1, cand=p, cap=64):
            return fn(Q, ldq, nq, sq, ss, q_sq, tau, cnt, rows, ldr, start, r_sq, ids, Dp, tiles, n_tiles, cand, cap, None)
        return call

    for name, unit in (("cdml_ivf_filter_f32", b"multiples of 4"), ("cdml_ivf_filter_f16", b"multiples of 8")):
        f = launch(getattr(lib, name))
        cases = [(dict(**{a: None}), b"null") for a in ("Q", "sq", "ss", "q_sq", "tau", "cnt", "rows", "start", "r_sq", "ids", "tiles",
                                                        "cand")]
        cases += [(dict(n_tiles=0), b"bad size"), (dict(nq=0), b"bad size"), (dict(Dp=0), b"bad size"), (dict(nq=-3), b"bad size"),
                  (dict(Dp=48), b"multiple of 32"), (dict(Dp=16), b"multiple of 32"),
                  (dict(cap=0), b"power of two"), (dict(cap=-64), b"power of two"), (dict(cap=96), b"power of two"),
                  (dict(ldq=70), unit), (dict(ldr=70), unit), (dict(ldq=32), b">= Dp"), (dict(ldr=32), b">= Dp"),
                  (dict(Q=odd), b"aligned"), (dict(rows=odd), b"aligned"), (dict(tiles=odd), b"aligned"), (dict(cand=odd4), b"8-B aligned")]
        for kw, word in cases:
            rc = f(**kw)
            assert rc < 0 and word in lib.cdml_last_error() and name[5:].encode() in lib.cdml_last_error(), \
                (name, kw, rc, word, lib.cdml_last_error())
    # a candidate table on an 8-B boundary and fp32 strides that are multiples of 4 but not 8 pass the f32 checks' words
    assert launch(lib.cdml_ivf_filter_f16)(ldq=68) < 0 and b"multiples of 8" in lib.cdml_last_error()


# ---- refusals by name ---------------------------------------------------------------------------------------------------------
def test_refusals_by_name_need_no_gpu():
    from cdml_amd import hardneg, knn
    q = torch.randn(5, 8)
    for storage in ("f32", "f16"):
        idx = _blank(6, 100, storage=storage)              # the checks come before any device work
        with pytest.raises(ValueError, match="scan must be one of"):
            idx.search(q, 5, 2, scan="tau")
        with pytest.raises(ValueError, match="scan must be one of"):
            idx.search(q, 5, 2, scan=None)
        with pytest.raises(ValueError, match="filter_cap and seed_probes belong to scan=\"filter\""):
            idx.search(q, 5, 2, filter_cap=64)
        with pytest.raises(ValueError, match="filter_cap and seed_probes belong to scan=\"filter\""):
            idx.search(q, 5, 2, scan="buffer", seed_probes=1)
        for bad in (0, 32, 96, 63, 1 << 17, -64, 64.5):
            with pytest.raises(ValueError, match="filter_cap must be a power of two"):
                idx.search(q, 5, 2, scan="filter", filter_cap=bad)
        for bad in (0, 3, -1, 1.5):
            with pytest.raises(ValueError, match=r"seed_probes must be in \[1, nprobe = 2\]"):
                idx.search(q, 5, 2, scan="filter", seed_probes=bad)
        with pytest.raises(ValueError, match="k must be"):                # the existing checks still come first
            idx.search(q, 0, 2, scan="filter")
        with pytest.raises(ValueError, match="nprobe must be"):
            idx.search(q, 5, 7, scan="filter", seed_probes=7)
    with pytest.raises(ValueError, match="refine and base"):
        _blank(6, 100).search(q, 5, 2, refine=8, scan="filter")
    x = torch.randn(10, 8)
    with pytest.raises(ValueError, match="mine_lists takes scan"):
        hardneg.mine_lists(x, 4, scan="filter")                            # the exact search has no scan mode
    with pytest.raises(ValueError, match="mine_lists takes scan"):
        hardneg.mine_lists(x, 4, nlist=2, nprobe=1, scan="tau")
    assert knn.IVFIndex.SCANS == ("buffer", "filter")


# ---- the pass-through ------------------------------------------------------------------------------------------------------------
def test_scan_is_accepted_and_forwarded(monkeypatch):
    import __graft_entry__ as g
    g.build()
    from cdml_amd import evaluate, hardneg, knn, predict, train
    for fn, name in ((knn.IVFIndex.search, "scan"), (hardneg.mine_lists, "scan"), (train.TrainStep.refresh_negative_lists, "scan"),
                     (train.Trainer.__init__, "negative_scan")):
        assert inspect.signature(fn).parameters[name].default == "buffer", fn
    sig = inspect.signature(knn.IVFIndex.search).parameters
    assert sig["filter_cap"].default is None and sig["seed_probes"].default is None
    seen = {}

    # mine_lists -> IVFIndex.search
    class FakeIndex:
        def search(self, e, k, nprobe, **kw):
            seen["search"] = kw
            return None, torch.arange(k).repeat(e.shape[0], 1)

        def prepare(self, e):
            return e
    monkeypatch.setattr(knn.IVFIndex, "build", classmethod(lambda cls, e, nlist, **kw: FakeIndex()))
    hardneg.mine_lists(torch.randn(12, 8), 4, device="cpu", nlist=2, nprobe=1, scan="filter")
    assert seen["search"]["scan"] == "filter"
    hardneg.mine_lists(torch.randn(12, 8), 4, device="cpu", nlist=2, nprobe=1)
    assert seen["search"]["scan"] == "buffer"

    # TrainStep.refresh_negative_lists -> mine_lists
    def fake_mine(emb, k, **kw):
        seen["mine"] = kw
        return "lists"
    monkeypatch.setattr(hardneg, "mine_lists", fake_mine)
    step = types.SimpleNamespace(neg_lists=torch.zeros(12, 4, dtype=torch.int32), table=None, pairs=None, device="cpu",
                                 _list_predictor=types.SimpleNamespace(embed_table=lambda table, rows: "emb"),
                                 set_negative_lists=lambda lists: seen.__setitem__("set", lists))
    assert train.TrainStep.refresh_negative_lists(step, 4, nlist=2, nprobe=1, scan="filter") == "lists"
    assert seen["mine"]["scan"] == "filter" and seen["set"] == "lists"
    train.TrainStep.refresh_negative_lists(step, 4, nlist=2, nprobe=1)
    assert seen["mine"]["scan"] == "buffer"

    # Trainer -> TrainStep.refresh_negative_lists
    class Stop(Exception):
        pass

    def refresh(k, **kw):
        seen["refresh"] = kw
        raise Stop()
    monkeypatch.setattr(predict, "Prediction", lambda **kw: None)
    monkeypatch.setattr(evaluate, "Evaluation", lambda *a, **kw: None)
    ts = types.SimpleNamespace(batch_global=4, neg_lists=torch.zeros(12, 4, dtype=torch.int32), mode="npair", var_ws=None, params=None,
                               device="cpu", global_step=0, refresh_negative_lists=refresh)
    for scan in ("filter", None):
        kw = {} if scan is None else {"negative_scan": scan}
        tr = train.Trainer(ts, 1, 64, refresh_negatives_every=1, negative_nlist=2, negative_nprobe=1, **kw)
        assert tr.negative_scan == (scan or "buffer")
        with pytest.raises(Stop):
            tr.run()
        assert seen["refresh"]["scan"] == (scan or "buffer")
