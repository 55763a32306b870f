"""CPU-side checks of the product-quantised lists of the IVF index (include/cdml_ivf_pq.h, cdml_amd.knn.IVFIndex(storage="pq")):
header == binding table == library, the argument errors of the four entry points (before any HIP call), the host models of
tests/ivf_pq_ref.py against their own mutations, the refusals by name, the state_dict key rule for all three storages, the
chunk-cost arithmetic, ``ivf_tables`` with default tile arguments against a recorded table, and the share of the recovery
fixture's queries that meet the derived condition."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_select as xs  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                # tests/test_gpu_knn.py's TOL, restated (that module is marked gpu as a whole)
NAMES = ["cdml_ivf_pq_tile", "cdml_ivf_scan_pq", "cdml_pq_encode", "cdml_pq_lut"]


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def _lib():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    return _lib, _lib.load_library()


# ---- header == table == library ---------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree():
    _l, lib = _lib()
    text = open(os.path.join(ROOT, "include", "cdml_ivf_pq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_l.SIGNATURES_IVF_PQ) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _l.SIGNATURES_IVF_PQ[s][1]
    assert not set(syms) & (set(_l.SIGNATURES) | set(_l.SIGNATURES_IVF) | set(_l.SIGNATURES_IVF_F16) | set(_l.SIGNATURES_IVF_FILTER))
    for h in ("cdml.h", "cdml_ivf.h", "cdml_ivf_f16.h", "cdml_ivf_filter.h"):
        assert "_pq" not in open(os.path.join(ROOT, "include", h)).read()
    import __graft_entry__ as g
    assert g.IVF_PQ_KERNELS == ("k_ivf_scan_pq", "k_pq_encode")


def test_argument_errors_need_no_gpu():
    _l, lib = _lib()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16
    odd4 = C.c_void_p(260)

    def enc(x=p, ldx=64, n=10, cb=p, M=8, dsub=8, codes=p, ldc=8, dist=None, ldd=0):
        return lib.cdml_pq_encode(x, ldx, n, cb, M, dsub, codes, ldc, dist, ldd, None)

    def lut(Q=p, ldq=64, nq=4, cb=p, M=8, dsub=8, out=p):
        return lib.cdml_pq_lut(Q, ldq, nq, cb, M, dsub, out, None)

    def scan(lut=p, nq=8, sq=p, ss=p, so=p, codes=p, ldc=8, start=p, M=8, tiles=p, n_tiles=1, scores=p):
        return lib.cdml_ivf_scan_pq(lut, nq, sq, ss, so, codes, ldc, start, M, tiles, n_tiles, scores, None)

    s, r = C.c_int(0), C.c_int(0)

    def tile(M=8, ps=C.byref(s), pr=C.byref(r)):
        return lib.cdml_ivf_pq_tile(M, ps, pr)

    bad_m = (0, 4, 12, 72, -8)
    cases = [(enc, dict(x=None), b"null"), (enc, dict(cb=None), b"null"), (enc, dict(codes=None), b"null"),
             (enc, dict(n=0), b"positive"), (enc, dict(n=-3), b"positive"), (enc, dict(dsub=0), b"dsub"),
             (enc, dict(ldc=7), b"ldc >= M"), (enc, dict(ldx=63), b"ldx >= M dsub"), (enc, dict(dist=p, ldd=7), b"ldd >= M"),
             (lut, dict(Q=None), b"null"), (lut, dict(cb=None), b"null"), (lut, dict(out=None), b"null"),
             (lut, dict(nq=0), b"positive"), (lut, dict(dsub=0), b"dsub"), (lut, dict(ldq=63), b"ldq >= M dsub"),
             (lut, dict(out=odd), b"aligned"),
             (scan, dict(lut=None), b"null"), (scan, dict(sq=None), b"null"), (scan, dict(ss=None), b"null"),
             (scan, dict(so=None), b"null"), (scan, dict(codes=None), b"null"), (scan, dict(start=None), b"null"),
             (scan, dict(tiles=None), b"null"), (scan, dict(scores=None), b"null"),
             (scan, dict(nq=0), b"bad size"), (scan, dict(n_tiles=0), b"bad size"), (scan, dict(ldc=0), b"ldc >= M"),
             (scan, dict(M=16, ldc=8), b"ldc >= M"), (scan, dict(lut=odd), b"aligned"), (scan, dict(scores=odd), b"aligned"),
             (scan, dict(tiles=odd), b"aligned"), (scan, dict(codes=odd4), b"aligned"), (scan, dict(ldc=12), b"multiple of 8"),
             (tile, dict(ps=None), b"null"), (tile, dict(pr=None), b"null")]
    for fn in (enc, lut, scan, tile):
        cases += [(fn, dict(M=m), b"multiple of 8") for m in bad_m]
    for fn, kw, word in cases:
        rc = fn(**kw)
        assert rc < 0 and word in lib.cdml_last_error(), (kw, rc, word, lib.cdml_last_error())
    # the tile: S(M) = 64 // M slots of M KiB tables, R = 1024 rows
    for M in range(8, 72, 8):
        assert tile(M) == 0 and (s.value, r.value) == (64 // M, 1024)
        assert s.value >= 1 and s.value * M * 1024 <= 64 * 1024
    from cdml_amd import ops
    assert ops.ivf_pq_tile(32) == (2, 1024)


# ---- the models against their mutations --------------------------------------------------------------------------------------
def test_encode_ties_go_to_the_lower_code():
    c = pq.lossy_case(48, 8)
    xp = pq.xi_pad(c["xi"], c["Dp"])
    codes, dist = pq.encode(xp, c["cbi"])
    assert np.array_equal(codes, c["codes"]) and codes.dtype == np.int64 and dist.dtype == np.int64
    hi, _ = pq.encode(xp, c["cbi"], tie_higher=True)
    assert (hi != codes).any()
    for r, m, lo, h in c["tie_rows"]:
        assert codes[r, m] <= lo < h <= hi[r, m]
    # the decoded rows differ from the rows (lossy) and reproduce themselves under another encode
    xh = pq.decode(codes, c["cbi"])
    assert (xh != xp).any() and np.array_equal(pq.encode(xh, c["cbi"])[0], codes)
    # the search model sees the tie rule
    want = pq.search(pq.xi_pad(c["qi"], c["Dp"]), xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    assert np.array_equal(want[0], ref.search(c["d_pq"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])[0])
    assert _differs(pq.search(pq.xi_pad(c["qi"], c["Dp"]), xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51,
                              bad_queries=c["bad_queries"], tie_higher=True), want)


def test_lossless_case_is_the_f32_grid():
    for D, M in ((48, 8), (48, 32)):
        c = pq.lossless_case(D, M)
        assert c["safe"] < 2.0 ** 24 and np.array_equal(c["d"], c["d_pq"])
        assert np.array_equal(c["xhi"][:, :D], c["xi"]) and np.array_equal(c["probe"], ref.grid_case(D)["probe"])
        assert all(np.array_equal(c["xi"][t], c["xi"][c["src"]]) for t in c["dups"])
    assert (np.abs(pq.lossless_case(48, 32)["cbi"]) > xs.GRID).any()       # decoys where 9^dsub < 256


def test_adc_sums_in_ascending_m_and_uses_the_decoded_norm():
    # fp32 adds: 2^24 + 1 + 1 in ascending m loses both ones; descending keeps their sum
    table = np.zeros((1, 8, 256), dtype=np.float32)
    table[0, 0, 0], table[0, 6, 0], table[0, 7, 0] = 2.0 ** 24, 1.0, 1.0
    codes = np.zeros((1, 8), dtype=np.int64)
    up, down = pq.adc(table, codes), pq.adc(table, codes, descending_m=True)
    assert up.dtype == np.float32 and up[0, 0] == 2.0 ** 24 and down[0, 0] == 2.0 ** 24 + 2
    # int64 tables: exact, any order
    c = pq.lossy_case(48, 8)
    t = pq.lut(pq.xi_pad(c["qi"], c["Dp"]), c["cbi"])
    assert t.dtype == np.int64 and np.array_equal(pq.adc(t, c["codes"]), pq.adc(t, c["codes"], descending_m=True))
    assert np.array_equal(pq.adc(t, c["codes"]), pq.xi_pad(c["qi"], c["Dp"]) @ c["xhi"].T)
    assert np.array_equal(pq.pq_dist(pq.xi_pad(c["qi"], c["Dp"]), c["codes"], c["cbi"]), c["d_pq"])
    # the norm is the DECODED row's: with the original rows' norms the distances (and the answer) change
    xp = pq.xi_pad(c["xi"], c["Dp"])
    assert (pq.decoded_sqnorm(c["codes"], c["cbi"]) != pq.decoded_sqnorm(c["codes"], c["cbi"], of_rows=xp)).any()
    q = pq.xi_pad(c["qi"], c["Dp"])
    want = pq.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    assert _differs(pq.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"], of_rows=xp), want)


# ---- refusals, state, planning ---------------------------------------------------------------------------------------------------
def test_refusals_by_name_need_no_gpu(tmp_path):
    _lib()
    from cdml_amd import hardneg, knn
    x = torch.randn(300, 40)                                               # Dp = 64
    cent, assign = torch.zeros(3, 40), torch.zeros(300, dtype=torch.int64)
    cb = torch.zeros(8, 256, 8)
    assert knn.IVFIndex.STORAGES == ("f32", "f16", "pq") == knn.IVF_STORAGES
    with pytest.raises(ValueError, match="needs pq_m"):
        knn.IVFIndex.build(x, 2, storage="pq")
    for m in (4, 12, 72, 0, 8.5):
        with pytest.raises(ValueError, match="multiple of 8"):
            knn.IVFIndex.build(x, 2, storage="pq", pq_m=m)
    with pytest.raises(ValueError, match="does not divide"):
        knn.IVFIndex.build(x, 2, storage="pq", pq_m=24)
    for storage in ("f32", "f16"):
        with pytest.raises(ValueError, match="belongs to storage=\"pq\""):
            knn.IVFIndex.build(x, 2, storage=storage, pq_m=8)
        for kw in (dict(pq_iters=3), dict(pq_seed=1), dict(pq_train_rows=256)):
            with pytest.raises(ValueError, match="belong to storage=\"pq\""):
                knn.IVFIndex.build(x, 2, storage=storage, **kw)
        with pytest.raises(ValueError, match="codebooks belongs"):
            knn.IVFIndex.from_assignment(x, cent, assign, storage=storage, codebooks=cb)
    with pytest.raises(ValueError, match="needs codebooks"):
        knn.IVFIndex.from_assignment(x, cent, assign, storage="pq")
    for bad in (torch.zeros(8, 256, 4), torch.zeros(8, 255, 8), torch.zeros(8, 256, 8, dtype=torch.float64), torch.zeros(8, 2048),
                torch.zeros(8, 256, 8).numpy().astype(np.float64)):
        with pytest.raises(ValueError, match="codebooks must be"):
            knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=bad)
    with pytest.raises(ValueError, match="multiple of 8"):
        knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=torch.zeros(4, 256, 16))
    with pytest.raises(ValueError, match="at least 256 finite rows"):
        knn.IVFIndex.build(x[:200], 2, storage="pq", pq_m=8)
    xn = x.clone()
    xn[:50, 0] = float("nan")
    with pytest.raises(ValueError, match="at least 256 finite rows"):
        knn.IVFIndex.build(xn, 2, storage="pq", pq_m=8)
    with pytest.raises(ValueError, match="pq_train_rows"):
        knn.IVFIndex.build(x, 2, storage="pq", pq_m=8, pq_train_rows=100)
    with pytest.raises(ValueError, match="pq_iters"):
        knn.IVFIndex.build(x, 2, storage="pq", pq_m=8, pq_iters=-1)
    state = {"centroids": cent, "assign": assign, "l2_norm": True, "precision": "f32x3", "init_rows": torch.zeros(0),
             "objective": torch.zeros(0)}
    with pytest.raises(ValueError, match="holds no codebooks"):
        knn.IVFIndex.load_state_dict(state, x, storage="pq")
    with pytest.raises(ValueError, match="holds no codebooks"):
        knn.IVFIndex.load_state_dict(dict(state, storage="pq"), x)
    # search: the filter scan is refused by name, the re-rank is accepted
    idx = knn.IVFIndex._blank(6, 40, True, "cuda:0", "f32x3", "pq", 8)
    idx.n_rows = 300
    assert idx.storage == "pq" and idx.pq_m == 8 and not hasattr(idx, "rows")
    q = torch.randn(5, 40)
    with pytest.raises(ValueError, match="9f.2"):
        idx.search(q, 5, 2, scan="filter")
    with pytest.raises(ValueError, match="needs base"):
        idx.search(q, 5, 2, refine=8)
    with pytest.raises(ValueError, match="refine must be"):
        idx.search(q, 5, 2, refine=4, base=torch.zeros(300, 64))
    with pytest.raises(ValueError, match="decode belongs"):
        knn.IVFIndex._blank(6, 40, True, "cuda:0", "f32x3").decode(torch.zeros(1, dtype=torch.int64))
    # the call sites, before any device work
    assert knn._check_ivf_options("pq", 128, "buffer", (51,), 8) == 128
    assert knn._check_ivf_options("f16", 128, "buffer", (51,)) == 128
    with pytest.raises(ValueError, match="refine belongs"):
        knn._check_ivf_options("f32", 128, "buffer", (51,))
    for fn, kw in ((knn.ivf_knn, dict(base=x, k=5, nlist=2, nprobe=1)),
                   (knn.cross_knn, dict(embeddings=x, doc_location=150, nearest_num=5, nlist=2, nprobe=1)),
                   (knn.export, dict(embeddings=x, features=x, decode_map=list(range(300)), out_dir=str(tmp_path), doc_location=0,
                                     nearest_num=5, desim_nearest_num=3, nlist=2, nprobe=1))):
        with pytest.raises(ValueError, match="needs pq_m"):
            fn(storage="pq", **kw)
        with pytest.raises(ValueError, match="multiple of 8"):
            fn(storage="pq", pq_m=20, **kw)
        with pytest.raises(ValueError, match="belongs to storage=\"pq\""):
            fn(storage="f16", pq_m=8, **kw)
        with pytest.raises(ValueError, match="9f.2"):
            fn(storage="pq", pq_m=8, scan="filter", **kw)
    with pytest.raises(ValueError, match="feature_pq_m"):
        knn.export(x, x, list(range(300)), str(tmp_path), doc_location=0, nearest_num=5, desim_nearest_num=3, nlist=2, nprobe=1,
                   storage="pq", pq_m=8, feature_pq_m=12)
    assert not os.listdir(str(tmp_path))
    assert "pq_m" not in inspect.signature(hardneg.mine_lists).parameters     # (the miner is not taught pq_m: tests/test_gpu_ivf_pq.py)
    for fn, names in ((knn.IVFIndex.build, ("pq_m", "pq_iters", "pq_seed", "pq_train_rows")),
                      (knn.IVFIndex.from_assignment, ("codebooks",)), (knn.ivf_knn, ("pq_m",)), (knn.cross_knn, ("pq_m",)),
                      (knn.export, ("pq_m", "feature_pq_m"))):
        sig = inspect.signature(fn).parameters
        for nm in names:
            assert sig[nm].default is None, (fn, nm)
    sig = inspect.signature(knn.pq_train).parameters
    assert [sig[n].default for n in ("iters", "seed", "train_rows")] == [10, 0, None]
    with pytest.raises(ValueError, match="at least 256 finite rows"):
        knn.pq_train(torch.zeros(100, 64), 8)
    with pytest.raises(ValueError, match="does not divide"):
        knn.pq_train(torch.zeros(300, 64), 24)


def test_state_dict_key_rule():
    _lib()
    from cdml_amd import knn
    keys = ["centroids", "assign", "l2_norm", "precision", "init_rows", "objective"]
    for storage, want in (("f32", keys), ("f16", keys + ["storage"]), ("pq", keys + ["storage", "pq_m", "codebooks"])):
        idx = knn.IVFIndex._blank(3, 8, True, "cpu", "f32x3", storage, 8 if storage == "pq" else None)
        idx.centroids, idx.assign = torch.zeros(3, 8), torch.zeros(10, dtype=torch.int64)
        if storage == "pq":
            idx.codebooks = torch.ones(8, 256, 4)
        st = idx.state_dict()
        assert list(st) == want
        assert st.get("storage", "f32") == storage
    assert st["pq_m"] == 8 and torch.equal(st["codebooks"], torch.ones(8, 256, 4)) and st["codebooks"].device.type == "cpu"


def test_chunk_costs_hold_scores_and_tables():
    _lib()
    from cdml_amd import knn
    assert knn.pq_query_floats(32) == 256 * 32 and knn.pq_query_floats(8) == 2048
    # 10 queries of 1000 score floats each: 4 per chunk of 16 000 B without tables; with M = 8 tables (2048 floats a query) 1
    costs = np.full(10, 1000, dtype=np.int64)
    assert knn.ivf_plan_chunks(costs, 16000)[0] == (0, 4)
    ch = knn.ivf_plan_chunks(costs + knn.pq_query_floats(8), 16000)
    assert ch[0] == (0, 1) and len(ch) == 10
    for q0, q1 in knn.ivf_plan_chunks(costs + knn.pq_query_floats(8), 40000):
        assert 4 * (costs[q0:q1].sum() + (q1 - q0) * 2048) <= 40000
    with pytest.raises(ValueError, match="score_bytes"):                  # a query's own scores + table must fit
        knn.ivf_plan_chunks(costs + knn.pq_query_floats(8), 4 * 3000)


def test_ivf_tables_defaults_are_todays():
    """the table below was recorded from the tree before ``tile_slots`` / ``tile_rows`` existed"""
    _lib()
    from cdml_amd import knn
    probe = torch.tensor([[0, 2], [2, -1], [1, 2], [2, 0]], dtype=torch.int32)
    ll = torch.tensor([130, 0, 257], dtype=torch.int64)
    want = {"n_slots": 7, "n_floats": 1304, "n_tiles": 5, "slot_query": [0, 3, 2, 0, 1, 2, 3], "slot_start": [0, 2, 3, 7],
            "slot_off": [0, 132, 264, 264, 524, 784, 1044], "slot_of": [[0, 3], [4, -1], [2, 5], [6, 1]],
            "tiles": [[0, 0, 0, 0], [0, 0, 128, 0], [2, 0, 0, 0], [2, 0, 128, 0], [2, 0, 256, 0]]}
    for tb in (knn.ivf_tables(probe, ll), knn.ivf_tables(probe, ll, tile_slots=knn.IVF_TILE, tile_rows=knn.IVF_TILE)):
        assert list(tb) == list(want)
        for k, v in want.items():
            assert (tb[k].tolist() if torch.is_tensor(tb[k]) else tb[k]) == v, k
        assert tb["slot_query"].dtype == tb["slot_start"].dtype == tb["slot_of"].dtype == tb["tiles"].dtype == torch.int32
        assert tb["slot_off"].dtype == torch.int64
    sig = inspect.signature(knn.ivf_tables).parameters
    assert sig["tile_slots"].default == sig["tile_rows"].default == knn.IVF_TILE == 128
    # another tile changes the tile table alone
    tb = knn.ivf_tables(probe, ll, tile_slots=2, tile_rows=128)
    assert tb["n_tiles"] == 8 and tb["tiles"].tolist() == want["tiles"] + [[2, 2, 0, 0], [2, 2, 128, 0], [2, 2, 256, 0]]
    assert tb["slot_off"].tolist() == want["slot_off"] and tb["n_floats"] == want["n_floats"]
    tb = knn.ivf_tables(probe, ll, tile_slots=8, tile_rows=1024)
    assert tb["tiles"].tolist() == [[0, 0, 0, 0], [2, 0, 0, 0]]


def test_recovery_fixture_meets_the_condition_for_nine_queries_in_ten():
    """The fp64 model on the fp32 fixture (the GPU test computes the share again on the device's distances)."""
    x, q, cb = pq.recovery_fixture()
    assert x.shape == (pq.REC_N, pq.REC_D) and q.shape == (pq.REC_NQ, pq.REC_D) and cb.shape == (pq.REC_M, 256, 8)
    assert 0.8 < np.linalg.norm(x.astype(np.float64), axis=1).mean() < 1.2
    codes, _ = pq.encode(x, cb)
    d_true = pq.direct_dist(q, x)
    d_pq = pq.direct_dist(q, pq.decode(codes, cb))
    ok = pq.recoverable(d_true, d_pq, pq.REC_K, pq.REC_R, TOL)
    It, Ip = np.argsort(d_true, 1)[:, :pq.REC_K], np.argsort(d_pq, 1)[:, :pq.REC_K]
    print("recoverable share %.4f; PQ-only recall@%d %.4f" % (ok.mean(), pq.REC_K, ref.recall(Ip, It)))
    assert ok.mean() >= 0.9
    assert ref.recall(Ip, It) < 1.0                                       # (the re-rank has work to do)
