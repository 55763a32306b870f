"""CPU-side checks of residual product quantisation on the IVF index (include/cdml_ivf_pqr.h, cdml_amd.knn.IVFIndex(storage="pq",
pq_residual=True)): header == binding table == library for the three new symbols, their argument errors (before any HIP call),
the host models of tests/ivf_pqr_ref.py against their own mutations, the refusals by name, the state_dict key rule, the
chunk-cost arithmetic with the slot scalars, and the clustered fixture: the float64 model's residual codes reconstruct better
and recall more than its plain codes."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_pq_ref as pq  # noqa: E402
import ivf_pqr_ref as pqr  # noqa: E402
import ivf_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cdml_ivf_scan_pqr", "cdml_ivf_slot_dots", "cdml_pqr_encode"]


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
    text = open(os.path.join(ROOT, "include", "cdml_ivf_pqr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_l.SIGNATURES_IVF_PQR) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _l.SIGNATURES_IVF_PQR[s][1]
    # none of them in another table or declared by another header
    for name in dir(_l):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_IVF_PQR":
            assert not set(syms) & set(getattr(_l, name)), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "cdml_ivf_pqr.h":
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            assert not any(s in other for s in syms), h
    import __graft_entry__ as g
    assert g.IVF_PQR_KERNELS == ("k_ivf_scan_pqr", "k_pqr_encode")
    assert "IVF_PQR_KERNELS" in inspect.getsource(g._check_no_scratch) and "SIGNATURES_IVF_PQR" in inspect.getsource(g.build)


def test_argument_errors_need_no_gpu():
    _l, lib = _lib()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16
    odd4 = C.c_void_p(260)

    def enc(x=p, ldx=64, n=10, cen=p, ldcen=64, nlist=3, assign=p, cb=p, M=8, dsub=8, codes=p, ldc=8, dist=None, ldd=0):
        return lib.cdml_pqr_encode(x, ldx, n, cen, ldcen, nlist, assign, cb, M, dsub, codes, ldc, dist, ldd, None)

    def dots(Q=p, ldq=64, nq=4, cen=p, ldcen=64, Dp=64, sq=p, ss=p, nlist=3, out=p):
        return lib.cdml_ivf_slot_dots(Q, ldq, nq, cen, ldcen, Dp, sq, ss, nlist, out, None)

    def scan(lut=p, nq=8, sq=p, ss=p, so=p, sb=p, codes=p, ldc=8, start=p, M=8, tiles=p, n_tiles=1, scores=p):
        return lib.cdml_ivf_scan_pqr(lut, nq, sq, ss, so, sb, codes, ldc, start, M, tiles, n_tiles, scores, None)

    cases = [(enc, dict(x=None), b"null"), (enc, dict(cen=None), b"null"), (enc, dict(assign=None), b"null"),
             (enc, dict(cb=None), b"null"), (enc, dict(codes=None), b"null"),
             (enc, dict(n=0), b"positive"), (enc, dict(n=-3), b"positive"), (enc, dict(nlist=0), b"nlist"),
             (enc, dict(nlist=-2), b"nlist"), (enc, dict(dsub=0), b"dsub"), (enc, dict(ldc=7), b"ldc >= M"),
             (enc, dict(ldx=63), b"ldx >= M dsub"), (enc, dict(ldcen=63), b"ldcen >= M dsub"), (enc, dict(dist=p, ldd=7), b"ldd >= M"),
             (dots, dict(Q=None), b"null"), (dots, dict(cen=None), b"null"), (dots, dict(sq=None), b"null"),
             (dots, dict(ss=None), b"null"), (dots, dict(out=None), b"null"), (dots, dict(nq=0), b"bad size"),
             (dots, dict(Dp=0), b"bad size"), (dots, dict(nlist=0), b"nlist"), (dots, dict(ldq=63), b"ldq >= Dp"),
             (dots, dict(ldcen=63), b"ldcen >= Dp"),
             (scan, dict(lut=None), b"null"), (scan, dict(sq=None), b"null"), (scan, dict(ss=None), b"null"),
             (scan, dict(so=None), b"null"), (scan, dict(sb=None), b"null"), (scan, dict(codes=None), b"null"),
             (scan, dict(start=None), b"null"), (scan, dict(tiles=None), b"null"), (scan, dict(scores=None), b"null"),
             (scan, dict(nq=0), b"bad size"), (scan, dict(n_tiles=0), b"bad size"), (scan, dict(ldc=0), b"ldc >= M"),
             (scan, dict(M=16, ldc=8), b"ldc >= M"), (scan, dict(lut=odd), b"aligned"), (scan, dict(scores=odd), b"aligned"),
             (scan, dict(tiles=odd), b"aligned"), (scan, dict(codes=odd4), b"aligned"), (scan, dict(ldc=12), b"multiple of 8")]
    for fn in (enc, scan):
        cases += [(fn, dict(M=m), b"multiple of 8") for m in (0, 4, 12, 72, -8)]
    for fn, kw, word in cases:
        rc = fn(**kw)
        assert rc < 0 and word in lib.cdml_last_error(), (kw, rc, word, lib.cdml_last_error())
        assert b"pqr" in lib.cdml_last_error() or b"slot_dots" in lib.cdml_last_error()


# ---- the models against their mutations --------------------------------------------------------------------------------------
def test_grid_cases_hold_their_own_claims():
    for D, M in ((48, 8), (48, 32)):
        c = pqr.lossless_case(D, M)
        listed = c["assign"] >= 0                                          # (the unlisted NaN row has codes 0)
        assert c["safe"] < 2.0 ** 24 and np.array_equal(c["d"][:, listed], c["d_pq"][:, listed])
        assert np.array_equal(c["xhi"][listed, :D], c["xi"][listed])
        assert np.array_equal(c["probe"], ref.grid_case(D)["probe"]) and np.array_equal(c["c"], ref.grid_case(D)["c"])
        assert all(np.array_equal(c["xi"][t], c["xi"][c["src"]]) for t in c["dups"])
        assert len({int(c["assign"][t]) for t in c["dups"]} | {int(c["assign"][c["src"]])}) == 2       # a duplicate in another list
        assert (c["ci"] != 0).any() and not np.array_equal(c["xi"], c["plain"]["xi"])
    c = pqr.lossy_case(48, 8)
    assert c["safe"] < 2.0 ** 24 and (c["d"] != c["d_pq"]).any() and len(c["tie_rows"]) == pq.LOSSY_TIES
    # the int64 search model through base + tables == ivf_ref.search on the decoded rows
    q, xp = pq.xi_pad(c["qi"], c["Dp"]), pq.xi_pad(c["xi"], c["Dp"])
    args = (c["assign"], c["nlist"], c["probe"], 51)
    want = ref.search(c["d_pq"], *args, bad_queries=c["bad_queries"])
    assert not _differs(pqr.search(q, xp, c["ci"], c["cbi"], *args, bad_queries=c["bad_queries"]), want)
    assert np.array_equal(pqr.slot_dot(q, c["ci"]), q @ c["ci"].T)
    # an assign of -1: codes 0
    codes, _ = pqr.encode(xp, c["ci"], c["assign"], c["cbi"])
    assert (codes[c["nan_row"]] == 0).all() and c["assign"][c["nan_row"]] == -1


def test_residual_is_against_the_rows_own_centroid():
    c = pqr.lossy_case(48, 8)
    q, xp = pq.xi_pad(c["qi"], c["Dp"]), pq.xi_pad(c["xi"], c["Dp"])
    args = (c["assign"], c["nlist"], c["probe"], 51)
    want = pqr.search(q, xp, c["ci"], c["cbi"], *args, bad_queries=c["bad_queries"])
    codes, _ = pqr.encode(xp, c["ci"], c["assign"], c["cbi"])
    wrong, _ = pqr.encode(xp, c["ci"], c["assign"], c["cbi"], wrong_centroid=True)
    assert np.array_equal(codes, c["codes"]) and (wrong != codes).any()
    assert _differs(pqr.search(q, xp, c["ci"], c["cbi"], *args, bad_queries=c["bad_queries"], wrong_centroid=True), want)
    # and the plain encoder of the rows themselves is another one
    assert (pq.encode(xp, c["cbi"])[0] != codes).any()


def test_adc_starts_from_the_base_and_uses_the_decoded_norm():
    # fp32 adds: base 2^24, then 1 + 1: from the base both ones are lost; added last their sum survives
    table = np.zeros((1, 8, 256), dtype=np.float32)
    table[0, 0, 0], table[0, 1, 0] = 1.0, 1.0
    codes = np.zeros((1, 8), dtype=np.int64)
    base = np.full((1, 1), 2.0 ** 24, dtype=np.float32)
    first, last = pqr.adc(table, codes, base), pqr.adc(table, codes, base, base_last=True)
    assert first.dtype == np.float32 and first[0, 0] == 2.0 ** 24 and last[0, 0] == 2.0 ** 24 + 2
    # on the clustered fixture's float tables the two orders give different bits somewhere
    f = pqr.clustered_fixture()
    t = pq.lut(f["q"][:20], f["cb_res"]).astype(np.float32)
    b = pqr.slot_dot(f["q"][:20], f["cent"])[:, f["assign"]]
    assert (pqr.adc(t, f["codes_res"], b) != pqr.adc(t, f["codes_res"], b, base_last=True)).any()
    # int64: exact in any order, and equal to <q, x^>
    c = pqr.lossy_case(48, 8)
    q = pq.xi_pad(c["qi"], c["Dp"])
    ti, bi = pq.lut(q, c["cbi"]), pqr.slot_dot(q, c["ci"])[:, np.maximum(c["assign"], 0)]
    assert np.array_equal(pqr.adc(ti, c["codes"], bi), pqr.adc(ti, c["codes"], bi, base_last=True))
    assert np.array_equal(pqr.adc(ti, c["codes"], bi), q @ c["xhi"].T)
    # the norm is the DECODED row's (centroid + codewords): with the codewords' norm alone the answer changes
    a = c["assign"]
    assert (pqr.decoded_sqnorm(c["codes"], c["ci"], a, c["cbi"]) != pqr.decoded_sqnorm(c["codes"], c["ci"], a, c["cbi"], of_residual=True)).any()
    xp = pq.xi_pad(c["xi"], c["Dp"])
    args = (a, c["nlist"], c["probe"], 51)
    want = pqr.search(q, xp, c["ci"], c["cbi"], *args, bad_queries=c["bad_queries"])
    assert _differs(pqr.search(q, xp, c["ci"], c["cbi"], *args, bad_queries=c["bad_queries"], of_residual=True), want)


def test_slot_dot_order_is_a_function_of_dp_alone():
    rng = np.random.RandomState(3)
    for Dp in (32, 64, 96, 256):
        q, cent = rng.randn(7, Dp).astype(np.float32), rng.randn(5, Dp).astype(np.float32)
        b = pqr.slot_dot_f32(q, cent)
        assert b.dtype == np.float32 and np.abs(b - pqr.slot_dot(q, cent)).max() <= 1e-5
        assert np.array_equal(pqr.slot_dot_f32(q[::-1], cent[::-1])[::-1, ::-1], b)       # (q, c) alone


# ---- refusals, state, planning ---------------------------------------------------------------------------------------------------
def test_refusals_by_name_need_no_gpu(tmp_path):
    _lib()
    from cdml_amd import hardneg, knn
    x = torch.randn(300, 40)                                               # Dp = 64
    cent, assign = torch.zeros(3, 40), torch.zeros(300, dtype=torch.int64)
    for storage in ("f32", "f16"):
        with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
            knn.IVFIndex.build(x, 2, storage=storage, pq_residual=True)
        with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
            knn.IVFIndex.from_assignment(x, cent, assign, storage=storage, pq_residual=True)
        with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
            knn.IVFIndex._blank(3, 40, True, "cpu", "f32x3", storage, None, True)
        with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
            knn._check_ivf_options(storage, 0, "buffer", (5,), None, True)
    assert knn._check_ivf_options("pq", 128, "buffer", (51,), 8, True) == 128
    assert knn._check_ivf_options("f16", 128, "buffer", (51,), None, False) == 128
    for fn, kw in ((knn.ivf_knn, dict(base=x, k=5, nlist=2, nprobe=1)),
                   (knn.cross_knn, dict(embeddings=x, doc_location=150, nearest_num=5, nlist=2, nprobe=1)),
                   (knn.export, dict(embeddings=x, features=x, decode_map=list(range(300)), out_dir=str(tmp_path), doc_location=0,
                                     nearest_num=5, desim_nearest_num=3, nlist=2, nprobe=1))):
        assert inspect.signature(fn).parameters["pq_residual"].default is False
        for storage in ("f32", "f16"):
            with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
                fn(storage=storage, pq_residual=True, **kw)
        with pytest.raises(ValueError, match="needs pq_m"):
            fn(storage="pq", pq_residual=True, **kw)
        with pytest.raises(ValueError, match="9f.2"):                     # the filter scan stays refused for pq
            fn(storage="pq", pq_m=8, pq_residual=True, scan="filter", **kw)
    with pytest.raises(ValueError, match="pq_residual belongs to storage=\"pq\""):
        knn.cross_knn(x, 150, nearest_num=5, pq_residual=True)            # (the exact cross search)
    assert not os.listdir(str(tmp_path))
    for fn in (knn.IVFIndex.build, knn.IVFIndex.from_assignment, knn.IVFIndex._blank, knn._check_ivf_options):
        assert inspect.signature(fn).parameters["pq_residual"].default is False
    assert list(inspect.signature(knn.IVFIndex._blank).parameters)[:8] == ["nlist", "D", "l2_norm", "device", "precision", "storage",
                                                                           "pq_m", "pq_residual"]
    assert list(inspect.signature(knn._check_ivf_options).parameters) == ["storage", "refine", "scan", "ks", "pq_m", "pq_residual"]
    # pq_train: centroids and assign together or not at all
    sig = inspect.signature(knn.pq_train).parameters
    assert list(sig) == ["X_prepared", "pq_m", "iters", "seed", "train_rows", "centroids", "assign"]
    assert sig["centroids"].default is None and sig["assign"].default is None
    X = torch.zeros(300, 64)
    with pytest.raises(ValueError, match="centroids and assign together"):
        knn.pq_train(X, 8, centroids=torch.zeros(3, 64))
    with pytest.raises(ValueError, match="centroids and assign together"):
        knn.pq_train(X, 8, assign=assign)
    with pytest.raises(ValueError, match="centroids fp32"):
        knn.pq_train(X, 8, centroids=torch.zeros(3, 40), assign=assign)
    with pytest.raises(ValueError, match="every finite row needs an assign"):
        knn.pq_train(X, 8, centroids=torch.zeros(3, 64), assign=assign - 1)
    # the search of a residual index: the filter scan is refused by name
    idx = knn.IVFIndex._blank(6, 40, True, "cuda:0", "f32x3", "pq", 8, True)
    idx.n_rows = 300
    assert idx.pq_residual is True and knn.IVFIndex._blank(6, 40, True, "cpu", "f32x3", "pq", 8).pq_residual is False
    with pytest.raises(ValueError, match="9f.2"):
        idx.search(torch.randn(5, 40), 5, 2, scan="filter")
    # the miner is not taught any of this
    assert "pq_residual" not in inspect.signature(hardneg.mine_lists).parameters
    assert "pq_m" not in inspect.signature(hardneg.mine_lists).parameters
    from cdml_amd import train
    assert "pq_residual" not in inspect.signature(train.TrainStep.refresh_negative_lists).parameters
    assert "pq_residual" not in inspect.signature(train.Trainer.__init__).parameters


def test_state_dict_key_rule():
    _lib()
    from cdml_amd import knn
    keys = ["centroids", "assign", "l2_norm", "precision", "init_rows", "objective"]
    for storage, residual, want in (("f32", False, keys), ("f16", False, keys + ["storage"]),
                                    ("pq", False, keys + ["storage", "pq_m", "codebooks"]),
                                    ("pq", True, keys + ["storage", "pq_m", "codebooks", "pq_residual"])):
        idx = knn.IVFIndex._blank(3, 8, True, "cpu", "f32x3", storage, 8 if storage == "pq" else None, residual)
        idx.centroids, idx.assign = torch.zeros(3, 8), torch.zeros(10, dtype=torch.int64)
        if storage == "pq":
            idx.codebooks = torch.ones(8, 256, 4)
        st = idx.state_dict()
        assert list(st) == want
        assert st.get("pq_residual", False) is residual
    assert "pq_residual" in inspect.getsource(knn.IVFIndex.load_state_dict)


def test_chunk_costs_hold_scores_tables_and_slot_scalars():
    _lib()
    from cdml_amd import knn
    assert knn.pq_query_floats(8) == 2048 and knn.pq_query_floats(8, 0) == 2048          # the plain index's, unchanged
    assert knn.pq_query_floats(8, 16) == 2048 + 16 and knn.pq_query_floats(32, 4) == 256 * 32 + 4
    costs = np.full(10, 1000, dtype=np.int64)
    # 3048 floats a plain query: 3 queries fit 4 * 9150 B; with nprobe = 4 slot scalars (3052 floats) only 2
    budget = 4 * 9150
    assert knn.ivf_plan_chunks(costs + knn.pq_query_floats(8), budget)[0] == (0, 3)
    assert knn.ivf_plan_chunks(costs + knn.pq_query_floats(8, 4), budget)[0] == (0, 2)
    for q0, q1 in knn.ivf_plan_chunks(costs + knn.pq_query_floats(8, 4), 40000):
        assert 4 * (costs[q0:q1].sum() + (q1 - q0) * (2048 + 4)) <= 40000
    with pytest.raises(ValueError, match="score_bytes"):                  # a query's scores + table + scalars must fit
        knn.ivf_plan_chunks(costs + knn.pq_query_floats(8, 4), 4 * 3051)
    assert "pq_query_floats(self.pq_m, nprobe if self.pq_residual else 0)" in inspect.getsource(knn.IVFIndex._scan_buffered)


# ---- the clustered fixture ---------------------------------------------------------------------------------------------------------
def test_clustered_fixture_residual_codes_reconstruct_and_recall_better():
    """The float64 model (its own Lloyd's, tests/ivf_pqr_ref.py) at nlist 32 / nprobe 4, M = 8, k = 10 measured: reconstruction
    MSE plain 0.1380, residual 0.1068; recall@10 of the codes plain 0.4635, residual 0.5260 (a gap above 0.03, so the
    fixture stays at nlist 32 / nprobe 4).  No tolerance: the inequalities themselves."""
    f = pqr.clustered_fixture()
    assert f["x"].shape == (pqr.CL_N, pqr.CL_D) and f["x"].dtype == np.float32 and np.array_equal(f["q"], f["x"][:pqr.CL_NQ])
    assert np.abs(np.linalg.norm(f["x"].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert f["cent"].shape == (pqr.CL_NLIST, pqr.CL_D) and f["probe"].shape == (pqr.CL_NQ, pqr.CL_NPROBE)
    print("clustered fixture: MSE plain %.4f residual %.4f; recall@%d plain %.4f residual %.4f"
          % (f["mse_plain"], f["mse_res"], pqr.CL_K, f["recall_plain"], f["recall_res"]))
    assert f["mse_res"] < f["mse_plain"]
    assert f["recall_res"] > f["recall_plain"]
