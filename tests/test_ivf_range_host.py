"""CPU-side checks of the range search of the IVF index (include/cdml_ivf_range.h, cdml_amd.knn.IVFIndex.range_search): header ==
binding table == library, the argument errors of the two new launches (before any HIP call), ``knn.range_compact`` on hand-made
candidate lists, the host model of tests/ivf_range_ref.py against its mutations, the refusals by name, the chunk costs and the
one-query ``result_bytes`` refusal by hand values, and the constants existing tests pin."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_range_ref as rng_ref  # noqa: E402
import ivf_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cdml_ivf_filter_pq", "cdml_ivf_filter_pqr"]


def _blank(nlist, n_listed, storage="f32", D=8, **kw):
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn
    idx = knn.IVFIndex._blank(nlist, D, True, "cpu", "f32x3", storage, **kw)
    idx.n_listed = n_listed
    return idx


# ---- header == table == library ---------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib, ops
    lib = _lib.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdml_ivf_range.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.SIGNATURES_IVF_RANGE) == NAMES
    for s, n_args in zip(NAMES, (18, 19)):
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.SIGNATURES_IVF_RANGE[s][1] and len(getattr(lib, s).argtypes) == n_args
    # the scans' arguments with the filter's set in place of slot_off and scores: the pointer / integer pattern, by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES_IVF_RANGE[NAMES[0]][1] == [p, i, p, p, p, p, p, p, l, p, p, p, i, p, i, p, i, p]
    assert _lib.SIGNATURES_IVF_RANGE[NAMES[1]][1] == [p, i, p, p, p, p, p, p, p, l, p, p, p, i, p, i, p, i, p]
    others = [getattr(_lib, t) for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_IVF_RANGE"]
    assert not any(set(NAMES) & set(t) for t in others)
    assert callable(ops.ivf_filter_pq) and callable(ops.ivf_filter_pqr)
    for h in ("cdml.h", "cdml_ivf_filter.h", "cdml_ivf_pq.h", "cdml_ivf_pqr.h", "cdml_ivf_pq4.h"):
        assert "ivf_filter_pq" not in open(os.path.join(ROOT, "include", h)).read()
    assert g.IVF_RANGE_KERNELS == ("k_ivf_filter_pq",) and "IVF_RANGE_KERNELS" in inspect.getsource(g._check_no_scratch)
    assert "SIGNATURES_IVF_RANGE" in inspect.getsource(g.build) and "SIGNATURES_IVF_RANGE" in inspect.getsource(_lib.load_library)


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16
    odd4 = C.c_void_p(260)                                # 4-B aligned, not 8

    def plain(lut=p, nq=8, sq=p, ss=p, q_sq=p, tau=p, cnt=p, codes=p, ldc=16, start=p, r_sq=p, ids=p, M=16, tiles=p, n_tiles=1,
              cand=p, cap=64):
        return lib.cdml_ivf_filter_pq(lut, nq, sq, ss, q_sq, tau, cnt, codes, ldc, start, r_sq, ids, M, tiles, n_tiles, cand, cap, None)

    def residual(lut=p, nq=8, sq=p, ss=p, base=p, q_sq=p, tau=p, cnt=p, codes=p, ldc=16, start=p, r_sq=p, ids=p, M=16, tiles=p,
                 n_tiles=1, cand=p, cap=64):
        return lib.cdml_ivf_filter_pqr(lut, nq, sq, ss, base, q_sq, tau, cnt, codes, ldc, start, r_sq, ids, M, tiles, n_tiles, cand,
                                       cap, None)

    pointers = ["lut", "sq", "ss", "q_sq", "tau", "cnt", "codes", "start", "r_sq", "ids", "tiles", "cand"]
    for name, f, ptrs in (("ivf_filter_pq", plain, pointers), ("ivf_filter_pqr", residual, pointers + ["base"])):
        cases = [({a: None}, b"null") for a in ptrs]
        cases += [(dict(nq=0), b"bad size"), (dict(nq=-3), b"bad size"), (dict(n_tiles=0), b"bad size"),
                  (dict(M=0), b"M must be"), (dict(M=12), b"M must be"), (dict(M=72), b"M must be"), (dict(M=-8), b"M must be"),
                  (dict(ldc=8), b"ldc >= M"), (dict(ldc=20), b"multiple of 8"),
                  (dict(lut=odd), b"aligned"), (dict(tiles=odd), b"aligned"), (dict(codes=odd4), b"aligned"),
                  (dict(cap=0), b"power of two"), (dict(cap=-64), b"power of two"), (dict(cap=96), b"power of two"),
                  (dict(cand=odd4), b"cand must be 8-B aligned")]
        for kw, word in cases:
            rc = f(**kw)
            err = lib.cdml_last_error()
            assert rc < 0 and word in err and err.startswith(name.encode() + b":"), (name, kw, rc, word, err)


# ---- range_compact ------------------------------------------------------------------------------------------------------------
def _bits(v):
    return int(np.float32(v).view(np.int32))


def test_range_compact_on_hand_made_candidates():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn
    cap = 4
    junk = (_bits(-7.0), 999)                              # what a slot behind the count may hold: never read
    cand = np.array([
        [(_bits(2.0), 5), (_bits(0.5), 9), (_bits(2.0), 3), junk],               # cnt 3, scrambled; the tie at 2.0 broken by id
        [junk, junk, junk, junk],                                                 # cnt 0
        [(_bits(1.0), 8), (_bits(0.0), 8), (_bits(np.inf), 1), (_bits(1.0), 2)],  # cnt 9 > cap: the first cap slots; d = 0 and +inf
        [(_bits(3.0), 0), junk, junk, junk],                                      # cnt 1
    ], dtype=np.int32)
    cnt = np.array([3, 0, 9, 1], dtype=np.int32)
    lims, D, I = knn.range_compact(torch.from_numpy(cand), torch.from_numpy(cnt), cap)
    assert lims.dtype == torch.int64 and D.dtype == torch.float32 and I.dtype == torch.int64
    assert lims.tolist() == [0, 3, 3, 7, 8]
    assert D.tolist() == [0.5, 2.0, 2.0, 0.0, 1.0, 1.0, float("inf"), 3.0]
    assert I.tolist() == [9, 3, 5, 8, 2, 8, 1, 0]
    wl, wD, wI = rng_ref.compact(cand, cnt, cap)
    assert np.array_equal(lims.numpy(), wl) and np.array_equal(D.numpy(), wD) and np.array_equal(I.numpy(), wI)
    # a larger random table with many ties, against the model; cand may be longer than [m, cap, 2] and flat
    r = np.random.RandomState(0)
    m, cap = 37, 64
    cand = np.stack([(r.randint(0, 6, size=(m, cap)) * 0.25).astype(np.float32).view(np.int32),
                     r.randint(0, 50, size=(m, cap)).astype(np.int32)], 2)
    cnt = r.randint(0, 2 * cap, size=m).astype(np.int32)
    cnt[:3] = (0, cap, cap + 1)
    flat = torch.cat([torch.from_numpy(cand).reshape(-1), torch.full((11,), -1, dtype=torch.int32)])
    got = knn.range_compact(flat, torch.from_numpy(cnt), cap)
    want = rng_ref.compact(cand, cnt, cap)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(got, want))
    none = knn.range_compact(torch.zeros((2, cap, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), cap)
    assert none[0].tolist() == [0, 0, 0] and none[1].numel() == 0 and none[2].numel() == 0


# ---- the model against its mutations ---------------------------------------------------------------------------------------------
def test_model_rules_against_their_mutations():
    # lists {2, 3} and {0, 1}; radius 5 ties with rows 0 and 3
    d = np.array([[5.0, 9.0, -1.0, 5.0]])
    assign, probe = np.array([1, 1, 0, 0]), np.array([[0, 1]])
    lims, D, I = rng_ref.range_search(d, assign, 2, probe, 5.0)
    assert lims.tolist() == [0, 3] and I.tolist() == [2, 0, 3] and D.tolist() == [0.0, 5.0, 5.0]      # clamped, (d, id) order
    lost = rng_ref.range_search(d, assign, 2, probe, 5.0, strict=True)
    assert lost[2].tolist() == [2]                                        # `<` loses the ties at the radius
    assert rng_ref.range_search(d, assign, 2, np.array([[0, -1]]), 5.0)[2].tolist() == [2, 3]
    for r in (-1.0, float("nan")):
        assert rng_ref.range_search(d, assign, 2, probe, r)[0].tolist() == [0, 0]
    assert rng_ref.range_search(d, assign, 2, probe, 0.0)[2].tolist() == [2]                             # the clamp decides at radius 0
    assert rng_ref.range_search(d, assign, 2, probe, np.inf)[2].tolist() == [2, 0, 3, 1]
    assert rng_ref.range_search(d, assign, 2, probe, np.inf, bad_queries=(0,))[0].tolist() == [0, 0]
    # an unlisted row never comes back, unless the mutation lists it
    a2 = np.array([1, -1, 0, 0])
    assert rng_ref.range_search(d, a2, 2, probe, np.inf)[2].tolist() == [2, 0, 3]
    assert rng_ref.range_search(d, a2, 2, probe, np.inf, list_unlisted=True)[2].tolist() == [2, 0, 3, 1]
    # on the grid: the k-th distance as radius returns at least k rows whose first k are the search's; the mid-gap radius
    # equals no model distance, and `<` and `<=` agree there
    c = ref.grid_case(48)
    args = (c["d"], c["assign"], c["nlist"], c["probe"])
    for k in ref.GRID_KS:
        rad = rng_ref.kth_radius(*args, k, bad_queries=c["bad_queries"])
        lims, D, I = rng_ref.range_search(*args, rad, bad_queries=c["bad_queries"])
        Dk, Ik = ref.search(*args, k, bad_queries=c["bad_queries"])
        n = np.diff(lims)
        strict = np.diff(rng_ref.range_search(*args, rad, bad_queries=c["bad_queries"], strict=True)[0])
        assert n[ref.GRID_NAN_QUERY] == 0 and n[ref.GRID_FEW] == 6 and (strict < n).sum() > 200           # the tie at the radius
        for q in range(ref.GRID_NQ):
            m = min(k, n[q])
            assert np.array_equal(I[lims[q]:lims[q] + m], Ik[q, :m]) and np.array_equal(D[lims[q]:lims[q] + m], Dk[q, :m])
            assert (D[lims[q] + m:lims[q + 1]] == rad[q]).all()
    gap = rng_ref.gap_radius(*args, 20, bad_queries=c["bad_queries"])
    a = rng_ref.range_search(*args, gap, bad_queries=c["bad_queries"])
    b = rng_ref.range_search(*args, gap, bad_queries=c["bad_queries"], strict=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.diff(a[0]).max() > 20


# ---- refusals, by name, before any device work ---------------------------------------------------------------------------------
def test_refusals_by_name_need_no_gpu():
    from cdml_amd import knn
    q = torch.randn(5, 8)
    for storage, kw in (("f32", {}), ("f16", {}), ("pq", dict(pq_m=8)), ("pq", dict(pq_m=8, pq_residual=True))):
        idx = _blank(6, 100, storage, **kw)
        for bad in (0, 32, 96, 63, 1 << 17, -64, 64.5, True):
            with pytest.raises(ValueError, match="range_cap must be a power of two"):
                idx.range_search(q, 1.0, 2, range_cap=bad)
        for bad in (torch.zeros(4), torch.zeros(5, 1), torch.zeros(()), np.zeros(6, np.float32)):
            with pytest.raises(ValueError, match=r"radius must be a float or an \[nq = 5\] tensor"):
                idx.range_search(q, bad, 2)
        with pytest.raises(ValueError, match="nprobe must be"):
            idx.range_search(q, 1.0, 7)
        with pytest.raises(ValueError, match="query / index dimension mismatch"):
            idx.range_search(torch.randn(5, 9), 1.0, 2)
        with pytest.raises(ValueError, match="probe must be an integer"):
            idx.range_search(q, 1.0, 2, probe=torch.zeros((5, 3), dtype=torch.int64))
        with pytest.raises(ValueError, match="probe must be an integer"):
            idx.range_search(q, 1.0, 2, probe=torch.zeros((5, 2)))
        with pytest.raises(ValueError, match=r"probe ids must lie in \[-1, nlist = 6\)"):
            idx.range_search(q, 1.0, 2, probe=torch.full((5, 2), 6))
        with pytest.raises(ValueError, match="result_bytes = 100 is less than"):
            idx.range_search(q, 1.0, 2, result_bytes=100)
        idx.n_listed = 0
        with pytest.raises(ValueError, match="the index lists no row"):
            idx.range_search(q, 1.0, 2)
    pq4 = _blank(6, 100, "pq", pq_m=8, pq_bits=4)
    with pytest.raises(ValueError, match="range_search has no launch for pq_bits=4"):
        pq4.range_search(q, 1.0, 2)
    with pytest.raises(ValueError, match="ivf_range needs radius"):
        knn.ivf_range(torch.randn(10, 8))
    with pytest.raises(ValueError, match="storage must be one of"):
        knn.ivf_range(torch.randn(10, 8), radius=1.0, storage="f8")
    with pytest.raises(ValueError, match="needs pq_m"):
        knn.ivf_range(torch.randn(10, 8), radius=1.0, storage="pq")
    sig = inspect.signature(knn.IVFIndex.range_search).parameters
    assert list(sig) == ["self", "queries", "radius", "nprobe", "probe", "range_cap", "result_bytes", "stats"]
    assert all(sig[n].default is None for n in ("probe", "range_cap", "result_bytes", "stats"))


# ---- chunk costs ------------------------------------------------------------------------------------------------------------------
def test_chunk_costs_and_the_one_query_refusal_by_hand():
    from cdml_amd import knn
    f32 = _blank(6, 100)
    assert f32.range_costs(3, 4, 256).tolist() == [512, 512, 512] and f32.range_costs(3, 4, 256).dtype == np.int64
    assert _blank(6, 100, "f16").range_costs(2, 16, 64).tolist() == [128, 128]
    pq = _blank(6, 100, "pq", D=32, pq_m=16)
    assert pq.range_costs(2, 4, 64).tolist() == [128 + 256 * 16] * 2 == [128 + knn.pq_query_floats(16)] * 2
    pqr = _blank(6, 100, "pq", D=32, pq_m=16, pq_residual=True)
    assert pqr.range_costs(2, 4, 64).tolist() == [128 + 256 * 16 + 4] * 2
    # 10 queries of 512 floats = 2 KiB each: 4 a chunk under 8 KiB, 1 a chunk under 2 KiB, refused under 2 KiB - 1
    assert f32._range_plan(10, 4, 256, 8192) == [(0, 4), (4, 8), (8, 10)]
    assert f32._range_plan(10, 4, 256, 1 << 30) == [(0, 10)]
    assert f32._range_plan(3, 4, 256, 2048) == [(0, 1), (1, 2), (2, 3)]
    assert f32._range_plan(0, 4, 256, 2048) == []
    with pytest.raises(ValueError, match=r"result_bytes = 2047 is less than the 2048 bytes of one query's 256 candidate slots"):
        f32._range_plan(3, 4, 256, 2047)
    # what the second pass asks: cap2 = 2^20 slots need 8 MiB for one query
    with pytest.raises(ValueError, match=r"result_bytes = 1048576 is less than the 8388608 bytes"):
        f32._range_plan(1, 4, 1 << 20, 1 << 20)
    with pytest.raises(ValueError, match=r"less than the 16896 bytes of one query's 64 candidate slots and lookup table"):
        pq._range_plan(2, 4, 64, 16895)
    assert pq._range_plan(2, 4, 64, 16896) == [(0, 1), (1, 2)]


def test_constants_existing_tests_pin_are_unchanged():
    from cdml_amd import knn
    assert knn.IVFIndex.SCANS == ("buffer", "filter") and knn.IVFIndex.STORAGES == ("f32", "f16", "pq")
    assert knn.IVF_SCANS == ("buffer", "filter") and knn.IVF_STORAGES == ("f32", "f16", "pq")
    assert knn.IVFIndex.RANGE_CAP == 256 and (knn.IVFIndex.FILTER_CAP_MIN, knn.IVFIndex.FILTER_CAP_MAX) == (64, 65536)
    idx = _blank(6, 100, "pq", pq_m=8)
    with pytest.raises(ValueError, match="9f.2"):                         # search keeps refusing the filter scan on pq lists
        idx.search(torch.randn(5, 8), 5, 2, scan="filter")
