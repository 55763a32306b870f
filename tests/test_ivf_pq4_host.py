"""CPU-side checks of the 4-bit product-quantised lists of the IVF index (include/cdml_ivf_pq4.h, cdml_amd.knn.IVFIndex(storage="pq",
pq_bits=4)): header == binding table == library for the four new symbols, every argument error of the four entry points (before
any HIP call), the tile against its stated formula, the host models of tests/ivf_pq4_ref.py against their own single mutations
(the high nibble taken as the even subspace, plain ascending-m sums instead of pair-first, a tie to the higher code, r_sq of the
undecoded row), the refusals by name, the state_dict key rule (4 bits adds exactly "pq_bits", 8 bits adds nothing), the chunk
arithmetic, and the share of the recovery fixture's queries that meet the derived condition."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_pq4_ref as p4  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                # tests/test_gpu_knn.py's TOL, restated (that module is marked gpu as a whole)
NAMES = ["cdml_ivf_pq4_tile", "cdml_ivf_scan_pq4", "cdml_pq4_encode", "cdml_pq4_lut"]


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
    text = open(os.path.join(ROOT, "include", "cdml_ivf_pq4.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_l.SIGNATURES_IVF_PQ4) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _l.SIGNATURES_IVF_PQ4[s][1]
    # the argument lists are the 8-bit entry points', one for one
    for s in syms:
        assert _l.SIGNATURES_IVF_PQ4[s] == _l.SIGNATURES_IVF_PQ[s.replace("pq4", "pq")], s
    # none of them in another table or declared by another header
    for name in dir(_l):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_IVF_PQ4":
            assert not set(syms) & set(getattr(_l, name)), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "cdml_ivf_pq4.h":
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            assert not any(s in other for s in syms), h
    import __graft_entry__ as g
    assert g.IVF_PQ4_KERNELS == ("k_ivf_scan_pq4", "k_pq4_encode")
    assert "IVF_PQ4_KERNELS" in inspect.getsource(g._check_no_scratch) and "SIGNATURES_IVF_PQ4" in inspect.getsource(g.build)
    # the scan is built for two blocks a CU: the build refuses an instance above 128 VGPRs, and the build at hand is below it
    assert g.VGPR_CEILINGS == {"k_ivf_scan_pq4": 128} and "VGPR_CEILINGS" in inspect.getsource(g._check_no_scratch)
    rem = os.path.join(ROOT, "build", "obj", "ivf_pq4.remarks")
    if os.path.exists(rem):                               # (written when the object was compiled here)
        text = open(rem).read()
        scans = re.findall(r"Function Name: \S*k_ivf_scan_pq4\S*.*?\n.*? VGPRs: (\d+)", text, flags=re.S)
        assert len(scans) == 8 and max(int(v) for v in scans) <= 128


def test_argument_errors_need_no_gpu():
    _l, lib = _lib()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16
    odd4 = C.c_void_p(260)

    def enc(x=p, ldx=64, n=10, cb=p, M=8, dsub=4, codes=p, ldc=8, dist=None, ldd=0):
        return lib.cdml_pq4_encode(x, ldx, n, cb, M, dsub, codes, ldc, dist, ldd, None)

    def lut(Q=p, ldq=64, nq=4, cb=p, M=8, dsub=4, out=p):
        return lib.cdml_pq4_lut(Q, ldq, nq, cb, M, dsub, out, None)

    def scan(lut=p, nq=8, sq=p, ss=p, so=p, codes=p, ldc=8, start=p, M=8, tiles=p, n_tiles=1, scores=p):
        return lib.cdml_ivf_scan_pq4(lut, nq, sq, ss, so, codes, ldc, start, M, tiles, n_tiles, scores, None)

    s, r = C.c_int(0), C.c_int(0)

    def tile(M=8, ps=C.byref(s), pr=C.byref(r)):
        return lib.cdml_ivf_pq4_tile(M, ps, pr)

    bad_m = (0, 4, 12, 72, -8)
    cases = [(enc, dict(x=None), b"null"), (enc, dict(cb=None), b"null"), (enc, dict(codes=None), b"null"),
             (enc, dict(n=0), b"positive"), (enc, dict(n=-3), b"positive"), (enc, dict(dsub=0), b"dsub"), (enc, dict(dsub=-1), b"dsub"),
             (enc, dict(ldc=7), b"ldc >= M"), (enc, dict(ldx=63), b"ldx >= 2 M dsub"), (enc, dict(dist=p, ldd=15), b"ldd >= 2 M"),
             (enc, dict(dist=p, ldd=8), b"ldd >= 2 M"),                                             # (M floats are not enough)
             (lut, dict(Q=None), b"null"), (lut, dict(cb=None), b"null"), (lut, dict(out=None), b"null"),
             (lut, dict(nq=0), b"positive"), (lut, dict(dsub=0), b"dsub"), (lut, dict(ldq=63), b"ldq >= 2 M dsub"),
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
        assert rc < 0 and word in lib.cdml_last_error() and b"pq4" in lib.cdml_last_error(), (kw, rc, word, lib.cdml_last_error())
    # the accepted edge: dist with exactly 2 M floats a row is not refused for its ldd (it fails later, on nothing: no launch
    # is made here because x is refused first)
    assert enc(x=None, dist=p, ldd=16) < 0 and b"null" in lib.cdml_last_error()


def test_tile_is_its_stated_formula():
    """S(M) = min(16, 512 / M) slots (integer division) of 128 M-byte tables in at most 64 KiB of LDS, R = 1024 rows"""
    _l, lib = _lib()
    s, r = C.c_int(0), C.c_int(0)
    from cdml_amd import ops
    for M in range(8, 72, 8):
        assert lib.cdml_ivf_pq4_tile(M, C.byref(s), C.byref(r)) == 0 and (s.value, r.value) == (min(16, 512 // M), 1024)
        assert s.value >= 1 and s.value * 128 * M <= 64 * 1024
        assert ops.ivf_pq4_tile(M) == (s.value, 1024)
        assert ops.ivf_pq4_tile(M)[0] >= 8 * ops.ivf_pq_tile(M)[0] or ops.ivf_pq4_tile(M)[0] == 16   # an eighth of the table each
    assert ops.ivf_pq4_tile(32) == (16, 1024) and ops.ivf_pq4_tile(8) == (16, 1024) and ops.ivf_pq4_tile(64) == (8, 1024)
    assert ops.ivf_pq4_tile(40) == (12, 1024)


# ---- the models against their mutations --------------------------------------------------------------------------------------
def test_pack_puts_the_even_subspace_in_the_low_nibble():
    codes = np.array([[1, 2, 15, 0], [0, 9, 7, 7]], dtype=np.int64)
    packed = p4.pack(codes)
    assert packed.dtype == np.uint8 and packed.tolist() == [[0x21, 0x0F], [0x90, 0x77]]
    assert np.array_equal(p4.unpack(packed), codes)
    assert p4.pack(codes, high_is_even=True).tolist() == [[0x12, 0xF0], [0x09, 0x77]]
    assert np.array_equal(p4.unpack(p4.pack(codes, high_is_even=True), high_is_even=True), codes)
    # the mutation reaches the search: the bytes read with the nibbles swapped give another answer
    c = p4.lossy_case(48, 16)
    q, xp = p4.xi_pad(c["qi"], c["Dp"]), p4.xi_pad(c["xi"], c["Dp"])
    want = p4.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    assert np.array_equal(want[0], ref.search(c["d_pq"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])[0])
    assert np.array_equal(want[1], ref.search(c["d_pq"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])[1])
    assert _differs(p4.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"],
                              high_is_even=True), want)
    assert np.array_equal(c["packed"], p4.pack(c["codes"])) and c["packed"].shape == (c["n"], c["pq_m"])


def test_encode_ties_go_to_the_lower_code():
    c = p4.lossy_case(48, 16)
    assert len(c["tie_rows"]) == p4.LOSSY_TIES == 12 and c["cbi"].shape == (16, 16, 4)
    xp = p4.xi_pad(c["xi"], c["Dp"])
    codes, dist = p4.encode(xp, c["cbi"])
    assert np.array_equal(codes, c["codes"]) and codes.dtype == np.int64 and dist.dtype == np.int64 and codes.max() < 16
    hi, _ = p4.encode(xp, c["cbi"], tie_higher=True)
    assert (hi != codes).any()
    for r, m, lo, h in c["tie_rows"]:
        assert codes[r, m] <= lo < h <= hi[r, m]
    xh = p4.decode(codes, c["cbi"])
    assert (xh != xp).any() and np.array_equal(p4.encode(xh, c["cbi"])[0], codes)
    q = p4.xi_pad(c["qi"], c["Dp"])
    want = p4.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    assert _differs(p4.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"],
                              tie_higher=True), want)


def test_grid_builders_hold_their_assertions_with_16_codewords():
    for D, Ms in ((48, 16), (48, 64), (256, 64), (256, 128)):
        c = p4.lossless_case(D, Ms)
        assert c["safe"] < 2.0 ** 24 and c["safe"] <= 7273 and np.array_equal(c["d"], c["d_pq"])
        assert c["cbi"].shape == (Ms, 16, c["Dp"] // Ms) and c["Ms"] == Ms and c["pq_m"] == Ms // 2
        assert np.array_equal(c["xhi"][:, :D], c["xi"]) and np.array_equal(c["probe"], ref.grid_case(D)["probe"])
        assert all(np.array_equal(c["xi"][t], c["xi"][c["src"]]) for t in c["dups"])
    assert (np.abs(p4.lossless_case(48, 64)["cbi"]) > p4.xs.GRID).any()     # decoys where 9^dsub < 16
    assert not (np.abs(p4.lossless_case(256, 128)["cbi"]) > p4.xs.GRID).any()
    for (D, Ms), share in (((48, 16), 1.00), ((256, 128), 0.80)):
        c = p4.lossy_case(D, Ms)
        assert c["safe"] < 2.0 ** 24 and c["safe"] <= 7273 and len(c["tie_rows"]) == 12
        assert round(c["lossy_share"], 2) == share


def test_adc_adds_the_pair_first_and_uses_the_decoded_norm():
    # fp32 adds: (2^24 + 1) + 1 loses both ones in plain ascending m; the pair (1 + 1) added first survives
    table = np.zeros((1, 4, 16), dtype=np.float32)
    table[0, 0, 0], table[0, 2, 0], table[0, 3, 0] = 2.0 ** 24, 1.0, 1.0
    codes = np.zeros((1, 4), dtype=np.int64)
    pair, plain = p4.adc4(table, codes), p4.adc4(table, codes, plain_m=True)
    assert pair.dtype == np.float32 and pair[0, 0] == 2.0 ** 24 + 2 and plain[0, 0] == 2.0 ** 24
    # Gaussian tables: the two orders differ somewhere, and plain_m is ivf_pq_ref.adc
    rng = np.random.RandomState(3)
    t = rng.randn(5, 32, 16).astype(np.float32)
    cs = rng.randint(0, 16, size=(300, 32))
    a, b = p4.adc4(t, cs), p4.adc4(t, cs, plain_m=True)
    assert a.shape == (5, 300) and (a != b).any() and np.array_equal(b, pq.adc(t, cs)) and np.abs(a - b).max() < 1e-5
    # int64 tables: exact, any order, and equal to the inner products with the decoded rows
    c = p4.lossy_case(48, 16)
    q = p4.xi_pad(c["qi"], c["Dp"])
    ti = p4.lut(q, c["cbi"])
    assert ti.dtype == np.int64 and ti.shape == (q.shape[0], 16, 16)
    assert np.array_equal(p4.adc4(ti, c["codes"]), p4.adc4(ti, c["codes"], plain_m=True))
    assert np.array_equal(p4.adc4(ti, c["codes"]), q @ c["xhi"].T)
    assert np.array_equal(p4.pq_dist(q, c["codes"], c["cbi"]), c["d_pq"])
    # the norm is the DECODED row's: with the original rows' norms the distances (and the answer) change
    xp = p4.xi_pad(c["xi"], c["Dp"])
    assert (p4.decoded_sqnorm(c["codes"], c["cbi"]) != p4.decoded_sqnorm(c["codes"], c["cbi"], of_rows=xp)).any()
    want = p4.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    assert _differs(p4.search(q, xp, c["cbi"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"], of_rows=xp), want)


# ---- refusals, state, planning ---------------------------------------------------------------------------------------------------
def test_refusals_by_name_need_no_gpu(tmp_path):
    _lib()
    from cdml_amd import hardneg, knn
    x = torch.randn(300, 40)                                               # Dp = 64
    cent, assign = torch.zeros(3, 40), torch.zeros(300, dtype=torch.int64)
    cb4, cb8 = torch.zeros(16, 16, 4), torch.zeros(8, 256, 8)
    assert knn.PQ_BITS == (4, 8) and knn.PQ4_CODEWORDS == 16 and knn.PQ4_TRAIN_ROWS == 4096
    for bits in (2, 16, 0, "4", 4.5, None, True):
        with pytest.raises(ValueError, match="pq_bits must be one of"):
            knn.IVFIndex.build(x, 2, storage="pq", pq_m=8, pq_bits=bits)
    for storage in ("f32", "f16"):
        with pytest.raises(ValueError, match="pq_bits belongs to storage=\"pq\""):
            knn.IVFIndex.build(x, 2, storage=storage, pq_bits=4)
        with pytest.raises(ValueError, match="pq_bits belongs to storage=\"pq\""):
            knn.IVFIndex.from_assignment(x, cent, assign, storage=storage, pq_bits=4)
        with pytest.raises(ValueError, match="pq_bits belongs to storage=\"pq\""):
            knn.IVFIndex._blank(3, 40, True, "cpu", "f32x3", storage, None, False, 4)
        assert knn.IVFIndex._blank(3, 40, True, "cpu", "f32x3", storage, None, False, 8).pq_bits == 8    # (the default names nothing)
    with pytest.raises(ValueError, match="2 pq_m = 128 subspaces"):
        knn.IVFIndex.build(x, 2, storage="pq", pq_m=64, pq_bits=4)
    knn._check_pq_bits("pq", 4, 32, 64)                                    # 2 * 32 divides 64
    with pytest.raises(ValueError, match="pq_bits=4 with pq_residual=True"):
        knn.IVFIndex.build(x, 2, storage="pq", pq_m=8, pq_bits=4, pq_residual=True)
    with pytest.raises(ValueError, match="pq_bits=4 with pq_residual=True"):
        knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=cb4, pq_residual=True)
    with pytest.raises(ValueError, match="at least 16 finite rows"):
        knn.IVFIndex.build(x[:12], 2, storage="pq", pq_m=8, pq_bits=4)
    xn = x[:20].clone()
    xn[:8, 0] = float("nan")
    with pytest.raises(ValueError, match="at least 16 finite rows"):
        knn.IVFIndex.build(xn, 2, storage="pq", pq_m=8, pq_bits=4)
    with pytest.raises(ValueError, match="pq_train_rows"):
        knn.IVFIndex.build(x, 2, storage="pq", pq_m=8, pq_bits=4, pq_train_rows=10)
    # codebooks: the shape says the bits; a contradicting pq_bits and a wrong shape are refused
    for bad in (torch.zeros(16, 16, 2), torch.zeros(15, 16, 4), torch.zeros(16, 17, 4), torch.zeros(16, 16, 4, dtype=torch.float64),
                torch.zeros(16, 64)):
        with pytest.raises(ValueError, match="codebooks must be"):
            knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=bad)
    with pytest.raises(ValueError, match="multiple of 8"):
        knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=torch.zeros(8, 16, 8))    # pq_m = 4
    with pytest.raises(ValueError, match="pq_bits=8 contradicts codebooks"):
        knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=cb4, pq_bits=8)
    with pytest.raises(ValueError, match="pq_bits=4 contradicts codebooks"):
        knn.IVFIndex.from_assignment(x, cent, assign, storage="pq", codebooks=cb8, pq_bits=4)
    assert knn.IVFIndex._check_codebooks(cb4, 64)[1:] == (8, 4) and knn.IVFIndex._check_codebooks(cb8, 64)[1:] == (8, 8)
    assert knn.IVFIndex._check_codebooks(cb4, 64, 4)[1:] == (8, 4) and knn.IVFIndex._check_codebooks(cb8, 64, 8)[1:] == (8, 8)
    # search: the filter scan stays refused by name, the re-rank is accepted
    idx = knn.IVFIndex._blank(6, 40, True, "cuda:0", "f32x3", "pq", 8, False, 4)
    idx.n_rows = 300
    assert idx.storage == "pq" and idx.pq_m == 8 and idx.pq_bits == 4 and tuple(idx.pq_objective.shape) == (16, 0)
    q = torch.randn(5, 40)
    with pytest.raises(ValueError, match="9f.2"):
        idx.search(q, 5, 2, scan="filter")
    with pytest.raises(ValueError, match="needs base"):
        idx.search(q, 5, 2, refine=8)
    # the call sites, before any device work
    for fn, kw in ((knn.ivf_knn, dict(base=x, k=5, nlist=2, nprobe=1)),
                   (knn.cross_knn, dict(embeddings=x, doc_location=150, nearest_num=5, nlist=2, nprobe=1)),
                   (knn.export, dict(embeddings=x, features=x, decode_map=list(range(300)), out_dir=str(tmp_path), doc_location=0,
                                     nearest_num=5, desim_nearest_num=3, nlist=2, nprobe=1))):
        assert inspect.signature(fn).parameters["pq_bits"].default == 8
        with pytest.raises(ValueError, match="pq_bits must be one of"):
            fn(storage="pq", pq_m=8, pq_bits=5, **kw)
        for storage in ("f32", "f16"):
            with pytest.raises(ValueError, match="pq_bits belongs to storage=\"pq\""):
                fn(storage=storage, pq_bits=4, **kw)
        with pytest.raises(ValueError, match="pq_bits=4 with pq_residual=True"):
            fn(storage="pq", pq_m=8, pq_bits=4, pq_residual=True, **kw)
        with pytest.raises(ValueError, match="needs pq_m"):
            fn(storage="pq", pq_bits=4, **kw)
        with pytest.raises(ValueError, match="9f.2"):                      # the filter scan stays refused for pq
            fn(storage="pq", pq_m=8, pq_bits=4, scan="filter", **kw)
        with pytest.raises(ValueError, match="2 pq_m = 128 subspaces"):    # Dp = 64: known at the call site, no index is begun
            fn(storage="pq", pq_m=64, pq_bits=4, **kw)
    y = torch.randn(300, 70)                                               # Dp = 96: 2 * 8 divides it, 2 * 32 does not
    with pytest.raises(ValueError, match="2 pq_m = 64 subspaces"):         # the raw-feature index, before the embedding search
        knn.export(x, y, list(range(300)), str(tmp_path), doc_location=0, nearest_num=5, desim_nearest_num=3, nlist=2, nprobe=1,
                   feature_nlist=2, feature_nprobe=1, storage="pq", pq_m=8, feature_pq_m=32, pq_bits=4)
    with pytest.raises(ValueError, match="pq_bits belongs to storage=\"pq\""):
        knn.cross_knn(x, 150, nearest_num=5, pq_bits=4)                    # (the exact cross search)
    assert not os.listdir(str(tmp_path))
    assert "pq_bits" not in inspect.signature(hardneg.mine_lists).parameters  # (the miner is not taught it)
    assert inspect.signature(knn.IVFIndex.build).parameters["pq_bits"].default == 8
    assert inspect.signature(knn.IVFIndex._blank).parameters["pq_bits"].default == 8
    assert inspect.signature(knn.IVFIndex.from_assignment).parameters["pq_bits"].default is None   # (None: what the codebooks say)
    sig = inspect.signature(knn.pq4_train).parameters
    assert list(sig) == ["X_prepared", "pq_m", "iters", "seed", "train_rows"]
    assert [sig[n].default for n in ("iters", "seed", "train_rows")] == [10, 0, None]
    with pytest.raises(ValueError, match="at least 16 finite rows"):
        knn.pq4_train(torch.zeros(12, 64), 8)
    with pytest.raises(ValueError, match="2 pq_m = 128 subspaces"):
        knn.pq4_train(torch.zeros(300, 64), 64)
    with pytest.raises(ValueError, match="does not divide"):
        knn.pq4_train(torch.zeros(300, 64), 24)
    assert knn._check_pq_train(300, 10, None, 4) == (300, 10) and knn._check_pq_train(10 ** 6, 3, None, 4) == (4096, 3)
    assert knn._check_pq_train(10 ** 6, 3, None) == (65536, 3)             # (8 bits: unchanged)


def test_state_dict_key_rule():
    """4 bits adds exactly "pq_bits"; the 8-bit, f16 and f32 states stay key for key what they are"""
    _lib()
    from cdml_amd import knn
    keys = ["centroids", "assign", "l2_norm", "precision", "init_rows", "objective"]
    states = {}
    for name, storage, bits, want in (("f32", "f32", 8, keys), ("f16", "f16", 8, keys + ["storage"]),
                                      ("pq8", "pq", 8, keys + ["storage", "pq_m", "codebooks"]),
                                      ("pq4", "pq", 4, keys + ["storage", "pq_m", "codebooks", "pq_bits"])):
        idx = knn.IVFIndex._blank(3, 8, True, "cpu", "f32x3", storage, 8 if storage == "pq" else None, False, bits)
        idx.centroids, idx.assign = torch.zeros(3, 8), torch.zeros(10, dtype=torch.int64)
        if storage == "pq":
            idx.codebooks = torch.ones(16, 16, 2) if bits == 4 else torch.ones(8, 256, 4)
        states[name] = st = idx.state_dict()
        assert list(st) == want, name
        assert st.get("storage", "f32") == storage and st.get("pq_bits", 8) == bits
    assert set(states["pq4"]) - set(states["pq8"]) == {"pq_bits"} and states["pq4"]["pq_bits"] == 4
    assert states["pq4"]["pq_m"] == 8 and torch.equal(states["pq4"]["codebooks"], torch.ones(16, 16, 2))
    assert "pq_bits" in inspect.getsource(knn.IVFIndex.load_state_dict)


def test_chunk_costs_hold_scores_and_the_small_tables():
    _lib()
    from cdml_amd import knn
    sig = inspect.signature(knn.pq_query_floats).parameters
    assert list(sig) == ["pq_m", "nprobe", "bits"] and sig["nprobe"].default == 0 and sig["bits"].default == 8
    assert knn.pq_query_floats(32, bits=4) == 32 * 32 == knn.pq_query_floats(32) // 8 and knn.pq_query_floats(8, 0, 4) == 256
    assert knn.pq_query_floats(8) == 2048 and knn.pq_query_floats(8, 16) == 2048 + 16 and knn.pq_query_floats(8, bits=8) == 2048
    # 10 queries of 1000 score floats each under 16 000 B: 4 a chunk without tables, 1 with the 8-bit tables (2048 floats a
    # query), 3 with the 4-bit ones (256 floats)
    costs = np.full(10, 1000, dtype=np.int64)
    assert knn.ivf_plan_chunks(costs, 16000)[0] == (0, 4)
    assert knn.ivf_plan_chunks(costs + knn.pq_query_floats(8), 16000)[0] == (0, 1)
    ch = knn.ivf_plan_chunks(costs + knn.pq_query_floats(8, bits=4), 16000)
    assert ch[0] == (0, 3) and len(ch) == 4
    for q0, q1 in knn.ivf_plan_chunks(costs + knn.pq_query_floats(8, bits=4), 40000):
        assert 4 * (costs[q0:q1].sum() + (q1 - q0) * 256) <= 40000
    with pytest.raises(ValueError, match="score_bytes"):                  # a query's own scores + table must fit
        knn.ivf_plan_chunks(costs + knn.pq_query_floats(8, bits=4), 4 * 1255)
    assert "pq_query_floats(self.pq_m, bits=4)" in inspect.getsource(knn.IVFIndex._scan_buffered)


def test_recovery_fixture_meets_the_condition_for_nine_queries_in_ten():
    """The fp64 model on the fp32 fixture (the GPU test computes the share again on the device's distances): 200 of 200 queries
    meet the condition; recall@10 of the codes alone is 0.933; the mean row norm 0.96."""
    x, q, cb = p4.recovery_fixture()
    assert x.shape == (p4.REC_N, p4.REC_D) and q.shape == (p4.REC_NQ, p4.REC_D) and cb.shape == (p4.REC_MS, 16, 4)
    assert p4.REC_MS == 2 * p4.REC_M == 16
    assert 0.8 < np.linalg.norm(x.astype(np.float64), axis=1).mean() < 1.2
    codes, _ = p4.encode(x, cb)
    d_true = p4.direct_dist(q, x)
    d_pq = p4.direct_dist(q, p4.decode(codes, cb))
    ok = p4.recoverable(d_true, d_pq, p4.REC_K, p4.REC_R, TOL)
    It, Ip = np.argsort(d_true, 1)[:, :p4.REC_K], np.argsort(d_pq, 1)[:, :p4.REC_K]
    print("recoverable share %.4f; codes-only recall@%d %.4f" % (ok.mean(), p4.REC_K, ref.recall(Ip, It)))
    assert ok.mean() >= 0.9
    assert ref.recall(Ip, It) < 1.0                                       # (the re-rank has work to do)
