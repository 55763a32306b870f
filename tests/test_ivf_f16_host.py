"""CPU-side checks of the fp16 lists of the IVF index (include/cdml_ivf_f16.h, cdml_amd.knn.IVFIndex(storage="f16")): header ==
binding table == library, the argument errors of the two entry points (before any HIP call), the host models of
tests/ivf_f16_ref.py against their own mutations, the refusals of IVFIndex / mine_lists by name, the state_dict key rule and
the share of the recovery fixture's queries that meet the derived condition."""
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
import ivf_f16_ref as f16  # noqa: E402
import ivf_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                # tests/test_gpu_knn.py's TOL, restated (that module is marked gpu as a whole)


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


# ---- header == table == library ---------------------------------------------------------------------------------------------
def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cdml_ivf_f16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_table_and_library_agree():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    syms = _header_symbols()
    assert syms == sorted(_lib.SIGNATURES_IVF_F16) == ["cdml_ivf_refine", "cdml_ivf_scan_f16"]
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.SIGNATURES_IVF_F16[s][1]
    assert not set(syms) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_IVF))
    # the two headers existing tests count stay as they were
    for h in ("cdml.h", "cdml_ivf.h"):
        assert "ivf_scan_f16" not in open(os.path.join(ROOT, "include", h)).read()


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16

    def scan(Q=p, ldq=64, nq=8, sq=p, ss=p, so=p, rows=p, ldr=64, start=p, Dp=64, tiles=p, n_tiles=1, scores=p):
        return lib.cdml_ivf_scan_f16(Q, ldq, nq, sq, ss, so, rows, ldr, start, Dp, tiles, n_tiles, scores, None)

    def refine(Q=p, ldq=64, nq=8, base=p, ldb=64, n_rows=100, Dp=64, cand=p, r=32, k=8, bd=p, bi=p):
        return lib.cdml_ivf_refine(Q, ldq, nq, base, ldb, n_rows, Dp, cand, r, k, bd, bi, None)

    cases = [(scan, dict(Q=None), b"null"), (scan, dict(rows=None), b"null"), (scan, dict(sq=None), b"null"),
             (scan, dict(ss=None), b"null"), (scan, dict(so=None), b"null"), (scan, dict(start=None), b"null"),
             (scan, dict(tiles=None), b"null"), (scan, dict(scores=None), b"null"),
             (scan, dict(n_tiles=0), b"bad size"), (scan, dict(nq=0), b"bad size"), (scan, dict(Dp=0), b"bad size"),
             (scan, dict(Dp=48), b"multiple of 32"), (scan, dict(Dp=16), b"multiple of 32"),
             (scan, dict(ldq=68), b"multiples of 8"), (scan, dict(ldr=68), b"multiples of 8"),
             (scan, dict(ldq=32), b">= Dp"), (scan, dict(ldr=32), b">= Dp"),
             (scan, dict(Q=odd), b"aligned"), (scan, dict(rows=odd), b"aligned"), (scan, dict(tiles=odd), b"aligned"),
             (scan, dict(scores=odd), b"aligned"),
             (refine, dict(Q=None), b"null"), (refine, dict(base=None), b"null"), (refine, dict(cand=None), b"null"),
             (refine, dict(bd=None), b"null"), (refine, dict(bi=None), b"null"),
             (refine, dict(nq=0), b"bad size"), (refine, dict(n_rows=0), b"bad size"), (refine, dict(Dp=0), b"bad size"),
             (refine, dict(ldq=32), b"bad size"), (refine, dict(ldb=63), b"bad size"),
             (refine, dict(k=0), b"k <= r"), (refine, dict(k=33), b"k <= r"), (refine, dict(r=129, k=8), b"k <= r"),
             (refine, dict(r=0, k=0), b"k <= r")]
    for fn, kw, word in cases:
        rc = fn(**kw)
        assert rc < 0 and word in lib.cdml_last_error(), (kw, rc, word, lib.cdml_last_error())


# ---- the models ---------------------------------------------------------------------------------------------------------------
def test_quantise_and_the_unlisting_rule():
    x = np.array([[1.0, 2.0 ** -11 + 1.0, 0.1], [65504.0, 65519.0, -65519.9], [65520.0, 0.0, 0.0], [0.0, -1e5, 0.0],
                  [np.nan, 0.0, 0.0]], dtype=np.float32)
    h = f16.quantise(x)
    assert h.dtype == np.float16 and h[0, 1] == 1.0                       # a tie rounds to even
    assert np.array_equal(h, torch.from_numpy(x).to(torch.float16).numpy(), equal_nan=True)
    assert np.isfinite(h[1]).all() and np.isinf(h[2, 0]) and np.isinf(h[3, 1])
    assert f16.listed_assign([0, 1, 1, 0, 1], x).tolist() == [0, 1, -1, -1, -1]
    assert f16.lost_queries(x) == (2, 3, 4)
    # on the grid rounding is the identity and the scan model is ivf_ref's own
    c = ref.grid_case(48)
    assert np.array_equal(f16.quantise(c["x"]).astype(np.float32), c["x"], equal_nan=True)
    assert np.array_equal(f16.listed_assign(c["assign"], c["x"]), c["assign"]) and f16.lost_queries(c["q"]) == c["bad_queries"]
    want = ref.search(c["d"], c["assign"], c["nlist"], c["probe"], 51, bad_queries=c["bad_queries"])
    got = f16.scan_search(c["q"], c["x"], c["assign"], c["nlist"], c["probe"], 51)
    fin = want[0] != xs.INF_I
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0][fin], want[0][fin] * c["unit"])
    # an overflowing row is nobody's neighbour, an overflowing query finds nothing; their neighbours are unaffected
    rng = np.random.RandomState(0)
    b, q = rng.randn(40, 8).astype(np.float32), rng.randn(6, 8).astype(np.float32)
    assign, probe = rng.randint(0, 3, size=40), np.tile(np.arange(3), (6, 1))
    clean = f16.scan_search(q, b, assign, 3, probe, 5)
    b2, q2 = b.copy(), q.copy()
    b2[int(clean[1][0, 0]), 3] = 1e5
    q2[4, 0] = 1e5
    hit = f16.scan_search(q2, b2, assign, 3, probe, 5)
    assert int(clean[1][0, 0]) not in hit[1] and (hit[1][4] == -1).all() and np.isinf(hit[0][4]).all()
    keep = [i for i in range(6) if i != 4 and int(clean[1][0, 0]) not in clean[1][i]]
    assert keep and np.array_equal(hit[1][keep], clean[1][keep]) and np.array_equal(hit[0][keep], clean[0][keep])


def _refine_case():
    """6 queries x 128 candidates over 300 grid rows: duplicates (ties), NO_ID entries in front of r, better rows behind r"""
    rng = np.random.RandomState(12)
    n, nq, D, r = 300, 6, 32, 40
    xi = xs.grid_rows(n, D, rng)
    qi = xs.grid_rows(nq, D, rng)
    xs.plant(xi, [(7, [3, 250]), (100, [101])])
    cand = np.stack([rng.permutation(n)[:xs.LIST] for _ in range(nq)]).astype(np.int64)
    cand[:, 5], cand[:, 6], cand[:, 7] = 250, 7, 3                        # the tie inside r
    cand[:, 10] = xs.NO_ID
    cand[2, :r] = xs.NO_ID                                                # a query with no candidate inside r
    cand[3, 60:] = xs.NO_ID
    for i in range(nq):                                                   # the query's own nearest row sits behind r
        best = int(np.argmin(((qi[i] - xi) ** 2).sum(1)))
        cand[i][cand[i] == best] = (best + 1) % n
        cand[i, r + 3] = best
    qi[1] = xi[n - 1]                                                     # the row a clamped NO_ID would gather is this query's best
    return xi, qi, cand, r


def test_refine_model_and_its_mutations():
    xi, qi, cand, r = _refine_case()
    k = 8
    want = f16.refine(qi, xi, cand, r, k)
    assert want[0].dtype == np.int64 and (want[1][2] == -1).all() and (want[0][2] == xs.INF_I).all()
    assert xs.NO_ID not in want[1]
    d_all = xs.grid_dist(qi, xi)                                          # on integers the expansion IS the direct form
    for i in (0, 1, 3, 4, 5):
        c = cand[i, :r]
        c = c[c != xs.NO_ID]
        o = np.lexsort((c, d_all[i, c]))[:k]
        assert np.array_equal(want[1][i], c[o]) and np.array_equal(want[0][i], d_all[i, c[o]])
    assert _differs(f16.refine(qi, xi, cand, r, k, tie_larger=True), want)
    assert _differs(f16.refine(qi, xi, cand, r, k, sentinel_is_row=True), want)
    assert _differs(f16.refine(qi, xi, cand, r, k, r_is_whole_list=True), want)
    assert not _differs(f16.refine(qi, xi, cand, r, k, expanded=True), want)          # ... so this mutation needs floats:
    # two rows 2^-13 apart in one coordinate: the direct form sees 2^-26, the float32 expansion rounds it away
    x = np.full((3, 32), 0.5, dtype=np.float32)
    x[1, 4] += 2.0 ** -13
    x[2, 9] += 2.0 ** -12
    q = x[:1].copy()
    cf = np.full((1, xs.LIST), xs.NO_ID, dtype=np.int64)
    cf[0, :3] = [2, 1, 0]
    got = f16.refine(q, x, cf, 3, 3)
    assert got[1].tolist() == [[0, 1, 2]] and got[0].tolist() == [[0.0, 2.0 ** -26, 2.0 ** -24]]
    assert _differs(f16.refine(q, x, cf, 3, 3, expanded=True), got)
    # a NaN distance is no candidate
    x[1, 0] = np.nan
    got = f16.refine(q, x, cf, 3, 3)
    assert got[1].tolist() == [[0, 2, -1]] and np.isinf(got[0][0, 2])
    assert np.array_equal(f16.direct_dist(q, x[[0, 2]])[0], [0.0, 2.0 ** -24])


def test_rounding_bound_holds_on_unit_rows():
    E = f16.rounding_bound()
    assert E == 2.0 ** -8 + 2.0 ** -20
    x, q = f16.recovery_fixture()
    d = f16.direct_dist(q, x)
    dr = f16.rounded_dist(q, x)
    assert np.abs(dr - d).max() <= E
    assert np.abs(dr - d).max() > 16 * TOL                                # (and rounding is far above the fp32 tolerance: the re-rank matters)


def test_recovery_fixture_meets_the_condition_for_nine_queries_in_ten():
    """The share is computed here with the numpy Lloyd model's lists (the GPU test computes it again on the device's)."""
    x, q = f16.recovery_fixture()
    nlist, nprobe, k, r = 16, 4, 8, 32
    assert x.shape == (1024, 32) and np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1).max() < 1e-6
    init = np.sort(np.random.RandomState(0).permutation(len(x))[:nlist])
    C, a, _ = ref.lloyd(x, init, 10)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    dc = (q64 * q64).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * q64 @ C.T
    ok = f16.recoverable(f16.direct_dist(q, x), ref.probes(dc, nprobe), a, nlist, k, r, TOL)
    print("recoverable share %.4f" % ok.mean())
    assert ok.mean() >= 0.9


# ---- refusals and state ---------------------------------------------------------------------------------------------------------
def test_refusals_by_name_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import hardneg, knn
    x = torch.randn(10, 8)
    with pytest.raises(ValueError, match="storage"):
        knn.IVFIndex.build(x, 2, storage="f8")
    with pytest.raises(ValueError, match="storage"):
        knn.IVFIndex.from_assignment(x, torch.zeros(3, 8), torch.zeros(10, dtype=torch.int64), storage="fp16")
    with pytest.raises(ValueError, match="storage"):
        knn.IVFIndex.load_state_dict({"centroids": torch.zeros(3, 8), "assign": torch.zeros(10, dtype=torch.int64), "l2_norm": True,
                                      "precision": "f32x3", "storage": "bf16"}, x)
    with pytest.raises(ValueError, match="storage"):
        knn.IVFIndex._blank(6, 8, True, "cuda:0", "f32x3", "half")
    q = torch.randn(5, 8)
    b = torch.zeros(40, 32)
    f32 = knn.IVFIndex._blank(6, 8, True, "cuda:0", "f32x3")              # the checks come before any device work
    assert f32.storage == "f32"
    with pytest.raises(ValueError, match="refine"):
        f32.search(q, 5, 2, refine=8, base=b)
    with pytest.raises(ValueError, match="refine and base"):
        f32.search(q, 5, 2, base=b)
    h = knn.IVFIndex._blank(6, 8, True, "cuda:0", "f32x3", "f16")
    h.n_rows = 40
    for r in (4, 129, -1):
        with pytest.raises(ValueError, match="refine must be"):
            h.search(q, 5, 2, refine=r, base=b)
    with pytest.raises(ValueError, match="needs base"):
        h.search(q, 5, 2, refine=8)
    with pytest.raises(ValueError, match="base is read only"):
        h.search(q, 5, 2, base=b)
    for bad in (torch.zeros(39, 32), torch.zeros(40, 8), torch.zeros(40, 64), torch.zeros(40, 32, dtype=torch.float16),
                torch.zeros(40, 32, dtype=torch.float64), torch.zeros(40, 32).numpy(), torch.zeros(40 * 32),
                torch.zeros(40, 32)):                                     # (the last one: a CPU tensor for an index on the device)
        with pytest.raises(ValueError, match="base must be"):
            h.search(q, 5, 2, refine=8, base=bad)
    with pytest.raises(ValueError, match="k must be"):                    # the existing checks still come first
        h.search(q, 0, 2, refine=8, base=b)
    with pytest.raises(ValueError, match="dimension mismatch"):
        h.prepare(torch.zeros(4, 9))
    with pytest.raises(ValueError, match="storage and refine"):
        hardneg.mine_lists(x, 4, storage="f16")
    with pytest.raises(ValueError, match="storage and refine"):
        hardneg.mine_lists(x, 4, refine=8)
    # the keywords exist where the issue puts them, with today's defaults
    from cdml_amd import train
    for fn, names in ((knn.IVFIndex.build, ("storage",)), (knn.IVFIndex.from_assignment, ("storage",)),
                      (knn.IVFIndex.search, ("refine", "base")), (hardneg.mine_lists, ("storage", "refine")),
                      (train.TrainStep.refresh_negative_lists, ("storage", "refine")),
                      (train.Trainer.__init__, ("negative_storage", "negative_refine"))):
        sig = inspect.signature(fn).parameters
        for nm in names:
            assert sig[nm].default in ("f32", 0, None), (fn, nm)


def test_state_dict_key_rule():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn
    keys = ["centroids", "assign", "l2_norm", "precision", "init_rows", "objective"]
    for storage, want in (("f32", keys), ("f16", keys + ["storage"])):
        idx = knn.IVFIndex._blank(3, 8, True, "cpu", "f32x3", storage)
        idx.centroids, idx.assign = torch.zeros(3, 8), torch.zeros(10, dtype=torch.int64)
        st = idx.state_dict()
        assert list(st) == want
        assert st.get("storage", "f32") == storage
