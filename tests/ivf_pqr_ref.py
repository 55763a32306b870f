"""Host models of RESIDUAL product quantisation on the IVF index (include/cdml_ivf_pqr.h; cdml_amd.knn.IVFIndex(storage="pq",
pq_residual=True)), on top of ``ivf_pq_ref`` and ``ivf_ref``: the encoder of the row minus its list's centroid (fp64; int64 on
exact grids; the lowest code on a tie), the decoded row centroid + codewords, the slot scalar <q, centroid>, the ADC sum that
starts from it (fp32 adds in ascending m), the search (``ivf_ref.search`` on the distances of the decoded rows), two grid
builders over ``ivf_ref.grid_case`` and the clustered fixture with its float64 Lloyd's.  Every rule has a switch that turns it
into the single mutation tests/test_ivf_pqr_host.py must see.

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402
import ivf_pq_ref as pq  # noqa: E402
import ivf_ref as ref  # noqa: E402

CODEWORDS = pq.CODEWORDS


# ---- the format ----------------------------------------------------------------------------------------------------------------
def residual(x, cent, assign, wrong_centroid=False):
    """x - cent[assign] (int64 / float64; an assign of -1 takes centroid 0: such a row is unlisted and its codes are not
    read).  Mutation ``wrong_centroid``: the NEXT list's centroid."""
    x, cent = pq._num(x), pq._num(cent)
    a = np.maximum(np.asarray(assign, np.int64), 0)
    if wrong_centroid:
        a = (a + 1) % len(cent)
    return x - cent[a]


def encode(x, cent, assign, cb, wrong_centroid=False):
    """(codes int64 [n, M], dist [n, M]) of the residuals; a row with assign outside [0, nlist) gets codes 0, dist +inf"""
    codes, dist = pq.encode(residual(x, cent, assign, wrong_centroid), cb)
    bad = (np.asarray(assign) < 0) | (np.asarray(assign) >= len(cent))
    codes[bad] = 0
    if dist.dtype.kind == "f":
        dist[bad] = np.inf
    return codes, dist


def decode(codes, cent, assign, cb):
    """[n, Dp]: centroid of the row's list + the concatenated residual codewords"""
    return np.asarray(cent)[np.maximum(np.asarray(assign, np.int64), 0)] + pq.decode(codes, cb)


def slot_dot(q, cent):
    """[nq, nlist]: b(q, c) = <q, cent[c]> (int64 / float64)"""
    return pq._num(q) @ pq._num(cent).T


def slot_dot_f32(q, cent):
    """the kernel's order in float32: 64 lane-strided fma chains over ascending j, then the xor fold 32, 16, ..., 1 (numpy
    has no fma: the chains are summed in float64 and rounded once per step, which is what an fma does)"""
    q, cent = np.asarray(q, np.float32), np.asarray(cent, np.float32)
    Dp = q.shape[1]
    p = np.zeros((q.shape[0], cent.shape[0], 64), dtype=np.float32)
    for j0 in range(0, Dp, 64):
        w = min(64, Dp - j0)
        prod = q[:, None, j0:j0 + w].astype(np.float64) * cent[None, :, j0:j0 + w].astype(np.float64)
        p[:, :, :w] = (prod + p[:, :, :w].astype(np.float64)).astype(np.float32)
    lanes = np.arange(64)
    for w in (32, 16, 8, 4, 2, 1):
        p = p + p[:, :, lanes ^ w]
    return p[:, :, 0]


def adc(table, codes, base, base_last=False):
    """[nq, n]: s~ = (((base + LUT[0][code_0]) + LUT[1][code_1]) + ...), ``base`` [nq, n] the slot scalar of (query, the row's
    list).  A float table is summed in float32 as the kernel sums it; an int64 table exactly.  Mutation ``base_last``: the
    plain sum first, the base added at the end."""
    table, codes = np.asarray(table), np.asarray(codes, np.int64)
    if table.dtype.kind != "i":
        table, base = table.astype(np.float32), np.asarray(base).astype(np.float32)
    if base_last:
        return pq.adc(table, codes) + base
    acc = base
    for m in range(table.shape[1]):
        acc = acc + table[:, m, codes[:, m]]
    return acc


def decoded_sqnorm(codes, cent, assign, cb, of_residual=False):
    """|x^|^2 of the decoded rows.  Mutation ``of_residual``: |r^|^2, the norm of the codewords alone."""
    v = pq._num(pq.decode(codes, cb) if of_residual else decode(codes, cent, assign, cb))
    return (v * v).sum(1)


def pqr_dist(q, codes, cent, assign, cb, **rule):
    """[nq, n] unclamped d~ = (|q|^2 + |x^|^2) - 2 s~ through the base and the tables (int64 on grids, float64 otherwise)"""
    qn = pq._num(q)
    base = slot_dot(q, cent)[:, np.maximum(np.asarray(assign, np.int64), 0)]
    s = adc(pq.lut(q, cb), codes, base, base_last=rule.get("base_last", False))
    s = s if s.dtype.kind == "i" else s.astype(np.float64)
    return ((qn * qn).sum(1)[:, None] + decoded_sqnorm(codes, cent, assign, cb, rule.get("of_residual", False))[None, :]) - 2 * s


def search(q, x, cent, cb, assign, nlist, probe, k, bad_queries=(), **rule):
    """the residual index at refine = 0: ``ivf_ref.search`` on the distances of the decoded rows"""
    x = np.asarray(x)
    a = np.array(assign, dtype=np.int64)
    if x.dtype.kind == "f":
        bad = ~np.isfinite(x).all(1)
        a[bad] = -1
        x = np.where(bad[:, None], 0, x)
    codes, _ = encode(x, cent, a, cb, wrong_centroid=rule.pop("wrong_centroid", False))
    return ref.search(pqr_dist(q, codes, cent, a, cb, **rule), a, nlist, probe, k, bad_queries=bad_queries)


# ---- grid cases ----------------------------------------------------------------------------------------------------------------
def _finish(c, p, ei, cbi, name):
    """the residual case of ``ivf_ref.grid_case`` c: rows = integer centroid of their list + the integer residuals ``ei``
    [n, Dp] (zero in the pad columns), residual codebooks ``cbi``; ``p`` the plain pq case the residuals came from"""
    u, unit, D, n = xs.PIPE_UNIT, c["unit"], c["D"], c["n"]
    M, _, dsub = cbi.shape
    Dp = M * dsub
    ci = pq.xi_pad(np.rint(c["c"].astype(np.float64) / u).astype(np.int64), Dp)
    assert np.array_equal((ci[:, :D] * u).astype(np.float32), c["c"]) and (ei[:, D:] == 0).all()
    a = c["assign"]
    xr = ei + ci[np.maximum(a, 0)]                                        # int64 [n, Dp]: the rows
    codes, dist = encode(xr, ci, a, cbi)
    xh = decode(codes, ci, a, cbi)
    qi = pq.xi_pad(c["qi"], Dp)
    q, x, xd = qi * u, xr * u, xh * u
    safe = xs.assert_select_exact_safe((q * q).sum(1), (x * x).sum(1), unit, [q], [x], xg.PAIRS1)
    safe = max(safe, xs.assert_select_exact_safe((q * q).sum(1), (xd * xd).sum(1), unit, [q], [xd], xg.PAIRS1))
    # every base, every LUT entry and every partial sum base + LUT[0] + ... is an integer number of units below 2^24
    base, table = slot_dot(qi, ci), pq.lut(qi, cbi)
    assert base.dtype.kind == "i" and table.dtype.kind == "i"
    assert float(np.abs(base).max() + np.abs(table).max(2).sum(1).max()) < 2.0 ** 24
    assert float(pq.sub_dist(residual(xr, ci, a), cbi).max()) < 2.0 ** 24
    xf = x[:, :D].astype(np.float32)
    xf[c["nan_row"], 3] = np.nan
    out = dict(c)
    out.update(name=name, xi=xr[:, :D], x=xf, ci=ci, cbi=cbi, cb=(cbi * u).astype(np.float32), codes=codes, dist=dist, xhi=xh, M=M,
               Dp=Dp, safe=safe, d=xs.grid_dist(c["qi"], xr[:, :D]), d_pq=xs.grid_dist(qi, xh), plain=p)
    assert np.array_equal(pqr_dist(qi, codes, ci, a, cbi), out["d_pq"])
    return out


def lossless_case(D, M):
    """Integer centroids (``ivf_ref.grid_case``'s); rows = the centroid of their list + one of 256 distinct small-grid
    codewords per subspace (``ivf_pq_ref.lossless_case``'s codebooks and picks): encoding the residual loses nothing, so the
    search IS the f32 index's on the same (centroids, assign).  The planted duplicates are kept: a duplicate in ANOTHER list
    than its source needs the residual source + (c_source - c_other), planted as a codeword where it is none."""
    def make():
        c = ref.grid_case(D)
        p = pq.lossless_case(D, M)
        rng = xg.case_rng("ivfpqr-lossless", D, M)
        u = xs.PIPE_UNIT
        cbi, codes = p["cbi"].copy(), p["codes"].copy()
        Dp, dsub = p["Dp"], p["Dp"] // M
        ci = pq.xi_pad(np.rint(c["c"].astype(np.float64) / u).astype(np.int64), Dp)
        a, src = c["assign"], c["src"]
        e_src = pq.decode(codes[src:src + 1], cbi)[0]
        for t in c["dups"]:
            need = e_src + ci[a[src]] - ci[a[t]]
            for m in range(M):
                v = need[m * dsub:(m + 1) * dsub]
                hit = np.nonzero((cbi[m] == v).all(1))[0]
                if len(hit) == 0:                                          # plant it over a codeword the source does not use
                    free = [k for k in rng.permutation(CODEWORDS) if k != codes[src, m] and (m + 1) * dsub <= D]
                    cbi[m, free[0]] = v
                    hit = [free[0]]
                codes[t, m] = hit[0]
        for m in range(M):
            assert len({tuple(w) for w in cbi[m]}) == CODEWORDS
        ei = pq.decode(codes, cbi)
        out = _finish(c, p, ei, cbi, "ivf pqr lossless D=%d M=%d" % (D, M))
        assert np.array_equal(out["codes"][a >= 0], codes[a >= 0]) and (out["dist"][a >= 0] == 0).all()
        assert np.array_equal(out["d"][:, a >= 0], out["d_pq"][:, a >= 0]) and all(np.array_equal(out["xi"][t], out["xi"][src]) for t in c["dups"])
        return out
    return xs.cached(("ivfpqr-lossless", D, M), make)


def lossy_case(D, M):
    """Random grid residuals (``ivf_pq_ref.lossy_case``'s rows, read as residuals) on the integer centroids, with its
    LOSSY_TIES planted encode ties now ties of the RESIDUAL encoder.  ``tie_rows``: (row, subspace, low code, high code)."""
    def make():
        c = ref.grid_case(D)
        p = pq.lossy_case(D, M)
        out = _finish(c, p, pq.xi_pad(p["xi"], p["Dp"]), p["cbi"], "ivf pqr lossy D=%d M=%d" % (D, M))
        listed = c["assign"] >= 0
        assert np.array_equal(out["codes"][listed], p["codes"][listed]) and (out["dist"][listed] > 0).mean() > 0.5
        d_all = pq.sub_dist(residual(pq.xi_pad(out["xi"], out["Dp"]), out["ci"], c["assign"]), out["cbi"])
        for r, m, lo, hi in p["tie_rows"]:
            assert listed[r] and d_all[r, m, lo] == 1 and d_all[r, m, hi] == 1 and out["dist"][r, m] == 1 and out["codes"][r, m] <= lo
        out["tie_rows"] = p["tie_rows"]
        return out
    return xs.cached(("ivfpqr-lossy", D, M), make)


def grid_want(c, k, probe=None):
    """(D float32 tensor, I int64 tensor) of a residual grid case from the int64 model on the DECODED rows"""
    return pq.grid_want(c, k, probe=probe)


# ---- the clustered fixture -------------------------------------------------------------------------------------------------------
CL_D, CL_M, CL_N, CL_NQ, CL_K, CL_CENTRES, CL_NLIST, CL_NPROBE, CL_ITERS = 64, 8, 4000, 200, 10, 62, 32, 4, 10


def _lloyd_codebook(v, iters, init):
    """float64 Lloyd's on sub-vectors v [n, dsub] from the codewords v[init]; an empty codeword keeps its value"""
    cw = v[init].copy()
    for _ in range(iters):
        d = ((v[:, None, :] - cw[None]) ** 2).sum(2)
        code = d.argmin(1)
        for k in np.unique(code):
            cw[k] = v[code == k].mean(0)
    return cw


def clustered_fixture():
    """RandomState(7): 62 centres randn(62, 64); 4 000 rows = a random centre + 0.5 randn, l2-normalised, float32; queries =
    the first 200 rows.  The float64 model: nlist 32 centroids (``ivf_ref.lloyd``, 10 iterations from 32 permuted rows), the
    nearest-centroid assignment, plain and residual codebooks (M = 8; Lloyd's from the same 256 permuted rows, 10
    iterations).  Returns a dict (cached): x, q float32; cent float32 [32, 64]; assign; cb_plain, cb_res float32; probe
    (nprobe 4); true (the exact top-10 ids, fp64); mse_plain, mse_res; recall_plain, recall_res (recall@10 of the codes at
    refine 0 against ``true``)."""
    def make():
        rng = np.random.RandomState(7)
        centres = rng.randn(CL_CENTRES, CL_D)
        x = centres[rng.randint(0, CL_CENTRES, size=CL_N)] + 0.5 * rng.randn(CL_N, CL_D)
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        q = x[:CL_NQ].copy()
        perm = rng.permutation(CL_N)
        xd = x.astype(np.float64)
        cent = ref.lloyd(xd, np.sort(perm[:CL_NLIST]), CL_ITERS)
        cent = np.asarray(cent[0] if isinstance(cent, tuple) else cent).astype(np.float32)
        d_c = pq.direct_dist(x, cent)
        assign = d_c.argmin(1).astype(np.int64)
        probe = np.argsort(pq.direct_dist(q, cent), 1, kind="stable")[:, :CL_NPROBE].astype(np.int64)
        e = residual(x, cent, assign)
        init = np.sort(perm[:CODEWORDS])
        dsub = CL_D // CL_M
        cb_plain = np.stack([_lloyd_codebook(xd[:, m * dsub:(m + 1) * dsub], CL_ITERS, init) for m in range(CL_M)]).astype(np.float32)
        cb_res = np.stack([_lloyd_codebook(e[:, m * dsub:(m + 1) * dsub], CL_ITERS, init) for m in range(CL_M)]).astype(np.float32)
        d_true = pq.direct_dist(q, x)
        true = np.argsort(d_true, 1, kind="stable")[:, :CL_K]
        codes_p, _ = pq.encode(x, cb_plain)
        codes_r, _ = encode(x, cent, assign, cb_res)
        xh_p, xh_r = pq.decode(codes_p, cb_plain), decode(codes_r, cent, assign, cb_res)
        out = dict(x=x, q=q, cent=cent, assign=assign, probe=probe, cb_plain=cb_plain, cb_res=cb_res, true=true, d_true=d_true,
                   codes_plain=codes_p, codes_res=codes_r,
                   mse_plain=float(((xd - xh_p) ** 2).sum(1).mean()), mse_res=float(((xd - xh_r) ** 2).sum(1).mean()))
        for name, xh in (("plain", xh_p), ("res", xh_r)):
            d = pq.direct_dist(q, xh)
            out["d_" + name] = d
            _, I = ref.search(d, assign, CL_NLIST, probe, CL_K)
            out["I_" + name] = I
            out["recall_" + name] = ref.recall(I, true)
        return out
    return xs.cached(("ivfpqr-clustered",), make)
