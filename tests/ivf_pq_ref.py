"""Host models of the product-quantised lists of the IVF index (include/cdml_ivf_pq.h; cdml_amd.knn.IVFIndex(storage="pq")):
the encoder (fp64; int64 on exact grids; the lowest code on a tie), the decoded rows, the lookup tables and the ADC sum (fp32
adds in ascending m), the search (``ivf_ref.search`` on the distances of the decoded rows), two grid builders on top of
``ivf_ref.grid_case`` and the recovery fixture.  Every rule has a switch that turns it into the single mutation
tests/test_ivf_pq_host.py must see.

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402
import ivf_ref as ref  # noqa: E402

CODEWORDS = 256


def _num(a):
    a = np.asarray(a)
    return a.astype(np.int64) if a.dtype.kind in "iu" else a.astype(np.float64)


# ---- the format ----------------------------------------------------------------------------------------------------------------
def sub_dist(x, cb):
    """[n, M, 256]: d(c) = sum_j (x[m dsub + j] - cb[m][c][j])^2 (int64 for integer operands, float64 otherwise)"""
    x, cb = _num(x), _num(cb)
    M, _, dsub = cb.shape
    return np.stack([((x[:, None, m * dsub:(m + 1) * dsub] - cb[m][None]) ** 2).sum(2) for m in range(M)], 1)


def encode(x, cb, tie_higher=False):
    """(codes int64 [n, M], dist [n, M]): the lowest c attaining the minimum of d(c).  Mutation ``tie_higher``: the highest."""
    d = sub_dist(x, cb)
    if tie_higher:
        codes = CODEWORDS - 1 - d[:, :, ::-1].argmin(2)
    else:
        codes = d.argmin(2)
    return codes.astype(np.int64), np.take_along_axis(d, codes[:, :, None], 2)[:, :, 0]


def decode(codes, cb):
    """[n, M dsub]: the concatenated codewords"""
    cb = np.asarray(cb)
    M = cb.shape[0]
    return cb[np.arange(M)[None, :], np.asarray(codes, np.int64)].reshape(len(codes), -1)


def lut(q, cb):
    """[nq, M, 256]: LUT[q][m][c] = <q_m, cb[m][c]> (int64 / float64)"""
    q, cb = _num(q), _num(cb)
    M, _, dsub = cb.shape
    return np.einsum("qmj,mcj->qmc", q.reshape(q.shape[0], M, dsub), cb)


def adc(table, codes, descending_m=False):
    """[nq, n]: s~ = ((LUT[0][code_0] + LUT[1][code_1]) + ...) over ascending m.  A float table is summed in float32 as the
    kernel sums it; an int64 table exactly.  Mutation ``descending_m``: the sum runs from the last subspace down."""
    table, codes = np.asarray(table), np.asarray(codes, np.int64)
    M = table.shape[1]
    if table.dtype.kind != "i":
        table = table.astype(np.float32)
    order = range(M - 1, -1, -1) if descending_m else range(M)
    acc = None
    for m in order:
        v = table[:, m, codes[:, m]]
        acc = v if acc is None else acc + v
    return acc


def decoded_sqnorm(codes, cb, of_rows=None):
    """|x^|^2 of the decoded rows.  Mutation ``of_rows``: the norms of these (the original) rows instead."""
    v = _num(decode(codes, cb) if of_rows is None else of_rows)
    return (v * v).sum(1)


def pq_dist(q, codes, cb, **rule):
    """[nq, n] unclamped d~ = (|q|^2 + |x^|^2) - 2 s~ through the tables (int64 on grids, float64 otherwise)"""
    qn = _num(q)
    s = adc(lut(q, cb), codes, descending_m=rule.get("descending_m", False))
    s = s if s.dtype.kind == "i" else s.astype(np.float64)
    return ((qn * qn).sum(1)[:, None] + decoded_sqnorm(codes, cb, rule.get("of_rows"))[None, :]) - 2 * s


def search(q, x, cb, assign, nlist, probe, k, bad_queries=(), **rule):
    """the pq index at refine = 0: ``ivf_ref.search`` on the distances of the decoded rows (a non-finite row is unlisted)"""
    x = np.asarray(x)
    a = np.array(assign, dtype=np.int64)
    if x.dtype.kind == "f":
        bad = ~np.isfinite(x).all(1)
        a[bad] = -1
        x = np.where(bad[:, None], 0, x)
    codes, _ = encode(x, cb, tie_higher=rule.pop("tie_higher", False))
    return ref.search(pq_dist(q, codes, cb, **rule), a, nlist, probe, k, bad_queries=bad_queries)


def encode_bound(dsub):
    """eps with |d^(c) - d(c)| <= eps d(c) for the fp32 encoder: a difference (one rounding), its square inside an fma and
    dsub accumulations of non-negative terms, each 1 + 2^-24 at most: (1 + u)^(dsub + 2) - 1 <= 1.01 (dsub + 2) u.  The
    chosen c^ has d^(c^) <= d^(c*), so d(c^) - d(c*) <= eps (d(c^) + d(c*)) <= 2 eps d(c^)."""
    return 1.01 * (dsub + 2) * 2.0 ** -24


# ---- grid cases ----------------------------------------------------------------------------------------------------------------
def _pad_dims(D, M):
    Dp = (D + 31) // 32 * 32
    assert Dp % M == 0
    return Dp, Dp // M


def _distinct_codewords(rng, nreal, dsub):
    """int64 [256, dsub]: distinct codewords, grid values on the first ``nreal`` columns and zeros behind; where the grid
    holds fewer than 256 vectors the rest are decoys outside [-GRID, GRID] in column 0; (n_grid = the usable ones come first
    before the shuffle) returns (codewords, usable bool [256])"""
    G = xs.GRID
    cw = np.zeros((CODEWORDS, dsub), dtype=np.int64)
    usable = np.zeros(CODEWORDS, dtype=bool)
    if nreal and (2 * G + 1) ** nreal >= CODEWORDS:
        seen = set()
        while len(seen) < CODEWORDS:
            seen.add(tuple(rng.randint(-G, G + 1, size=nreal)))
        cw[:, :nreal] = np.array(sorted(seen))
        usable[:] = True
    else:
        grid = np.array(np.meshgrid(*[np.arange(-G, G + 1)] * nreal, indexing="ij")).reshape(nreal, -1).T if nreal else \
            np.zeros((1, 0), dtype=np.int64)
        ng = len(grid)
        cw[:ng, :nreal] = grid
        usable[:ng] = True
        cw[ng:, 0] = G + 1 + np.arange(CODEWORDS - ng)                  # decoys: never the nearest of a grid sub-vector
    o = rng.permutation(CODEWORDS)
    return cw[o], usable[o]


def _finish(c, xi, cbi, codes, name):
    """the case dict of redrawn rows ``xi`` over ``ivf_ref.grid_case``'s queries, centroids, assignment and probes"""
    u, unit = xs.PIPE_UNIT, c["unit"]
    D = c["D"]
    Dp = cbi.shape[0] * cbi.shape[2]
    qi = np.zeros((c["qi"].shape[0], Dp), dtype=np.int64)
    qi[:, :D] = c["qi"]
    xh = decode(codes, cbi)                                               # int64 [n, Dp]
    q, x, xd = qi * u, xi * u, xh * u
    safe = xs.assert_select_exact_safe((q * q).sum(1), (x * x).sum(1), unit, [q[:, :D]], [x], xg.PAIRS1)
    safe = max(safe, xs.assert_select_exact_safe((q * q).sum(1), (xd * xd).sum(1), unit, [q], [xd], xg.PAIRS1))
    # the tables: every LUT entry and every partial ADC sum is an integer number of units below 2^24
    table = lut(qi, cbi)
    assert float(np.abs(table).sum(1).max()) < 2.0 ** 24 and float(sub_dist(xi_pad(xi, Dp), cbi).max()) < 2.0 ** 24
    xf = x.astype(np.float32)
    xf[c["nan_row"], 3] = np.nan
    out = dict(c)
    out.update(name=name, xi=xi, x=xf, cbi=cbi, cb=(cbi * u).astype(np.float32), codes=codes, xhi=xh, M=cbi.shape[0], Dp=Dp,
               safe=safe, d=xs.grid_dist(c["qi"], xi), d_pq=xs.grid_dist(qi, xh))
    return out


def xi_pad(xi, Dp):
    out = np.zeros((xi.shape[0], Dp), dtype=np.int64)
    out[:, :xi.shape[1]] = xi
    return out


def lossless_case(D, M):
    """``ivf_ref.grid_case(D)`` with rows redrawn from 256 distinct grid codewords per subspace (decoys outside [-4, 4]
    where 9^dsub < 256; a pad subspace's only usable codeword is the zero one): encoding loses nothing, so the pq search IS
    the f32 index's.  The planted duplicates are kept."""
    def make():
        c = ref.grid_case(D)
        rng = xg.case_rng("ivfpq-lossless", D, M)
        Dp, dsub = _pad_dims(D, M)
        n = c["n"]
        cbi = np.zeros((M, CODEWORDS, dsub), dtype=np.int64)
        codes = np.zeros((n, M), dtype=np.int64)
        for m in range(M):
            nreal = min(max(D - m * dsub, 0), dsub)
            cbi[m], usable = _distinct_codewords(rng, nreal, dsub)
            if nreal == 0:                                                # rows are zero here: the zero codeword alone
                usable = (cbi[m] == 0).all(1)
                assert usable.sum() == 1
            codes[:, m] = rng.choice(np.nonzero(usable)[0], size=n)
        codes[c["dups"]] = codes[c["src"]]
        xi = decode(codes, cbi)[:, :D]
        assert np.abs(xi).max() <= xs.GRID and (decode(codes, cbi)[:, D:] == 0).all()
        got, dist = encode(xi_pad(xi, Dp), cbi)
        assert np.array_equal(got, codes) and (dist == 0).all()
        return _finish(c, xi, cbi, codes, "ivf pq lossless D=%d M=%d" % (D, M))
    return xs.cached(("ivfpq-lossless", D, M), make)


LOSSY_TIES = 12


def lossy_case(D, M):
    """``ivf_ref.grid_case(D)`` with random grid rows against 256 arbitrary distinct grid codewords per subspace (dsub >= 3),
    and LOSSY_TIES planted encode ties: a sub-vector at distance 1 from two codewords (x + e_0 at the LOWER code, x - e_0 at
    a higher one) and from no codeword nearer.  ``tie_rows``: (row, subspace, low code, high code)."""
    def make():
        c = ref.grid_case(D)
        rng = xg.case_rng("ivfpq-lossy", D, M)
        Dp, dsub = _pad_dims(D, M)
        assert (2 * xs.GRID + 1) ** dsub >= CODEWORDS
        n = c["n"]
        xi = xs.grid_rows(n, D, rng)
        xs.plant(xi, [(c["src"], c["dups"])])
        xp = xi_pad(xi, Dp)
        cbi = np.stack([_distinct_codewords(rng, dsub, dsub)[0] for _ in range(M)])
        ties = []
        m_real = [m for m in range(M) if (m + 1) * dsub <= D]
        rows = [r for r in rng.permutation(n) if r not in [c["src"], c["nan_row"]] + list(c["dups"])]
        for r in rows:
            if len(ties) == LOSSY_TIES:
                break
            m = int(m_real[len(ties) % len(m_real)])
            v = xp[r, m * dsub:(m + 1) * dsub]
            lo, hi = sorted(rng.choice(CODEWORDS, size=2, replace=False).tolist())
            a, b = v.copy(), v.copy()
            a[0], b[0] = v[0] + 1, v[0] - 1
            others = np.delete(cbi[m], [lo, hi], axis=0)
            if abs(v[0]) >= xs.GRID or any((others == t).all(1).any() for t in (a, b, v)):
                continue
            if any(t[0] == m and (t[2] in (lo, hi) or t[3] in (lo, hi)) for t in ties):
                continue
            cbi[m, lo], cbi[m, hi] = a, b
            ties.append((int(r), m, lo, hi))
        assert len(ties) == LOSSY_TIES
        for m in range(M):
            assert len({tuple(w) for w in cbi[m]}) == CODEWORDS
        codes, dist = encode(xp, cbi)
        d_all = sub_dist(xp, cbi)
        for r, m, lo, hi in ties:                                         # the tie is THE minimum, and the lower code wins
            assert dist[r, m] == 1 and d_all[r, m, lo] == 1 and d_all[r, m, hi] == 1 and codes[r, m] <= lo
        assert (dist > 0).mean() > 0.5                                    # lossy indeed
        out = _finish(c, xi, cbi, codes, "ivf pq lossy D=%d M=%d" % (D, M))
        out["tie_rows"] = ties
        return out
    return xs.cached(("ivfpq-lossy", D, M), make)


def grid_want(c, k, probe=None):
    """(D float32 tensor, I int64 tensor) of a pq grid case from the int64 model on the DECODED rows"""
    import torch
    Dm, Im = ref.search(c["d_pq"], c["assign"], c["nlist"], c["probe"] if probe is None else probe, k, bad_queries=c["bad_queries"])
    return xs.from_units(Dm, c["unit"]), torch.from_numpy(Im)


# ---- recovery ----------------------------------------------------------------------------------------------------------------------
REC_D, REC_M, REC_N, REC_NQ, REC_K, REC_R, REC_NLIST = 64, 8, 4000, 200, 10, 128, 4


def recovery_fixture():
    """RandomState(7): codebooks randn(8, 256, 8); 4 000 rows = random codeword picks + 0.05 randn; 200 queries = rows + 0.1
    randn; everything scaled by 2^-3 (norms about 1) and stored as float32.  Returns (x, q, codebooks)."""
    rng = np.random.RandomState(7)
    dsub = REC_D // REC_M
    cb = rng.randn(REC_M, CODEWORDS, dsub)
    picks = rng.randint(0, CODEWORDS, size=(REC_N, REC_M))
    x = decode(picks, cb) + 0.05 * rng.randn(REC_N, REC_D)
    q = x[rng.choice(REC_N, size=REC_NQ, replace=False)] + 0.1 * rng.randn(REC_NQ, REC_D)
    s = 2.0 ** -3
    return (x * s).astype(np.float32), (q * s).astype(np.float32), (cb * s).astype(np.float32)


def direct_dist(q, x):
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * q @ x.T


def recoverable(d_true, d_pq, k, r, tol):
    """bool [nq] (all rows probed): e_q = max |d~ - d|, d_k = the k-th true distance; the condition #{rows: d~ <= d_k + e_q +
    4 tol} <= r.  A row of the true top k has d~ <= d_k + e_q (+ the device's own arithmetic, within 4 tol), so where at most r
    rows lie under that line the r candidates of the merge hold the whole true top k."""
    e = np.abs(d_pq - d_true).max(1)
    dk = np.sort(d_true, axis=1)[:, k - 1]
    return (d_pq <= (dk + e + 4 * tol)[:, None]).sum(1) <= r
