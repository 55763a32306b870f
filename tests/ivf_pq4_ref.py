"""Host models of the 4-bit product-quantised lists of the IVF index (include/cdml_ivf_pq4.h; cdml_amd.knn.IVFIndex(storage="pq",
pq_bits=4)).  ``ivf_pq_ref``'s ``encode``, ``decode``, ``lut``, ``sub_dist`` and ``direct_dist`` are generic in the codebook's
shape and serve codebooks [Ms, 16, dsub] as they are (on UNPACKED codes int64 [n, Ms]); added here: the nibble ``pack`` /
``unpack`` (the even subspace in the low nibble), ``adc4`` (fp32, the pair of a byte added first, then ascending bytes), ``pq_dist``
and ``search`` on top of it, the two grid builders of ``ivf_pq_ref`` with 16 codewords (cache keys of their own) and the recovery
fixture.  Every rule has a switch that turns it into the single mutation tests/test_ivf_pq4_host.py must see.

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

CODEWORDS = 16
decode, lut, sub_dist, direct_dist, recoverable, encode_bound, xi_pad = \
    pq.decode, pq.lut, pq.sub_dist, pq.direct_dist, pq.recoverable, pq.encode_bound, pq.xi_pad


# ---- the format ----------------------------------------------------------------------------------------------------------------
def encode(x, cb, tie_higher=False):
    """(codes int64 [n, Ms] UNPACKED, dist [n, Ms]): the lowest c attaining the minimum.  Mutation ``tie_higher``: the highest."""
    if not tie_higher:
        return pq.encode(x, cb)
    d = sub_dist(x, cb)
    codes = (d.shape[2] - 1 - d[:, :, ::-1].argmin(2)).astype(np.int64)
    return codes, np.take_along_axis(d, codes[:, :, None], 2)[:, :, 0]


def pack(codes, high_is_even=False):
    """uint8 [n, Ms / 2]: byte b = code(2b) | code(2b + 1) << 4.  Mutation ``high_is_even``: the even subspace in the HIGH nibble."""
    c = np.asarray(codes, np.int64)
    assert c.shape[1] % 2 == 0 and c.min() >= 0 and c.max() < CODEWORDS
    even, odd = c[:, 0::2], c[:, 1::2]
    return ((odd | even << 4) if high_is_even else (even | odd << 4)).astype(np.uint8)


def unpack(packed, high_is_even=False):
    """int64 [n, 2 M]: the per-subspace codes of packed bytes (``pack``'s inverse under the same rule)"""
    p = np.asarray(packed).astype(np.int64)
    lo, hi = p & 15, p >> 4
    return np.stack((hi, lo) if high_is_even else (lo, hi), 2).reshape(p.shape[0], -1)


def adc4(table, codes, plain_m=False):
    """[nq, n]: s~ = p_0 + p_1 + ... over ascending bytes b from p_0, p_b = LUT[2b][code(2b)] + LUT[2b + 1][code(2b + 1)] added
    FIRST.  ``codes`` are unpacked [n, Ms].  A float table is summed in float32 as the kernel sums it; an int64 table exactly.
    Mutation ``plain_m``: ((t_0 + t_1) + t_2) + t_3 ... in plain ascending m (``ivf_pq_ref.adc``'s order)."""
    table, codes = np.asarray(table), np.asarray(codes, np.int64)
    Ms = table.shape[1]
    if table.dtype.kind != "i":
        table = table.astype(np.float32)
    if plain_m:
        return pq.adc(table, codes)
    acc = None
    for b in range(Ms // 2):
        p = table[:, 2 * b, codes[:, 2 * b]] + table[:, 2 * b + 1, codes[:, 2 * b + 1]]
        acc = p if acc is None else acc + p
    return acc


def decoded_sqnorm(codes, cb, of_rows=None):
    return pq.decoded_sqnorm(codes, cb, of_rows)


def pq_dist(q, codes, cb, **rule):
    """[nq, n] unclamped d~ = (|q|^2 + |x^|^2) - 2 s~ through the 16-entry tables (int64 on grids, float64 otherwise); ``codes``
    unpacked"""
    qn = pq._num(q)
    s = adc4(lut(q, cb), codes, plain_m=rule.get("plain_m", False))
    s = s if s.dtype.kind == "i" else s.astype(np.float64)
    return ((qn * qn).sum(1)[:, None] + decoded_sqnorm(codes, cb, rule.get("of_rows"))[None, :]) - 2 * s


def search(q, x, cb, assign, nlist, probe, k, bad_queries=(), **rule):
    """the 4-bit index at refine = 0: ``ivf_ref.search`` on the distances of the decoded rows (a non-finite row is unlisted).
    Mutations: ``tie_higher``, ``high_is_even`` (the codes go through pack / a mismatched unpack), ``of_rows``, ``plain_m``."""
    x = np.asarray(x)
    a = np.array(assign, dtype=np.int64)
    if x.dtype.kind == "f":
        bad = ~np.isfinite(x).all(1)
        a[bad] = -1
        x = np.where(bad[:, None], 0, x)
    codes, _ = encode(x, cb, tie_higher=rule.pop("tie_higher", False))
    codes = unpack(pack(codes), high_is_even=rule.pop("high_is_even", False))    # the bytes as the kernel reads them
    return ref.search(pq_dist(q, codes, cb, **rule), a, nlist, probe, k, bad_queries=bad_queries)


# ---- grid cases ----------------------------------------------------------------------------------------------------------------
def _pad_dims(D, Ms):
    Dp = (D + 31) // 32 * 32
    assert Dp % Ms == 0 and Ms % 16 == 0
    return Dp, Dp // Ms


def _distinct_codewords(rng, nreal, dsub):
    """(int64 [16, dsub], usable bool [16]): ``ivf_pq_ref._distinct_codewords`` with 16 codewords -- grid values on the first
    ``nreal`` columns and zeros behind; where the grid holds fewer than 16 vectors (9^nreal < 16) the rest are decoys outside
    [-GRID, GRID] in column 0, never the nearest of a grid sub-vector"""
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
        cw[ng:, 0] = G + 1 + np.arange(CODEWORDS - ng)
    o = rng.permutation(CODEWORDS)
    return cw[o], usable[o]


def _finish(c, xi, cbi, codes, name):
    """``ivf_pq_ref._finish`` (every builder assertion: both ``assert_select_exact_safe``, tables and encoder distances below
    2^24) plus the packed bytes"""
    out = pq._finish(c, xi, cbi, codes, name)
    out.update(Ms=cbi.shape[0], pq_m=cbi.shape[0] // 2, packed=pack(codes))
    # a pair sum is a partial sum of the same non-negative bound: |t_2b| + |t_2b+1| <= sum_m |t_m| < 2^24 (checked there)
    return out


def lossless_case(D, Ms):
    """``ivf_ref.grid_case(D)`` with rows redrawn from 16 distinct grid codewords per subspace (decoys outside [-4, 4] where
    9^dsub < 16; a pad subspace's only usable codeword is the zero one): encoding loses nothing, so the 4-bit search IS the f32
    index's.  The planted duplicates are kept."""
    def make():
        c = ref.grid_case(D)
        rng = xg.case_rng("ivfpq4-lossless", D, Ms)
        Dp, dsub = _pad_dims(D, Ms)
        n = c["n"]
        cbi = np.zeros((Ms, CODEWORDS, dsub), dtype=np.int64)
        codes = np.zeros((n, Ms), dtype=np.int64)
        for m in range(Ms):
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
        return _finish(c, xi, cbi, codes, "ivf pq4 lossless D=%d Ms=%d" % (D, Ms))
    return xs.cached(("ivfpq4-lossless", D, Ms), make)


LOSSY_TIES = 12


def lossy_case(D, Ms):
    """``ivf_ref.grid_case(D)`` with random grid rows against 16 arbitrary distinct grid codewords per subspace (9^dsub >= 16),
    and LOSSY_TIES planted encode ties: a sub-vector at distance 1 from two codewords (x + e_0 at the LOWER code, x - e_0 at a
    higher one) and from no codeword nearer.  ``tie_rows``: (row, subspace, low code, high code)."""
    def make():
        c = ref.grid_case(D)
        rng = xg.case_rng("ivfpq4-lossy", D, Ms)
        Dp, dsub = _pad_dims(D, Ms)
        assert (2 * xs.GRID + 1) ** dsub >= CODEWORDS
        n = c["n"]
        xi = xs.grid_rows(n, D, rng)
        xs.plant(xi, [(c["src"], c["dups"])])
        xp = xi_pad(xi, Dp)
        cbi = np.stack([_distinct_codewords(rng, dsub, dsub)[0] for _ in range(Ms)])
        ties = []
        m_real = [m for m in range(Ms) if (m + 1) * dsub <= D]
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
        for m in range(Ms):
            assert len({tuple(w) for w in cbi[m]}) == CODEWORDS
        codes, dist = encode(xp, cbi)
        d_all = sub_dist(xp, cbi)
        for r, m, lo, hi in ties:                                         # the tie is THE minimum, and the lower code wins
            assert dist[r, m] == 1 and d_all[r, m, lo] == 1 and d_all[r, m, hi] == 1 and codes[r, m] <= lo
        assert (dist > 0).mean() > 0.5                                    # lossy indeed
        out = _finish(c, xi, cbi, codes, "ivf pq4 lossy D=%d Ms=%d" % (D, Ms))
        out["tie_rows"] = ties
        out["lossy_share"] = float((dist > 0).mean())
        return out
    return xs.cached(("ivfpq4-lossy", D, Ms), make)


def grid_want(c, k, probe=None):
    """(D float32 tensor, I int64 tensor) of a 4-bit grid case from the int64 model on the DECODED rows"""
    return pq.grid_want(c, k, probe)


# ---- recovery ----------------------------------------------------------------------------------------------------------------------
REC_D, REC_M, REC_MS, REC_N, REC_NQ, REC_K, REC_R, REC_NLIST = 64, 8, 16, 4000, 200, 10, 128, 4


def recovery_fixture():
    """RandomState(7): codebooks randn(16, 16, 4); 4 000 rows = random codeword picks + 0.05 randn; 200 queries = rows + 0.1
    randn; everything scaled by 2^-3 (norms about 1) and stored as float32.  Returns (x, q, codebooks)."""
    rng = np.random.RandomState(7)
    dsub = REC_D // REC_MS
    cb = rng.randn(REC_MS, CODEWORDS, dsub)
    picks = rng.randint(0, CODEWORDS, size=(REC_N, REC_MS))
    x = decode(picks, cb) + 0.05 * rng.randn(REC_N, REC_D)
    q = x[rng.choice(REC_N, size=REC_NQ, replace=False)] + 0.1 * rng.randn(REC_NQ, REC_D)
    s = 2.0 ** -3
    return (x * s).astype(np.float32), (q * s).astype(np.float32), (cb * s).astype(np.float32)
