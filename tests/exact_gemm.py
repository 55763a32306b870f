"""Exact-arithmetic operands and host models for the GEMM family.

Every GEMM test against fp64 under a tolerance lets two kinds of error through: a plane product summed twice in place
of another one (2^-18 per term, at the tolerance), and a wrong element read where the data happen to be alike.  The
operands built here make every partial sum of the product exactly representable in fp32, so ANY summation order gives
the same bits and the expected result is an integer computation on the host: the comparisons are ``torch.equal``.

* ``plane_operand``: each plane written directly -- entries from {-1, 0, 1} times the plane's scale.  The planes are
  deliberately NOT a valid split of one fp32 matrix: the plane GEMMs take planes as operands and must treat them as
  independent matrices, so (0,2) summed twice in place of (2,0) changes the result.
* ``expected``: sum over the documented plane pairs of A_p B_q^T (k-contiguous) or A_p^T B_q (k-strided) in float64.
* ``assert_exact_safe``: the condition under which zero tolerance is legitimate, computed, not assumed.
* ``probe_operands``: one-hot rows against large random integers: C[m][n] == B[n][pi(m)] bit for bit, so a wrong index
  is reported as the index that WAS read.

The pair lists are the kernels' documentation: PA / PB of the six-step period in csrc/gemm_bf16_256.hip
((A, B) = (hi,hi) (hi,mid) (mid,hi) (hi,lo) (lo,hi) (mid,mid), BArgs in csrc/gemm_bf16.h), the header of
csrc/gemm_bf16x3.hip (`products` = 3 keeps ah bh + ah bm + am bh) and of csrc/gemm_f16x2_256.hip (ah bh + ah bl + al bh).

Plain module, no pytest configuration; numpy and torch on the CPU only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402

PAIRS6 = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))
PAIRS3 = ((0, 0), (0, 1), (1, 0))
PAIRS_H2 = ((0, 0), (0, 1), (1, 0))
SCALES_BF16 = (1.0, 2.0 ** -6, 2.0 ** -12)
SCALES_F16 = (1.0, 2.0 ** -8)
UNIT_BF16 = 2.0 ** -12          # the smallest term of PAIRS6 under SCALES_BF16: (0,2), (2,0), (1,1)
UNIT_F16 = 2.0 ** -8
DENSITY = 2.0 / 3.0             # nonzero share of a plane's entries (test_exact_gemm_host.py asserts it suffices)
ALPHA = 0.25                    # leaky-relu slope of every epilogue here: a power of two keeps the result exact

# ---- the shapes of tests/test_gpu_exact_gemm.py (M, N, K), shared with the host tests ---------------------------------
X3_NT_SHAPES = ((256, 256, 128),      # the minimum
                (300, 512, 384),      # ragged M, six K-tiles, whole periods
                (1000, 512, 192),     # eight tiles: half tiles only, odd K-tile count
                (520, 256, 1344),     # with a workspace: the slab form
                (512, 256, 768))      # with colsum
X3_TN_SHAPES = ((256, 256, 256), (512, 256, 1536), (256, 512, 768))
F16_NT_SHAPES = ((256, 256, 192), (300, 512, 384), (520, 256, 1344))
F16_TN_SHAPES = ((256, 256, 384),)
BF16_NT_SHAPES = ((128, 128, 64), (200, 256, 192), (77, 256, 512), (4096, 1024, 256),
                  (200, 256, 2048))   # split-K of both tile sizes (no listed shape has K >= 1024)
BF16_TN_SHAPES = ((256, 256, 128), (512, 768, 1280))
BF16_TN2_SHAPES = ((256, 256, 256, 256, 128), (512, 768, 1280, 256, 1280))      # (M1, N1, M2, N2, K)
FC_SHAPES = ((15, 64, 64), (130, 96, 192), (257, 512, 256))                     # (M, K, N)
FC_SK_SHAPE = (777, 2048, 2048, 512, 128)                                       # (M, K1, N1, K2, N2): >= 256 tiles of 128 x 128
H2_PROBE_SCALE = 2.0 ** -6       # fp16 probe: integers below 2^21 times 2^-6 are inside fp16's range, hi + lo exact (11 + 10 bits)
# The probe's cases, (entry, kind, M, N, K, k_strided) in the probe's own convention -- C[M][N], contraction K; k_strided:
# operands [K][M], [K][N].  kind: "x3" (B split into three bf16 planes, integers below 2^22), "h2" (two fp16 planes of
# B 2^-6, below 2^21), "bf16" (|B| <= 128: bf16 numbers), "f32" (below 2^22).  Two shapes per entry: a ragged one and a
# multi-tile one where the entry takes ragged shapes (the k-strided entries take multiples of 256 only: two tile grids).
PROBE_CASES = (
    ("x3_nt", "x3", 300, 512, 384, False), ("x3_nt", "x3", 1000, 512, 192, False),
    ("x3_nt", "x3", 1000, 512, 256, False),                    # (three products: K = 192 legalised)
    ("x3_tn", "x3", 256, 512, 768, True), ("x3_tn", "x3", 512, 256, 1536, True),
    ("f16x2_nt", "h2", 300, 512, 384, False), ("f16x2_nt", "h2", 1000, 512, 256, False),
    ("f16x2_tn", "h2", 256, 512, 768, True), ("f16x2_tn", "h2", 512, 256, 1536, True),
    ("bf16_nt", "bf16", 200, 256, 128, False), ("bf16_nt", "bf16", 4096, 1024, 256, False),
    ("bf16_tn", "bf16", 256, 256, 128, True), ("bf16_tn", "bf16", 512, 768, 1280, True),
    # the joint launch's two products, at both of BF16_TN2_SHAPES
    ("bf16_tn2a/1", "bf16", 256, 256, 128, True), ("bf16_tn2a/2", "bf16", 256, 256, 128, True),
    ("bf16_tn2b/1", "bf16", 512, 768, 1280, True), ("bf16_tn2b/2", "bf16", 1280, 256, 1280, True),
    # fp32 layer (M, K, N) = (257, 512, 256) and (130, 96 | 128, 192): forward C[M][N] over K; data gradient C[M][K] over N;
    # weight gradient C[K][N] over the M rows (k-strided)
    ("fc_fwd", "f32", 257, 256, 512, False), ("fc_fwd", "f32", 130, 192, 96, False),
    ("fc_bwd_data", "f32", 257, 512, 256, False), ("fc_bwd_data", "f32", 130, 128, 192, False),
    ("fc_bwd_weight", "f32", 512, 256, 512, True), ("fc_bwd_weight", "f32", 128, 192, 130, True),
    ("fc_bwd_weight2/1", "f32", 2048, 2048, 777, True), ("fc_bwd_weight2/2", "f32", 512, 128, 777, True),   # FC_SK_SHAPE
)
PROBE_BOUND = {"x3": 2 ** 22, "h2": 2 ** 21, "bf16": 129, "f32": 2 ** 22}


def x3_legal_k(K, products):
    """the k-contiguous plane GEMMs walk K-tiles in pairs: where products * K / 64 is odd, the next legal K"""
    return K + 64 if (products * K // 64) % 2 else K


def case_rng(*key):
    """the generator of one test case: the host tests and the GPU tests build the same operands from it"""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(ord(c) for c in str(k)))) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


# ---- operands -------------------------------------------------------------------------------------------------------
def plane_operand(rows, cols, n_planes, rng, scales, density=DENSITY, dtype=torch.bfloat16):
    """(buffer, plane, planes): ``buffer`` = CPU tensor [rows][ld] in the layout the kernels read -- plane p at columns
    [p * plane, p * plane + cols), plane > cols, ld > n_planes * plane, everything else poison (a NaN: an element read
    from a gap shows in the result); ``planes`` = the per-plane float64 matrices [rows][cols], independent entries from
    {-1, 0, 1} times ``scales[p]``."""
    p_nz = density / 2.0
    planes = [rng.choice(np.array([-1.0, 0.0, 1.0]), size=(rows, cols), p=[p_nz, 1.0 - density, p_nz]) * scales[p]
              for p in range(n_planes)]
    plane = cols + 8
    ld = n_planes * plane + 8
    buf = fp.poisoned((rows, ld), dtype=dtype, device="cpu")
    for p in range(n_planes):
        buf[:, p * plane:p * plane + cols] = torch.from_numpy(planes[p]).to(dtype)
    return buf, plane, planes


def int_operand(rows, cols, rng, lo=-2, hi=2, dtype=torch.bfloat16, pad=8):
    """(buffer [rows][cols + pad] with a poisoned gap, float64 values): integers in [lo, hi]"""
    v = rng.randint(lo, hi + 1, size=(rows, cols)).astype(np.float64)
    buf = fp.poisoned((rows, cols + pad), dtype=dtype, device="cpu")
    buf[:, :cols] = torch.from_numpy(v).to(dtype)
    return buf, v


def expected(planesA, planesB, pairs, k_strided=False):
    """sum over ``pairs`` (p, q) of A_p @ B_q^T (operands [rows][K]) or, ``k_strided``, A_p^T @ B_q ([K][columns]); float64"""
    out = None
    for p, q in pairs:
        t = planesA[p].T @ planesB[q] if k_strided else planesA[p] @ planesB[q].T
        out = t if out is None else out + t
    return out


def _granule_exp(x):
    """the largest e with every entry of x a multiple of 2^e (x float64; all zero: +inf)"""
    x = np.asarray(x, dtype=np.float64)
    nz = x[x != 0]
    if nz.size == 0:
        return np.inf
    m, e = np.frexp(np.abs(nz))                       # |x| = m 2^e, m in [0.5, 1): m 2^53 is an integer
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64))       # trailing zeros of the 53-bit significand
    return float(np.min(e - 53 + tz))


def assert_exact_safe(planesA, planesB, pairs, unit, k_strided=False, extra=0.0):
    """Zero tolerance is legitimate: every term a_p b_q is a multiple of ``unit`` and, for every output element,
    (sum_k sum_pairs |a| |b| + extra) / unit < 2^24 -- every partial sum, in any order, is an integer multiple of
    ``unit`` below 2^24 units: exact in fp32.  ``extra``: the largest |bias| an epilogue adds.  Returns that maximum
    (in units)."""
    ue = np.log2(unit)
    assert ue == np.floor(ue), "unit must be a power of two"
    total = None
    for p, q in pairs:
        ga, gb = _granule_exp(planesA[p]), _granule_exp(planesB[q])
        assert ga + gb >= ue, "a term of pair (%d, %d) is not a multiple of the unit 2^%d: granules 2^%s 2^%s" % (p, q, ue, ga, gb)
        a, b = np.abs(planesA[p]), np.abs(planesB[q])
        t = a.T @ b if k_strided else a @ b.T
        total = t if total is None else total + t
    worst = (float(total.max()) + float(extra)) / unit
    assert worst < 2.0 ** 24, "the absolute sums reach %g units of 2^%d: not below 2^24" % (worst, ue)
    return worst


def resum_f32(planesA, planesB, pairs, order, k_strided=False, chunk=16):
    """the same sum re-associated in float32: k taken in ``order``, in chunks, the pairs' partial products (float32
    matrix products) added one after another into one float32 accumulator"""
    acc = None
    for i in range(0, len(order), chunk):
        ks = order[i:i + chunk]
        for p, q in pairs:
            if k_strided:
                t = planesA[p][ks].astype(np.float32).T @ planesB[q][ks].astype(np.float32)
            else:
                t = planesA[p][:, ks].astype(np.float32) @ planesB[q][:, ks].astype(np.float32).T
            acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def f32_exact(v):
    """float64 array -> torch.float32, asserting that nothing is rounded"""
    v = np.asarray(v, dtype=np.float64)
    w = v.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), v), "the expected value is not an fp32 number"
    return torch.from_numpy(w)


# ---- epilogue models (all exact: integer bias, alpha = 1/4, masks from the sign of integers) ---------------------------
def lrelu(v, alpha=ALPHA):
    return np.maximum(v, alpha * v)


def split_planes(v32, n_planes=3, dtype=torch.bfloat16):
    """the torch split of an fp32 tensor: hi = round(v), mid = round(v - hi), lo = round(v - hi - mid)"""
    out, r = [], v32.clone()
    for _ in range(n_planes):
        p = r.to(dtype)
        out.append(p)
        r = r - p.float()
    return out


def plane_buffer(planes, plane, ld, pattern=0):
    """planes (tensors [M][N]) laid out [M][ld], ``plane`` columns apart, over the poison of ``pattern``: what a plane
    output written into ``footprint.poisoned`` memory must equal, gaps included"""
    M, N = planes[0].shape
    buf = fp.poisoned((M, ld), dtype=planes[0].dtype, device="cpu", pattern=pattern)
    for p, t in enumerate(planes):
        buf[:, p * plane:p * plane + N] = t
    return buf


def pack_bits(positive):
    """bool [M][N] -> uint8 [M][N / 8]: bit j of byte b of row r = positive[r][8 b + j]"""
    return torch.from_numpy(np.packbits(np.asarray(positive, dtype=bool), axis=1, bitorder="little"))


def interleave8(planes):
    """planes (tensors [M][N], M % 8 == 0) -> flat k8-interleaved [n][M / 8][N][8]: element (p, r, c) at
    ((p M/8 + r/8) N + c) 8 + r % 8"""
    M, N = planes[0].shape
    return torch.stack([t.reshape(M // 8, 8, N).permute(0, 2, 1) for t in planes]).contiguous().reshape(-1)


def bits(t):
    """an integer view for bit comparisons (NaN poison compares equal to itself)"""
    return fp.bits_of(t)


# ---- the probe ---------------------------------------------------------------------------------------------------------
def probe_operands(M, N, K, rng, k_strided=False, bound=2 ** 22):
    """(A, B, pi): A one-hot, A[m][pi(m)] = 1 ([M][K]; ``k_strided``: A[pi(m)][m] = 1, [K][M]); pi a random map onto
    0..K-1 that hits every k when M >= K; B = random integers in (-bound, bound) as float32 ([N][K]; ``k_strided``:
    [K][N]).  Every partial sum of a subset of the planes of such an integer is an integer below 2^24, so the product is
    B[n][pi(m)] bit for bit under six products and hi + mid of it under three, in any order."""
    pi = np.concatenate([rng.permutation(K), rng.randint(0, K, size=max(M - K, 0))])[:M]
    pi = pi[rng.permutation(M)]
    A = np.zeros((M, K), dtype=np.float32)
    A[np.arange(M), pi] = 1.0
    B = rng.randint(-bound + 1, bound, size=(N, K)).astype(np.float32)
    if k_strided:
        A, B = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    return A, B, pi


def probe_expected(B, pi, k_strided=False):
    """C[m][n] = B[n][pi(m)] (k-strided: B[pi(m)][n]); B any array of the operand's shape (a plane sum, say)"""
    return B[pi, :] if k_strided else B[:, pi].T


def probe_report(C, B, pi, k_strided=False, want=None):
    """None if C == want (default: B[n][pi(m)]); else a sentence naming the first wrong (m, n), the k it should have read
    and, where the value found is some other B[n][k'], that k'"""
    C = np.asarray(C, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    want = probe_expected(B, pi, k_strided) if want is None else np.asarray(want, dtype=np.float64)
    bad = ~((C == want) | (np.isnan(C) & np.isnan(want)))
    if not bad.any():
        return None
    m, n = (int(v) for v in np.argwhere(bad)[0])
    col = B[:, n] if k_strided else B[n]
    hits = np.nonzero(col == C[m, n])[0]
    rows = np.nonzero(B[pi, n] == C[m, n])[0] if k_strided else np.nonzero(B[n, pi] == C[m, n])[0]
    where = ("the value found is B[n][k'] for k' = %s (k' - k = %s)" % (hits[:4].tolist(), (hits[:4] - pi[m]).tolist()) if hits.size
             else "the value found is no element of B's row n")
    if rows.size:
        where += "; it is the right value of output row(s) m' = %s" % rows[:4].tolist()
    return ("first wrong element (m, n) = (%d, %d): found %r, expected B[n][k = %d] = %r; %s; %d of %d elements wrong"
            % (m, n, float(C[m, n]), int(pi[m]), float(want[m, n]), where, int(bad.sum()), bad.size))


def assert_probe(C, B, pi, k_strided=False, want=None, what="probe"):
    msg = probe_report(C, B, pi, k_strided, want)
    assert msg is None, "%s: %s" % (what, msg)


# ---- mutations: what the check must be able to see (tests/test_exact_gemm_host.py) -------------------------------------
def pair_mutations(pairs, n_planes):
    """{name: mutated pair list}: every single mutation of the list"""
    out = {}
    for i, pq in enumerate(pairs):
        out["drop %s" % (pq,)] = tuple(x for j, x in enumerate(pairs) if j != i)
    swap = lambda a, b: tuple(b if x == a else x for x in pairs)
    out["(1,0) -> a second (0,1)"] = swap((1, 0), (0, 1))
    if n_planes == 3 and (2, 0) in pairs:
        out["(2,0) -> a second (0,2)"] = swap((2, 0), (0, 2))
        out["(0,2) -> a second (2,0)"] = swap((0, 2), (2, 0))
    if n_planes == 3:
        out["add (1,2)"] = tuple(pairs) + ((1, 2),)
        out["add (2,2)"] = tuple(pairs) + ((2, 2),)
    else:
        out["add (1,1)"] = tuple(pairs) + ((1, 1),)
    return out


def probe_mutations(pi, M, K, tile=256):
    """{name: (mutated pi, rows the mutation touches)}: the index errors the probe must see"""
    last = np.arange((M - 2) // tile * tile, M)                       # (from the tile of row M - 2 on: a one-row last tile has no m - 1)
    shifted = pi.copy()
    shifted[last[1:]] = pi[last[1:] - 1]                              # row m reads what row m - 1 should (last row tile)
    flip = lambda b: np.where((pi ^ b) < K, pi ^ b, pi - b)           # (K no multiple of 2 b: the last group's partner is below)
    return {"k ^ 1": (flip(1), np.arange(M)),
            "two 8-wide k groups swapped": (flip(8), np.arange(M)),
            "row m -> m - 1 in the last tile": (shifted, last[1:])}


# ---- the cases: one builder per family, so that the host tests check exactly what the GPU tests launch ---------------
def plane_case(tag, M, N, K, n_planes=3, k_strided=False):
    """operands of a plane GEMM: A [M][K], B [N][K] (``k_strided``: [K][M], [K][N]) as bf16 (3) or fp16 (2) planes"""
    rng = case_rng(tag, M, N, K)
    scales, dtype = (SCALES_BF16, torch.bfloat16) if n_planes == 3 else (SCALES_F16, torch.float16)
    sa, sb = ((K, M), (K, N)) if k_strided else ((M, K), (N, K))
    A, pa, Ap = plane_operand(sa[0], sa[1], n_planes, rng, scales, dtype=dtype)
    B, pb, Bp = plane_operand(sb[0], sb[1], n_planes, rng, scales, dtype=dtype)
    return dict(A=A, plane_a=pa, Ap=Ap, B=B, plane_b=pb, Bp=Bp, rng=rng, k_strided=k_strided,
                unit=UNIT_BF16 if n_planes == 3 else UNIT_F16)


def int_case(tag, M, N, K, k_strided=False, dtype=torch.bfloat16):
    """operands of a one-plane GEMM (bf16 or fp32): integers in {-2 .. 2}"""
    rng = case_rng(tag, M, N, K)
    sa, sb = ((K, M), (K, N)) if k_strided else ((M, K), (N, K))
    A, Av = int_operand(sa[0], sa[1], rng, dtype=dtype)
    B, Bv = int_operand(sb[0], sb[1], rng, dtype=dtype)
    return dict(A=A, Ap=[Av], B=B, Bp=[Bv], rng=rng, k_strided=k_strided, unit=1.0)


TN_COL0 = 256           # the k-strided plane cases are column windows [TN_COL0, TN_COL0 + M | N) of wider operands


def tn_window_case(M, N, K):
    """the k-strided plane case as a column window of operands TN_COL0 columns wider (the k8-interleaved entry's
    a_col0 / b_col0): Ap / Bp = the window's planes, Ap_full / Bp_full = the whole operands'"""
    c = plane_case("x3tn", M + TN_COL0, N + TN_COL0, K, k_strided=True)
    c["Ap_full"], c["Bp_full"] = c["Ap"], c["Bp"]
    c["Ap"] = [np.ascontiguousarray(p[:, TN_COL0:]) for p in c["Ap_full"]]
    c["Bp"] = [np.ascontiguousarray(p[:, TN_COL0:]) for p in c["Bp_full"]]
    return c


PAIRS1 = ((0, 0),)
BIAS_MAX = 8            # epilogue biases: integers in [-BIAS_MAX, BIAS_MAX]


def int_bias(n, rng):
    return rng.randint(-BIAS_MAX, BIAS_MAX + 1, size=n).astype(np.float64)


def int_aux(M, N, rng):
    """an integer-valued activation whose sign is the mask: {-2 .. 2}, zeros included (0 is not > 0)"""
    return rng.randint(-2, 3, size=(M, N)).astype(np.float64)


def all_plane_cases():
    """(name, case, pairs) of every plane-GEMM case of the GPU tests"""
    out = []
    for M, N, K in X3_NT_SHAPES:
        for products, pairs in ((6, PAIRS6), (3, PAIRS3)):
            Kl = x3_legal_k(K, products)
            out.append(("x3_nt %s products=%d" % ((M, N, Kl), products), plane_case("x3nt", M, N, Kl), pairs))
    for M, N, K in X3_TN_SHAPES:
        for products, pairs in ((6, PAIRS6), (3, PAIRS3)):
            out.append(("x3_tn %s products=%d" % ((M, N, K), products), tn_window_case(M, N, K), pairs))
    for M, N, K in F16_NT_SHAPES:
        Kl = x3_legal_k(K, 3)
        out.append(("f16x2_nt %s" % ((M, N, Kl),), plane_case("h2nt", M, N, Kl, n_planes=2), PAIRS_H2))
    for M, N, K in F16_TN_SHAPES:
        out.append(("f16x2_tn %s" % ((M, N, K),), plane_case("h2tn", M, N, K, n_planes=2, k_strided=True), PAIRS_H2))
    return out


def all_int_cases():
    """(name, case) of every one-plane case (bf16 and fp32 GEMMs) of the GPU tests"""
    out = []
    for M, N, K in BF16_NT_SHAPES:
        out.append(("bf16_nt %s" % ((M, N, K),), int_case("b16nt", M, N, K)))
    for M, N, K in BF16_TN_SHAPES:
        out.append(("bf16_tn %s" % ((M, N, K),), int_case("b16tn", M, N, K, k_strided=True)))
    for M1, N1, M2, N2, K in BF16_TN2_SHAPES:
        out.append(("bf16_tn2/1 %s" % ((M1, N1, K),), int_case("b16tn2a", M1, N1, K, k_strided=True)))
        out.append(("bf16_tn2/2 %s" % ((M2, N2, K),), int_case("b16tn2b", M2, N2, K, k_strided=True)))
    for M, K, N in FC_SHAPES:
        c = fc_case(M, K, N)
        out += [("fc_%s %s" % (key, (M, K, N)), c[key]) for key in ("fwd", "bwd_data", "bwd_weight")]
    M, K1, N1, K2, N2 = FC_SK_SHAPE
    out.append(("fc_bwd_weight2/1", int_case("fcsk1", K1, N1, M, k_strided=True, dtype=torch.float32)))
    out.append(("fc_bwd_weight2/2", int_case("fcsk2", K2, N2, M, k_strided=True, dtype=torch.float32)))
    return out


def fc_k64(K):
    """cdml_fc_bwd_data / cdml_fc_bwd_weight take K in multiples of 64: the next one"""
    return (K + 63) // 64 * 64


def fc_case(M, K, N):
    """the fp32 layer y[M][N] = x[M][K] W[K][N]: forward (A = x, B = W k-strided on one side only -- held as the
    product x . (W^T)^T), data gradient dx[M][K] = dy[M][N] W[K][N]^T, weight gradient dW[K][N] = x^T dy"""
    f32 = torch.float32
    Kb = fc_k64(K)
    rng = case_rng("fcfwd", M, K, N)
    x, xv = int_operand(M, K, rng, dtype=f32)
    W, Wv = int_operand(K, N, rng, dtype=f32)
    fwd = dict(A=x, Ap=[xv], B=W, Bp=[np.ascontiguousarray(Wv.T)], rng=rng, k_strided=False, unit=1.0)
    rng = case_rng("fcbwd", M, Kb, N)
    dy, dyv = int_operand(M, N, rng, dtype=f32)
    W2, W2v = int_operand(Kb, N, rng, dtype=f32)
    bwd = dict(A=dy, Ap=[dyv], B=W2, Bp=[W2v], rng=rng, k_strided=False, unit=1.0)
    return dict(fwd=fwd, bwd_data=bwd, bwd_weight=int_case("fcbww", Kb, N, M, k_strided=True, dtype=f32))


_PROBES = {}


def probe_case(entry, kind, M, N, K, k_strided):
    """One probe case, built once: the operands (A one-hot, B integers below PROBE_BOUND[kind], pi), the planes the
    kernel multiplies as float64 (``Ap``, ``Bp``: the torch split of B, of B 2^-6 for "h2"; one plane for "bf16" / "f32"),
    the pair list(s) and per pair list the plane sum ``src`` with C[m][n] = src[n][pi(m)] / ``unit``.  (``unit`` = the
    scale the entry undoes with out_scale: 2^-6 for "h2", else 1.)"""
    key = (entry, kind, M, N, K, k_strided)
    if key in _PROBES:
        return _PROBES[key]
    A, B, pi = probe_operands(M, N, K, case_rng("probe", entry, M, N, K, int(k_strided)), k_strided, PROBE_BOUND[kind])
    A64, zero = A.astype(np.float64), np.zeros(A.shape)
    if kind == "x3":
        Bp = [p.double().numpy() for p in split_planes(torch.from_numpy(B), 3, torch.bfloat16)]
        Ap, unit = [A64, zero, zero], 1.0
        srcs = {PAIRS6: Bp[0] + Bp[1] + Bp[2], PAIRS3: Bp[0] + Bp[1]}
    elif kind == "h2":
        Bp = [p.double().numpy() for p in split_planes(torch.from_numpy(B * np.float32(H2_PROBE_SCALE)), 2, torch.float16)]
        Ap, unit = [A64, zero], H2_PROBE_SCALE
        srcs = {PAIRS_H2: Bp[0] + Bp[1]}
    else:
        Ap, Bp, unit = [A64], [B.astype(np.float64)], 1.0
        srcs = {PAIRS1: Bp[0]}
    c = dict(entry=entry, kind=kind, shape=(M, N, K), k_strided=k_strided, A=A, B=B, pi=pi, Ap=Ap, Bp=Bp, unit=unit, srcs=srcs,
             name="%s %s" % (entry, (M, N, K)))
    _PROBES[key] = c
    return c


def probe_want(c, pairs):
    """asserts that the case is exact under ``pairs`` (computed: assert_exact_safe on the planes the kernel multiplies)
    and returns (src, want): want[m][n] = src[n][pi(m)] / unit, the value the entry must give"""
    assert_exact_safe(c["Ap"], c["Bp"], pairs, c["unit"], c["k_strided"])
    src = c["srcs"][pairs] / c["unit"]
    return src, probe_expected(src, c["pi"], c["k_strided"])


def probe_cases(entry):
    return [probe_case(*t) for t in PROBE_CASES if t[0] == entry]
