"""The exact-arithmetic GEMM tests' own footing (tests/exact_gemm.py), checked without a GPU, on the very operands
tests/test_gpu_exact_gemm.py launches:

* exactness -- ``assert_exact_safe`` holds for every shape, and the expectation is unchanged, bit for bit, under a float32
  re-summation in a shuffled k order: zero tolerance on the GPU is legitimate;
* sensitivity -- every single mutation of the pair list changes at least half of the output elements, and every index
  mutation of the probe at least half of the elements of the rows it touches (k ^ 1 and the swapped k groups touch every
  row; "row m reads row m - 1 in the last tile" touches that tile's rows only -- 44 of 300 -- so half of ALL outputs cannot
  be asked of it): the check can fail."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402

PLANE_CASES = xg.all_plane_cases()
INT_CASES = xg.all_int_cases()


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "collaborative-deep-metric-learning_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_pair_lists_are_the_documented_ones():
    """PAIRS6 against the kernels' own tables, read from the source: every `constexpr int PA[6] = {..}, PB[6] = {..}` of
    csrc/gemm_bf16_256.hip (the six-step period first, in PAIRS6's order; the resident-plane walks: the same set), the
    walk order BArgs documents (csrc/gemm_bf16.h) and the three-term sums in the headers of the two plane files"""
    tables = re.findall(r"constexpr int PA\[6\] = \{([^}]*)\}, PB\[6\] = \{([^}]*)\}", _src("gemm_bf16_256.hip"))
    assert len(tables) >= 2, "the PA / PB tables are no longer where the test reads them"
    lists = [tuple(zip(*(tuple(int(v) for v in t.split(",")) for t in ab))) for ab in tables]
    assert lists[0] == xg.PAIRS6, "the six-step period's (A, B) planes"
    for l in lists:
        assert len(l) == 6 and sorted(l) == sorted(xg.PAIRS6), l
    name = {"hi": 0, "mid": 1, "lo": 2}
    doc = re.search(r"walked\s+//\s+as \(A, B\) = ((?:\(\w+,\w+\) ?)+)", _src("gemm_bf16.h"))
    assert doc, "BArgs no longer documents the walk"
    assert tuple((name[a], name[b]) for a, b in re.findall(r"\((\w+),(\w+)\)", doc.group(1))) == xg.PAIRS6
    assert "ah bh + ah bm + am bh" in _src("gemm_bf16x3.hip") and xg.PAIRS3 == ((0, 0), (0, 1), (1, 0)) == xg.PAIRS6[:3]
    assert "ah bh + ah bl + al bh" in _src("gemm_f16x2_256.hip") and xg.PAIRS_H2 == ((0, 0), (0, 1), (1, 0))


@pytest.mark.parametrize("name,case,pairs", PLANE_CASES, ids=[c[0] for c in PLANE_CASES])
def test_plane_cases_are_exact_and_sensitive(name, case, pairs):
    Ap, Bp, ks = case["Ap"], case["Bp"], case["k_strided"]
    n_planes = len(Ap)
    worst = xg.assert_exact_safe(Ap, Bp, pairs, case["unit"], ks, extra=xg.BIAS_MAX)
    want = xg.expected(Ap, Bp, pairs, ks)
    K = Ap[0].shape[0] if ks else Ap[0].shape[1]
    assert K <= 3072
    order = np.random.RandomState(1).permutation(K)
    again = xg.resum_f32(Ap, Bp, pairs, order, ks)
    assert again.dtype == np.float32 and np.array_equal(again.astype(np.float64), want), "not order-independent"
    xg.f32_exact(want)
    # the layout: plane gaps and the row tail are there, and poisoned
    for buf, plane, planes in ((case["A"], case["plane_a"], case.get("Ap_full", Ap)), (case["B"], case["plane_b"], case.get("Bp_full", Bp))):
        cols = planes[0].shape[1]
        assert plane > cols and buf.shape[1] > n_planes * plane and plane % 8 == 0 and buf.shape[1] % 8 == 0
        assert torch.isnan(buf[:, cols:plane].float()).all() and torch.isnan(buf[:, n_planes * plane:].float()).all()
        for p in range(n_planes):
            assert np.array_equal(buf[:, p * plane:p * plane + cols].double().numpy(), planes[p])
    # every single mutation of the pair list is visible in at least half of the outputs
    shares = {}
    for mname, mpairs in xg.pair_mutations(pairs, n_planes).items():
        shares[mname] = float((xg.expected(Ap, Bp, mpairs, ks) != want).mean())
    print("%s: %.3g units at most; share of outputs each mutation changes: %s" % (name, worst, shares))
    low = {k: v for k, v in shares.items() if v < 0.5}
    assert not low, "mutations that change fewer than half of the outputs: %s" % low


@pytest.mark.parametrize("name,case", INT_CASES, ids=[c[0] for c in INT_CASES])
def test_integer_cases_are_exact(name, case):
    Ap, Bp, ks = case["Ap"], case["Bp"], case["k_strided"]
    xg.assert_exact_safe(Ap, Bp, xg.PAIRS1, 1.0, ks, extra=xg.BIAS_MAX)
    want = xg.expected(Ap, Bp, xg.PAIRS1, ks)
    K = Ap[0].shape[0] if ks else Ap[0].shape[1]
    order = np.random.RandomState(2).permutation(K)
    assert np.array_equal(xg.resum_f32(Ap, Bp, xg.PAIRS1, order, ks, chunk=64).astype(np.float64), want)
    assert float((want != 0).mean()) > 0.5                  # (a product that is mostly zero would check little)


PROBES = [xg.probe_case(*t) for t in xg.PROBE_CASES]


@pytest.mark.parametrize("c", PROBES, ids=[c["name"] for c in PROBES])
def test_probe_is_exact_and_names_the_index(c):
    """every probe case of the GPU tests (the same objects: xg.probe_case): exact under its pair list(s), the product is
    B[n][pi(m)] (the documented plane sum of it), unchanged under a shuffled float32 re-summation; every index mutation
    changes at least half of the elements of the rows it touches and is named by the report"""
    (M, N, K), ks = c["shape"], c["k_strided"]
    A, B, pi = c["A"], c["B"], c["pi"]
    assert A.shape == ((K, M) if ks else (M, K)) and B.shape == ((K, N) if ks else (N, K))
    assert set(pi.tolist()) == set(range(K)) or M < K, "every k is read by some row"
    assert (A.sum(0 if ks else 1) == 1).all()
    order = np.random.RandomState(3).permutation(K)
    for pairs in c["srcs"]:
        src, want = xg.probe_want(c, pairs)
        assert np.array_equal(xg.expected(c["Ap"], c["Bp"], pairs, ks) / c["unit"], want)
        assert np.array_equal(xg.resum_f32(c["Ap"], c["Bp"], pairs, order, ks, chunk=64).astype(np.float64) / c["unit"], want)
        xg.f32_exact(want)
    full = max(c["srcs"], key=len)
    src, want = xg.probe_want(c, full)
    assert np.array_equal(src, B.astype(np.float64)), "the full pair list gives the integer itself"
    assert xg.probe_report(want, src, pi, ks) is None
    for mname, (mpi, rows) in xg.probe_mutations(pi, M, K).items():
        assert mpi.min() >= 0 and mpi.max() < K
        got = xg.probe_expected(src, mpi, ks)
        share = float((got[rows] != want[rows]).mean())        # (of the rows the mutation touches: a last-tile error stays there)
        assert share >= 0.5, (mname, share)
        msg = xg.probe_report(got, src, pi, ks)
        assert msg is not None and "k' = " in msg, msg
        m = int(np.argwhere(got != want)[0][0])
        if c["kind"] != "bf16":                                # (|B| <= 128 repeats within a row: the first k' found may be another)
            assert "k' - k = [%d" % (int(mpi[m]) - int(pi[m])) in msg, msg   # the report names the index that was read


def test_epilogue_models():
    """the host models of the epilogues: bit packing, interleave, plane split"""
    pos = np.zeros((2, 16), dtype=bool)
    pos[0, 0] = pos[0, 9] = pos[1, 15] = True
    assert xg.pack_bits(pos).tolist() == [[1, 2], [0, 128]]
    planes = [torch.arange(16 * 4, dtype=torch.float32).reshape(16, 4) + 100 * p for p in range(3)]
    flat = xg.interleave8(planes)
    M, N = 16, 4
    for p, r, c in ((0, 0, 0), (1, 9, 3), (2, 15, 2)):
        assert flat[((p * M // 8 + r // 8) * N + c) * 8 + r % 8] == planes[p][r, c]
    v = torch.tensor([[1.0 + 2.0 ** -10 + 2.0 ** -20, -3.25, 0.0]])
    hi, mid, lo = xg.split_planes(v)
    assert torch.equal(hi.float() + mid.float() + lo.float(), v)
    assert np.array_equal(xg.lrelu(np.array([-4.0, 0.0, 8.0])), np.array([-1.0, 0.0, 8.0]))
    with pytest.raises(AssertionError):
        xg.f32_exact(np.array([1.0 + 2.0 ** -30]))
    with pytest.raises(AssertionError):                         # a term below the unit is refused
        xg.assert_exact_safe([np.array([[2.0 ** -13]])], [np.array([[1.0]])], xg.PAIRS1, xg.UNIT_BF16)
    with pytest.raises(AssertionError):                         # 2^24 units are refused
        xg.assert_exact_safe([np.full((1, 4096), 64.0)], [np.full((1, 4096), 64.0)], xg.PAIRS1, 1.0)
