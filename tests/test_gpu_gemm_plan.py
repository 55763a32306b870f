"""The K partition of the plane GEMMs pinned in REAL arithmetic.  tests/test_gpu_exact_gemm.py compares with integer sums,
which are exact in any order, so it cannot see a changed partition; here the operands are normal-distributed fp32 values
(split into planes by the project's own split entries), and a split-K call must equal, bit for bit, the fp32 sum in slab
order of UNSPLIT calls of the same entry on the slabs that csrc/gemm_plan.h plans (the rows of tests/data/gemm_plan_table.txt
for these shapes): every slab's K range, their number and the order of the combine pass show in the last bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cdml_amd import ops  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
H2_SCALE = 16.0                                             # the fp16 planes hold value * 2^4 (|value| < 2^12: far inside fp16's range)


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


def normal(rows, cols, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(rows, cols, generator=g, dtype=F32).to(dev)


def planes(v, n, dev):
    """fp32 [rows][cols] -> (the project's split of it [rows][n planes, `plane` apart], plane)"""
    rows, cols = v.shape
    plane = cols + 8
    dst = torch.zeros((rows, n * plane + 8), dtype=BF16 if n == 3 else F16, device=dev)
    if n == 3:
        ops.split_f32_bf16x3(v, dst, plane)
    else:
        ops.split_f32_f16x2(v, dst, plane, H2_SCALE)
    return dst, plane


def workspace(nbytes, dev):
    return torch.zeros(max(int(nbytes), 16) // 4 + 4, dtype=F32, device=dev)


def slab_sum(slabs):
    """k_x3_sum_slabs: slab 0, then the others added one by one in fp32"""
    s = slabs[0].clone()
    for z in slabs[1:]:
        s += z
    return s


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_x3_tn_is_the_slab_order_sum_of_its_planned_slabs(dev):
    """six products, M = N = 256, K = 1536: 144 K-tile steps in 6 slabs of 24 steps = 256 k; each window alone is unsplit"""
    M, N, K, n, k = 256, 256, 1536, 6, 256
    A3, pa = planes(normal(K, M, 1, dev), 3, dev)
    B3, pb = planes(normal(K, N, 2, dev), 3, dev)
    C = torch.zeros((M, N), dtype=F32, device=dev)
    ops.gemm_bf16x3_tn(A3, pa, B3, pb, C, M, N, K, products=6, workspace=workspace(ops.gemm_bf16x3_workspace(True, M, N, K, 6), dev))
    slabs = []
    for z in range(n):
        S = torch.zeros((M, N), dtype=F32, device=dev)
        ops.gemm_bf16x3_tn(A3[z * k:(z + 1) * k], pa, B3[z * k:(z + 1) * k], pb, S, M, N, k, products=6,
                           workspace=workspace(ops.gemm_bf16x3_workspace(True, M, N, k, 6), dev))
        slabs.append(S)
    assert same_bits(C, slab_sum(slabs))
    assert not same_bits(C, slab_sum(slabs[::-1]))           # (the data can tell an order: the comparison above is not vacuous)


def test_f16x2_tn_is_the_slab_order_sum_of_its_planned_slabs(dev):
    """two fp16 planes, M = N = 256, K = 3072: 144 steps (three per K-tile) in 6 slabs of 24 steps = 512 k"""
    M, N, K, n, k = 256, 256, 3072, 6, 512
    A2, pa = planes(normal(K, M, 3, dev), 2, dev)
    B2, pb = planes(normal(K, N, 4, dev), 2, dev)
    C = torch.zeros((M, N), dtype=F32, device=dev)
    ops.gemm_f16x2_tn(A2, pa, B2, pb, C, M, N, K, 1.0, workspace=workspace(ops.gemm_f16x2_workspace(True, M, N, K), dev))
    slabs = []
    for z in range(n):
        S = torch.zeros((M, N), dtype=F32, device=dev)
        ops.gemm_f16x2_tn(A2[z * k:(z + 1) * k], pa, B2[z * k:(z + 1) * k], pb, S, M, N, k, 1.0,
                          workspace=workspace(ops.gemm_f16x2_workspace(True, M, N, k), dev))
        slabs.append(S)
    assert same_bits(C, slab_sum(slabs))
    assert not same_bits(C, slab_sum(slabs[::-1]))


def test_x3_nt_is_the_sum_of_its_two_planned_slabs(dev):
    """six products, epilogue 3 with a workspace, M = N = 256, K = 1280: 120 steps; one row tile is the 60-step class: 2 slabs
    of 640 k.  A slab alone = the call on a column window of every plane: moved base, the same lda and plane stride, K = 640."""
    M, N, K, k = 256, 256, 1280, 640
    A3, pa = planes(normal(M, K, 5, dev), 3, dev)
    B3, pb = planes(normal(N, K, 6, dev), 3, dev)
    C = torch.zeros((M, N), dtype=F32, device=dev)
    ops.gemm_bf16x3_nt(ops.BE_F32, A3, pa, B3, pb, C, M, N, K, products=6,
                       workspace=workspace(ops.gemm_bf16x3_workspace(False, M, N, K, 6), dev))
    slabs = []
    for z in range(2):
        S = torch.zeros((M, N), dtype=F32, device=dev)
        ops.gemm_bf16x3_nt(ops.BE_F32, A3[:, z * k:], pa, B3[:, z * k:], pb, S, M, N, k, products=6,
                           workspace=workspace(ops.gemm_bf16x3_workspace(False, M, N, k, 6), dev))
        slabs.append(S)
    assert same_bits(C, slab_sum(slabs))
    # no workspace = ONE pass over K: other sums, so other last bits somewhere (seeds 5 / 6: they do differ)
    one = torch.zeros((M, N), dtype=F32, device=dev)
    ops.gemm_bf16x3_nt(ops.BE_F32, A3, pa, B3, pb, one, M, N, K, products=6)
    assert not same_bits(C, one)
