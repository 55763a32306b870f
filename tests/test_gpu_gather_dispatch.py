"""Which k_sample_gather instantiation the fused launcher picks (csrc/sampler_gather.hip over csrc/gather_plan.h): every cell
(row format, sampler mode, NCH bucket, interleaved copy, one step / several per launch) at the smallest shape that selects
it -- a 64-row catalogue, batch 8 (24 or 16 rows per step: whole groups of 8 for the interleaved copy), F at the bucket
edges -- against the unfused chain the format's own tests use as their identity, bit for bit: the ids of sample_uniform /
sample_inbatch / sample_listed, the rows of gather_rows / gather_rows_f16, the planes of split_f32_bf16x3 /
split_f32_f16x2, the copy of interleave8_bf16x3; and shift_out, kind_out and the out-of-catalogue flag.  A wrong rung
(a bucket too small for F) truncates rows; a wrong mode or format changes ids or bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, B, SEED, STEP, L = 64, 8, 31, 5, 4
N_PAIRS = 40                  # step 5 reads pairs 0..7, step 6 pairs 8..15: the out-of-catalogue id sits in pair 12
HARD = 0.5                    # half of the listed draws take the anchor's list
H2_SCALE = 16384.0            # include/cdml.h CDML_F16X2_X_SCALE

# fp32 table: NCH = ceil(F / 256) -> buckets 2 | 6 | 8 (three-plane and two-plane rows: 6 | 8); fp16 table: ceil(F / 512) -> 1 | 3 | 8
EDGES = {"f32": [512, 516, 1536, 1540, 2048], "x3": [512, 516, 1536, 1540, 2048], "h2": [512, 516, 1536, 1540, 2048],
         "x3k": [1536, 1540, 2048], "f16": [512, 520, 1536, 1544, 4096]}
MODES = {"f32": [0, 1, 2], "x3": [0, 1, 2], "x3k": [0, 1, 2], "h2": [0, 1], "f16": [0, 1, 2]}
CASES = [(fmt, mode, F, n_steps) for fmt in EDGES for mode in MODES[fmt] for F in EDGES[fmt] for n_steps in (1, 2)]


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import engine, engine_bf16, ops
    cdml_amd.load_library()
    rng = np.random.default_rng(7)
    a = rng.integers(0, N, size=N_PAIRS)
    p = (a + 1 + rng.integers(0, N - 1, size=N_PAIRS)) % N
    pairs = np.stack([a, p], 1).astype(np.int32)
    pairs[12, 0] = N + 5
    lists = rng.integers(0, N, size=(N, L)).astype(np.int32)
    lists[rng.random((N, L)) < 0.3] = -1

    class NS:
        pass
    ns = NS()
    ns.ops, ns.dev = ops, gpu
    ns.pairs, ns.lists = torch.from_numpy(pairs).to(gpu), torch.from_numpy(lists).to(gpu)
    tables = {}

    def table(f16, F):                       # one synthetic catalogue per (element type, F), shared by the cases
        if (f16, F) not in tables:
            mk = engine_bf16.FeatureTableF16 if f16 else engine.FeatureTable
            tables[(f16, F)] = mk.synthetic(N, F, 5, gpu).data
        return tables[(f16, F)]
    ns.table = table
    return ns


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _chain(cd, fmt, mode, F, table, ld, s):
    """(ids, shift, kind, rows, flag) of step STEP + s from the unfused entry points"""
    ops, dev = cd.ops, cd.dev
    R = B * (2 if mode == 1 else 3)
    idx = torch.full((R,), -9, dtype=torch.int32, device=dev)
    shift = torch.full((1,), -9, dtype=torch.int32, device=dev)
    kind = torch.full((B,), -9, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if mode == 0:
        ops.sample_uniform(cd.pairs, N, SEED, STEP + s, B, idx)
    elif mode == 1:
        ops.sample_inbatch(cd.pairs, SEED, STEP + s, B, idx, shift)
    else:
        ops.sample_listed(cd.pairs, N, SEED, STEP + s, B, cd.lists, HARD, idx, kind_out=kind)
    if fmt == "f16":
        want = torch.full((R, ld), 3.0, dtype=torch.bfloat16, device=dev)
        ops.gather_rows_f16(table, 0, idx, F, want, oob_flag=flag)
    elif fmt == "f32":
        want = torch.full((R, ld), 3.0, dtype=torch.float32, device=dev)
        ops.gather_rows(table, 0, idx, F, want, oob_flag=flag)
    else:
        planes = 2 if fmt == "h2" else 3
        plane = ld // planes
        rows = torch.full((R, plane), 3.0, dtype=torch.float32, device=dev)
        ops.gather_rows(table, 0, idx, F, rows, oob_flag=flag)
        want = torch.zeros((R, ld), dtype=torch.float16 if fmt == "h2" else torch.bfloat16, device=dev)
        if fmt == "h2":
            ops.split_f32_f16x2(rows, want, plane, H2_SCALE)
        else:
            ops.split_f32_bf16x3(rows, want, plane)
    return idx, shift, kind, want, flag


@pytest.mark.parametrize("fmt,mode,F,n_steps", CASES, ids=["%s-mode%d-F%d-steps%d" % c for c in CASES])
def test_the_fused_launch_is_the_unfused_chain(cd, fmt, mode, F, n_steps):
    ops, dev = cd.ops, cd.dev
    f16 = fmt == "f16"
    table = cd.table(f16, F)
    R = B * (2 if mode == 1 else 3)
    if f16:
        ld, dtype = (F + 7) // 8 * 8 + 8, torch.bfloat16
    elif fmt == "f32":
        ld, dtype = (F + 3) // 4 * 4 + 4, torch.float32
    else:
        planes = 2 if fmt == "h2" else 3
        ld, dtype = planes * ((F + 255) // 256 * 256), torch.float16 if fmt == "h2" else torch.bfloat16
    x = torch.full((n_steps, R, ld), 7.0, dtype=dtype, device=dev)
    idx = torch.full((n_steps, R), -9, dtype=torch.int32, device=dev)
    shift = torch.full((n_steps,), -9, dtype=torch.int32, device=dev)
    kind = torch.full((n_steps, B), -9, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    xk = torch.full((n_steps, R * ld), float("nan"), dtype=torch.bfloat16, device=dev) if fmt == "x3k" else None
    one = n_steps == 1
    pick = lambda t: None if t is None else (t[0] if one else t)
    if mode == 2:
        ops.sample_gather_listed(cd.pairs, SEED, STEP, B, table, F, cd.lists, HARD, pick(idx), pick(x), kind_out=pick(kind),
                                 n_steps=n_steps, oob_flag=flag, x_ki=pick(xk))
    else:
        ops.sample_gather(mode, cd.pairs, SEED, STEP, B, table, F, pick(idx), pick(x), shift_out=shift, n_steps=n_steps,
                          oob_flag=flag, x_ki=pick(xk))
    flags = 0
    for s in range(n_steps):
        want_idx, want_shift, want_kind, want, want_flag = _chain(cd, fmt, mode, F, table, ld, s)
        assert torch.equal(idx[s], want_idx), s
        if mode == 1:
            assert shift[s].item() == want_shift.item() and 1 <= shift[s].item() < B, s
        if mode == 2:
            assert torch.equal(kind[s], want_kind), s
        assert torch.equal(_bits(x[s]), _bits(want)), s                      # every row whole: the bucket holds F columns
        if xk is not None:
            il = torch.zeros(R * ld, dtype=torch.bfloat16, device=dev)
            ops.interleave8_bf16x3(x[s], ld // 3, R, ld // 3, il)
            assert torch.equal(_bits(xk[s]), _bits(il)), s
        flags |= int(want_flag.item())
    assert int(flag.item()) == flags == (1 if n_steps == 2 else 0)           # (pair 12 is read by the second step only)
    assert x[..., F - 1].float().abs().sum() > 0                            # the last column of the last chunk is data, not pad
    if mode == 2 and n_steps == 2:
        assert 0 < int(kind.sum()) < kind.numel()                            # both kinds of draw were made
