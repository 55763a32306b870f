"""tests/footprint.py checked on the CPU: every failure class the GPU footprint tests exist for -- an unwritten element, a
write in each guard zone, a result that depends on poisoned memory, a modified input -- is planted with a fake "kernel" on
CPU tensors and must be caught and located; plus the accounting of tests/footprint_table.py against include/cdml.h."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import footprint_table as table  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8]
ROWS, COLS, LD = 5, 12, 16


def _value(dtype, k=3):
    return torch.tensor(k, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_layout_alignment_and_poison(dtype):
    for pattern in (0, 1):
        g = fp.Guarded((ROWS, COLS), dtype, "cpu", ld=LD, pattern=pattern)
        assert g.view.shape == (ROWS, COLS) and g.view.stride() == (LD, 1) and g.view.data_ptr() % 4096 == 0
        assert g.start >= g.guard_bytes and g.raw.numel() - g.end >= g.guard_bytes
        want = fp.poison_scalar(dtype, pattern)
        assert bool((fp.bits_of(g.flat) == want).all()), "payload and row gaps hold the poison"
        assert bool((fp.bits_of(g.elems) == want).all()), "the guards hold the poison"
        if dtype.is_floating_point:
            assert bool(torch.isnan(g.flat.float()).all())
        g.assert_guards_intact()
    a, b = fp.poison_bits(dtype, 0), fp.poison_bits(dtype, 1)
    assert a != b and a not in (0, (1 << 8 * torch.empty((), dtype=dtype).element_size()) - 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("zone", ["front", "back", "gap_first_row", "gap_last_row"])
def test_a_planted_write_is_caught_and_located_in_each_zone(dtype, zone):
    g = fp.Guarded((ROWS, COLS), dtype, "cpu", ld=LD, pattern=1)
    g.fill_from(torch.ones(ROWS, COLS))
    g.assert_guards_intact()
    e0 = (g.start - g.lo) // g.es                      # the payload's first element in the element view
    if zone == "front":
        g.elems[e0 - 1] = _value(dtype)                # the last element of the front guard
        expect = ("front guard", "element 1 before")
    elif zone == "back":
        g.elems[e0 + ROWS * LD] = _value(dtype)        # the first element of the back guard
        expect = ("back guard", "element 0 after")
    elif zone == "gap_first_row":
        g.flat[0, COLS] = _value(dtype)
        expect = ("row gap", "row 0, column %d" % COLS)
    else:
        g.flat[ROWS - 1, LD - 1] = _value(dtype)
        expect = ("row gap", "row %d, column %d" % (ROWS - 1, LD - 1))
    with pytest.raises(AssertionError) as ei:
        g.assert_guards_intact("C")
    msg = str(ei.value)
    assert expect[0] in msg and expect[1] in msg and msg.startswith("C:"), msg
    g.rearm(0)
    g.assert_guards_intact()                           # re-poisoned: clean again, under the other pattern
    assert g.pattern == 0


def test_a_masked_out_element_counts_as_gap():
    mask = torch.ones(ROWS, COLS, dtype=torch.bool)
    mask[2, 4:8] = False                               # e.g. the gap between two planes, a row a contract leaves alone
    g = fp.Guarded((ROWS, COLS), torch.bfloat16, "cpu", ld=LD, mask=mask)
    g.fill_from(torch.ones(ROWS, COLS))
    g.assert_guards_intact()
    assert g.payload().numel() == ROWS * COLS - 4
    g.view[2, 5] = 1.0
    with pytest.raises(AssertionError, match="masked-out element.*row 2, column 5"):
        g.assert_guards_intact()


def _fake_kernel(dtype, bug=None):
    """run(pattern) of a fake launch: out = a + 1 elementwise, through guarded buffers (a with a row gap)."""
    src = (torch.arange(ROWS * COLS).reshape(ROWS, COLS) % 7).to(dtype)

    def run(pattern):
        a = fp.Guarded((ROWS, COLS), dtype, "cpu", ld=LD, pattern=pattern).fill_from(src)
        out = fp.Guarded((ROWS, COLS), dtype, "cpu", ld=LD, pattern=pattern)
        res = a.view + torch.ones((), dtype=dtype)
        if bug == "gap":
            if dtype == torch.bfloat16:                            # reads the operand's row gap: poison leaks in
                # (fp32 add, then the truncating fp32 -> bf16 cast many kernels use: the NaN keeps its payload; a cast that
                # canonicalises NaNs gives the same NaN under both patterns -- that case is the reference comparison's)
                s = (res[1, 2].float() + a.flat[1, COLS + 1].float()).reshape(1)
                res[1, 2] = (s.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)[0]
            else:
                res[1, 2] = res[1, 2] + a.flat[1, COLS + 1]
        if bug == "nan":
            res[3, 3] = float("nan")                               # a NaN the kernel writes on purpose
        out.view.copy_(res)
        if bug == "unwritten":
            out.rearm(pattern)
            res[2, 5] = out.view[2, 5]
            out.view.copy_(res)                                    # everything but (2, 5) is stored
        out.assert_guards_intact()
        a.assert_guards_intact()
        return out.payload()
    return run


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fully_written_accepts_a_correct_kernel(dtype):
    got = fp.assert_fully_written(_fake_kernel(dtype))
    assert got["out"].shape == (ROWS, COLS)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_unwritten_payload_element_is_caught(dtype):
    with pytest.raises(AssertionError) as ei:
        fp.assert_fully_written(_fake_kernel(dtype, "unwritten"))
    assert "never written" in str(ei.value) and "(2, 5)" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_dependence_on_the_poison_is_caught(dtype):
    with pytest.raises(AssertionError) as ei:
        fp.assert_fully_written(_fake_kernel(dtype, "gap"))
    assert "(1, 2)" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
def test_a_canonical_nan_written_by_the_kernel_is_not_reported(dtype):
    got = fp.assert_fully_written(_fake_kernel(dtype, "nan"))
    assert bool(torch.isnan(got["out"][3, 3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_frozen_catches_a_one_bit_change(dtype):
    t = (torch.arange(24).reshape(4, 6) % 5).to(dtype)
    u = torch.ones(3, dtype=dtype)
    with fp.frozen(t, u):
        pass
    with pytest.raises(AssertionError, match=r"b was modified: element 0"):
        with fp.frozen(t, u, names=("a", "b")):
            i = fp.bits_of(u)
            i[0] ^= 1
            u.copy_(i.view(dtype))
    with pytest.raises(AssertionError, match=r"input 0 was modified.*\(2, 3\)"):
        with fp.frozen(t[:, :4]):                      # a strided view
            i = fp.bits_of(t)
            i[2, 3] ^= 1
            t.copy_(i.view(dtype))


# ---- accounting: every cdml_* declaration of the header is in exactly one of the three lists ----------------------------------------
def _header_names():
    h = open(os.path.join(ROOT, "include", "cdml.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return re.findall(r"\b(cdml_\w+)\s*\(", h)


def test_every_entry_point_is_accounted_for():
    names = _header_names()
    assert len(names) == len(set(names)) and len(names) > 100
    in_table = set(table.abi_names_in_table())
    no_launch, not_yet = set(table.NO_LAUNCH), set(table.NOT_YET)
    assert len(table.NOT_YET) == len(not_yet), "a name twice in NOT_YET"
    for a, b, what in ((in_table, no_launch, "the table and NO_LAUNCH"), (in_table, not_yet, "the table and NOT_YET"),
                       (no_launch, not_yet, "NO_LAUNCH and NOT_YET")):
        assert not (a & b), "in both %s: %s" % (what, sorted(a & b))
    listed = in_table | no_launch | not_yet
    missing = sorted(set(names) - listed)
    assert not missing, "declared in include/cdml.h without a footprint entry, NO_LAUNCH or NOT_YET: %s" % missing
    stale = sorted(listed - set(names))
    assert not stale, "listed but not declared in include/cdml.h: %s" % stale
    assert all(isinstance(r, str) and r for r in table.NO_LAUNCH.values()), "every NO_LAUNCH name carries its reason"


def test_no_required_launch_is_postponed():
    in_table = set(table.abi_names_in_table())
    assert not (set(table.REQUIRED) & set(table.NOT_YET)), sorted(set(table.REQUIRED) & set(table.NOT_YET))
    assert not (set(table.REQUIRED) - in_table), sorted(set(table.REQUIRED) - in_table)
    ids = [e["id"] for e in table.ENTRIES]
    assert len(ids) == len(set(ids))
    assert not (set(table.REQUIRED_ENTRY_IDS) - set(ids)), sorted(set(table.REQUIRED_ENTRY_IDS) - set(ids))
    for e in table.ENTRIES:
        assert e["abi"] and e["operands"] and e["ref"] and e["tol"], e["id"]
    assert set(table.OPERANDS) == set(ids), "one structured operand list per entry"
    for k, ops_ in table.OPERANDS.items():
        assert ops_ and all(r in ("in", "out", "inout", "ws") for _, r in ops_), k
        assert any(r in ("out", "inout") for _, r in ops_), "%s writes nothing?" % k


def test_every_table_entry_has_its_launch_code():
    """the table is data, the launches live in tests/test_gpu_footprint.py: importing it touches no GPU"""
    import test_gpu_footprint as launches
    ids = {e["id"] for e in table.ENTRIES}
    assert set(launches.LAUNCH) == ids, (sorted(ids - set(launches.LAUNCH)), sorted(set(launches.LAUNCH) - ids))
