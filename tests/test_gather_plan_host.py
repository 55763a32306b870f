"""The sampler + gather entry points' argument checks and launch plans (csrc/gather_plan.h) on the CPU:
tests/host/gather_plan_table.cpp -- a host program that includes only that header -- prints, for each of the eight fused
and three unfused entry points, the status and the full error text of every single-fault variation of a valid call and the
plan (rows per triplet, grid, NCH bucket, interleaved copy) of the valid ones; the table is the committed
tests/data/gather_plan_table.txt, generated from the library of the commit before the checks were gathered in the header
(its entry points called with placeholder pointers on a machine without a GPU -- every check returns before a HIP call --
and its launch arithmetic for the valid rows).  No GPU, and no call into the library here."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gemm_plan_host import host_compiler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "gather_plan_table.txt")
ENTRIES = ["sample_gather", "sample_gather_f16", "sample_gather_x3", "sample_gather_x3k", "sample_gather_h2",
           "sample_gather_listed", "sample_gather_listed_x3", "sample_gather_listed_f16",
           "gather_rows", "gather_rows_x3", "gather_rows_f16"]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_plan") / "gather_plan_table")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "gather_plan_table.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_the_plan_table_is_the_committed_one(table):
    want = open(TABLE).read()
    assert len(want.splitlines()) == 648
    assert table == want


def test_the_table_covers_every_entry_point_and_every_instantiation():
    """every entry point has valid and refused rows; the valid rows reach every NCH bucket of their format, with and
    without the interleaved copy, in every mode the format has (rows per triplet 3 and 2)"""
    rows = [ln.split('"') for ln in open(TABLE).read().splitlines()]
    head = [r[0].split() for r in rows]
    assert sorted({h[1] for h in head}) == sorted(ENTRIES)
    for e in ENTRIES:
        st = {int(h[3]) for h in head if h[1] == e}
        assert 0 in st and -1 in st and -3 in st and -4 in st, e
    seen, at_f = {}, {}
    for h, r in zip(head, rows):
        if int(h[3]) == 0:
            rpt, grid, nch, ki = (int(v) for v in r[2].split())
            assert 1 <= grid <= 2048
            seen.setdefault((h[0], h[1].startswith("sample_gather")), set()).add((nch, ki, rpt))
            m = re.search(r"_F(\d+)", h[2])
            if m:
                at_f.setdefault(h[1], {}).setdefault(int(m.group(1)), set()).add(nch)
    # both sides of every edge of the entry's own bucket list: the largest F a bucket holds, and one 16-B chunk more
    buckets = {"f32": ([2, 6, 8], [2, 4, 6, 8], 4), "x3": ([6, 8], [2, 4, 6, 8], 4), "h2": ([6, 8], None, 4), "f16": ([1, 3, 8], [1, 3, 8], 8)}
    for h in head:
        fused = h[1].startswith("sample_gather")
        b, per_chunk = buckets[h[0]][0 if fused else 1], buckets[h[0]][2]
        for lo, hi in zip(b, b[1:]):
            assert at_f[h[1]][64 * per_chunk * lo] == {lo} and at_f[h[1]][64 * per_chunk * lo + per_chunk] == {hi}, (h[1], lo, hi)
    nchs = lambda k: {c[0] for c in seen[k]}
    assert nchs(("f32", True)) == {2, 6, 8} and nchs(("x3", True)) == {6, 8} and nchs(("h2", True)) == {6, 8}
    assert nchs(("f16", True)) == {1, 3, 8}
    assert nchs(("f32", False)) == nchs(("x3", False)) == {2, 4, 6, 8} and nchs(("f16", False)) == {1, 3, 8}
    assert {(n, k) for n, k, _ in seen[("x3", True)]} == {(6, 0), (6, 1), (8, 0), (8, 1)}
    assert all({c[2] for c in seen[(f, True)]} == {2, 3} for f in ("f32", "x3", "h2", "f16"))


def test_the_plan_header_enters_the_build_id(tmp_path):
    """a library built before an edit of csrc/gather_plan.h (or of csrc/require.h, which it includes) must not pass for
    current: both are among the hashed sources"""
    from cdml_amd import _lib
    csrc = tmp_path / "csrc"
    shutil.copytree(os.path.join(ROOT, "collaborative-deep-metric-learning_amd", "csrc"), csrc)
    before = _lib.source_id(str(csrc))
    assert before == _lib.source_id()
    for name in ("gather_plan.h", "require.h"):
        with open(csrc / name, "a") as f:
            f.write("\n// edited\n")
        after = _lib.source_id(str(csrc))
        assert after != before
        before = after
