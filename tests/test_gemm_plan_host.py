"""The K-split plan of the plane GEMMs (csrc/gemm_plan.h) on the CPU: tests/host/gemm_plan_table.cpp -- a host program
that includes only that header -- asserts the plan's properties row by row and prints the table; the table is the committed
tests/data/gemm_plan_table.txt (generated from the arithmetic of the commit before the plan was gathered in the header), and
its workspace column is what the built library's workspace queries answer.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "gemm_plan_table.txt")


def host_compiler():
    """ROCm's clang as a plain C++ compiler, else the system's"""
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("c++"),
              shutil.which("g++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_table")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "gemm_plan_table.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr                      # (a plan property that fails names its row)
    return r.stdout


def test_the_plan_table_is_the_committed_one(table):
    want = open(TABLE).read()
    assert len(want.splitlines()) == 1764                   # 252 shapes x (nt 3 / 6, nt_f16, tn 3 / 6, tn_f16, bf16_tn)
    assert table == want


def test_the_workspace_column_is_what_the_library_answers(table):
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    query = {"nt": lambda M, N, K, p: lib.cdml_gemm_bf16x3_workspace(0, M, N, K, p),
             "tn": lambda M, N, K, p: lib.cdml_gemm_bf16x3_workspace(1, M, N, K, p),
             "nt_f16": lambda M, N, K, p: lib.cdml_gemm_f16x2_workspace(0, M, N, K),
             "tn_f16": lambda M, N, K, p: lib.cdml_gemm_f16x2_workspace(1, M, N, K),
             "bf16_tn": lambda M, N, K, p: lib.cdml_gemm_bf16_tn_workspace(M, N, K)}
    seen = set()
    for ln in table.splitlines():
        f = ln.split()
        M, N, K, products = (int(v) for v in f[1:5])
        assert query[f[0]](M, N, K, products) == int(f[-1]), ln
        seen.add(f[0])
    assert seen == set(query)


def test_the_plan_header_enters_the_build_id(tmp_path):
    """a library built before an edit of csrc/gemm_plan.h must not pass for current: the header is one of the hashed sources"""
    from cdml_amd import _lib
    csrc = tmp_path / "csrc"
    shutil.copytree(os.path.join(ROOT, "collaborative-deep-metric-learning_amd", "csrc"), csrc)
    before = _lib.source_id(str(csrc))
    assert before == _lib.source_id()
    with open(csrc / "gemm_plan.h", "a") as f:
        f.write("\n// edited\n")
    assert _lib.source_id(str(csrc)) != before
