#!/usr/bin/env python3
"""Proof that a source-only change of the tile GEMM kernels is only a change of the source: compile csrc/gemm_bf16_256.hip
and csrc/gemm_f16x2_256.hip of two trees to gfx950 assembly with build()'s flags and compare the kernels' machine code.

    python tools/isa_ab.py                 # the parent commit (a temporary git worktree of HEAD~) against the working tree
    python tools/isa_ab.py --rev HEAD      # the last commit against uncommitted edits
    python tools/isa_ab.py --a DIR --b DIR # two checked-out trees
    python tools/isa_ab.py --sources gemm_bf16x3.hip gemm_bf16.hip   # other translation units of csrc/
    python tools/isa_ab.py --names ...     # ... and the two trees' kernels must carry the same demangled names

A kernel is its instructions plus its .amdhsa_kernel descriptor block (registers, LDS, scratch).  What may differ without
the code differing is canonicalised: the kernel's own mangled name, the __hip_cuid_* symbol, comments, and the function
number inside .LBB<n>_<m> / .Lfunc_end<n> labels.  The two trees are compared as MULTISETS of kernel bodies -- a refactor
may rename template arguments, so names are reported and not matched -- unless --names asks for it: a benchmark or a
profile that finds its kernels by name then needs the two trees' multisets of demangled names (llvm-cxxfilt) equal as well.
For a kernel that DIFFERS the report adds the descriptor lines that differ and the difference of the two kernels' counts of
v_ / ds_ / global_ / buffer_ opcodes: what a change that is accepted on measurements has to show.
Host tool: no GPU.  Exit status 0 = every kernel identical and the counts equal (and, with --names, the names)."""
import argparse
import collections
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "collaborative-deep-metric-learning_amd"
SOURCES = ("gemm_bf16_256.hip", "gemm_f16x2_256.hip")

Kernel = collections.namedtuple("Kernel", "name body n_instr")


def canonical(lines, name):
    """The lines of one kernel with everything that may legitimately differ taken out."""
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].replace(name, "@KERNEL")
        ln = re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln)
        ln = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI)\d+", r".\1", ln)
        ln = " ".join(ln.split())
        if ln:
            out.append(ln)
    return out


def kernels(asm):
    """Cut a device assembly file into kernels: from the kernel's label to the end of its descriptor block."""
    lines = asm.splitlines()
    found = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        start = max(j for j in range(i) if lines[j].split(";", 1)[0].strip() == name + ":")
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        body = canonical(lines[start:end + 1], name)
        code = body[:body.index(".amdhsa_kernel @KERNEL")]
        n_instr = sum(1 for c in code if not c.startswith(".") and not c.endswith(":"))
        found.append(Kernel(name, "\n".join(body), n_instr))
    return found


def split_body(k):
    """(instruction lines, descriptor lines) of a Kernel"""
    body = k.body.split("\n")
    cut = body.index(".amdhsa_kernel @KERNEL")
    return [c for c in body[:cut] if not c.startswith(".") and not c.endswith(":")], body[cut + 1:-1]


def differences(a, b):
    """Report lines on two kernels whose bodies differ: the descriptor lines that differ, and the difference of their counts
    of vector, LDS and memory opcodes (scalar code and branches left out: address arithmetic moves freely between the two)."""
    (ca, da), (cb, db) = split_body(a), split_body(b)
    fa, fb = (dict(ln.split(None, 1) for ln in d if " " in ln) for d in (da, db))
    out = ["    descriptor: %s %s -> %s" % (key, fa.get(key, "(none)"), fb.get(key, "(none)"))
           for key in sorted(set(fa) | set(fb)) if fa.get(key) != fb.get(key)] or ["    descriptor: the same"]
    na, nb = (collections.Counter(c.split()[0] for c in code if c.startswith(("v_", "ds_", "global_", "buffer_"))) for code in (ca, cb))
    out += ["    opcodes: " + (", ".join("%s %d -> %d" % (op, na[op], nb[op]) for op in sorted(set(na) | set(nb)) if na[op] != nb[op])
                               or "the same counts of v_ / ds_ / global_ / buffer_ opcodes")]
    return out


def compare(a, b):
    """(report lines, ok) for two lists of Kernel compared as multisets of bodies."""
    rest = collections.defaultdict(list)
    for k in b:
        rest[k.body].append(k)
    report, ok = [], len(a) == len(b)
    unmatched = []
    for k in a:
        if rest[k.body]:
            o = rest[k.body].pop(0)
            report.append("identical  %6d instr  %s  ==  %s" % (k.n_instr, k.name, o.name))
        else:
            unmatched.append(k)
    left = [o for ks in rest.values() for o in ks]
    for k in unmatched:                                    # pair the leftovers for the report by the likeness of their names
        o = max(left, key=lambda x: difflib.SequenceMatcher(None, k.name, x.name).ratio(), default=None)
        if o is not None:
            left.remove(o)
        report.append("DIFFERS    %6d instr  %s  !=  %s" % (k.n_instr, k.name, "%s (%d instr)" % (o.name, o.n_instr) if o else "(missing)"))
        if o is not None:                                  # (further lines of the same report entry)
            report[-1] += "".join("\n  " + ln for ln in differences(k, o))
        ok = False
    for o in left:
        report.append("DIFFERS    %6d instr  (missing)  !=  %s" % (o.n_instr, o.name))
        ok = False
    if len(a) != len(b):
        report.append("kernel counts differ: %d against %d" % (len(a), len(b)))
    return report, ok


def demangled(names):
    """The demangled form of each mangled kernel name, by ROCm's llvm-cxxfilt, else the system's c++filt (a name the
    demangler does not know stays mangled -- which compares just as well)."""
    import shutil
    filt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        raise RuntimeError("--names needs llvm-cxxfilt or c++filt")
    r = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(names)
    return out


def compare_names(a, b):
    """(report lines, ok) for two lists of demangled names compared as multisets."""
    ca, cb = collections.Counter(a), collections.Counter(b)
    report = ["NAME only in A (x%d): %s" % (n, k) for k, n in sorted((ca - cb).items())]
    report += ["NAME only in B (x%d): %s" % (n, k) for k, n in sorted((cb - ca).items())]
    return report or ["names: the same %d demangled kernel names" % len(a)], ca == cb


def build_flags():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    return list(__graft_entry__.HIPCC_FLAGS)


def assemble(tree, src, flags, out):
    csrc = os.path.join(tree, PKG, "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-I" + csrc, "--cuda-device-only", "-S", "-o", out, src]
    r = subprocess.run(cmd, cwd=csrc, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write("\n".join(ln for ln in r.stderr.splitlines() if "error" in ln)[-4000:] + "\n")
        raise RuntimeError("hipcc failed: " + " ".join(cmd))
    return open(out).read()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", default="HEAD~", help="revision checked out as tree A when --a is not given")
    ap.add_argument("--a", help="tree A (a checkout of the repository)")
    ap.add_argument("--b", default=ROOT, help="tree B (default: the working tree)")
    ap.add_argument("--sources", nargs="+", default=list(SOURCES), metavar="FILE.hip",
                    help="the translation units of csrc/ to compare (default: the two of the tile GEMM)")
    ap.add_argument("--names", action="store_true", help="also require the same multiset of demangled kernel names")
    args = ap.parse_args()
    sources = tuple(args.sources)
    flags = build_flags()
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        a = args.a
        if a is None:
            a = os.path.join(tmp, "a")
            subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", "--force", a, args.rev], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        try:
            jobs = [(side, tree, src) for src in sources for side, tree in (("a", a), ("b", args.b))]
            with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
                asm = dict(zip([(j[0], j[2]) for j in jobs],
                               ex.map(lambda j: assemble(j[1], j[2], flags, os.path.join(tmp, j[0] + "_" + j[2] + ".s")), jobs)))
        finally:
            if args.a is None:
                subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", a], check=False)
    print("A = %s, B = %s; flags: %s" % (args.a or args.rev, os.path.relpath(args.b, ROOT) if args.b != ROOT else "working tree",
                                         " ".join(flags)))
    for src in sources:
        ka, kb = kernels(asm[("a", src)]), kernels(asm[("b", src)])
        report, same = compare(ka, kb)
        ok = ok and same
        print("%s: %d kernels against %d, %d instructions against %d, sha256 of the canonical bodies %s / %s" % (
            src, len(ka), len(kb), sum(k.n_instr for k in ka), sum(k.n_instr for k in kb),
            hashlib.sha256("\n".join(sorted(k.body for k in ka)).encode()).hexdigest()[:16],
            hashlib.sha256("\n".join(sorted(k.body for k in kb)).encode()).hexdigest()[:16]))
        if args.names:
            more, same = compare_names(demangled([k.name for k in ka]), demangled([k.name for k in kb]))
            report += more
            ok = ok and same
        for ln in report:
            print("  " + ln)
    print("RESULT: %s" % (("every kernel identical" + (", every name the same" if args.names else "")) if ok else "DIFFERENCES"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
