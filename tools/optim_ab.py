#!/usr/bin/env python3
"""Time the LARS entry points of csrc/optim.hip under two builds of the library, at the production layer shapes (segments
1536 x 5120, 5120, 5120 x 256, 256): cdml_lars_multi, and the cdml_lars_multi_norms + 2 x cdml_lars_matrix(_h2) chain
with one bf16 copy, three bf16 planes and two fp16 planes.  The acceptance test of a source-only change after which
tools/isa_ab.py finds the kernels behind these entries (k_lars_multi_apply, k_rule_matrix<*, 1>) not identical.

    python tools/optim_ab.py --a PARENT/libcdml_hip.so --b collaborative-deep-metric-learning_amd/lib/libcdml_hip.so

Each measurement is a fresh child process (this file with --child) that loads ONE library through CDML_LIB_PATH -- the C
ABI is the same, so this tree's ops.py drives both -- warms up, and brackets --launches calls of every case with device
events.  The parent process never opens the GPU; it alternates A and B for --rounds rounds and prints per case A's median,
B's median and A's spread (max - min over its rounds), in microseconds per call.  Exit status 1 if some B median exceeds
A's median by more than A's spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1536, 5120), (5120, 256))


def child(launches, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from cdml_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    (F, H), (_, D) = SHAPES
    segs, o = [], 0
    for n in (F * H, H, H * D, D):
        segs.append((o, n))
        o += n
    w = torch.randn(o, device=dev) * 0.05
    g = torch.randn(o, device=dev) * 1e-3
    acc = torch.zeros(o, device=dev)
    scratch = torch.zeros(max(ops.lars_scratch_floats(), ops.lars_multi_scratch_floats()), device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    tick = ops.new_tickets(dev)

    def matrix(planes, dtype=torch.bfloat16, **kw):
        W1T = torch.zeros(H, planes * F, dtype=dtype, device=dev)
        W2T = torch.zeros(D, planes * H, dtype=dtype, device=dev)
        W2 = torch.zeros(H, planes * D, dtype=dtype, device=dev)
        pt1, pt2, pc2 = (F, H, D) if planes > 1 else (0, 0, 0)

        def run():
            ops.lars_multi_norms(w, g, segs, scratch)
            ops.lars_matrix(w, g, acc, segs, 0, 1, F, H, 1e-3, scratch, wt=W1T, plane_t=pt1, **kw)
            ops.lars_matrix(w, g, acc, segs, 2, 3, H, D, 1e-3, scratch, wt=W2T, wc=W2, plane_t=pt2, plane_c=pc2,
                            step_dev=step, tickets=tick, **kw)
        return run

    cases = {
        "lars_multi": lambda: ops.lars_multi(w, g, acc, segs, 1e-3, scratch, step_dev=step, tickets=tick),
        "lars_matrix bf16": matrix(1),
        "lars_matrix 3 planes": matrix(3),
        "lars_matrix_h2 2 planes": matrix(2, torch.float16, h2_scale=64.0),
    }
    out = {}
    for name, run in cases.items():
        for _ in range(warmup):
            run()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            run()
        t1.record()
        torch.cuda.synchronize()
        out[name] = t0.elapsed_time(t1) * 1e3 / launches
    print("OPTIM_AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", help="the parent's libcdml_hip.so")
    ap.add_argument("--b", help="this tree's libcdml_hip.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.launches, args.warmup)
    if not (args.a and args.b and args.rounds >= 5 and args.launches >= 200):
        ap.error("--a and --b, at least 5 rounds of at least 200 launches")
    times = {"a": [], "b": []}
    for r in range(args.rounds):
        for side in ("a", "b"):
            env = dict(os.environ, CDML_LIB_PATH=os.path.abspath(getattr(args, side)))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches),
                                "--warmup", str(args.warmup)], env=env, stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode:                                 # nothing more is started on the GPU after a failure
                print("round %d, side %s: the child ended with status %d" % (r, side, p.returncode))
                return 2
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("OPTIM_AB ")][-1]
            times[side].append(json.loads(line[len("OPTIM_AB "):]))
            print("round %d %s %s" % (r, side, line), flush=True)
    ok = True
    print("| entry points | parent median (us) | new median (us) | parent spread (us) |")
    print("|---|---|---|---|")
    for name in times["a"][0]:
        a, b = [t[name] for t in times["a"]], [t[name] for t in times["b"]]
        ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
        ok = ok and mb <= ma + spread
        print("| %s | %.2f | %.2f | %.2f |%s" % (name, ma, mb, spread, "" if mb <= ma + spread else "  <-- slower"))
    print("RESULT: %s" % ("no entry slower than the parent's median + spread" if ok else "SLOWER"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
