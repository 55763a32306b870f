#!/usr/bin/env python3
"""Bit-equality A/B of the N-pair family's launches between two builds of the library (a refactor's acceptance test).

--dump OUT.npz   (GPU) calls every cdml_npair_* entry once per case on fixed, seeded inputs and saves every output buffer:
                 lse, stats, the statistics workspace (row partials, column chunks, closs), colpart, lse_col, W in each
                 format, the ring's rows / ids / slot images, the operand images, de of the positive fold.  The library is
                 the tree's, or the one CDML_LIB_PATH names (tools/experiments/mk_variant.py builds variants).
--compare A B    (CPU) asserts that the two dumps hold the same arrays, bit for bit.

The inputs: S = randint(-64, 64) / 64 (exactly representable), video ids drawn from range(64) so the validity masks bite
in every row, plus ids = None; both values of `symmetric`, the logQ bias on and off, t = 0.1.  The shapes are the smallest
that reach every path: in-batch B = 518 at lds = 520 (three column chunks, the last of 6 rows; a W tail of 2; row-loop
lanes with 2 and 3 columns), memory M = 1032 at mem_col = 520, the ring push B = 172, M = 516, D = 68 at steps start - 1,
start and start + 3, mixed B = 516 with 4-wide gaps before the uniform and the memory block (and M = 0), data-parallel
B = 260 of G = 1040 at col0 0 and 780 with the two folds over world = 4.  Every output starts from a fixed fill, so what a
launch leaves untouched is compared too.
usage: python tools/npair_ab.py --dump OUT.npz | --compare A.npz B.npz"""
import argparse
import os
import sys

import numpy as np

T = 0.1
FILL = -7.0


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "the dumps hold different arrays: %s" % sorted(set(A.files) ^ set(B.files))
    bad = []
    for k in sorted(A.files):
        x, y = A[k], B[k]
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad.append(k)
    print("%d arrays, %d differ" % (len(A.files), len(bad)))
    assert not bad, "not bit-identical: %s" % bad[:20]


def dump(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cdml_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261018)
    out = {}

    def keep(name, t):
        t = t.detach().cpu().contiguous()
        out[name] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()

    def scores(rows, cols, ld):
        s = np.zeros((rows, ld), np.float32)
        s[:, :cols] = rng.integers(-64, 64, (rows, cols)) / 64.0
        return torch.from_numpy(s).to(dev)

    ints = lambda n, lo=0: torch.from_numpy(rng.integers(lo, 64, n).astype(np.int32)).to(dev)
    lq = lambda n: torch.from_numpy((-rng.integers(1, 64, n) / 8.0).astype(np.float32)).to(dev)
    f32 = lambda *s: torch.full(s, FILL, dtype=torch.float32, device=dev)
    bf = lambda *s: torch.full(s, FILL, dtype=torch.bfloat16, device=dev)
    zws = lambda nbytes: torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
    cases = [(i, s, b) for i in (1, 0) for s in (1, 0) for b in (0, 1)]

    # ---- in-batch and memory chains: statistics, W in the three formats (in-batch block, then the memory block) ----
    B, lds, M, mc = 518, 520, 1032, 520
    S, Sm = scores(B, B, lds), scores(B, mc + M, mc + M)
    ids, mid, bias, mbias = ints(2 * B), ints(M, lo=-8), lq(2 * B), lq(M)
    for i, sym, b in cases:
        rows, bi, mb, tag = (ids if i else None), (bias if b else None), (mbias if b else None), "ids%d_sym%d_bias%d" % (i, sym, b)
        lse, st, ws = f32(2 * B), f32(4), zws(ops.npair_workspace(B))
        if b:
            ops.npair_logq_stats(S, rows, B, bi, T, sym, lse, st, ws)
        else:
            ops.npair_stats(S, rows, B, T, sym, lse, st, ws)
        W3, Wf, W16 = bf(B, 3 * lds), f32(B, lds), bf(B, lds)
        if b:
            ops.npair_logq_grad_x3(S, rows, B, bi, T, sym, lse, W3, lds)
            ops.npair_logq_grad_f32(S, rows, B, bi, T, sym, lse, Wf)
        else:
            ops.npair_grad_x3(S, rows, B, T, sym, lse, W3, lds)
            ops.npair_grad_f32(S, rows, B, T, sym, lse, Wf)
        ops.npair_grad_bf16(S, rows, B, T, sym, lse, W16, bias=bi)
        for n, t in (("lse", lse), ("stats", st), ("ws", ws), ("W3", W3), ("Wf", Wf), ("W16", W16)):
            keep("inbatch/%s/%s" % (tag, n), t)
        K = mc + M
        lse, st, ws = f32(2 * B), f32(4), zws(ops.npair_memory_workspace(B, M))
        if b:
            ops.npair_memory_logq_stats(Sm, rows, B, bi, mc, mid, mb, T, sym, lse, st, ws)
        else:
            ops.npair_memory_stats(Sm, rows, B, mc, mid, T, sym, lse, st, ws)
        W3, Wf, W16 = bf(B, 3 * K), f32(B, K), bf(B, K)
        if b:
            ops.npair_logq_grad_x3(Sm, rows, B, bi, T, sym, lse, W3, K)
            ops.npair_memory_logq_grad_x3(Sm, rows, B, mc, mid, mb, T, sym, lse, W3, K)
            ops.npair_logq_grad_f32(Sm, rows, B, bi, T, sym, lse, Wf)
            ops.npair_memory_logq_grad_f32(Sm, rows, B, mc, mid, mb, T, sym, lse, Wf)
        else:
            ops.npair_grad_x3(Sm, rows, B, T, sym, lse, W3, K)
            ops.npair_memory_grad_x3(Sm, rows, B, mc, mid, T, sym, lse, W3, K)
            ops.npair_grad_f32(Sm, rows, B, T, sym, lse, Wf)
            ops.npair_memory_grad_f32(Sm, rows, B, mc, mid, T, sym, lse, Wf)
        ops.npair_grad_bf16(Sm, rows, B, T, sym, lse, W16, bias=bi)
        ops.npair_memory_grad_bf16(Sm, rows, B, mc, mid, T, sym, lse, W16, mem_bias=mb)
        for n, t in (("lse", lse), ("stats", st), ("ws", ws), ("W3", W3), ("Wf", Wf), ("W16", W16)):
            keep("memory/%s/%s" % (tag, n), t)

    # ---- the ring push (no write, first slots, wrapped slots; no images, three-plane images, one-plane images) and the
    # operand images of precision bf16 ----
    B, M, D, start = 172, 516, 68, 5
    P = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(dev)
    ids = ints(2 * B)
    for step in (start - 1, start, start + 3):
        for dev_step in (0, 1):
            sd = torch.tensor([step - 1], dtype=torch.int64, device=dev) if dev_step else None
            s0, tag = (1 if dev_step else step), "step%d_dev%d" % (step, dev_step)
            mem, mi = f32(M, D), torch.full((M,), -1, dtype=torch.int32, device=dev)
            ops.npair_memory_push(P, ids, B, D, s0, sd, start, mem, mi)
            keep("push/%s/plain/mem" % tag, mem), keep("push/%s/plain/ids" % tag, mi)
            mem, mi, R3, T3 = f32(M, D), torch.full((M,), -1, dtype=torch.int32, device=dev), bf(M, 3 * D), bf(D, 3 * M)
            ops.npair_memory_push(P, ids, B, D, s0, sd, start, mem, mi, R3=R3, plane_r=D, T3=T3, plane_t=M)
            for n, t in (("mem", mem), ("ids", mi), ("R3", R3), ("T3", T3)):
                keep("push/%s/x3/%s" % (tag, n), t)
            mem, mi, R, Tt = f32(M, D), torch.full((M,), -1, dtype=torch.int32, device=dev), bf(M, D), bf(D, M)
            ops.npair_memory_push_bf16(P, ids, B, D, s0, sd, start, mem, mi, R, Tt)
            for n, t in (("mem", mem), ("ids", mi), ("R", R), ("T", Tt)):
                keep("push/%s/bf16/%s" % (tag, n), t)
    e = torch.from_numpy(rng.standard_normal((2 * B, D)).astype(np.float32)).to(dev)
    A16, P16, PT16 = bf(B, 72), bf(B, 72), bf(D, 176)
    ops.npair_operands_bf16(e, B, D, A16, P16, PT16)
    keep("operands/A", A16), keep("operands/P", P16), keep("operands/PT", PT16)

    # ---- mixed negatives: gaps of 4 columns before the uniform and the memory block; M = 0; the plane split ----
    B, nc, mc, M, D = 516, 520, 1040, 1032, 68
    ids3, mid, bias, mbias = ints(3 * B), ints(M, lo=-8), lq(2 * B), lq(M)
    for Mx in (M, 0):
        span = mc + M if Mx else nc + B
        S = scores(B, span, span)
        for i, sym, b in cases:
            rows, bi, tag = (ids3 if i else None), (bias if b else None), "M%d_ids%d_sym%d_bias%d" % (Mx, i, sym, b)
            mi, mb = (mid if Mx else None), (mbias if Mx and b else None)
            lse, st, ws = f32(2 * B), f32(4), zws(ops.npair_mixed_workspace(B, Mx))
            a = (S, rows, B, nc, mc if Mx else 0, mi, bi, -3.0 if b else 0.0, mb, T, sym)
            ops.npair_mixed_stats(*a, lse, st, ws)
            W3, Wf = bf(B, 3 * span), f32(B, span)
            ops.npair_mixed_grad_x3(*a, lse, W3, span)
            ops.npair_mixed_grad_f32(*a, lse, Wf)
            for n, t in (("lse", lse), ("stats", st), ("ws", ws), ("W3", W3), ("Wf", Wf)):
                keep("mixed/%s/%s" % (tag, n), t)
    e3 = torch.from_numpy(rng.standard_normal((3 * B, D)).astype(np.float32)).to(dev)
    A3, R3, T3 = bf(B, 3 * D), bf(nc + B, 3 * D), bf(D, 3 * (nc + B))
    ops.npair_mixed_split_x3(e3, B, D, A3, D, R3, D, T3, nc + B, nc)
    keep("mixed/split/A3", A3), keep("mixed/split/R3", R3), keep("mixed/split/T3", T3)

    # ---- data-parallel: four ranks' local statistics, the column fold over them, then ranks 0 and 3 ----
    B, G, world, D = 260, 1040, 4, 68
    ids_all = ints(2 * G)
    Sr = [scores(B, G, G) for _ in range(world)]
    for i, sym in ((1, 1), (1, 0), (0, 1), (0, 0)):
        rows, tag = (ids_all if i else None), "ids%d_sym%d" % (i, sym)
        cp_all, lse_row, wss = f32(world, G, 2), [f32(B) for _ in range(world)], []
        for r in range(world):
            wss.append(zws(ops.npair_dp_workspace(B, G)))
            ops.npair_dp_local_stats(Sr[r], rows, B, G, r * B, T, sym, lse_row[r], cp_all[r], wss[r])
            keep("dp/%s/rank%d/lse_row" % (tag, r), lse_row[r]), keep("dp/%s/rank%d/ws" % (tag, r), wss[r])
        lse_col = f32(G)
        if sym:
            ops.npair_dp_col_fold(cp_all, lse_col)
        keep("dp/%s/colpart" % tag, cp_all), keep("dp/%s/lse_col" % tag, lse_col)
        for r in (0, 3):
            st, W3, Wf = f32(4), bf(B, 3 * G), f32(B, G)
            ops.npair_dp_stats(Sr[r], B, G, r * B, T, sym, lse_col, st, wss[r])
            ops.npair_dp_grad_x3(Sr[r], rows, B, G, r * B, T, sym, lse_row[r], lse_col, W3, G)
            ops.npair_dp_grad_f32(Sr[r], rows, B, G, r * B, T, sym, lse_row[r], lse_col, Wf)
            for n, t in (("stats", st), ("W3", W3), ("Wf", Wf)):
                keep("dp/%s/rank%d/%s" % (tag, r, n), t)
    recv = torch.from_numpy(rng.standard_normal((world, B, D)).astype(np.float32)).to(dev)
    de = f32(2 * B, D)
    ops.npair_dp_pos_fold(recv, B, D, de)
    keep("dp/pos_fold/de", de)

    torch.cuda.synchronize()
    np.savez(path, **out)
    print("dumped %d arrays to %s (library: %s)" % (len(out), path, os.environ.get("CDML_LIB_PATH") or "the tree's"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="OUT.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    elif args.dump:
        dump(args.dump)
    else:
        ap.error("--dump OUT.npz or --compare A.npz B.npz")


if __name__ == "__main__":
    main()
