#!/usr/bin/env python3
"""Time of the exact retrieval ranks (evaluate.py Evaluation.ranks: the plane GEMM with the rank count as its epilogue) at
the reference catalogue size -- 343 455 unit rows of 256 (faiss_knn.py:389) and 65 536 directed co-watch pairs -- beside
the kNN export (knn.knn_search, k = 51) on the same queries, which does strictly more work (a first block of score
blocks, the filter epilogue and the list merges).  One JSON line per precision.  The rank pass's rate counts
2 nq N Dp flops (fp32 products) and is given as a fraction of the bf16 MFMA peak / 6 (f32x3: six plane products per fp32
product) or / 3 (f16x2: three fp16 ones).
usage: python tools/rank_eval_bench.py [--reps R] [--precision f32x3,f16x2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdml_amd import knn, ops  # noqa: E402
from cdml_amd.evaluate import Evaluation  # noqa: E402

BF16_PEAK = 2.5e15          # MI355X dense bf16 / fp16 MFMA (spec)


def timed(fn, reps):
    fn()                                                     # warm-up: code objects, allocator
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), float(min(out)), float(max(out))


def time_count_launch(e, queries, prec, reps):
    """The rank-count launch alone (device events): all queries x the whole catalogue, operands prepared as ranks() does."""
    h2 = prec == "f16x2"
    n = e.shape[0]
    B = knn._device_matrix(e, e.device, 256, 128 if h2 else 64)
    Dp = B.shape[1]
    b_sq = torch.zeros(B.shape[0], dtype=torch.float32, device=e.device)
    ops.row_sqnorm(B[:n], Dp, b_sq)
    if h2:
        B3, s = knn._planes_h2(B, Dp)
    else:
        B3 = knn._planes(B, Dp)
    a, p = queries[:, 0], queries[:, 1]
    QA, q_sq = B3.index_select(0, a), b_sq.index_select(0, a)
    a32, p32 = a.to(torch.int32).contiguous(), p.to(torch.int32).contiguous()
    tau = torch.full((len(a),), 1.5, dtype=torch.float32, device=e.device)
    cnt = torch.zeros(len(a), dtype=torch.int32, device=e.device)

    def launch():
        if h2:
            ops.rank_count_h2(QA, Dp, B3, Dp, len(a), B3.shape[0], Dp, 1.0 / (s * s), q_sq, b_sq, tau, p32, a32, 0, n, cnt)
        else:
            ops.rank_count_x3(QA, Dp, B3, Dp, len(a), B3.shape[0], Dp, q_sq, b_sq, tau, p32, a32, 0, n, cnt)
    launch()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        launch()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=343455)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="f32x3,f16x2")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    e = torch.randn(args.n, args.dim, device=dev, generator=g)
    e = e / e.norm(dim=1, keepdim=True)
    cw = np.random.RandomState(1).randint(0, args.n, size=(args.pairs, 2))
    cw = cw[cw[:, 0] != cw[:, 1]]
    ev = Evaluation(None, [], device=dev)
    for prec in args.precision.split(","):
        queries, pos = ev.ranks(e, cw, symmetric=False, precision=prec)
        nq = int(queries.shape[0])
        Dp = knn._round_up(args.dim, 128 if prec == "f16x2" else 64)
        t_rank = timed(lambda: ev.ranks(e, cw, symmetric=False, precision=prec), args.reps)
        count_ms = time_count_launch(e, queries, prec, args.reps)
        qrows = e.index_select(0, queries[:, 0])
        t_knn = timed(lambda: knn.knn_search(e, qrows, 51, l2_norm=False, precision=prec), args.reps)
        flops = 2.0 * nq * args.n * Dp
        peak = BF16_PEAK / (3 if prec == "f16x2" else 6)
        print(json.dumps({"tool": "rank_eval_bench", "precision": prec, "catalogue": args.n, "dim": args.dim,
                          "queries": nq, "rank_ms": round(t_rank[0] * 1e3, 2),
                          "rank_ms_min_max": [round(t_rank[1] * 1e3, 2), round(t_rank[2] * 1e3, 2)],
                          "rank_fp32_tflops": round(flops / t_rank[0] / 1e12, 2),
                          "rank_frac_of_bf16_peak_over_%d" % (3 if prec == "f16x2" else 6): round(flops / t_rank[0] / peak, 3),
                          "count_launch_ms": round(count_ms, 2),
                          "count_launch_frac": round(flops / (count_ms * 1e-3) / peak, 3),
                          "knn51_ms": round(t_knn[0] * 1e3, 2),
                          "knn51_ms_min_max": [round(t_knn[1] * 1e3, 2), round(t_knn[2] * 1e3, 2)],
                          "mean_rank": float(pos.double().mean() + 1.0), "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
