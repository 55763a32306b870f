#!/usr/bin/env python3
"""Step time of the N-pair loss with a cross-batch memory of M negatives, and its chain stage by stage.

Whole steps (CUDA events around `steps` eager steps after `warmup`, which also fill the ring): TrainStep(mode="npair",
memory_size=M) for M in `--memory` (multiples of B; 0 = the in-batch loss) on a 1 M x 1500 synthetic catalogue, H 5000,
D 256, Adam, precision f32x3.  Then, for M > 0, the loss chain of ops.npair_loss(memory=...) on the step's own embedded
rows, each stage timed alone (median of `reps`): the splits of A and of P into [P; Mem]'s operand images, S = A [P; Mem]^T,
the statistics, the W planes (in-batch block + memory block), dA = W [P; Mem], dP = W^T A and the ring push.
usage: python tools/npair_memory_bench.py [--batch 8192] [--memory 0,8192,32768] [--steps 20] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdml_amd import engine, ops, train  # noqa: E402
from npair_bench import event_ms, step_ms  # noqa: E402


def chain(ts, reps):
    """the memory chain on ts.ws.e, stage by stage (ms), with the bytes / flops that set each stage's floor"""
    B, L, w, m = ts.B, ts.layout, ts.npair_ws, ts.npair_memory
    Dq, K, M, e, idx, de = w.Dq, m.K, m.M, ts.ws.e, ts.idx, ts.ws.de
    A, P = e[0::2], e[1::2]
    t, sym = ts.temperature, ts.symmetric
    st = {}
    st["split"] = event_ms(lambda: (ops.split_f32_bf16x3(A, w.A3, Dq), ops.split_f32_bf16x3(P, m.PM3[:B], Dq),
                                    ops.split_f32_bf16x3(P, m.PMT3, K, transpose=True)), reps)
    st["S = A [P;Mem]^T"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, w.A3, Dq, m.PM3, Dq, m.S, B, K, Dq,
                                                                workspace=m.gemm_ws), reps)
    st["stats"] = event_ms(lambda: ops.npair_memory_stats(m.S, idx, B, B, m.ids, t, sym, w.lse, ts.stats, w.ws), reps)
    st["W planes"] = event_ms(lambda: (ops.npair_grad_x3(m.S, idx, B, t, sym, w.lse, m.W3, K),
                                       ops.npair_memory_grad_x3(m.S, idx, B, B, m.ids, t, sym, w.lse, m.W3, K)), reps)
    st["dA = W [P;Mem]"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, m.W3, K, m.PMT3, K, de[0::2], B, Dq, K,
                                                               workspace=m.gemm_ws), reps)
    st["dP = W^T A"] = event_ms(lambda: ops.gemm_bf16x3_tn(m.W3, K, w.A3, Dq, de[1::2], B, Dq, B, workspace=m.gemm_ws), reps)
    # (the push at the step number the ring already holds: it rewrites slots with the same values' successors)
    st["push"] = event_ms(lambda: ops.npair_memory_push(P, idx, B, L.Dp, 0, ts.step_dev, m.start, m.rows, m.ids,
                                                        R3=m.PM3[B:], plane_r=Dq, T3=m.PMT3[:, B:], plane_t=K), reps)
    state = m.state_dict()
    st["whole chain"] = event_ms(lambda: ops.npair_loss(e, idx, B, L.Dp, t, sym, "f32x3", de=de, stats=ts.stats, ws=w,
                                                        memory=m, step=0, step_dev=ts.step_dev), reps)
    m.load(state["rows"], state["ids"])
    flop = 2.0 * B * K * Dq
    info = {"S_bytes_MB": B * K * 4 / 1e6, "W_planes_bytes_MB": B * K * 6 / 1e6,
            "S TFLOP/s (fp32 equiv)": round(flop / (st["S = A [P;Mem]^T"] * 1e-3) / 1e12, 1),
            "dA TFLOP/s (fp32 equiv)": round(flop / (st["dA = W [P;Mem]"] * 1e-3) / 1e12, 1),
            "stats GB/s (S read, + the in-batch block symmetric)": round(
                (B * K + (B * B if sym else 0)) * 4 / (st["stats"] * 1e-3) / 1e9, 1),
            "W GB/s (S read + planes written)": round(B * K * 10 / (st["W planes"] * 1e-3) / 1e9, 1),
            "ring_fill": float((m.ids >= 0).float().mean().item()), "M": M}
    return {k: round(v, 4) for k, v in st.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--memory", default="0,8192,32768")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, D, B = 1500, 5000, 256, args.batch
    table = engine.FeatureTable.synthetic(args.rows, F, seed=0, device=dev)
    rng = np.random.default_rng(0)
    p = rng.integers(0, args.rows, size=(4 * args.rows, 2))
    pairs = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    res = {"rows": args.rows, "F": F, "H": H, "D": D, "B": B, "precision": "f32x3", "optimizer": "adam", "steps": args.steps}
    for M in (int(x) for x in args.memory.split(",")):
        ts = train.TrainStep(table, pairs, B, output_size=D, hidden_size=H, mode="npair", optimizer="adam",
                             base_learning_rate=0.01, device=dev, precision="f32x3", memory_size=M)
        r = {"ms_per_step": round(step_ms(ts, args.steps, args.warmup), 4), "loss": round(ts.loss(), 6)}
        if M:
            r["chain_ms"], r["chain_info"] = chain(ts, args.reps)
        res["M=%d" % M] = r
        print(json.dumps({"B": B, "M": M, **r}), flush=True)
        del ts
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
