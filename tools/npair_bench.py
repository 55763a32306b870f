#!/usr/bin/env python3
"""Step time of the multi-class N-pair loss against the hinge steps, and the loss chain launch by launch.

Whole steps (CUDA events around `steps` eager steps after `warmup`): mode "npair" against "inbatch" and "semihard" on a
1 M x 1500 synthetic catalogue, H 5000, D 256, Adam, precision f32x3, at B = 4096 and 8192 pairs.  Then the chain of
ops.npair_loss on the step's own embedded rows, each launch timed alone (median of `reps`): the operand splits, the S
product, the row / column statistics, the W planes and the two gradient products.
usage: python tools/npair_bench.py [--steps 20] [--warmup 5] [--reps 10] [--batches 4096,8192] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdml_amd import engine, ops, train  # noqa: E402


def event_ms(fn, reps):
    """median milliseconds of fn() by CUDA events over reps launches"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def step_ms(ts, steps, warmup):
    for _ in range(warmup):
        ts.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        ts.step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def chain(ts, reps):
    """the loss chain on ts.ws.e, launch by launch (ms), with the bytes / flops that set each stage's floor"""
    B, L, w = ts.B, ts.layout, ts.npair_ws
    Dq, e, idx, de = w.Dq, ts.ws.e, ts.idx, ts.ws.de
    A, P = e[0::2], e[1::2]
    t, sym = ts.temperature, ts.symmetric
    st = {}
    st["split"] = event_ms(lambda: (ops.split_f32_bf16x3(A, w.A3, Dq), ops.split_f32_bf16x3(P, w.P3, Dq),
                                    ops.split_f32_bf16x3(P, w.PT3, B, transpose=True)), reps)
    st["S = A P^T"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, w.A3, Dq, w.P3, Dq, w.S, B, B, Dq, workspace=w.gemm_ws), reps)
    st["row/col stats"] = event_ms(lambda: ops.npair_stats(w.S, idx, B, t, sym, w.lse, ts.stats, w.ws), reps)
    st["W planes"] = event_ms(lambda: ops.npair_grad_x3(w.S, idx, B, t, sym, w.lse, w.W3, B), reps)
    st["dA = W P"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, w.W3, B, w.PT3, B, de[0::2], B, Dq, B, workspace=w.gemm_ws), reps)
    st["dP = W^T A"] = event_ms(lambda: ops.gemm_bf16x3_tn(w.W3, B, w.A3, Dq, de[1::2], B, Dq, B, workspace=w.gemm_ws), reps)
    st["whole chain"] = event_ms(lambda: ops.npair_loss(e, idx, B, L.Dp, t, sym, "f32x3", de=de, stats=ts.stats, ws=w), reps)
    gemm_flop = 2.0 * B * B * Dq                       # one fp32 product; six bf16 plane products on the MFMA
    info = {"S_bytes_MB": B * B * 4 / 1e6, "W_planes_bytes_MB": B * B * 6 / 1e6, "fp32_GFLOP_per_product": gemm_flop / 1e9}
    for k in ("S = A P^T", "dA = W P", "dP = W^T A"):
        info[k + " TFLOP/s (fp32 equiv)"] = round(gemm_flop / (st[k] * 1e-3) / 1e12, 1)
    info["stats GB/s (S read, +1 pass symmetric)"] = round(B * B * 4 * (2 if sym else 1) / (st["row/col stats"] * 1e-3) / 1e9, 1)
    info["W GB/s (S read + planes written)"] = round(B * B * 10 / (st["W planes"] * 1e-3) / 1e9, 1)
    return {k: round(v, 4) for k, v in st.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--batches", default="4096,8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, D = 1500, 5000, 256
    table = engine.FeatureTable.synthetic(args.rows, F, seed=0, device=dev)
    rng = np.random.default_rng(0)
    p = rng.integers(0, args.rows, size=(4 * args.rows, 2))
    pairs = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    res = {"rows": args.rows, "F": F, "H": H, "D": D, "precision": "f32x3", "optimizer": "adam", "steps": args.steps}
    for B in (int(b) for b in args.batches.split(",")):
        r = {}
        for mode in ("inbatch", "semihard", "npair"):
            ts = train.TrainStep(table, pairs, B, output_size=D, hidden_size=H, mode=mode, optimizer="adam",
                                 base_learning_rate=0.01, device=dev, precision="f32x3")
            r[mode + "_ms_per_step"] = round(step_ms(ts, args.steps, args.warmup), 4)
            r[mode + "_loss"] = round(ts.loss(), 6)
            if mode == "npair":
                r["npair_chain_ms"], r["npair_chain_info"] = chain(ts, args.reps)
            del ts
            torch.cuda.empty_cache()
        r["npair_minus_inbatch_ms"] = round(r["npair_ms_per_step"] - r["inbatch_ms_per_step"], 4)
        res["B=%d" % B] = r
        print(json.dumps({"B": B, **r}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
