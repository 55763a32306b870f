#!/usr/bin/env python3
"""Step time of the N-pair loss on the config-4 precision (fp16 catalogue, bf16 MFMA) and its chain launch by launch.

Whole steps (CUDA events around `steps` eager steps after `warmup`; `rounds` rounds that alternate the configurations, the
median and the min .. max spread reported) on a 1 M x 1500 synthetic catalogue, H 5000, D 256, Adam:
  (a) the bf16 in-batch hinge step          TrainStep(mode="inbatch", precision="bf16") on the fp16 catalogue
  (b) the bf16 N-pair step                  TrainStep(mode="npair",   precision="bf16")
  (c) the f32x3 N-pair step                 the same on an fp32 catalogue
at B = 4096 and 8192 pairs, memory M = 0 and 4 B, logQ off and "stream".  Then the chain of ops.npair_loss on (b)'s own
embedded rows, each launch timed alone (median of `reps`): operands / S / stats / W / dA / dP / push, with the bytes that
set each stage's floor.
usage: python tools/npair_bf16_bench.py [--steps 20] [--warmup 5] [--rounds 3] [--reps 10] [--batches 4096,8192] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdml_amd import engine, engine_bf16, ops, train  # noqa: E402


def event_ms(fn, reps):
    """median milliseconds of fn() by CUDA events over reps launches (after two warm-up launches)"""
    fn(), fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def window_ms(ts, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        ts.step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def chain(ts, reps):
    """the bf16 loss chain on ts.ws.e, launch by launch (ms)"""
    B, L, w, m, q = ts.B, ts.layout, ts.npair_ws, ts.npair_memory, ts.npair_logq
    Dq, Dp, e, idx, de = w.Dq, L.Dp, ts.ws.e, ts.idx, ts.ws.de
    t, sym = ts.temperature, ts.symmetric
    if m is None:
        K, P16, PT16, S, W16, gws, M = B, w.P16, w.PT16, w.S, w.W16, w.gemm_ws, 0
    else:
        K, P16, PT16, S, W16, gws, M = m.K, m.PM16, m.PMT16, m.S, m.W16, m.gemm_ws, m.M
    bias = w.bias if q is not None else None
    mem_bias = m.bias if (q is not None and m is not None) else None
    oA = de[0::2] if w.dA is None else w.dA
    oP = de[1::2] if w.dP is None else w.dP
    st = {}
    if q is not None:
        st["logq gather"] = event_ms(lambda: q.gather(idx, B, None if m is None else m.ids, bias, mem_bias), reps)
    st["operands"] = event_ms(lambda: ops.npair_operands_bf16(e, B, Dp, w.A16, P16, PT16), reps)
    st["S = A [P; Mem]^T"] = event_ms(lambda: ops.gemm_bf16_nt(ops.BE_F32, w.A16, P16, S, B, K, Dq, workspace=gws), reps)

    def stats():
        if m is None and bias is None:
            ops.npair_stats(S, idx, B, t, sym, w.lse, ts.stats, w.ws)
        elif m is None:
            ops.npair_logq_stats(S, idx, B, bias, t, sym, w.lse, ts.stats, w.ws)
        elif bias is None:
            ops.npair_memory_stats(S, idx, B, B, m.ids, t, sym, w.lse, ts.stats, w.ws)
        else:
            ops.npair_memory_logq_stats(S, idx, B, bias, B, m.ids, mem_bias, t, sym, w.lse, ts.stats, w.ws)

    def wplane():
        ops.npair_grad_bf16(S, idx, B, t, sym, w.lse, W16, bias=bias)
        if m is not None:
            ops.npair_memory_grad_bf16(S, idx, B, B, m.ids, t, sym, w.lse, W16, mem_bias=mem_bias)
    st["stats"] = event_ms(stats, reps)
    st["W"] = event_ms(wplane, reps)
    st["dA = W [P; Mem]"] = event_ms(lambda: ops.gemm_bf16_nt(ops.BE_F32, W16, PT16, oA, B, Dq, K, workspace=gws), reps)
    st["dP = W^T A"] = event_ms(lambda: ops.gemm_bf16_tn(W16, w.A16, oP, B, Dq, B, workspace=gws), reps)
    if m is not None:
        # (timed into the slots the next step overwrites anyway: step counter as it stands)
        st["push"] = event_ms(lambda: ops.npair_memory_push_bf16(e[1::2, :Dp], idx, B, Dp, 0, ts.step_dev, m.start, m.rows, m.ids,
                                                                 m.PM16[B:], m.PMT16[:, B:]), reps)
    st["sum of stages"] = sum(st.values())
    info = {"K": K, "S_bytes_MB": B * K * 4 / 1e6, "W_bytes_MB": B * K * 2 / 1e6,
            "operand_bytes_MB": (2 * B * Dp * 4 + 3 * B * Dq * 2) / 1e6,
            "stats GB/s (S read, +1 in-batch pass symmetric)": round((B * K + (B * B if sym else 0)) * 4 / (st["stats"] * 1e-3) / 1e9, 1),
            "W GB/s (S read + W written)": round(B * K * 6 / (st["W"] * 1e-3) / 1e9, 1)}
    for k, flop in (("S = A [P; Mem]^T", 2.0 * B * K * Dq), ("dA = W [P; Mem]", 2.0 * B * K * Dq), ("dP = W^T A", 2.0 * B * B * Dq)):
        info[k + " TFLOP/s"] = round(flop / (st[k] * 1e-3) / 1e12, 1)
    return {k: round(v, 4) for k, v in st.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--batches", default="4096,8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, D = 1500, 5000, 256
    t16 = engine_bf16.FeatureTableF16.synthetic(args.rows, F, seed=0, device=dev)
    t32 = engine.FeatureTable.synthetic(args.rows, F, seed=0, device=dev)
    rng = np.random.default_rng(0)
    p = rng.integers(0, args.rows, size=(4 * args.rows, 2))
    pairs = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    res = {"rows": args.rows, "F": F, "H": H, "D": D, "optimizer": "adam", "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds}

    def make(table, mode, precision, **kw):
        return train.TrainStep(table, pairs, B, output_size=D, hidden_size=H, mode=mode, optimizer="adam",
                               base_learning_rate=0.01, device=dev, precision=precision, **kw)
    for B in (int(b) for b in args.batches.split(",")):
        for M in (0, 4 * B):
            for logq in (None, "stream"):
                kw = {}
                if M:
                    kw["memory_size"] = M
                if logq:
                    kw["logq"] = logq
                steps = {"a_bf16_inbatch": make(t16, "inbatch", "bf16"), "b_bf16_npair": make(t16, "npair", "bf16", **kw),
                         "c_f32x3_npair": make(t32, "npair", "f32x3", **kw)}
                for ts in steps.values():
                    for _ in range(args.warmup):
                        ts.step()
                times = {k: [] for k in steps}
                for _ in range(args.rounds):               # the configurations alternate: a drift of the machine hits all three
                    for k, ts in steps.items():
                        times[k].append(window_ms(ts, args.steps))
                r = {"B": B, "M": M, "logq": logq or "off"}
                for k, v in times.items():
                    r[k + "_ms"] = round(float(np.median(v)), 4)
                    r[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
                r["npair_minus_inbatch_bf16_ms"] = round(r["b_bf16_npair_ms"] - r["a_bf16_inbatch_ms"], 4)
                r["b_loss"], r["c_loss"] = round(steps["b_bf16_npair"].loss(), 6), round(steps["c_f32x3_npair"].loss(), 6)
                r["chain_ms"], r["chain_info"] = chain(steps["b_bf16_npair"], args.reps)
                res["B=%d M=%d logq=%s" % (B, M, logq or "off")] = r
                print(json.dumps(r), flush=True)
                del steps, ts
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
