#!/usr/bin/env python3
"""Step time of the N-pair loss with mixed negative sampling (uniform catalogue negatives), and its chain stage by stage.

Whole steps (CUDA events around `steps` eager steps after `warmup`, which also fill the ring) on a 1 M x 1500 synthetic
catalogue, H 5000, D 256, Adam, precision f32x3, for B in `--batch` and M in {0, 2B}: (a) TrainStep(mode="uniform"), the hinge
step with the same R = 3B tower; (b) TrainStep(mode="npair", memory_size=M), the in-batch loss; (c) the same with
uniform_negatives=True.  Then the chain of ops.npair_mixed_loss on the step's own embedded rows, each stage timed alone
(median of `reps`): the plane split of A, P, N, S = A [P; N; Mem]^T, the statistics, the W planes (one launch), dA, dP + dN
and the ring push.
usage: python tools/npair_mixed_bench.py [--batch 4096,8192] [--steps 20] [--warmup 5] [--out FILE]"""
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
    """the mixed chain on ts.ws.e, stage by stage (ms)"""
    B, L, w = ts.B, ts.layout, ts.npair_mixed
    Dq, K, e, idx, de, ring = w.Dq, w.K, ts.ws.e, ts.idx, ts.ws.de, w.ring
    nc, mc, mid = w.neg_col, w.mem_col, (w.ring.ids if w.ring is not None else None)
    t, sym = ts.temperature, ts.symmetric
    st = {}
    st["split"] = event_ms(lambda: ops.npair_mixed_split_x3(e, B, L.Dp, w.A3, Dq, w.R3, Dq, w.T3, K, nc), reps)
    st["S = A [P;N;Mem]^T"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, w.A3, Dq, w.R3, Dq, w.S, B, K, Dq,
                                                                  workspace=w.gemm_ws), reps)
    st["stats"] = event_ms(lambda: ops.npair_mixed_stats(w.S, idx, B, nc, mc, mid, None, 0.0, None, t, sym, w.lse, ts.stats,
                                                         w.ws), reps)
    st["W planes"] = event_ms(lambda: ops.npair_mixed_grad_x3(w.S, idx, B, nc, mc, mid, None, 0.0, None, t, sym, w.lse, w.W3, K),
                              reps)
    st["dA = W [P;N;Mem]"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, w.W3, K, w.T3, K, de[0::3], B, Dq, K,
                                                                 workspace=w.gemm_ws), reps)
    st["dP + dN"] = event_ms(lambda: (ops.gemm_bf16x3_tn(w.W3, K, w.A3, Dq, de[1::3], B, Dq, B, workspace=w.gemm_ws),
                                      ops.gemm_bf16x3_tn(w.W3[:, nc:], K, w.A3, Dq, de[2::3], B, Dq, B, workspace=w.gemm_ws)),
                             reps)
    if ring is not None:
        w.rows2.view(B, 2).copy_(idx.view(B, 3)[:, :2])
        st["push"] = event_ms(lambda: ops.npair_memory_push(e[1::3], w.rows2, B, L.Dp, 0, ts.step_dev, ring.start, ring.rows,
                                                            ring.ids, R3=w.R3[mc:], plane_r=Dq, T3=w.T3[:, mc:], plane_t=K), reps)
        state = ring.state_dict()
    st["whole chain"] = event_ms(lambda: ops.npair_mixed_loss(e, idx, B, L.Dp, t, sym, "f32x3", de=de, stats=ts.stats, ws=w,
                                                              step=0, step_dev=ts.step_dev), reps)
    if ring is not None:
        ring.load(state["rows"], state["ids"])
    flop = 2.0 * B * K * Dq
    info = {"K": K, "S_bytes_MB": B * K * 4 / 1e6, "W_planes_bytes_MB": B * K * 6 / 1e6,
            "S TFLOP/s (fp32 equiv)": round(flop / (st["S = A [P;N;Mem]^T"] * 1e-3) / 1e12, 1),
            "dA TFLOP/s (fp32 equiv)": round(flop / (st["dA = W [P;N;Mem]"] * 1e-3) / 1e12, 1),
            "W GB/s (S read + planes written)": round(B * K * 10 / (st["W planes"] * 1e-3) / 1e9, 1)}
    return {k: round(v, 4) for k, v in st.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--batch", default="4096,8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, D = 1500, 5000, 256
    table = engine.FeatureTable.synthetic(args.rows, F, seed=0, device=dev)
    rng = np.random.default_rng(0)
    p = rng.integers(0, args.rows, size=(4 * args.rows, 2))
    pairs = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    res = {"rows": args.rows, "F": F, "H": H, "D": D, "precision": "f32x3", "optimizer": "adam", "steps": args.steps}
    mk = lambda B, **kw: train.TrainStep(table, pairs, B, output_size=D, hidden_size=H, optimizer="adam",
                                         base_learning_rate=0.01, device=dev, precision="f32x3", **kw)
    for B in (int(x) for x in args.batch.split(",")):
        ts = mk(B, mode="uniform")
        uniform = round(step_ms(ts, args.steps, args.warmup), 4)
        del ts
        torch.cuda.empty_cache()
        for M in (0, 2 * B):
            r = {"uniform_hinge_ms": uniform}
            for name, kw in (("inbatch_npair_ms", {}), ("mixed_ms", {"uniform_negatives": True})):
                ts = mk(B, mode="npair", memory_size=M, **kw)
                r[name] = round(step_ms(ts, args.steps, args.warmup), 4)
                if kw:
                    r["loss"] = round(ts.loss(), 6)
                    r["chain_ms"], r["chain_info"] = chain(ts, args.reps)
                del ts
                torch.cuda.empty_cache()
            res["B=%d,M=%d" % (B, M)] = r
            print(json.dumps({"B": B, "M": M, **r}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
