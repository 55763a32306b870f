#!/usr/bin/env python3
"""The data-parallel N-pair loss's LOCAL chain on one GPU, stage by stage: what one rank of a world of G / B ranks
computes between the collectives.  The gathered positives are synthetic (unit rows, distinct ids) and nothing is
communicated -- wire time cannot be measured on one GPU.

Stages (median of `reps`, CUDA events; precision f32x3, D 256): the splits of A and of the G gathered positives into
their operand images, S_r = A_r P_all^T, the local statistics (rows + column partials), the column fold + stats, the W_r
planes, dA = W_r P_all, the partial dP = W_r^T A_r over all G columns, and the rank-order fold of the received dP blocks.
G = 8B at B = 8192 cannot be produced today: W_r's planes exceed the plane GEMMs' 2 GiB operand range (ops.NPairDP refuses
the shape); asking for it records the refusal instead of a row.
usage: python tools/npair_dp_bench.py [--batch 8192] [--worlds 1,2,4] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdml_amd import ops  # noqa: E402
from npair_bench import event_ms  # noqa: E402


def chain(B, W, D, reps, dev, t=0.1, sym=True):
    G = B * W
    try:
        ws = ops.NPairDP(B, G, D, "f32x3", dev)
    except ValueError as e:
        return None, {"refused": str(e)}
    g = torch.Generator(device=dev)
    g.manual_seed(G)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, D, device=dev, generator=g), dim=1)
    e = torch.zeros((2 * B, D), device=dev)
    e[0::2] = unit(B)
    e[1::2] = torch.nn.functional.normalize(e[0::2] + 0.3 * unit(B), dim=1)
    ws.wire[:, :D].copy_(unit(G))                                   # every rank's positives; this rank is rank 0
    ws.wire[:B, :D].copy_(e[1::2])
    ws.wire.view(torch.int32)[:, D:D + 2].copy_(torch.arange(2 * G, dtype=torch.int32, device=dev).view(G, 2))
    de, stats = torch.zeros_like(e), torch.zeros(4, device=dev)
    A, P, Dq = e[0::2], ws.P_all(), ws.Dq
    st = {}
    st["split"] = event_ms(lambda: (ops.split_f32_bf16x3(A, ws.A3, Dq), ops.split_f32_bf16x3(P, ws.PA3, Dq),
                                    ops.split_f32_bf16x3(P, ws.PAT3, G, transpose=True)), reps)
    st["S = A P_all^T"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, ws.A3, Dq, ws.PA3, Dq, ws.S, B, G, Dq,
                                                              workspace=ws.gemm_ws), reps)
    ops.npair_dp_phase1(e, 0, ws, t, sym)
    st["local stats"] = event_ms(lambda: ops.npair_dp_local_stats(ws.S, ws.ids_all, B, G, 0, t, sym, ws.lse_row, ws.colpart,
                                                                  ws.ws), reps)
    for r in range(W):                                              # (the other ranks' partials: copies of this one's)
        ws.colpart_all[r].copy_(ws.colpart)
    st["fold + stats"] = event_ms(lambda: (ops.npair_dp_col_fold(ws.colpart_all, ws.lse_col),
                                           ops.npair_dp_stats(ws.S, B, G, 0, t, sym, ws.lse_col, stats, ws.ws)), reps)
    st["W planes"] = event_ms(lambda: ops.npair_dp_grad_x3(ws.S, ws.ids_all, B, G, 0, t, sym, ws.lse_row, ws.lse_col, ws.W3, G),
                              reps)
    st["dA = W P_all"] = event_ms(lambda: ops.gemm_bf16x3_nt(ops.BE_F32, ws.W3, G, ws.PAT3, G, de[0::2], B, Dq, G,
                                                             workspace=ws.gemm_ws), reps)
    st["partial dP = W^T A"] = event_ms(lambda: ops.gemm_bf16x3_tn(ws.W3, G, ws.A3, Dq, ws.dP_part, G, Dq, B,
                                                                   workspace=ws.gemm_ws), reps)
    st["dP fold"] = event_ms(lambda: ops.npair_dp_phase3(ws, de), reps)
    st["local chain"] = event_ms(lambda: (ops.npair_dp_phase1(e, 0, ws, t, sym),
                                          ops.npair_dp_phase2(e, 0, ws, t, sym, de=de, stats=stats),
                                          ops.npair_dp_phase3(ws, de)), reps)
    flop = 2.0 * B * G * Dq
    info = {"S_bytes_MB": B * G * 4 / 1e6, "W_planes_bytes_MB": B * G * 6 / 1e6,
            "S TFLOP/s (fp32 equiv)": round(flop / (st["S = A P_all^T"] * 1e-3) / 1e12, 1),
            "dA TFLOP/s (fp32 equiv)": round(flop / (st["dA = W P_all"] * 1e-3) / 1e12, 1),
            "partial dP TFLOP/s (fp32 equiv)": round(flop / (st["partial dP = W^T A"] * 1e-3) / 1e12, 1),
            "local stats GB/s (S read twice: rows, columns)": round(2 * B * G * 4 / (st["local stats"] * 1e-3) / 1e9, 1),
            "W GB/s (S read + planes written)": round(B * G * 10 / (st["W planes"] * 1e-3) / 1e9, 1),
            "wire_bytes": {"positives + ids (all-gather, sent)": B * (D + ops.NPAIR_DP_WIRE_PAD) * 4,
                           "column partials (all-gather, sent)": 8 * G, "dP blocks (all-to-all, sent)": (W - 1) * B * D * 4},
            "loss": round(float(stats[0].item()), 6)}
    return {k: round(v, 4) for k, v in st.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--worlds", default="1,2,4")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"B": args.batch, "D": args.dim, "precision": "f32x3"}
    for W in (int(x) for x in args.worlds.split(",")):
        ms, info = chain(args.batch, W, args.dim, args.reps, dev)
        res["G=%dB" % W] = {"chain_ms": ms, "info": info}
        print(json.dumps({"B": args.batch, "G": args.batch * W, "chain_ms": ms, "info": info}), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
