#!/usr/bin/env python3
"""Cost and effect of popularity-weighted negatives (TrainStep(negative_weights=...), include/cdml_negweights.h).

  --gather   the fused sampler + gather launch at the headline shape (`--rows` x 1500 fp32 catalogue, default 10 M;
             B = 8192; three-plane rows with the k8-interleaved copy; one step per launch): sampler mode 0 against mode 3
             with unigram^0.75 weights over Zipf counts at bits = 16 and 20 -- the variants ALTERNATE inside every round,
             `--rounds` rounds of `--reps` launches each, and the medians and the rounds' spread are reported
  --chain    the mixed N-pair chain's statistics and W launches at B = 8192, D = 256 (precision f32x3, no memory): the
             scalar lq_u against the per-negative vector, alternating the same way
  --skew     a seeded learning A/B on the skewed clustered catalogue of tools/npair_logq_bench.py --skew: recall@10 of
             held-out pairs by decile of the target's popularity, uniform against unigram^0.75 negatives, in the hinge (mode
             "uniform") and in the mixed softmax (mode "npair", uniform_negatives, logq="stream")
usage: python tools/negweights_bench.py [--gather] [--chain] [--skew] [--rows N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdml_amd import engine, ops, train  # noqa: E402
from cdml_amd.negweights import NegativeWeights  # noqa: E402
from npair_bench import event_ms  # noqa: E402


def alternate(variants, rounds, reps):
    """{name: (median ms over the rounds' medians, smallest, largest)}: every round times each variant in turn"""
    seen = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    for _ in range(rounds):
        for k, fn in variants.items():
            seen[k].append(event_ms(fn, reps))
    return {k: {"ms": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in seen.items()}


def gather(args, res):
    dev = torch.device("cuda:0")
    F, B, n = 1500, args.batch, args.rows
    table = engine.FeatureTable.synthetic(n, F, seed=0, device=dev)
    rng = np.random.default_rng(0)
    p = rng.integers(0, n, size=(1 << 22, 2))
    pairs = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    counts = 1e7 / (1.0 + rng.permutation(n))                              # Zipf counts, the popular rows scattered
    plane = (F + 255) // 256 * 256
    R = 3 * B
    x = torch.zeros((R, 3 * plane), dtype=torch.bfloat16, device=dev)
    xk = torch.zeros(3 * R * plane, dtype=torch.bfloat16, device=dev)
    idx = torch.zeros(R, dtype=torch.int32, device=dev)
    kind = torch.zeros(B, dtype=torch.int32, device=dev)
    shift = torch.zeros(1, dtype=torch.int32, device=dev)
    oob = torch.zeros(1, dtype=torch.int32, device=dev)
    step = [0]

    def mode0():
        step[0] += 1
        ops.sample_gather(0, pairs, 1234, step[0], B, table.data, F, idx, x, shift_out=shift, oob_flag=oob, x_ki=xk)

    variants = {"mode0": mode0}
    out = {"rows": n, "F": F, "B": B, "format": "x3k", "rounds": args.rounds, "reps": args.reps}
    for bits in (16, 20):
        nw = NegativeWeights.from_counts(counts, power=0.75, bits=bits)
        t = nw.tables(dev)
        span = np.diff(nw.coarse.numpy().astype(np.int64))               # rows a bucket's search runs over, less one
        out["bits%d" % bits] = {"n_live": nw.n_live, "largest_span": int(span.max()),
                                "search_steps_max": int(np.ceil(np.log2(span.max() + 1))),
                                "largest_share": float(nw.quanta.max().item() / 2.0 ** 32)}

        def mode3(t=t):
            step[0] += 1
            ops.sample_gather_weighted(pairs, 1234, step[0], B, table.data, F, t, idx, x, kind_out=kind, oob_flag=oob, x_ki=xk)
        variants["mode3_bits%d" % bits] = mode3
    out.update(alternate(variants, args.rounds, args.reps))
    out["weighted_share"] = float(kind.float().mean().item())
    res["gather"] = out
    print(json.dumps({"gather": out}), flush=True)


def chain(args, res):
    dev = torch.device("cuda:0")
    B, D, t = args.batch, 256, 0.1
    ws = ops.NPairMixed(B, D, "f32x3", dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    ws.S.copy_(torch.rand(ws.S.shape, generator=g) * 2 - 1)
    ids = torch.randperm(50 * B, generator=g)[:3 * B].to(torch.int32).to(dev)
    ws.bias.copy_(torch.randn(2 * B, generator=g) - 8)
    nb = (torch.randn(B, generator=g) - 8).to(dev)
    stats = torch.zeros(4, dtype=torch.float32, device=dev)
    nc, mc, K = ws.neg_col, ws.mem_col, ws.K
    variants = {}
    for name, lq in (("scalar", -8.0), ("vector", nb)):
        variants["stats_" + name] = lambda lq=lq: ops.npair_mixed_stats(ws.S, ids, B, nc, mc, None, ws.bias, lq, None, t, True,
                                                                        ws.lse, stats, ws.ws)
        variants["W_" + name] = lambda lq=lq: ops.npair_mixed_grad_x3(ws.S, ids, B, nc, mc, None, ws.bias, lq, None, t, True,
                                                                      ws.lse, ws.W3, K)
    out = {"B": B, "D": D, "precision": "f32x3", "rounds": args.rounds, "reps": args.reps}
    out.update(alternate(variants, args.rounds, args.reps))
    res["chain"] = out
    print(json.dumps({"chain": out}), flush=True)


def skew(args, res):
    from cdml_amd.evaluate import Evaluation
    from oracle import tower as otower
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    K, per, F = 512, 8, 96
    N = K * per
    cid = np.repeat(np.arange(K), per)
    feats = (rng.standard_normal((K, F))[cid] + 1.2 * rng.standard_normal((N, F))).astype(np.float32)
    pop = 1.0 / np.arange(1, N + 1) ** args.zipf
    prob = np.empty(N)
    prob[rng.permutation(N)] = pop / pop.sum()
    mate = lambda a: rng.choice(np.flatnonzero(cid == cid[a]))
    tp = np.array([(a, mate(a)) for a in rng.choice(N, args.pairs, p=prob)])
    tp = tp[tp[:, 0] != tp[:, 1]].astype(np.int32)
    held = np.array([(a, mate(a)) for a in rng.integers(0, N, 4000)])
    held = held[held[:, 0] != held[:, 1]]
    count = np.bincount(tp.reshape(-1), minlength=N)
    order = np.argsort(np.argsort(count[held[:, 1]], kind="stable"), kind="stable")
    decile = order * 10 // len(held)                   # 0 = the least co-watched targets, 9 = the most
    table = engine.FeatureTable.from_numpy(feats, dev)
    ev = Evaluation(None, [], device=dev)
    unigram = NegativeWeights.from_counts(count, power=0.75)
    out = {"zipf": args.zipf, "pairs": len(tp), "steps": args.skew_steps, "B": 256, "seed": args.seed,
           "rows_with_weight": int((unigram.quanta > 0).sum()), "rows": N}
    for loss, kw in (("hinge", dict(mode="uniform")),
                     ("mixed_softmax_logq_stream", dict(mode="npair", uniform_negatives=True, logq="stream"))):
        for name, w in (("uniform", None), ("unigram0.75", unigram)):
            ts = train.TrainStep(table, torch.as_tensor(tp).to(dev), 256, hidden_size=512, output_size=64, optimizer="adam",
                                 base_learning_rate=0.003, device=dev, negative_weights=w, **kw)
            for _ in range(args.skew_steps):
                ts.step()
            W = [v.detach().cpu().numpy().astype(np.float64) for v in ts.params.unpadded()]
            emb = otower.vnet_forward(feats.astype(np.float64), *W, dtype=np.float64)["l2_norm"].astype(np.float32)
            r = {"loss": round(ts.loss(), 4), "recall@10": round(ev.retrieval_metrics(emb, held, ks=(10,))["recall@10"], 4),
                 "by_decile": [round(ev.retrieval_metrics(emb, held[decile == d], ks=(10,))["recall@10"], 4) for d in range(10)]}
            if w is not None:
                r["weighted_share"] = round(ts.weighted_share(), 4)
            out["%s,%s" % (loss, name)] = r
            print(json.dumps({"skew": loss, "negatives": name, **r}), flush=True)
    res["skew"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--pairs", type=int, default=40000)
    ap.add_argument("--skew-steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    for on, fn in ((args.gather, gather), (args.chain, chain), (args.skew, skew)):
        if on:
            fn(args, res)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
