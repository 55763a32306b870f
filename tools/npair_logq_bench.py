#!/usr/bin/env python3
"""Step time of the N-pair loss with the sampling-bias (logQ) correction, its launches, and a popularity-skewed A/B.

Whole steps (CUDA events around `steps` eager steps after `warmup`): TrainStep(mode="npair", logq=...) with the correction
off, from a fixed table (the log of each video's share of the co-watch pairs) and from the streaming estimator, for B in
`--batch` and M in {0, 4B} (`--memory-factor`), on a 1 M x 1500 synthetic catalogue, H 5000, D 256, Adam, precision
f32x3.  Then the chain's launches on the step's own embedded rows, each timed alone (median of `reps`): the statistics
and the W planes with and without the bias, the gather and the estimator's update.
--skew: a seeded learning A/B on the clustered catalogue of test_gpu_npair.test_npair_training_raises_recall with
Zipf-drawn anchors (exponent `--zipf`), without and with logq="stream": recall@10 of held-out pairs (uniform anchors) by
decile of the target's popularity in the training pairs (Evaluation.retrieval_metrics).
usage: python tools/npair_logq_bench.py [--batch 4096,8192] [--memory-factor 0,4] [--steps 20] [--warmup 5] [--skew]
       [--skip-timing] [--out FILE]"""
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
    """the launches the correction touches, on ts.ws.e (ms): statistics and W with and without the bias, gather, update"""
    B, w, m, src = ts.B, ts.npair_ws, ts.npair_memory, ts.npair_logq
    idx, t, sym = ts.idx, ts.temperature, ts.symmetric
    st = {}
    if m is None:
        S, W3, K = w.S, w.W3, B
        st["stats"] = event_ms(lambda: ops.npair_stats(S, idx, B, t, sym, w.lse, ts.stats, w.ws), reps)
        st["stats logq"] = event_ms(lambda: ops.npair_logq_stats(S, idx, B, w.bias, t, sym, w.lse, ts.stats, w.ws), reps)
        st["W planes"] = event_ms(lambda: ops.npair_grad_x3(S, idx, B, t, sym, w.lse, W3, K), reps)
        st["W planes logq"] = event_ms(lambda: ops.npair_logq_grad_x3(S, idx, B, w.bias, t, sym, w.lse, W3, K), reps)
        st["gather"] = event_ms(lambda: src.gather(idx, B, None, w.bias, None), reps)
    else:
        S, W3, K = m.S, m.W3, m.K
        st["stats"] = event_ms(lambda: ops.npair_memory_stats(S, idx, B, B, m.ids, t, sym, w.lse, ts.stats, w.ws), reps)
        st["stats logq"] = event_ms(lambda: ops.npair_memory_logq_stats(S, idx, B, w.bias, B, m.ids, m.bias, t, sym, w.lse,
                                                                        ts.stats, w.ws), reps)
        st["W planes"] = event_ms(lambda: (ops.npair_grad_x3(S, idx, B, t, sym, w.lse, W3, K),
                                           ops.npair_memory_grad_x3(S, idx, B, B, m.ids, t, sym, w.lse, W3, K)), reps)
        st["W planes logq"] = event_ms(lambda: (ops.npair_logq_grad_x3(S, idx, B, w.bias, t, sym, w.lse, W3, K),
                                                ops.npair_memory_logq_grad_x3(S, idx, B, B, m.ids, m.bias, t, sym, w.lse,
                                                                              W3, K)), reps)
        st["gather"] = event_ms(lambda: src.gather(idx, B, m.ids, w.bias, m.bias), reps)
    if isinstance(src, ops.LogQEstimator):
        state = src.state_dict()
        st["update"] = event_ms(lambda: src.update(idx, B, 0, ts.step_dev), reps)
        src.load(state)
    return {k: round(v, 4) for k, v in st.items()}


def timing(args, res):
    dev = torch.device("cuda:0")
    F, H, D = 1500, 5000, 256
    table = engine.FeatureTable.synthetic(args.rows, F, seed=0, device=dev)
    rng = np.random.default_rng(0)
    p = rng.integers(0, args.rows, size=(4 * args.rows, 2))
    p = p[p[:, 0] != p[:, 1]]
    pairs = torch.as_tensor(p, dtype=torch.int32).to(dev)
    deg = np.bincount(p.reshape(-1), minlength=args.rows).astype(np.float64) + 1.0
    fixed = torch.as_tensor(np.log(deg / deg.sum()), dtype=torch.float32)
    res.update({"rows": args.rows, "F": F, "H": H, "D": D, "precision": "f32x3", "optimizer": "adam", "steps": args.steps})
    for B in (int(x) for x in args.batch.split(",")):
        for M in (int(x) * B for x in args.memory_factor.split(",")):
            for name, src in (("off", None), ("fixed", fixed), ("stream", "stream")):
                ts = train.TrainStep(table, pairs, B, output_size=D, hidden_size=H, mode="npair", optimizer="adam",
                                     base_learning_rate=0.01, device=dev, precision="f32x3", memory_size=M, logq=src)
                r = {"ms_per_step": round(step_ms(ts, args.steps, args.warmup), 4), "loss": round(ts.loss(), 6)}
                if src is not None:
                    r["launch_ms"] = chain(ts, args.reps)
                res["B=%d M=%d logq=%s" % (B, M, name)] = r
                print(json.dumps({"B": B, "M": M, "logq": name, **r}), flush=True)
                del ts
                torch.cuda.empty_cache()


def skew(args, res):
    from cdml_amd.evaluate import Evaluation
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
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
    out = {"zipf": args.zipf, "pairs": len(tp), "steps": args.skew_steps, "B": 256, "seed": args.seed}
    for name, src in (("off", None), ("stream", "stream")):
        ts = train.TrainStep(table, torch.as_tensor(tp).to(dev), 256, hidden_size=512, output_size=64, mode="npair",
                             optimizer="adam", base_learning_rate=0.003, device=dev, logq=src)
        for _ in range(args.skew_steps):
            ts.step()
        W = [w.detach().cpu().numpy().astype(np.float64) for w in ts.params.unpadded()]
        emb = otower.vnet_forward(feats.astype(np.float64), *W, dtype=np.float64)["l2_norm"].astype(np.float32)
        r = {"loss": round(ts.loss(), 4), "recall@10": round(ev.retrieval_metrics(emb, held, ks=(10,))["recall@10"], 4),
             "by_decile": [round(ev.retrieval_metrics(emb, held[decile == d], ks=(10,))["recall@10"], 4) for d in range(10)]}
        out[name] = r
        print(json.dumps({"skew": name, **r}), flush=True)
    res["skew"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--batch", default="4096,8192")
    ap.add_argument("--memory-factor", default="0,4")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--pairs", type=int, default=40000)
    ap.add_argument("--skew-steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if not args.skip_timing:
        timing(args, res)
    if args.skew:
        skew(args, res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
