#!/usr/bin/env python3
"""Cost of hard negatives drawn from per-video candidate lists (TrainStep(negative_lists=...)).

On a synthetic `--rows` x 1500 catalogue (default 1 M), H 5000, D 256, Adam, for B in `--batch` and L = 32:
  * ms/step of the uniform hinge step (gather_ahead "auto") against the listed step at h in {0.5, 1.0} -- the listed step
    fetches one step per launch (gather_ahead 1), so the uniform step is also timed at gather_ahead=1 to tell the two
    costs apart -- on precision "f32x3", and the same on an fp16 table in precision "bf16";
  * the fused gather's own launch (median of `--reps` launches by events, one step per launch): sampler mode 0 against
    mode 2 into the step's own buffers;
  * one TrainStep.refresh_negative_lists(k = 32) at `--refresh-rows` rows (default 343 455), F 1500, wall clock.
The lists are random catalogue ids (the worst case for the list read: no locality).
usage: python tools/hardneg_bench.py [--batch 4096,8192] [--steps 20] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdml_amd import engine, engine_bf16, hardneg, ops, train  # noqa: E402
from npair_bench import event_ms, step_ms  # noqa: E402

L = 32


def gather_ms(ts, reps, lists=None, h=1.0):
    """the fused sampler + gather launch alone, one step per launch, into the step's buffers"""
    x = ts._xa[0] if ts.gather_ahead > 1 else ts.ws.x_hat
    idx = ts._idxa[0] if ts.gather_ahead > 1 else ts.idx
    xk = getattr(ts, "_xka", None)
    xk = xk[0] if xk is not None else (ts.ws.xk if (ts.x3 and getattr(ts.ws, "kint", False)) else None)
    if lists is None:
        fn = lambda: ops.sample_gather(0, ts.pairs, ts.seed, 7, ts.B, ts.table.data, ts.table.feature_size, idx, x,
                                       shift_out=ts.shift, oob_flag=ts.oob, x_ki=xk)
    else:
        kind = torch.zeros(ts.B, dtype=torch.int32, device=ts.device)
        fn = lambda: ops.sample_gather_listed(ts.pairs, ts.seed, 7, ts.B, ts.table.data, ts.table.feature_size, lists, h, idx,
                                              x, kind_out=kind, oob_flag=ts.oob, x_ki=xk)
    fn()
    return event_ms(fn, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--refresh-rows", type=int, default=343455)
    ap.add_argument("--batch", default="4096,8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, H, D = 1500, 5000, 256
    rng = np.random.default_rng(0)
    p = rng.integers(0, args.rows, size=(4 * args.rows, 2))
    pairs = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    lists = torch.randint(0, args.rows, (args.rows, L), dtype=torch.int32, device=dev)
    res = {"rows": args.rows, "F": F, "H": H, "D": D, "L": L, "optimizer": "adam", "steps": args.steps}
    for precision, mk_table in (("f32x3", engine.FeatureTable), ("bf16", engine_bf16.FeatureTableF16)):
        table = mk_table.synthetic(args.rows, F, seed=0, device=dev)
        mk = lambda B, **kw: train.TrainStep(table, pairs, B, output_size=D, hidden_size=H, optimizer="adam", mode="uniform",
                                             base_learning_rate=0.01, device=dev, precision=precision, **kw)
        for B in (int(x) for x in args.batch.split(",")):
            r = {}
            ts = mk(B)
            r["uniform_ms"] = round(step_ms(ts, args.steps, args.warmup), 4)
            r["uniform_gather_ahead"] = ts.gather_ahead
            r["gather_uniform_ms"] = round(gather_ms(ts, args.reps), 4)
            for h in (0.5, 1.0):
                r["gather_listed_h%.1f_ms" % h] = round(gather_ms(ts, args.reps, lists, h), 4)
            del ts
            torch.cuda.empty_cache()
            ts = mk(B, gather_ahead=1)
            r["uniform_ahead1_ms"] = round(step_ms(ts, args.steps, args.warmup), 4)
            del ts
            torch.cuda.empty_cache()
            for h in (0.5, 1.0):
                ts = mk(B, negative_lists=lists, hard_fraction=h)
                r["listed_h%.1f_ms" % h] = round(step_ms(ts, args.steps, args.warmup), 4)
                r["hard_share_h%.1f" % h] = round(ts.hard_share(), 4)
                del ts
                torch.cuda.empty_cache()
            res["%s,B=%d" % (precision, B)] = r
            print(json.dumps({"precision": precision, "B": B, **r}), flush=True)
        del table
        torch.cuda.empty_cache()
    # one refresh at the export's catalogue size: embed with the current weights, self-kNN, filter, copy
    n = args.refresh_rows
    table = engine.FeatureTable.synthetic(n, F, seed=1, device=dev)
    p = rng.integers(0, n, size=(2 * n, 2))
    rp = torch.as_tensor(p[p[:, 0] != p[:, 1]], dtype=torch.int32).to(dev)
    ts = train.TrainStep(table, rp, 4096, output_size=D, hidden_size=H, optimizer="adam", mode="uniform", device=dev,
                         precision="f32x3", negative_lists=hardneg.empty_lists(n, L), hard_fraction=1.0)
    ts.step()
    for name in ("refresh_first_s", "refresh_s"):
        torch.cuda.synchronize()
        t0 = time.time()
        ts.refresh_negative_lists(L)
        torch.cuda.synchronize()
        res[name] = round(time.time() - t0, 3)
    res["refresh_rows"] = n
    print(json.dumps({k: res[k] for k in ("refresh_rows", "refresh_first_s", "refresh_s")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
