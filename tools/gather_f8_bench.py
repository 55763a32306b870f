#!/usr/bin/env python3
"""The fp8 catalogue against the fp16 one, both in the same run (include/cdml_f8.h):
  * the fused sampler + gather launch of each at config 4's shape -- 10 M x 1500 table, B = 8192, sampler modes 0 and 1,
    1 / 4 / 8 steps per launch; the two formats' launches ALTERNATE, event pairs around 10 back-to-back launches, fresh steps
    every launch (re-fetched rows would be served by the Infinity Cache); min / median / max over the iterations, and the
    algorithmic bytes (F table elements read + F bf16 written per row) over the median;
  * the config-4 step (TrainStep, mode "uniform", eager) on both tables;
  * the catalogue bytes of both.
The yardstick of the fp8 launch is the fp16 launch of the same run, its margin that launch's own min-to-max spread.
Run a variant library with CDML_LIB_PATH=build/variants/libcdml_<tag>.so (tools/experiments/mk_variant.py).
usage: python tools/gather_f8_bench.py [iters] [rows] [step_iters]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from cdml_amd import engine_bf16, ops, train  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10000000
step_iters = int(sys.argv[3]) if len(sys.argv) > 3 else 30
F, B = 1500, 8192
dev = torch.device("cuda:0")
tag = os.path.basename(os.environ.get("CDML_LIB_PATH", "product"))
tables = {"fp16": engine_bf16.FeatureTableF16.synthetic(N, F, 0, dev), "fp8": engine_bf16.FeatureTableF8.synthetic(N, F, 0, dev)}
pairs = torch.from_numpy(bench.synth_pairs(N, 600000, seed=0)).to(dev)
for name, t in tables.items():
    nbytes = t.data.numel() * t.data.element_size() + (t.scale.numel() * 4 if name == "fp8" else 0)
    print("[%s] %s catalogue %d x %d: %.2f GB (%d B per row)" % (tag, name, N, F, nbytes / 1e9, nbytes // N), flush=True)
row_bytes = {"fp16": 2 * F + 2 * F, "fp8": F + 2 * F}

for mode, rpt in ((0, 3), (1, 2)):
    for K in (1, 4, 8):
        R = B * rpt
        x = torch.empty((K, R, 1536), dtype=torch.bfloat16, device=dev)
        idx = torch.empty((K, R), dtype=torch.int32, device=dev)
        shift = torch.zeros(K, dtype=torch.int32, device=dev)

        def fn(t, s):
            if K == 1:
                ops.sample_gather(mode, pairs, 1234, s, B, t.data, F, idx[0], x[0], shift_out=shift)
            else:
                ops.sample_gather(mode, pairs, 1234, s, B, t.data, F, idx, x, shift_out=shift, n_steps=K)
        for s in range(3):
            for t in tables.values():
                fn(t, s * K)
        torch.cuda.synchronize()
        ev = {name: [] for name in tables}
        for it in range(iters):
            for name, t in tables.items():                # alternating: both formats see the same machine
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for j in range(10):
                    fn(t, 100 + (it * 10 + j) * K)
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        med = {}
        for name in tables:
            ms = np.array([a.elapsed_time(b) for a, b in ev[name]]) / 10
            med[name] = float(np.median(ms))
            gb = K * R * row_bytes[name] / 1e9
            print("[%s] %-4s gather mode=%d steps/launch=%d rows=%6d  min %.4f  median %.4f  max %.4f ms/launch -> %.0f GB/s = %.3f "
                  "of 8 TB/s" % (tag, name, mode, K, K * R, ms.min(), med[name], ms.max(), gb / med[name] * 1e3, gb / med[name] / 8.0),
                  flush=True)
        print("[%s] mode=%d steps/launch=%d: fp8 / fp16 launch time = %.3f (bytes alone: 0.750)"
              % (tag, mode, K, med["fp8"] / med["fp16"]), flush=True)

# the config-4 step on both tables: eager, the fused gather inside (several steps per launch, TrainStep's gather_ahead)
steps = {name: train.TrainStep(t, pairs, B, mode="uniform", precision="bf16", device=dev) for name, t in tables.items()}
for ts in steps.values():
    for _ in range(8):
        ts.step()
torch.cuda.synchronize()
ev = {name: [] for name in steps}
for it in range(step_iters):
    for name, ts in steps.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(8):
            ts.step()
        b.record()
        ev[name].append((a, b))
torch.cuda.synchronize()
for name, ts in steps.items():
    ms = np.array([a.elapsed_time(b) for a, b in ev[name]]) / 8
    print("[%s] config-4 step (uniform, eager, B=%d, gather_ahead=%d) on the %s table: min %.4f  median %.4f  max %.4f ms/step -> "
          "%.2f M triplets/s; loss %.6f" % (tag, B, ts.gather_ahead, name, ms.min(), float(np.median(ms)), ms.max(),
                                           B / float(np.median(ms)) / 1e3, ts.loss()), flush=True)
