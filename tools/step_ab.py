#!/usr/bin/env python3
"""Bit-equality A/B of the training step, inference and the fusion tower between two trees of the PACKAGE over one built
library (the acceptance test of a Python-side refactor: csrc/ unchanged, so the kernels are the same and every difference
is the package's).

--dump OUT.npz   (GPU) runs every case below on fixed, seeded inputs with ``ops.call`` wrapped, and saves per case the flat
                 parameters, the last step's flat gradient, the optimizer slots, ``stats``, ``ws.e``, for precision f16x2 the
                 plane scales with ``changes`` and ``calibrated``, for a trainable catalogue its rows and their m / v -- and
                 the ordered list of C entries with their non-pointer arguments (a pointer counts as null or not), from the
                 construction to the last step: the same launches in the same order with the same scalars.
                 ``--tree DIR``: import the package from DIR (an export of the parent commit) instead of this tree; the
                 library is the one CDML_LIB_PATH names, or that tree's.
--compare A B    (CPU) asserts that the two dumps hold the same arrays, bit for bit, and the same launch lists.

The shapes are the smallest that reach every branch: a catalogue of 5 000 rows, F = H = 300, D = 64 -- the plane layouts pad
to 512 / 512 / 256 (Fp % 512 == 0: dW1 in two row blocks), the fp32 layout to 320 / 384 / 64 (ragged); B = 128 for
"uniform", "inbatch", "semihard" (384 or 256 rows, multiples of 128; 2B = 256: the fused miner), B = 256 for "npair"; six
steps, so the f16x2 check steps 0, 1, 2 and 4 are in.  Cases: every allowed precision x mode with Adam; LARS and momentum,
clipping + regulariser, use_graph (eight steps), a state_dict round trip and tower_backward with the data-parallel hooks
for every precision; train_table on f32 / f32x3 / f16x2; gather_ahead = 2; memory + streaming logQ on npair (f32x3, bf16);
uniform_negatives; negative_lists; CDML_X3_KI=1 and CDML_X3_TRANSPOSED=1 around the construction; Prediction.predict and
embed_table (300 rows in chunks of 128) on the four precisions; FusionTower forward + backward on f32 / f32x3 / f16x2.
usage: python tools/step_ab.py --dump OUT.npz [--tree DIR] | --compare A.npz B.npz"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

N, F, H, D = 5000, 300, 300, 64
PRECISIONS = ("f32", "f32x3", "f32x3-3", "f16x2", "bf16")
MODES = ("uniform", "inbatch", "semihard", "npair")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "the dumps hold different arrays: %s" % sorted(set(A.files) ^ set(B.files))
    bad = []
    for k in sorted(A.files):
        x, y = A[k], B[k]
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad.append(k)
            if k.endswith("/launches"):
                la, lb = json.loads(x.tobytes()), json.loads(y.tobytes())
                i = next((i for i, (p, q) in enumerate(zip(la, lb)) if p != q), min(len(la), len(lb)))
                print("%s: %d against %d launches, first difference at %d: %s | %s"
                      % (k, len(la), len(lb), i, la[i:i + 1], lb[i:i + 1]))
    n_l = sum(k.endswith("/launches") for k in A.files)
    print("%d arrays (%d launch lists), %d differ" % (len(A.files), n_l, len(bad)))
    assert not bad, "not bit-identical: %s" % bad[:20]


def dump(path, tree):
    import torch
    sys.path.insert(0, os.path.abspath(tree))
    from cdml_amd import engine, engine_bf16, engine_x3, fusion, ops, predict, train
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261018)
    out, launches = {}, []

    real_call = ops.call

    def recording_call(name, *args):
        rec = [name]
        for a in args:
            if isinstance(a, ctypes.c_void_p):
                rec.append("ptr" if a.value else "null")
            elif isinstance(a, ctypes.Array):
                rec.append([int(v) for v in a])
            elif isinstance(a, ctypes._SimpleCData):
                rec.append(a.value)
            else:
                rec.append(a.item() if hasattr(a, "item") else a)
        launches.append(rec)
        return real_call(name, *args)
    ops.call = recording_call

    def keep(name, t):
        t = t.detach().cpu().contiguous()
        out[name] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()

    def case_done(tag):
        torch.cuda.synchronize()
        out[tag + "/launches"] = np.frombuffer(json.dumps(launches).encode(), np.uint8)
        del launches[:]

    pr = rng.integers(0, N, (4096, 2)).astype(np.int32)
    pr[:, 1] = np.where(pr[:, 1] == pr[:, 0], (pr[:, 0] + 1) % N, pr[:, 1])
    pairs = torch.from_numpy(pr).to(dev)
    table = lambda p: (engine_bf16.FeatureTableF16 if p == "bf16" else engine.FeatureTable).synthetic(N, F, 0, dev)
    tables = {}

    def frozen(p):
        k = p == "bf16"
        if k not in tables:
            tables[k] = table(p)
        return tables[k]

    def step_of(p, mode="uniform", B=None, tab=None, **kw):
        B = B or (256 if mode == "npair" else 128)
        return train.TrainStep(tab or frozen(p), pairs, B, hidden_size=H, output_size=D, mode=mode, precision=p, device=dev, **kw)

    def keep_step(tag, ts):
        torch.cuda.synchronize()
        keep(tag + "/flat", ts.params.flat), keep(tag + "/grad", ts.params.grad)
        for k in ("m", "v") if ts.optimizer == "adam" else ("acc",):
            keep(tag + "/" + k, getattr(ts, k))
        keep(tag + "/stats", ts.stats), keep(tag + "/e", ts.ws.e)
        sc = getattr(ts.ws, "scales", None)
        if sc is not None:
            out[tag + "/scales"] = np.array([sc.state()[k] for k in sorted(sc.state())] + [sc.changes, sc.calibrated], np.float64)
        if ts.train_table:
            keep(tag + "/table", ts.table.data), keep(tag + "/tab_m", ts.tab_m), keep(tag + "/tab_v", ts.tab_v)

    def run(tag, p, steps=6, **kw):
        ts = step_of(p, **kw)
        for _ in range(steps):
            ts.step()
        keep_step(tag, ts)
        case_done(tag)
        return ts

    npair_ok = lambda p: p in ("f32", "f32x3", "bf16")
    for p in PRECISIONS:
        for mode in MODES:
            if mode != "npair" or npair_ok(p):
                run("adam/%s/%s" % (p, mode), p, mode=mode)
        for opt in ("lars", "momentum"):
            run("%s/%s" % (opt, p), p, optimizer=opt)
        run("clip_reg/%s" % p, p, clip_gradient_norm=0.5, regularization_penalty=1.0, l2_penalty=1e-3)
        run("graph/%s" % p, p, steps=8, use_graph=True)
        # a checkpoint after three steps, loaded into a fresh step, two more steps
        ts = run("resume/%s/before" % p, p, steps=3)
        state = ts.state_dict()
        ts2 = step_of(p)
        ts2.load_state_dict(state)
        ts2.step(), ts2.step()
        keep_step("resume/%s/after" % p, ts2)
        case_done("resume/%s/after" % p)
        # tower_backward with the data-parallel hooks, called directly (the module is the workspace class's)
        ts = step_of(p)
        back = sys.modules[type(ts.ws).__module__].tower_backward
        seen = []
        ts.fetch(), ts.forward_loss()
        back(ts.params, ts.ws, after_w1=lambda: seen.append(len(launches)))
        keep("hooks/%s/after_w1/grad" % p, ts.params.grad)
        ts.forward_loss()
        back(ts.params, ts.ws, w1_chunks=2, after_w1_chunk=lambda lo, hi: seen.extend((lo, hi, len(launches))))
        keep("hooks/%s/chunks/grad" % p, ts.params.grad)
        out["hooks/%s/seen" % p] = np.array(seen, np.int64)
        case_done("hooks/%s" % p)
    for p in ("f32", "f32x3", "f16x2"):
        run("train_table/%s" % p, p, tab=table(p), train_table=True)
    run("gather_ahead2", "f32x3", gather_ahead=2)
    for p in ("f32x3", "bf16"):
        run("npair_memory_logq/%s" % p, p, mode="npair", memory_size=512, logq="stream")
    run("uniform_negatives", "f32x3", mode="npair", uniform_negatives=True)
    lists = torch.from_numpy(rng.integers(0, N, (N, 8)).astype(np.int32))
    run("negative_lists", "f32x3", negative_lists=lists, hard_fraction=0.75)
    for var, B in (("CDML_X3_KI", 128), ("CDML_X3_TRANSPOSED", 256)):      # (read at construction; transposed: rows % 256)
        os.environ[var] = "1"
        try:
            ts = step_of("f32x3", B=B)
        finally:
            del os.environ[var]
        assert ts.ws.kint if var == "CDML_X3_KI" else ts.ws.transposed
        for _ in range(6):
            ts.step()
        keep_step(var, ts)
        case_done(var)

    # ---- inference: predict on raw rows, embed_table in chunks of 128 (bf16 reads its fp16 table only) ----
    raw = torch.from_numpy(rng.random((300, F), dtype=np.float32)).to(dev)
    for p in ("f32", "f32x3", "f16x2", "bf16"):
        L = {"f32": engine.TowerLayout, "bf16": engine_bf16.layout_bf16}.get(p, engine_x3.layout_x3)(F, H, D)
        pred = predict.Prediction(params=engine.VNetParams(L, dev, 42), precision=p)
        small = (engine_bf16.FeatureTableF16 if p == "bf16" else engine.FeatureTable).synthetic(300, F, 1, dev)
        if p != "bf16":
            keep("predict/%s/raw" % p, pred.predict(raw))
        keep("predict/%s/table" % p, pred.embed_table(small, 128))
        case_done("predict/%s" % p)

    # ---- the fusion tower at its smallest plane-kernel sizes: visual 256 -> 256 -> 256, doc 64 -> 64 -> 256, 128 rows ----
    x = torch.from_numpy(rng.random((128, 320), dtype=np.float32)).to(dev)
    de = torch.from_numpy(rng.standard_normal((128, 256)).astype(np.float32) / 64).to(dev)
    for net in ("MultiplyNet", "ResNet"):
        for p in ("f32", "f32x3", "f16x2"):
            fp = fusion.FusionParams(net, dev, doc_size=64, visual_size=256, hidden_v=256, hidden_d=64, output_size=256)
            tower = fusion.FusionTower(fp, 128, precision=p)
            assert (tower.vx3 is None) == (p == "f32")
            for step in (0, 1):
                tower.refresh_planes(step)
                keep("fusion/%s/%s/e%d" % (net, p, step), tower.forward(x))
                tower.backward(de)
                keep("fusion/%s/%s/grad%d" % (net, p, step), fp.grad)
            case_done("fusion/%s/%s" % (net, p))

    np.savez(path, **out)
    print("dumped %d arrays to %s (package: %s, library: %s)"
          % (len(out), path, os.path.dirname(os.path.abspath(ops.__file__)), os.environ.get("CDML_LIB_PATH") or "the tree's"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="OUT.npz")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    elif args.dump:
        dump(args.dump, args.tree)
    else:
        ap.error("--dump OUT.npz or --compare A.npz B.npz")


if __name__ == "__main__":
    main()
