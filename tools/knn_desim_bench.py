#!/usr/bin/env python3
"""Stage times of the kNN export (faiss_knn.main) at the reference's scale: 343 455 rows, 1 628-d raw features (k = 26),
256-d embeddings (k = 81); strict (doc_location = n) and a cross split.  Stages timed separately, each after a
synchronize: the raw-feature kNN, the embedding kNN, desim (prep + the greedy walk; the walk's kernel time alone from
CUDA events over a few repeats, with its gathered bytes per second) and the text writer.  Inputs are clustered (rows in
groups of ~8 around shared centres in both spaces) so that desim removes something.
usage: python tools/knn_desim_bench.py [--n N] [--doc D] [--out DIR]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdml_amd import knn, ops  # noqa: E402


def clustered(n, width, seed, dev, cluster=8, noise=0.5):
    gw = torch.Generator(device=dev)
    gw.manual_seed(1234)
    which = torch.randint(0, n // cluster + 1, (n,), generator=gw, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn((n // cluster + 1, width), generator=g, device=dev, dtype=torch.float32)
    return centres[which] + noise * torch.randn((n, width), generator=g, device=dev, dtype=torch.float32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    r = fn()
    torch.cuda.synchronize()
    return r, time.time() - t0


def desim_kernel(eI, fI, fD, reps=5):
    """(prep seconds, walk seconds) by CUDA events, the median of ``reps`` launches each"""
    n_f = fI.shape[0]
    e32 = eI.to(torch.int32).contiguous()
    ff = torch.empty((n_f, 32), dtype=torch.int32, device=eI.device)
    out = torch.empty_like(e32)
    tp, tw = [], []
    for _ in range(reps):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        ops.knn_desim_prep(fI, fD, min(31, fI.shape[1]), 1.4, ff)     # (fI[...][:, :31] of a 26-wide list: all 26)
        b.record()
        ops.knn_desim(e32, ff, out)
        c.record()
        c.synchronize()
        tp.append(a.elapsed_time(b) / 1e3)
        tw.append(b.elapsed_time(c) / 1e3)
    return sorted(tp)[reps // 2], sorted(tw)[reps // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=343455)
    ap.add_argument("--doc", type=int, default=250000, help="doc_location of the cross run")
    ap.add_argument("--out", default=None, help="directory for the text lists (default: a temporary one, removed)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.n
    feats = clustered(n, 1628, 5, dev)
    emb = clustered(n, 256, 6, dev, noise=0.8)
    knn.knn_search(emb[:8192], emb[:8192], 81)                       # warm-up: library, kernels, allocator
    (fD, fI), t_f = timed(lambda: knn.knn_search(feats, feats, 26))
    del feats
    print("raw-feature kNN   n=%d D=1628 (padded 1664) k=26: %.3f s" % (n, t_f))
    out_dir = a.out or tempfile.mkdtemp(prefix="knn_desim_bench_")
    decode = ["%032x" % i for i in range(n)]
    try:
        for mode in ("strict", "cross"):
            if mode == "strict":
                (D, I), t_e = timed(lambda: knn.knn_search(emb, emb, 81))
            else:
                (D, I), t_e = timed(lambda: knn.cross_knn(emb, a.doc, nearest_num=81))
            (Id, t_d) = timed(lambda: knn.desim(I, fI, fD))
            t_prep, t_walk, out = desim_kernel(I, fI, fD)
            assert torch.equal(out.to(torch.int64), Id)
            kept0 = int((I >= 0).sum())
            ke = I.shape[1]
            lines = int((I >= 0).sum())                              # gathered: one 128-B filtered row per valid neighbour
            gathered = lines * 128
            _, t_w = timed(lambda: knn.write_knn(out_dir, D, Id, decode, split_num=10, prefix=mode + "_knn"))
            print("%-6s embedding kNN k=%d%s: %.3f s" % (mode, ke, "" if mode == "strict" else " (doc_location %d)" % a.doc, t_e))
            print("%-6s desim (host call, incl. id conversion): %.2f ms; prep %.3f ms, walk %.3f ms: %.2f GB gathered, %.0f GB/s;"
                  " kept %d of %d" % (mode, 1e3 * t_d, 1e3 * t_prep, 1e3 * t_walk, gathered / 1e9, gathered / t_walk / 1e9,
                                      int((Id >= 0).sum()), kept0))
            print("%-6s writer (10 files): %.2f s" % (mode, t_w))
    finally:
        if a.out is None:
            shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
