#!/usr/bin/env python3
"""Stage times of ``knn.export`` with and without IVF indexes, in ONE call: 343 455 rows, 1 628-d raw
features (k = 26), 256-d embeddings (k = 81), strict and a cross split.  Per mode three exports: the exact path with the host
writer, and the IVF path (nlist 1024, nprobe 16) with f32 lists and with f16 lists re-ranked over 128 candidates, both with the
device writer and the audit over 1 024 sampled rows.  The raw-feature lists do not depend on the mode, so the cross exports take
the strict export's through ``feature_knn=`` (their feature stage is the strict one's).  Then both writers on the same lists,
their files compared byte for byte.  Inputs are clustered: raw features in groups of ~8 (desim removes something), embeddings
in groups of ~200 (most of a row's 80 neighbours are closer than 1.4, so the writer has 80 entries per line to format).
Every time is taken after a synchronize; peak memory is ``torch.cuda.max_memory_allocated`` at the end of the stage.
``--ivf-only`` skips the exact exports and the host writer (a catalogue for which they take too long).
usage: python tools/knn_export_bench.py [--n N] [--doc D] [--nlist L] [--nprobe P] [--audit M] [--ivf-only] [--storages f32,f16]
                                        [--out DIR] [--json FILE]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdml_amd import knn  # noqa: E402


def clustered(n, width, seed, dev, cluster, noise):
    gw = torch.Generator(device=dev)
    gw.manual_seed(1234 + cluster)
    which = torch.randint(0, n // cluster + 1, (n,), generator=gw, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn((n // cluster + 1, width), generator=g, device=dev, dtype=torch.float32)
    return centres[which] + noise * torch.randn((n, width), generator=g, device=dev, dtype=torch.float32)


def same_files(a, b, prefix):
    names = sorted(f for f in os.listdir(a) if f.startswith(prefix))
    for f in names:
        with open(os.path.join(a, f), "rb") as fa, open(os.path.join(b, f), "rb") as fb:
            while True:
                x, y = fa.read(1 << 24), fb.read(1 << 24)
                if x != y:
                    return False
                if not x:
                    break
    return bool(names)


def row(tag, st):
    stages = ("feature_knn", "embedding_knn", "desim", "write", "audit")
    cells = ["%s %.3f s" % (s, st[s]["seconds"]) if s in st else "%s -" % s for s in stages]
    peak = max(v["max_memory_allocated"] for v in st.values())
    print("%-22s %s; peak %.2f GB" % (tag, "; ".join(cells), peak / 1e9), flush=True)
    if "audit" in st:
        a = st["audit"]
        print("%-22s recall: embedding %d / %d, feature %d / %d; desim rows equal %d / %d, kept %d / %d (Jaccard)"
              % ("", a["e_hits"], a["e_possible"], a["f_hits"], a["f_possible"], a["desim_rows_equal"], a["audit_rows"],
                 a["desim_kept_intersection"], a["desim_kept_union"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=343455)
    ap.add_argument("--doc", type=int, default=250000, help="doc_location of the cross run")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--audit", type=int, default=1024)
    ap.add_argument("--ivf-only", action="store_true")
    ap.add_argument("--storages", default="f32,f16")
    ap.add_argument("--modes", default="strict,cross")
    ap.add_argument("--out", default=None, help="directory for the exports (default: a temporary one, removed)")
    ap.add_argument("--json", default=None, help="write every stage's numbers here")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.n
    feats = clustered(n, 1628, 5, dev, 8, 0.5)
    emb = clustered(n, 256, 6, dev, 200, 0.6)
    decode = ["%032x" % i for i in range(n)]
    knn.knn_search(emb[:8192], emb[:8192], 81)                       # warm-up: library, kernels, allocator
    root = a.out or tempfile.mkdtemp(prefix="knn_export_bench_")
    report = {"n": n, "doc_location": a.doc, "nlist": a.nlist, "nprobe": a.nprobe, "audit_rows": a.audit, "runs": {}}
    configs = [] if a.ivf_only else [("exact", {})]
    for s in a.storages.split(","):
        configs.append(("ivf-" + s, dict(nlist=a.nlist, nprobe=a.nprobe, feature_nlist=a.nlist, feature_nprobe=a.nprobe, storage=s,
                                         refine=128 if s == "f16" else 0, writer="device", audit_rows=a.audit)))
    try:
        for mode in a.modes.split(","):
            loc = n if mode == "strict" else a.doc
            for tag, kw in configs:
                out = os.path.join(root, mode + "-" + tag)
                first = os.path.join(root, a.modes.split(",")[0] + "-" + tag)
                kw = dict(kw)
                if out != first:                                     # the raw-feature lists of the first mode's export
                    kw.update(feature_knn=first, feature_nlist=0, feature_nprobe=0)
                torch.cuda.reset_peak_memory_stats(dev)
                st = {}
                t0 = time.time()
                D, Id = knn.export(emb, feats, decode, out, doc_location=loc, nearest_num=81, desim_nearest_num=26,
                                   split_num=10, stats=st, **kw)
                torch.cuda.synchronize()
                st_total = time.time() - t0
                row(mode + " " + tag, st)
                print("%-22s export() as a whole, .npy files included: %.2f s" % ("", st_total), flush=True)
                report["runs"][mode + "-" + tag] = dict(st, total_seconds=st_total)
                for f in os.listdir(out):                            # keep what a later export reads; the rest is gigabytes
                    if f not in ("fD.npy", "fI.npy", "export_audit.json"):
                        os.remove(os.path.join(out, f))
            # both writers on the same lists (the last export's), files compared
            kept = int(((Id[:, 1:] > 0) & (D[:, 1:] > 0) & (D[:, 1:] < 1.4)).sum())
            times = {}
            for writer in (("device",) if a.ivf_only else ("host", "device")):
                torch.cuda.synchronize()
                t0 = time.time()
                knn.write_knn(os.path.join(root, "w-" + writer), D, Id, decode, split_num=10, prefix=mode + "_knn", writer=writer)
                torch.cuda.synchronize()
                times[writer] = time.time() - t0
            same = None if a.ivf_only else same_files(os.path.join(root, "w-host"), os.path.join(root, "w-device"), mode + "_knn")
            print("%-22s writers on the same lists: %d kept entries (%.1f per line); %s; files identical: %s"
                  % (mode, kept, kept / n, ", ".join("%s %.2f s" % kv for kv in times.items()), same), flush=True)
            report["runs"][mode + "-writers"] = dict(times, kept_entries=kept, identical=same)
            del D, Id
            for writer in times:
                shutil.rmtree(os.path.join(root, "w-" + writer), ignore_errors=True)
    finally:
        if a.out is None:
            shutil.rmtree(root, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
