"""Times the range search of the IVF index (cdml_amd.knn.IVFIndex.range_search) beside the buffered
``search(k = 128)`` of the same call, by device events, each shape warmed.

    python tools/ivf_range_bench.py              # 343 455 x 256, self-search, 1 024 lists, nprobe in {4, 16},
                                                 # storages f32, f16, pq (M = 32) plain and residual
    python tools/ivf_range_bench.py --n 50000 --nlist 128 --nprobe 4 --storage f32 pq

Radii, per storage and nprobe: every query's own k-th distance of that buffered search for k = 10 and 51 (a per-query
tensor), and ONE global radius, the median of the 51st distances.  Per run one JSON line: the stage times of ``range_search``
itself (its own calls wrapped between device events: tables, lut, slot_dots, filter, compact, and everything of the second
pass as one stage), results per query, the share of the queries that went through the second pass, and as the yardstick the
buffered search's total -- for pq its scan + merge beside the filter launch.  Rows are tools/ivf_bench.py's Gaussian mixtures.
No test gates a time."""
import argparse
import collections
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_bench import catalogue, staged_search, timed  # noqa: E402

STAGES = {"knn.ivf_tables": "tables", "knn.range_compact": "compact", "ops.pq_lut": "lut", "ops.ivf_slot_dots": "slot_dots",
          "ops.ivf_filter_f32": "filter", "ops.ivf_filter_f16": "filter", "ops.ivf_filter_pq": "filter", "ops.ivf_filter_pqr": "filter"}


def staged_range(idx, queries, radius, nprobe, knn, ops, range_cap, probe):
    """``idx.range_search`` with its stage calls between device events: (ms by stage, (lims, D, I), stats).  The stages of the
    second pass (any launch with another capacity than ``range_cap``) are summed into "second_pass"."""
    ms = collections.defaultdict(float)
    mods = {"knn": knn, "ops": ops}
    phase = {"second": False}
    saved = {}

    def wrap(stage, fn):
        def f(*a, **kw):
            t, out = timed(lambda: fn(*a, **kw))
            ms["second_pass" if phase["second"] else stage] += t
            return out
        return f

    inner = idx._range_filter

    def range_filter(Qc, q_sq, pc, tau, cap):
        phase["second"] = cap != range_cap
        return inner(Qc, q_sq, pc, tau, cap)
    try:
        for name, stage in STAGES.items():
            mod, attr = name.split(".")
            saved[name] = getattr(mods[mod], attr)
            setattr(mods[mod], attr, wrap(stage, saved[name]))
        idx._range_filter = range_filter
        st = {}
        total, res = timed(lambda: idx.range_search(queries, radius, nprobe, probe=probe, range_cap=range_cap, stats=st))
    finally:
        for name, fn in saved.items():
            mod, attr = name.split(".")
            setattr(mods[mod], attr, fn)
        del idx._range_filter
    ms["total"] = total
    return dict(ms), res, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=343455)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--storage", nargs="*", default=["f32", "f16", "pq", "pqr"], choices=["f32", "f16", "pq", "pqr"])
    ap.add_argument("--pq-m", type=int, default=32)
    ap.add_argument("--range-cap", type=int, default=256)
    a = ap.parse_args()
    from cdml_amd import knn, ops
    dev = torch.device("cuda:0")
    x = catalogue(a.n, a.dim, dev)
    idx = knn.IVFIndex.build(x, a.nlist, iters=a.iters, device=dev)
    indexes = []
    for storage in a.storage:
        if storage == "f32":
            indexes.append((storage, idx))
        elif storage == "f16":
            indexes.append((storage, knn.IVFIndex.load_state_dict(idx.state_dict(), x, device=dev, storage="f16")))
        else:
            residual = storage == "pqr"
            cb, _ = knn.pq_train(idx.prepare(x), a.pq_m, **({"centroids": idx._C, "assign": idx.assign} if residual else {}))
            state = dict(idx.state_dict(), codebooks=cb, **({"pq_residual": True} if residual else {}))
            indexes.append((storage, knn.IVFIndex.load_state_dict(state, x, device=dev, storage="pq")))
    k_top = ops.knn_list_capacity()
    for nprobe in a.nprobe:
        for storage, index in indexes:
            budget = index.default_score_bytes()
            staged_search(index, x[:8192], k_top, nprobe, knn, ops, budget)                               # warm
            bms, Db, _, bst = staged_search(index, x, k_top, nprobe, knn, ops, budget)                    # the yardstick
            probe = bst["probe"]
            radii = [("k10", Db[:, 9].contiguous()), ("k51", Db[:, 50].contiguous()), ("median51", float(Db[:, 50].median()))]
            staged_range(index, x[:8192], radii[1][1][:8192].contiguous(), nprobe, knn, ops, a.range_cap, probe[:8192])  # warm
            for name, radius in radii:
                ms, (lims, _, _), st = staged_range(index, x, radius, nprobe, knn, ops, a.range_cap, probe)
                per_q = (lims[1:] - lims[:-1]).double()
                line = {"what": "ivf_range", "storage": storage, "n": a.n, "dim": a.dim, "nlist": a.nlist, "nprobe": nprobe,
                        "radius": name, "range_cap": a.range_cap, "range_ms": round(ms.pop("total"), 3),
                        "stages_ms": {s: round(v, 3) for s, v in sorted(ms.items())}, "chunks": len(st["chunks"]),
                        "results_per_query": round(float(per_q.mean()), 2), "results_per_query_max": int(per_q.max()),
                        "second_pass_share": round(st["second_pass"] / a.n, 5), "second_cap": st["second_cap"],
                        "buffer_search_k128_ms": round(sum(bms.values()), 3),
                        "buffer_stages_ms": {s: round(v, 3) for s, v in bms.items()}}
                if storage in ("pq", "pqr"):
                    line.update(pq_m=a.pq_m, buffer_scan_plus_merge_ms=round(bms["scan"] + bms["merge"], 3),
                                filter_ms=round(ms.get("filter", 0.0), 3))
                print(json.dumps(line), flush=True)
                del lims


if __name__ == "__main__":
    main()
