"""Times the IVF index (cdml_amd.knn.IVFIndex) against the exact search of the same size, by device events, each shape warmed.

    python tools/ivf_bench.py                    # 343 455 x 256, self-search, k = 51, nlist in {256, 1024}, nprobe in {4, 16}
    python tools/ivf_bench.py --big              # 10 M x 256, self-search, k = 40, nlist in {4096, 16384}, nprobe in {8, 16, 32}
                                                 # (recall on a 65 536-query sample)
    python tools/ivf_bench.py --n 50000 --nlist 64 --nprobe 4 8 --k 20
    python tools/ivf_bench.py --storage f32 f16 --refine 128   # fp16 lists beside the fp32 ones over the same (centroids, assign)
    python tools/ivf_bench.py --storage f16 pq --pq-m 32 --refine 128   # product-quantised lists (32 bytes a row) beside the fp16 ones
    python tools/ivf_bench.py --storage pq --pq-m 16 32 --pq-residual 0 1 --refine 0 128   # residual codes beside the plain ones, per M
    python tools/ivf_bench.py --storage f16 pq --pq-m 32 --pq-bits 8 4 --refine 0 128 --repeats 3   # 4-bit codes (two a byte, 16-entry tables) beside the 8-bit ones
    python tools/ivf_bench.py --scan buffer filter             # the threshold-filter scan beside the buffered one, same index, same call

Per run one JSON line: build time by stage (one assignment, one centroid update, the whole build), search time by stage
(coarse / tables / scan / merge), the scan's FLOP from the tile table over its kernel time, recall@k against the exact search,
max / mean list length, scanned share.  With --storage f16 the line of the fp16 index (storage "f16": the lists re-derived from
the fp32 index's centroids and assign) follows the fp32 one: the same stages plus the re-rank, issued and useful scan TF/s,
the index's bytes, and recall@k for refine 0 and --refine.  With --storage pq (--pq-m M) the line of the pq index follows in the
same way: the codebooks trained once per nlist (pq_train_ms) and the catalogue encoded (pq_encode_ms), the stages with the lookup
tables ("lut") and the table-lookup scan apart, the scan's lookups per second instead of FLOP/s.  With --pq-residual 1 the line of the
residual pq index (codes of the row minus its list's centroid; the same (centroids, assign)) follows, with the slot scalars' launch
("slot_dots") as a stage of its own.  With --pq-bits 8 4 the line of the 4-bit index (include/cdml_ivf_pq4.h; the same bytes per row, the
same (centroids, assign)) follows the 8-bit one, with its own training and encoding times; --repeats N times every buffered search N
times and reports the median per stage, with the min and max of the total and of the scan ("search_ms_spread", "scan_ms_spread").  With --scan filter a line "scan": "filter" follows every buffered
line (under --score-bytes and under every --filter-score-bytes): the stages seed scan / seed merge / filter / merge_list /
re-search, issued and useful TF/s of the seed scan and of the filter, the peak score + candidate bytes of a chunk, the candidates
appended per query, the re-searched share, and whether (D, I) equal the buffered search's bit for bit.  Rows are Gaussian mixtures (n / 64 centres, noise 0.5) so that lists mean something.
No test gates a time."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def catalogue(n, D, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn(max(n // 64, 1), D, device=dev, generator=g)
    which = torch.randint(0, centres.shape[0], (n,), device=dev, generator=g)
    return centres[which] + 0.5 * torch.randn(n, D, device=dev, generator=g)


def staged_search(idx, queries, k, nprobe, knn, ops, score_bytes, refine=0, base=None):
    """IVFIndex.search stage by stage (the same calls), every stage between device events; (ms by stage, D, I, stats)"""
    ms = {"coarse": 0.0, "tables": 0.0, "scan": 0.0, "merge": 0.0}
    dev = idx.device
    cap = ops.knn_list_capacity()
    f16, pq = idx.storage == "f16", idx.storage == "pq"
    tile = {}
    if f16:
        ms["round"] = 0.0
    pqr = pq and idx.pq_residual
    pq4 = pq and idx.pq_bits == 4
    if pq:
        ms["lut"] = 0.0
        if pqr:
            ms["slot_dots"] = 0.0
        tile["tile_slots"], tile["tile_rows"] = (ops.ivf_pq4_tile if pq4 else ops.ivf_pq_tile)(idx.pq_m)
    if refine:
        ms["refine"] = 0.0

    def coarse():
        Q = idx._prepared(queries, dev, idx.l2_norm)
        q_sq = torch.zeros(Q.shape[0], dtype=torch.float32, device=dev)
        ops.row_sqnorm(Q, Q.shape[1], q_sq)
        return Q, q_sq, idx._probes(Q, nprobe).to(torch.int32)
    ms["coarse"], (Q, q_sq, probe) = timed(coarse)
    nq = Q.shape[0]
    best_d = torch.empty((nq, cap), dtype=torch.float32, device=dev)
    best_i = torch.empty((nq, cap), dtype=torch.int32, device=dev)
    cand_d = torch.empty_like(best_d) if refine else best_d
    cand_i = torch.empty_like(best_i) if refine else best_i

    def plan():
        ld = (idx.list_len + 3) // 4 * 4
        p = probe.to(torch.int64)
        costs = torch.where(p >= 0, ld[p.clamp(min=0)], torch.zeros_like(p)).sum(1).cpu().numpy()
        if pq:
            costs = costs + knn.pq_query_floats(idx.pq_m, nprobe if pqr else 0, idx.pq_bits)
        return knn.ivf_plan_chunks(costs, score_bytes, max_queries=(2 ** 31 - 1) // nprobe)
    t, chunks = timed(plan)
    ms["tables"] += t
    tiles = useful = floats = 0
    for q0, q1 in chunks:
        pc = probe[q0:q1].contiguous()
        t, tb = timed(lambda: knn.ivf_tables(pc, idx.list_len, **tile))
        ms["tables"] += t
        if tb["n_slots"] == 0:
            best_d[q0:q1], best_i[q0:q1] = float("inf"), 0x7fffffff
            continue
        scores = torch.empty(max(tb["n_floats"], 4), dtype=torch.float32, device=dev)
        if f16:
            def rounded():
                Qh = Q[q0:q1].to(torch.float16)
                ops.row_sqnorm(Qh.float(), Qh.shape[1], q_sq[q0:q1])
                return Qh
            t, Qh = timed(rounded)
            ms["round"] += t
        if pq and tb["n_tiles"]:
            lut = torch.empty((q1 - q0, 2 * idx.pq_m, 16) if pq4 else (q1 - q0, idx.pq_m, 256), dtype=torch.float32, device=dev)
            t, _ = timed(lambda: (ops.pq4_lut if pq4 else ops.pq_lut)(Q[q0:q1], idx.codebooks, lut))
            ms["lut"] += t
            if pq4:
                t, _ = timed(lambda: ops.ivf_scan_pq4(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], idx.codes,
                                                      idx.list_start, tb["tiles"], scores))
            elif pqr:
                slot_base = torch.empty(tb["n_slots"], dtype=torch.float32, device=dev)
                t, _ = timed(lambda: ops.ivf_slot_dots(Q[q0:q1], idx._C, tb["slot_query"], tb["slot_start"], slot_base))
                ms["slot_dots"] += t
                t, _ = timed(lambda: ops.ivf_scan_pqr(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], slot_base,
                                                      idx.codes, idx.list_start, tb["tiles"], scores))
            else:
                t, _ = timed(lambda: ops.ivf_scan_pq(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], idx.codes,
                                                     idx.list_start, tb["tiles"], scores))
            ms["scan"] += t
            del lut
        elif tb["n_tiles"]:
            if f16:
                t, _ = timed(lambda: ops.ivf_scan_f16(Qh, tb["slot_query"], tb["slot_start"], tb["slot_off"], idx.rows,
                                                      idx.list_start, tb["tiles"], scores))
            else:
                t, _ = timed(lambda: ops.ivf_scan_f32(Q[q0:q1], tb["slot_query"], tb["slot_start"], tb["slot_off"], idx.rows,
                                                      idx.list_start, tb["tiles"], scores))
            ms["scan"] += t
        t, _ = timed(lambda: ops.ivf_merge(scores, tb["slot_off"], tb["slot_of"], pc, idx.list_start, idx.ids, idx.r_sq,
                                           q_sq[q0:q1], refine or k, cand_d[q0:q1], cand_i[q0:q1]))
        ms["merge"] += t
        if refine:
            t, _ = timed(lambda: ops.ivf_refine(Q[q0:q1], base, cand_i[q0:q1], refine, k, best_d[q0:q1], best_i[q0:q1]))
            ms["refine"] += t
        tiles += tb["n_tiles"]
        floats += tb["n_floats"]
        cnt = (tb["slot_start"][1:] - tb["slot_start"][:-1]).to(torch.int64)
        useful += int((cnt * idx.list_len).sum())
    I = best_i[:, :k].to(torch.int64)
    I[I == 0x7fffffff] = -1
    Dp = Q.shape[1]
    stats = {"chunks": len(chunks), "tiles": tiles, "score_bytes": 4 * floats,
             "scan_flop_tiles": 2.0 * tiles * knn.IVF_TILE * knn.IVF_TILE * Dp, "scan_flop_useful": 2.0 * useful * Dp, "probe": probe}
    if pq:                                                    # lookups (one LDS gather + one add each) in place of FLOP
        per_row = idx.pq_m * (2 if pq4 else 1)                # (4-bit: two gathers a byte)
        stats.update(scan_lookups_tiles=float(tiles) * tile["tile_slots"] * tile["tile_rows"] * per_row,
                     scan_lookups_useful=float(useful) * per_row)
    return ms, best_d[:, :k], I, stats


def staged_filter_search(idx, queries, k, nprobe, knn, ops, score_bytes, refine=0, base=None, filter_cap=None, seed_probes=None):
    """IVFIndex.search(scan="filter") stage by stage (the same calls as IVFIndex._scan_filtered), every stage between device
    events; (ms by stage, D, I, stats)"""
    ms = {"coarse": 0.0, "tables": 0.0, "seed_scan": 0.0, "seed_merge": 0.0, "filter": 0.0, "merge_list": 0.0, "research": 0.0}
    dev = idx.device
    cap = ops.knn_list_capacity()
    f16 = idx.storage == "f16"
    if f16:
        ms["round"] = 0.0
    if refine:
        ms["refine"] = 0.0
    keep = refine or k
    s = seed_probes or idx.default_seed_probes(keep, nprobe)
    cap_f = filter_cap or idx.default_filter_cap(keep)

    def coarse():
        Q = idx._prepared(queries, dev, idx.l2_norm)
        q_sq = torch.zeros(Q.shape[0], dtype=torch.float32, device=dev)
        ops.row_sqnorm(Q, Q.shape[1], q_sq)
        return Q, q_sq, idx._probes(Q, nprobe).to(torch.int32)
    ms["coarse"], (Q, q_sq, probe) = timed(coarse)
    nq, Dp = Q.shape
    best_d = torch.empty((nq, cap), dtype=torch.float32, device=dev)
    best_i = torch.empty((nq, cap), dtype=torch.int32, device=dev)
    cand_d = torch.empty_like(best_d) if refine else best_d
    cand_i = torch.empty_like(best_i) if refine else best_i
    seed_p, rest_p = probe.clone(), probe.clone()
    seed_p[:, s:] = -1
    rest_p[:, :s] = -1
    t, chunks = timed(lambda: knn.ivf_plan_chunks(idx.filter_costs(probe, s, cap_f), score_bytes, max_queries=(2 ** 31 - 1) // nprobe))
    ms["tables"] += t
    tiles = {"seed": 0, "filter": 0}
    useful = {"seed": 0, "filter": 0}
    peak = n_appended = 0
    redo = []
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    for q0, q1 in chunks:
        m = q1 - q0
        pc = seed_p[q0:q1].contiguous()
        t, tb = timed(lambda: knn.ivf_tables(pc, idx.list_len))
        ms["tables"] += t
        Qc = Q[q0:q1]
        if f16:
            def rounded():
                Qh = Q[q0:q1].to(torch.float16)
                ops.row_sqnorm(Qh.float(), Dp, q_sq[q0:q1])
                return Qh
            t, Qc = timed(rounded)
            ms["round"] += t
        peak = max(peak, 4 * tb["n_floats"] + 8 * cap_f * m)
        if tb["n_slots"] == 0:
            cand_d[q0:q1], cand_i[q0:q1] = float("inf"), 0x7fffffff
        else:
            scores = torch.empty(max(tb["n_floats"], 4), dtype=torch.float32, device=dev)
            if tb["n_tiles"]:
                t, _ = timed(lambda: (ops.ivf_scan_f16 if f16 else ops.ivf_scan_f32)(
                    Qc, tb["slot_query"], tb["slot_start"], tb["slot_off"], idx.rows, idx.list_start, tb["tiles"], scores))
                ms["seed_scan"] += t
            t, _ = timed(lambda: ops.ivf_merge(scores, tb["slot_off"], tb["slot_of"], pc, idx.list_start, idx.ids, idx.r_sq,
                                               q_sq[q0:q1], keep, cand_d[q0:q1], cand_i[q0:q1]))
            ms["seed_merge"] += t
            del scores
            tiles["seed"] += tb["n_tiles"]
            useful["seed"] += int(((tb["slot_start"][1:] - tb["slot_start"][:-1]).to(torch.int64) * idx.list_len).sum())
        if s < nprobe:
            pr = rest_p[q0:q1].contiguous()
            t, tr = timed(lambda: knn.ivf_tables(pr, idx.list_len))
            ms["tables"] += t
            if tr["n_tiles"]:
                tau = cand_d[q0:q1, keep - 1].contiguous()
                cnt = torch.zeros(m, dtype=torch.int32, device=dev)
                cand = torch.empty((m, cap_f, 2), dtype=torch.int32, device=dev)
                t, _ = timed(lambda: (ops.ivf_filter_f16 if f16 else ops.ivf_filter_f32)(
                    Qc, tr["slot_query"], tr["slot_start"], q_sq[q0:q1], tau, cnt, idx.rows, idx.list_start, idx.r_sq, idx.ids,
                    tr["tiles"], cand, cap_f))
                ms["filter"] += t
                over = cnt > cap_f
                n_over, n_app = torch.stack([over.sum(), cnt.sum()]).tolist()
                n_appended += n_app
                t, _ = timed(lambda: ops.knn_merge_list(cand, cnt, cap_f, m, keep, cand_d[q0:q1], cand_i[q0:q1], overflow))
                ms["merge_list"] += t
                if n_over:
                    redo.append(torch.nonzero(over).flatten() + q0)
                tiles["filter"] += tr["n_tiles"]
                useful["filter"] += int(((tr["slot_start"][1:] - tr["slot_start"][:-1]).to(torch.int64) * idx.list_len).sum())
        if refine:
            t, _ = timed(lambda: ops.ivf_refine(Q[q0:q1], base, cand_i[q0:q1], refine, k, best_d[q0:q1], best_i[q0:q1]))
            ms["refine"] += t
    n_redo = 0
    if redo:                                                  # (as IVFIndex._scan_filtered: the buffered search of these queries)
        def again():
            ix = torch.cat(redo)
            po = probe.index_select(0, ix)
            ld = (idx.list_len + 3) // 4 * 4
            pl = po.to(torch.int64)
            own = int(torch.where(pl >= 0, ld[pl.clamp(min=0)], torch.zeros_like(pl)).sum(1).max())
            bd = torch.empty((ix.numel(), cap), dtype=torch.float32, device=dev)
            bi = torch.empty((ix.numel(), cap), dtype=torch.int32, device=dev)
            cd_ = torch.empty_like(bd) if refine else bd
            ci_ = torch.empty_like(bi) if refine else bi
            idx._scan_buffered(Q.index_select(0, ix), q_sq.index_select(0, ix), po, k, refine, base, max(int(score_bytes), 4 * own),
                               bd, bi, cd_, ci_)
            best_d[ix], best_i[ix] = bd, bi
            return int(ix.numel())
        ms["research"], n_redo = timed(again)
    I = best_i[:, :k].to(torch.int64)
    I[I == 0x7fffffff] = -1
    fl = 2.0 * knn.IVF_TILE * knn.IVF_TILE * Dp
    stats = {"chunks": len(chunks), "seed_probes": s, "filter_cap": cap_f, "peak_bytes": peak, "n_appended": n_appended,
             "refiltered": n_redo, "tiles": tiles, "flop_tiles": {w: fl * v for w, v in tiles.items()},
             "flop_useful": {w: 2.0 * v * Dp for w, v in useful.items()}, "probe": probe}
    return ms, best_d[:, :k], I, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--nlist", type=int, nargs="*", default=None)
    ap.add_argument("--nprobe", type=int, nargs="*", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sample", type=int, default=65536, help="queries of the recall sample when n is above it (--big)")
    ap.add_argument("--score-bytes", type=int, default=None)
    ap.add_argument("--storage", nargs="*", default=["f32"], choices=["f32", "f16", "pq"], help="list formats to time, over one (centroids, assign)")
    ap.add_argument("--pq-m", type=int, nargs="*", default=[32], help="bytes per listed row of the pq index (one index per value)")
    ap.add_argument("--pq-residual", type=int, nargs="*", default=[0], choices=[0, 1],
                    help="0 = plain codes, 1 = codes of the row minus its list's centroid (one index per value)")
    ap.add_argument("--pq-bits", type=int, nargs="*", default=[8], choices=[8, 4],
                    help="8 = one code a byte (256 codewords), 4 = two codes a byte (16 codewords each); one index per value")
    ap.add_argument("--repeats", type=int, default=1, help="timed runs of every buffered search (median per stage, spread of the total)")
    ap.add_argument("--refine", type=int, nargs="*", default=[0],
                    help="re-rank depths r of the f16 / pq index (k <= r <= 128); 0 = none, always run")
    ap.add_argument("--scan", nargs="*", default=["buffer"], choices=["buffer", "filter"],
                    help="search modes to time over the same index; \"filter\" is compared with the buffered search of the same call")
    ap.add_argument("--filter-score-bytes", type=int, nargs="*", default=[], help="further budgets for the filter runs (e.g. 1073741824)")
    ap.add_argument("--filter-cap", type=int, default=None)
    ap.add_argument("--seed-probes", type=int, default=None)
    a = ap.parse_args()
    from cdml_amd import knn, ops
    dev = torch.device("cuda:0")
    n = a.n or (10_000_000 if a.big else 343455)
    k = a.k or (40 if a.big else 51)
    nlists = a.nlist or ([4096, 16384] if a.big else [256, 1024])
    nprobes = a.nprobe or ([8, 16, 32] if a.big else [4, 16])
    refines = sorted(set([0] + list(a.refine)))
    x = catalogue(n, a.dim, dev)
    # the exact search of the same size, in the same call (warmed); at --big on the sample only
    sample = None
    if a.big or n >= 4_000_000:
        sample = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:a.sample]
    xq = x if sample is None else x[sample]
    knn.knn_search(x[:4096], x[:4096], k, device=dev)
    exact_ms, (_, Ie) = timed(lambda: knn.knn_search(x, xq, k, device=dev))
    print(json.dumps({"what": "exact", "n": n, "nq": xq.shape[0], "dim": a.dim, "k": k, "ms": round(exact_ms, 3)}), flush=True)
    for nlist in nlists:
        knn.IVFIndex.build(x[:max(4 * nlist, 4096)], min(nlist, 64), iters=1, device=dev)                 # warm the build's launches
        build_ms, idx = timed(lambda: knn.IVFIndex.build(x, nlist, iters=a.iters, device=dev))
        X = idx._prepared(x, dev, True)
        assign_ms, _ = timed(lambda: knn.knn_search(idx._C, X, 1, l2_norm=False, device=dev))
        C2 = idx._C.clone()
        order = torch.argsort(idx.assign.clamp(min=0), stable=True).to(torch.int32)
        update_ms, _ = timed(lambda: ops.ivf_centroid_sums(X, order, idx.list_start, C2, X.shape[1]))
        del X
        lens = idx.list_len.double()
        score_bytes = a.score_bytes or idx.default_score_bytes()
        indexes = []
        for storage in a.storage:
            if storage == "f32":
                indexes.append((idx, None))
            elif storage == "pq":                                                                         # the same (centroids, assign), pq codes
                Xp = idx.prepare(x)
                for pq_m, bits, residual in [(m, b, r) for m in a.pq_m for b in a.pq_bits for r in a.pq_residual]:
                    if bits == 4 and residual:                                                            # (not built: DESIGN.md section 10)
                        print("ivf_bench: --pq-bits 4 with --pq-residual 1 is not built (the library refuses it by name): no "
                              "line for pq_m = %d" % pq_m, file=sys.stderr, flush=True)
                        continue
                    res = {"centroids": idx._C, "assign": idx.assign} if residual else {}
                    train = knn.pq4_train if bits == 4 else knn.pq_train
                    train(Xp[:4096], pq_m, iters=1)                                                       # warm
                    train_ms, (cb, obj) = timed(lambda: train(Xp, pq_m, **res))
                    codes = torch.empty((n, pq_m), dtype=torch.uint8, device=dev)
                    if bits == 4:
                        ops.pq4_encode(Xp[:4096], cb, codes)                                              # warm
                        encode_ms, _ = timed(lambda: ops.pq4_encode(Xp, cb, codes))
                    elif residual:
                        ops.pqr_encode(Xp[:4096], idx._C, idx.assign[:4096].contiguous(), cb, codes)  # warm
                        encode_ms, _ = timed(lambda: ops.pqr_encode(Xp, idx._C, idx.assign, cb, codes))
                    else:
                        encode_ms, _ = timed(lambda: ops.pq_encode(Xp, cb, codes))
                    del codes
                    state = dict(idx.state_dict(), codebooks=cb, **({"pq_residual": True} if residual else {}),
                                 **({"pq_bits": 4} if bits == 4 else {}))
                    h = knn.IVFIndex.load_state_dict(state, x, device=dev, storage="pq")
                    h.bench = {"pq_m": pq_m, "pq_bits": bits, "pq_residual": bool(residual), "pq_train_ms": round(train_ms, 2),
                               "pq_encode_ms": round(encode_ms, 3),
                               "pq_objective_last": float(obj[:, -1].sum()) if obj.shape[1] else None}
                    indexes.append((h, Xp if refines != [0] else None))
            else:                                                                                         # the same (centroids, assign), fp16 lists
                h = knn.IVFIndex.load_state_dict(idx.state_dict(), x, device=dev, storage="f16")
                indexes.append((h, h.prepare(x) if refines != [0] else None))
        for nprobe in nprobes:
            for index, base in indexes:
                for refine in ([0] if base is None else refines):
                    run_one(index, base, refine, nprobe, nlist, x, k, n, a, knn, ops, sample, Ie, xq, exact_ms, score_bytes,
                            build_ms, assign_ms, update_ms, lens)


def run_one(idx, base, refine, nprobe, nlist, x, k, n, a, knn, ops, sample, Ie, xq, exact_ms, score_bytes, build_ms, assign_ms,
            update_ms, lens):
    kw = dict(refine=refine, base=base) if refine else {}
    staged_search(idx, x[:8192], k, nprobe, knn, ops, score_bytes, **kw)                                  # warm
    ms, Db, I, st = staged_search(idx, x, k, nprobe, knn, ops, score_bytes, **kw)                         # the self-search, all rows
    spread = {}
    if a.repeats > 1:                                                                                     # median per stage; (D, I) of the first run
        runs = [ms] + [staged_search(idx, x, k, nprobe, knn, ops, score_bytes, **kw)[0] for _ in range(a.repeats - 1)]
        ms = {s: sorted(r[s] for r in runs)[len(runs) // 2] for s in ms}
        tot = [sum(r.values()) for r in runs]
        spread = {"repeats": a.repeats, "search_ms_spread": [round(min(tot), 3), round(max(tot), 3)],
                  "scan_ms_spread": [round(min(r["scan"] for r in runs), 3), round(max(r["scan"] for r in runs), 3)]}
    if "filter" in a.scan:
        run_filter(idx, refine, nprobe, nlist, x, k, n, a, knn, ops, score_bytes, Db, I, sum(ms.values()), ms, st, kw)
    if "buffer" not in a.scan:
        return
    Is = I if sample is None else I[sample]
    hit = found = 0
    for r0 in range(0, Is.shape[0], 32768):                                                               # (recall in row blocks)
        a_, b_ = Is[r0:r0 + 32768], Ie[r0:r0 + 32768]
        hit += int(((a_.unsqueeze(2) == b_.unsqueeze(1)).any(2) & (a_ >= 0)).sum())
        found += int((b_ >= 0).sum())
    recall = hit / max(found, 1)
    del I, Is
    total = sum(ms.values())
    lists = (idx.codes, idx.codebooks) if idx.storage == "pq" else (idx.rows,)
    index_bytes = sum(t.numel() * t.element_size() for t in lists + (idx.r_sq, idx.ids, idx.list_start, idx._C))
    extra = dict(getattr(idx, "bench", {}))
    if idx.storage == "pq":
        extra.update(scan_glookups_tiles=round(st["scan_lookups_tiles"] / max(ms["scan"], 1e-9) / 1e6, 2),
                     scan_glookups_useful=round(st["scan_lookups_useful"] / max(ms["scan"], 1e-9) / 1e6, 2),
                     list_bytes=idx.codes.numel())
    print(json.dumps({
        **extra, **spread, "what": "ivf", "storage": idx.storage, "refine": refine, "index_bytes": index_bytes,
        "n": n, "nq": n, "recall_queries": Ie.shape[0], "dim": a.dim, "k": k, "nlist": nlist, "nprobe": nprobe, "iters": a.iters,
        "build_ms": round(build_ms, 2), "assign_all_rows_ms": round(assign_ms, 3), "centroid_update_ms": round(update_ms, 3),
        "search_ms": round(total, 3), "stages_ms": {s: round(v, 3) for s, v in ms.items()},
        "exact_ms": round(exact_ms, 3), "exact_nq": xq.shape[0], "speedup": round(exact_ms / total, 2) if sample is None else None,
        "scan_tflops_tiles": None if idx.storage == "pq" else round(st["scan_flop_tiles"] / max(ms["scan"], 1e-9) / 1e9, 2),
        "scan_tflops_useful": None if idx.storage == "pq" else round(st["scan_flop_useful"] / max(ms["scan"], 1e-9) / 1e9, 2),
        "score_bytes": st["score_bytes"], "score_budget": score_bytes, "chunks": st["chunks"], "recall": round(recall, 4),
        "list_max_over_mean": round(float(lens.max() / lens.mean()), 2), "empty_lists": int((lens == 0).sum()),
        "scanned_share": round(idx.scanned_share(st["probe"]), 5), "nprobe_over_nlist": round(nprobe / nlist, 5)}), flush=True)

def run_filter(idx, refine, nprobe, nlist, x, k, n, a, knn, ops, score_bytes, Db, Ib, buffer_ms, buffer_stages, buffer_st, kw):
    """the filter scan over the same index and queries, under the buffered run's budget and every --filter-score-bytes"""
    fkw = dict(kw, filter_cap=a.filter_cap, seed_probes=a.seed_probes)
    staged_filter_search(idx, x[:8192], k, nprobe, knn, ops, score_bytes, **fkw)                          # warm
    tf = lambda flop, ms: round(flop / max(ms, 1e-9) / 1e9, 2)
    for budget in [score_bytes] + [b for b in a.filter_score_bytes if b != score_bytes]:
        ms, D, I, st = staged_filter_search(idx, x, k, nprobe, knn, ops, budget, **fkw)
        total = sum(ms.values())
        print(json.dumps({
            "what": "ivf", "scan": "filter", "storage": idx.storage, "refine": refine, "n": n, "nq": n, "dim": a.dim, "k": k,
            "nlist": nlist, "nprobe": nprobe, "seed_probes": st["seed_probes"], "filter_cap": st["filter_cap"],
            "search_ms": round(total, 3), "stages_ms": {s: round(v, 3) for s, v in ms.items()},
            "buffer_search_ms": round(buffer_ms, 3), "buffer_scan_ms": round(buffer_stages["scan"], 3),
            "buffer_merge_ms": round(buffer_stages["merge"], 3), "buffer_score_bytes": buffer_st["score_bytes"],
            "buffer_chunks": buffer_st["chunks"], "buffer_budget": score_bytes, "speedup_over_buffer": round(buffer_ms / total, 3),
            "seed_tflops_tiles": tf(st["flop_tiles"]["seed"], ms["seed_scan"]), "seed_tflops_useful": tf(st["flop_useful"]["seed"], ms["seed_scan"]),
            "filter_tflops_tiles": tf(st["flop_tiles"]["filter"], ms["filter"]),
            "filter_tflops_useful": tf(st["flop_useful"]["filter"], ms["filter"]),
            "peak_score_plus_candidate_bytes": st["peak_bytes"], "score_budget": budget, "chunks": st["chunks"],
            "n_appended_per_query": round(st["n_appended"] / max(n, 1), 2), "refiltered": st["refiltered"],
            "refiltered_share": round(st["refiltered"] / max(n, 1), 5),
            "equal_to_buffer": bool(torch.equal(D, Db) and torch.equal(I, Ib))}), flush=True)
        del D, I


if __name__ == "__main__":
    main()
