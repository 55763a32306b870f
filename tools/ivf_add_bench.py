"""Streaming build of the IVF index: ``IVFIndex.train`` on a sample, then ``add`` in chunks, per list
format -- what the stages cost, what the peak memory is, and what the one launch of an update (``ops.ivf_lists_move``) moves a
second against the torch plumbing that does the same job.

Shape: section 9f.5's -- 343 455 x 256 Gaussian-mixture rows (n / 64 centres, noise 0.5), 1 024 lists; storage f32 / f16 / pq
(pq_m 32, bits 8 and 4); chunks of 32 768 rows fed from host memory.  Per format and repeat:
  * device-event times of the stages of every ``add`` (copy-in, prepare, assign, encode, r_sq, the chunk's tables, the move), summed over
    the chunks, and the total; ``torch.cuda.max_memory_allocated`` over the adds;
  * the one-shot baseline in the same call: ``knn_search`` for the assignment plus ``from_assignment`` of the whole catalogue (device
    rows), its time and its peak memory; and whether the streamed index equals it bit for bit;
  * the move launch alone, on the buffers of the LAST chunk's update: achieved bytes/s (read + written: 2 n_new (row_bytes + 8)) against
    the torch alternative on the same buffers -- ``torch.cat`` of old and chunk + ``index_select`` by a precomputed map (the map's
    construction is not timed) -- per call over windows of 50 back-to-back calls, and the peak memory of either.
No threshold: the parent has no ``add``; the torch plumbing and the one-shot build are the baselines.  One JSON line per format and
repeat, and a summary line per format (median and spread)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("copy_in", "prepare", "assign", "encode", "r_sq", "tables", "move")


def catalogue(n, D, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn(max(n // 64, 1), D, device=dev, generator=g)
    which = torch.randint(0, centres.shape[0], (n,), device=dev, generator=g)
    return centres[which] + 0.5 * torch.randn(n, D, device=dev, generator=g)


class StageClock:
    """device events at the stage marks of ``IVFIndex.add``; ``totals()`` after a synchronise"""

    def __init__(self):
        self.marks = []
        self.last = None

    def start(self):
        self.last = torch.cuda.Event(enable_timing=True)
        self.last.record()

    def __call__(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, self.last, e))
        self.last = e

    def totals(self):
        torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for name, a, b in self.marks:
            out[name] += a.elapsed_time(b)
        return out


INNER = 50          # calls per timed window of ``timed``: one call of 30-300 us would measure the launch gap as much as the work


def timed(fn, repeats):
    """device-event milliseconds per call of ``repeats`` windows of INNER back-to-back calls of fn (after three warm-up calls)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / INNER)
    return ms


def same_index(a, b):
    payload = "codes" if a.storage == "pq" else "rows"
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("ids", "list_start", "list_len", "r_sq", "assign", payload)) \
        and (a.n_rows, a.n_listed) == (b.n_rows, b.n_listed)


def move_alone(idx, chunk, knn, ops, repeats):
    """the LAST update again, outside the index: the launch and the torch plumbing on the same buffers"""
    dev = idx.device
    name = idx._payload_name()
    X = idx._prepared(chunk.to(dev), dev, idx.l2_norm)
    _, Ia = knn.knn_search(idx._C, X, 1, l2_norm=False, device=dev, precision=idx.precision)
    payload, r_sq, a = idx._encode_block(X, Ia[:, 0])
    del X
    m = a.numel()
    key = torch.where(a >= 0, a, torch.full_like(a, idx.nlist))
    order = torch.argsort(key, stable=True)
    cnt = torch.bincount(key, minlength=idx.nlist + 1)
    add_start = torch.zeros(idx.nlist + 1, dtype=torch.int32, device=dev)
    add_start[1:] = torch.cumsum(cnt[:idx.nlist], 0)
    n_add = m - int(cnt[idx.nlist])
    order32 = order[:n_add].to(torch.int32)
    old_rows, old_ids, old_r_sq, kept_start = getattr(idx, name), idx.ids, idx.r_sq, idx.list_start
    new_start = kept_start + add_start
    n_old, n_new, id0 = idx.n_listed, idx.n_listed + n_add, idx.n_rows
    row_bytes = old_rows.shape[1] * old_rows.element_size()
    out = {}

    def launch():
        out["rows"] = torch.empty((n_new, old_rows.shape[1]), dtype=old_rows.dtype, device=dev)
        out["ids"] = torch.empty(n_new, dtype=torch.int32, device=dev)
        out["r_sq"] = torch.empty(n_new, dtype=torch.float32, device=dev)
        ops.ivf_lists_move(old_rows, old_ids, old_r_sq, None, payload, r_sq, order32, id0, kept_start, add_start, new_start,
                           out["rows"], out["ids"], out["r_sq"])

    # the torch alternative's map (not timed): destination position -> row of cat(old, chunk)
    lst = torch.repeat_interleave(torch.arange(idx.nlist, device=dev), (new_start[1:] - new_start[:-1]).long(), output_size=n_new)
    off = torch.arange(n_new, device=dev) - new_start[lst].long()
    kept_c = (kept_start[1:] - kept_start[:-1]).long()[lst]
    from_old = off < kept_c
    src_add = order[(add_start[lst].long() + off - kept_c).clamp(0, max(n_add - 1, 0))] + n_old
    mapping = torch.where(from_old, kept_start[lst].long() + off, src_add)
    add_ids = (id0 + torch.arange(m, device=dev)).to(torch.int32)
    del lst, off, kept_c, from_old, src_add
    alt = {}

    def plumbing():
        alt["rows"] = torch.cat([old_rows, payload]).index_select(0, mapping)
        alt["ids"] = torch.cat([old_ids, add_ids]).index_select(0, mapping)
        alt["r_sq"] = torch.cat([old_r_sq, r_sq]).index_select(0, mapping)

    res = {}
    for label, fn, keep in (("launch", launch, out), ("torch", plumbing, alt)):
        keep.clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ms = timed(fn, repeats)
        res[label + "_ms"] = ms
        res[label + "_peak_over_inputs_bytes"] = torch.cuda.max_memory_allocated(dev) - base
    res["equal"] = all(torch.equal(out[k], alt[k]) for k in ("rows", "ids", "r_sq"))
    res["bytes"] = 2 * n_new * (row_bytes + 8)
    res["n_new"], res["n_add"], res["row_bytes"], res["map_bytes"] = n_new, n_add, row_bytes, 8 * n_new
    for label in ("launch", "torch"):
        res[label + "_GBps"] = [res["bytes"] / (t * 1e-3) / 1e9 for t in res[label + "_ms"]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=343455)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=65536, help="rows train() sees")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--formats", nargs="*", default=["f32", "f16", "pq8", "pq4"], choices=["f32", "f16", "pq8", "pq4"])
    ap.add_argument("--pq-m", type=int, default=32)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_add_bench needs the GPU (there is no CPU path)")
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn, ops
    dev = torch.device("cuda:0")
    x = catalogue(args.n, args.dim, dev)
    x_host = x.cpu()
    sample = x[torch.randperm(args.n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:args.sample]].contiguous()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for fmt in args.formats:
        kw = {"f32": dict(storage="f32"), "f16": dict(storage="f16"),
              "pq8": dict(storage="pq", pq_m=args.pq_m, pq_bits=8, pq_iters=args.iters),
              "pq4": dict(storage="pq", pq_m=args.pq_m, pq_bits=4, pq_iters=args.iters)}[fmt]
        idx = knn.IVFIndex.train(sample, args.nlist, iters=args.iters, **kw)
        idx.add(x_host[:1024])                                # warm-up of every launch of the path
        totals, peaks, shots, shot_peaks, equal = [], [], [], [], []
        for rep in range(args.repeats):
            idx.reset()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            clock = StageClock()
            last = None
            for r0 in range(0, args.n, args.chunk):
                if r0 + args.chunk >= args.n:                 # the state before the last update, for move_alone
                    last = r0
                    break
                clock.start()
                idx.add(x_host[r0:r0 + args.chunk], block_rows=args.chunk, stages=clock)
            mv = move_alone(idx, x_host[last:], knn, ops, args.repeats) if rep == args.repeats - 1 else None
            torch.cuda.synchronize()
            clock.start()
            idx.add(x_host[last:], block_rows=args.chunk, stages=clock)
            st = clock.totals()
            peak = torch.cuda.max_memory_allocated(dev) - base if mv is None else None
            # the one-shot build of the same catalogue from device rows: the assignment call + from_assignment
            torch.cuda.synchronize()
            base2 = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            X = idx.prepare(x)
            _, Ia = knn.knn_search(idx._C, X, 1, l2_norm=False, device=dev, precision=idx.precision)
            del X
            fkw = dict(l2_norm=idx.l2_norm, precision=idx.precision, storage=idx.storage)
            if idx.storage == "pq":
                fkw.update(codebooks=idx.codebooks, pq_bits=idx.pq_bits)
            one = knn.IVFIndex.from_assignment(x, idx.centroids, Ia[:, 0], **fkw)
            b.record()
            torch.cuda.synchronize()
            shot_ms, shot_peak = a.elapsed_time(b), torch.cuda.max_memory_allocated(dev) - base2
            eq = same_index(idx, one)
            list_bytes = idx.n_listed * (getattr(idx, idx._payload_name()).shape[1] * getattr(idx, idx._payload_name()).element_size() + 8)
            del one, Ia
            rec = {"format": fmt, "repeat": rep, "n": args.n, "dim": args.dim, "nlist": args.nlist, "chunk": args.chunk,
                   "stages_ms": st, "add_total_ms": sum(st.values()), "add_peak_over_start_bytes": peak,
                   "one_shot_ms": shot_ms, "one_shot_peak_over_start_bytes": shot_peak, "equal_to_one_shot": eq,
                   "list_bytes": list_bytes, "n_listed": idx.n_listed}
            if mv is not None:
                rec["move_alone"] = mv
            emit(rec)
            totals.append(rec["add_total_ms"]), shots.append(shot_ms), equal.append(eq)
            if peak is not None:
                peaks.append(peak)
            shot_peaks.append(shot_peak)
        med = lambda v: sorted(v)[len(v) // 2]
        emit({"format": fmt, "summary": True, "add_total_ms_median": med(totals), "add_total_ms_min_max": [min(totals), max(totals)],
              "one_shot_ms_median": med(shots), "one_shot_ms_min_max": [min(shots), max(shots)],
              "add_peak_bytes_max": max(peaks) if peaks else None, "one_shot_peak_bytes_max": max(shot_peaks), "all_equal": all(equal)})


if __name__ == "__main__":
    main()
