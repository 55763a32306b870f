"""Host models of the IVF index's update launches (include/cdml_ivf_update.h): ``lists_move`` and ``locate`` in numpy, the
independent statement of what an updated index must hold (``truth``: a stable argsort of the FINAL catalogue by (assign, id)),
and the builders of the ragged cases the host and GPU tests share.  Plain module: no pytest, no torch, no GPU."""
import numpy as np

# the launch test's nine lists (tests/test_gpu_ivf_update.py): empty lists, a one-row list, lengths around a wave and a block
OLD_LENS = (0, 0, 1, 5, 64, 65, 0, 300, 2)
ADD_LENS = (0, 3, 0, 1, 64, 0, 0, 257, 1)
ROW_BYTES = (8, 16, 24, 40, 64, 128, 6016)


def starts(lens):
    """int32 [nlist + 1]: the exclusive scan of ``lens``"""
    out = np.zeros(len(lens) + 1, dtype=np.int32)
    out[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return out


def truth(payload, r_sq, assign, nlist):
    """(ids int32, list_start int32, rows, r_sq) of the catalogue ``payload`` [n, ...] under ``assign`` (-1 = unlisted): the rows
    sorted stably by (assign, id).  Knows nothing of old lists, chunks or maps."""
    a = np.asarray(assign, dtype=np.int64)
    key = np.where(a >= 0, a, nlist)
    order = np.argsort(key, kind="stable")
    n_listed = int((a >= 0).sum())
    ids = order[:n_listed]
    return ids.astype(np.int32), starts(np.bincount(key, minlength=nlist + 1)[:nlist]), payload[ids], np.asarray(r_sq)[ids]


def lists_move(old_rows, old_ids, old_r_sq, old_pos, add_rows, add_r_sq, add_order, id0, kept_start, add_start, new_start,
               added_first=False, ignore_old_pos=False, id_from_sorted=False):
    """(new_rows, new_ids, new_r_sq): the launch, destination position by destination position.  The three keyword flags are
    the single mutations the host test must see: a list's added rows placed before its kept rows, ``old_pos`` not applied,
    the id taken from the position in ``add_order`` instead of the chunk row."""
    nlist = len(new_start) - 1
    n_new = int(new_start[-1])
    like = old_rows if old_rows is not None and len(old_rows) else add_rows
    new_rows = np.zeros((n_new,) + tuple(like.shape[1:]), dtype=like.dtype)
    new_ids = np.full(n_new, -1, dtype=np.int32)
    new_r_sq = np.zeros(n_new, dtype=np.float32)
    for c in range(nlist):
        kept_c = int(kept_start[c + 1]) - int(kept_start[c])
        add_c = int(add_start[c + 1]) - int(add_start[c])
        for off in range(int(new_start[c + 1]) - int(new_start[c])):
            o = int(new_start[c]) + off
            if added_first:
                is_kept, koff, aoff = off >= add_c, off - add_c, off
            else:
                is_kept, koff, aoff = off < kept_c, off, off - kept_c
            if is_kept:
                p = int(kept_start[c]) + koff
                if old_pos is not None and not ignore_old_pos:
                    p = int(old_pos[p])
                new_rows[o], new_ids[o], new_r_sq[o] = old_rows[p], old_ids[p], old_r_sq[p]
            else:
                s = int(add_start[c]) + aoff
                j = int(add_order[s])
                new_rows[o], new_ids[o], new_r_sq[o] = add_rows[j], id0 + (s if id_from_sorted else j), add_r_sq[j]
    return new_rows, new_ids, new_r_sq


def locate(q_ids, assign, ids, list_start):
    """int32 [len]: the position of each id in its list (a binary search among the list's ascending ids), -1 where unlisted"""
    out = np.full(len(q_ids), -1, dtype=np.int32)
    for t, i in enumerate(np.asarray(q_ids, dtype=np.int64)):
        if not 0 <= i < len(assign) or not 0 <= assign[i] < len(list_start) - 1:
            continue
        lo, hi = int(list_start[assign[i]]), int(list_start[assign[i] + 1])
        p = lo + int(np.searchsorted(ids[lo:hi], i))
        if p < hi and ids[p] == i:
            out[t] = p
    return out


def move_case(seed, old_lens=OLD_LENS, add_lens=ADD_LENS, row_bytes=16, drop=False, old_unlisted=4, add_unlisted=3):
    """One update of a ragged index as the launch sees it, with its expected result from ``truth``.
    The old catalogue: sum(old_lens) listed rows in shuffled id order plus ``old_unlisted`` unlisted ids.  ``drop``: remove the
    first row of the first list with >= 3 rows, the last row of the next such list, the whole last non-empty list, and nothing
    else (so ``old_pos`` / ``kept_start`` are a real map); otherwise ``old_pos`` is None.  The chunk: sum(add_lens) rows for the
    lists in shuffled order plus ``add_unlisted`` rows in no list.  Payloads are random bytes [n, row_bytes], r_sq random fp32."""
    rng = np.random.RandomState(seed)
    nlist = len(old_lens)
    a_old = np.concatenate([np.repeat(np.arange(nlist), old_lens), np.full(old_unlisted, -1)]).astype(np.int64)
    rng.shuffle(a_old)
    n0 = len(a_old)
    cat_rows = rng.randint(0, 256, size=(n0, row_bytes)).astype(np.uint8)
    cat_rsq = rng.rand(n0).astype(np.float32)
    old_ids, old_start, old_rows, old_r_sq = truth(cat_rows, cat_rsq, a_old, nlist)
    a_kept = a_old.copy()
    old_pos = None
    kept_start = old_start
    dropped = np.zeros(0, dtype=np.int64)
    if drop:
        keep = np.ones(len(old_ids), dtype=bool)
        long_lists = [c for c in range(nlist) if old_lens[c] >= 3]
        whole = [c for c in range(nlist) if old_lens[c] > 0][-1]
        if len(long_lists) >= 2:
            keep[old_start[long_lists[0]]] = False                       # a list's first row
            keep[old_start[long_lists[1] + 1] - 1] = False               # a list's last row
        keep[old_start[whole]:old_start[whole + 1]] = False              # a whole list
        dropped = old_ids[~keep].astype(np.int64)
        a_kept[dropped] = -1
        old_pos = np.nonzero(keep)[0].astype(np.int32)
        cs = np.concatenate([[0], np.cumsum(keep)])
        kept_start = cs[old_start].astype(np.int32)
    a_add = np.concatenate([np.repeat(np.arange(nlist), add_lens), np.full(add_unlisted, -1)]).astype(np.int64)
    rng.shuffle(a_add)
    m = len(a_add)
    add_rows = rng.randint(0, 256, size=(m, row_bytes)).astype(np.uint8)
    add_r_sq = rng.rand(m).astype(np.float32)
    key = np.where(a_add >= 0, a_add, nlist)
    n_add = int((a_add >= 0).sum())
    add_order = np.argsort(key, kind="stable")[:n_add].astype(np.int32)
    add_start = starts(np.bincount(key, minlength=nlist + 1)[:nlist])
    new_start = (kept_start.astype(np.int64) + add_start).astype(np.int32)
    final_assign = np.concatenate([a_kept, a_add])
    want_ids, want_start, want_rows, want_r_sq = truth(np.concatenate([cat_rows, add_rows]), np.concatenate([cat_rsq, add_r_sq]),
                                                       final_assign, nlist)
    assert np.array_equal(want_start, new_start)
    return dict(nlist=nlist, row_bytes=row_bytes, old_rows=old_rows, old_ids=old_ids, old_r_sq=old_r_sq, old_start=old_start,
                old_pos=old_pos, kept_start=kept_start, add_rows=add_rows, add_r_sq=add_r_sq, add_order=add_order,
                add_start=add_start, new_start=new_start, id0=n0, n_new=int(new_start[-1]), dropped=dropped,
                final_assign=final_assign, want_rows=want_rows, want_ids=want_ids, want_r_sq=want_r_sq)


def model_of(case, **mutation):
    """``lists_move`` on a ``move_case``"""
    c = case
    return lists_move(c["old_rows"], c["old_ids"], c["old_r_sq"], c["old_pos"], c["add_rows"], c["add_r_sq"], c["add_order"], c["id0"],
                      c["kept_start"], c["add_start"], c["new_start"], **mutation)


def matches(got, case):
    return np.array_equal(got[0], case["want_rows"]) and np.array_equal(got[1], case["want_ids"]) \
        and np.array_equal(got[2].view(np.uint32), case["want_r_sq"].view(np.uint32))


# ---- the index fixture: D = 48, 7 lists from a hand-made assign with one empty list, 300 rows + a chunk of 130 -----------------
IDX_D, IDX_NLIST, IDX_N, IDX_CHUNK = 48, 7, 300, 130
IDX_EMPTY_LIST = 4
IDX_PQ_M = 8


def index_fixture(seed=11):
    """(x fp32 [300, 48], chunk fp32 [130, 48], centroids fp32 [7, 48], assign int64 [300]): Gaussian rows around seven
    centroids; ``assign`` is hand-made -- id % 7 with list 4 sent to list 5 (list 4 stays empty among the first 300 rows) and
    two ids unlisted -- since ``from_assignment`` takes any assignment.  The chunk's row 7 has a NaN coordinate and its row 9
    is 1e6 times a row (an fp16 overflow when the index does not normalise)."""
    rng = np.random.RandomState(seed)
    cent = rng.randn(IDX_NLIST, IDX_D).astype(np.float32)
    x = (cent[rng.randint(0, IDX_NLIST, IDX_N)] + 0.3 * rng.randn(IDX_N, IDX_D)).astype(np.float32)
    chunk = (cent[rng.randint(0, IDX_NLIST, IDX_CHUNK)] + 0.3 * rng.randn(IDX_CHUNK, IDX_D)).astype(np.float32)
    chunk[7, 5] = np.nan
    chunk[9] *= np.float32(1e6)
    assign = np.arange(IDX_N, dtype=np.int64) % IDX_NLIST
    assign[assign == IDX_EMPTY_LIST] = 5
    assign[[17, 203]] = -1
    return x, chunk, cent, assign
