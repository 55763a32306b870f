"""Write footprint of the two launches of the IVF index's update path (include/cdml_ivf_update.h) with tests/footprint.py's
poisoned, guarded buffers, under both poison patterns: the move stores every byte [0, row_bytes) of the rows [0, n_new) of the new
payload, every new id and r_sq, and nothing else -- not the row-stride gaps, not the rows past n_new, not the guards; the locate
stores exactly nq positions; every input comes back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import ivf_update_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu
PAST = 5                                 # rows of the new arrays past n_new: never written
GAP = 16                                 # bytes between two rows of the new payload


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.ops, ns.dev = ops, gpu
    return ns


def _dev(case, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {k: t(case[k]) for k in ("old_rows", "old_ids", "old_r_sq", "old_pos", "add_rows", "add_r_sq", "add_order", "kept_start",
                                    "add_start", "new_start")}


@pytest.mark.parametrize("row_bytes,drop", [(8, True), (24, False), (64, True), (6016, True)])
def test_lists_move_footprint(cd, row_bytes, drop):
    c = ur.move_case(3, row_bytes=row_bytes, drop=drop)
    d = _dev(c, cd.dev)
    n_new = c["n_new"]
    rows_mask = np.zeros((n_new + PAST, row_bytes), dtype=bool)
    rows_mask[:n_new] = True
    vec_mask = np.zeros(n_new + PAST, dtype=bool)
    vec_mask[:n_new] = True
    g_rows = fp.Guarded((n_new + PAST, row_bytes), torch.uint8, cd.dev, ld=row_bytes + GAP, mask=rows_mask)
    g_ids = fp.Guarded((n_new + PAST,), torch.int32, cd.dev, mask=vec_mask)
    g_rsq = fp.Guarded((n_new + PAST,), torch.float32, cd.dev, mask=vec_mask)
    inputs = [v for v in d.values() if v is not None]
    names = [k for k, v in d.items() if v is not None]

    def run(pattern):
        g_rows.rearm(pattern), g_ids.rearm(pattern), g_rsq.rearm(pattern)
        with fp.frozen(*inputs, names=names):
            cd.ops.ivf_lists_move(d["old_rows"], d["old_ids"], d["old_r_sq"], d["old_pos"], d["add_rows"], d["add_r_sq"],
                                  d["add_order"], c["id0"], d["kept_start"], d["add_start"], d["new_start"], g_rows.view[:n_new],
                                  g_ids.view, g_rsq.view)
            torch.cuda.synchronize()
        g_rows.assert_guards_intact("new_rows")                           # stride gaps, rows past n_new, guards
        g_ids.assert_guards_intact("new_ids")
        g_rsq.assert_guards_intact("new_r_sq")
        return {"rows": g_rows.payload(), "ids": g_ids.payload(), "r_sq": g_rsq.payload()}

    got = fp.assert_fully_written(run)
    assert np.array_equal(got["rows"].cpu().numpy().reshape(n_new, row_bytes), c["want_rows"])
    assert np.array_equal(got["ids"].cpu().numpy(), c["want_ids"])
    assert np.array_equal(got["r_sq"].cpu().numpy().view(np.uint32), c["want_r_sq"].view(np.uint32))


def test_locate_footprint(cd):
    c = ur.move_case(3, row_bytes=8, drop=True)
    n_rows = len(c["final_assign"])
    q = np.concatenate([np.arange(n_rows), [0, 5, 5, n_rows - 1]]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cd.dev)
    qd, ad, ids, start = t(q), t(c["final_assign"]), t(c["want_ids"]), t(c["new_start"])
    g_pos = fp.Guarded((len(q),), torch.int32, cd.dev)

    def run(pattern):
        g_pos.rearm(pattern)
        with fp.frozen(qd, ad, ids, start, names=["q_ids", "assign", "ids", "list_start"]):
            cd.ops.ivf_locate(qd, ad, ids, start, g_pos.view)
            torch.cuda.synchronize()
        g_pos.assert_guards_intact("pos")
        return {"pos": g_pos.payload()}

    got = fp.assert_fully_written(run)["pos"].cpu().numpy()
    assert np.array_equal(got, ur.locate(q, c["final_assign"], c["want_ids"], c["new_start"])) and (got == -1).any()
