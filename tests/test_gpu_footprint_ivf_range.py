"""Write footprint of the two filter scans over product-quantised lists (include/cdml_ivf_range.h) with tests/footprint.py's
poisoned, guarded buffers, under both poison patterns, on an exact integer case (tests/ivf_range_ref.py's tile case: every
distance an fp32 number, so the comparison is of bits): cnt[q] is the host model's count exactly; the first min(cnt, cap)
candidate slots of a query hold the model's set of (d, id) (any order; a query over its capacity: cap distinct members of the
set); nothing for tau = -1; the slots from min(cnt, cap) on, the guard bands and every input keep their bits."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import ivf_range_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
M, CAP = 16, 64
Q_OVER, Q_NONE = 0, 2                     # a query over its capacity (it probes the longest list); a query with tau = -1


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import knn, ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.dev = knn, ops, gpu
    return ns


@pytest.mark.parametrize("residual", [False, True])
def test_filter_pq_footprint(cd, residual):
    S, R = cd.ops.ivf_pq_tile(M)
    c = rr.tile_case(M, math.lcm(2 * M, 32), S, R, residual, tag="ivfrange-footprint")
    dev, nq = cd.dev, c["nq"]
    idx = cd.knn.IVFIndex.from_assignment(torch.from_numpy(c["x"]), torch.from_numpy(c["c"]), torch.from_numpy(c["assign"]),
                                          l2_norm=False, device=dev, storage="pq", codebooks=torch.from_numpy(c["cb"]),
                                          pq_residual=residual)
    probe = c["probe"]
    tau = rr.gap_radius(c["d"], c["assign"], c["nlist"], probe, 20)
    tau[Q_OVER], tau[Q_NONE] = np.inf, -1.0
    model = rr.range_search(c["d"], c["assign"], c["nlist"], probe, tau)
    counts = np.diff(model[0])
    assert counts[Q_OVER] > 2 * R > CAP and counts[Q_NONE] == 0 and ((counts > 0) & (counts <= CAP)).sum() > nq // 2
    Q = torch.from_numpy(c["q"]).to(dev)
    q_sq = torch.zeros(nq, dtype=torch.float32, device=dev)
    cd.ops.row_sqnorm(Q, Q.shape[1], q_sq)
    tau_d = torch.from_numpy((tau * c["unit"]).astype(np.float32)).to(dev)
    tb = cd.knn.ivf_tables(torch.from_numpy(probe).to(torch.int32).to(dev), idx.list_len, tile_slots=S, tile_rows=R)
    lut = torch.empty((nq, M, 256), dtype=torch.float32, device=dev)
    cd.ops.pq_lut(Q, idx.codebooks, lut)
    inputs = [lut, tb["slot_query"], tb["slot_start"], q_sq, tau_d, idx.codes, idx.list_start, idx.r_sq, idx.ids, tb["tiles"]]
    names = ["lut", "slot_query", "slot_start", "q_sq", "tau", "codes", "list_start", "r_sq", "ids", "tiles"]
    if residual:
        slot_base = torch.empty(tb["n_slots"], dtype=torch.float32, device=dev)
        cd.ops.ivf_slot_dots(Q, idx._C, tb["slot_query"], tb["slot_start"], slot_base)
        inputs.append(slot_base)
        names.append("slot_base")
    gc = fp.Guarded((nq, 2 * CAP), torch.int32, dev)
    gn = fp.Guarded((nq,), torch.int32, dev)
    for pattern in range(fp.N_PATTERNS):
        gc.rearm(pattern), gn.rearm(pattern)
        gn.fill_from(torch.zeros(nq, dtype=torch.int32))
        with fp.frozen(*inputs, names=names):
            if residual:
                cd.ops.ivf_filter_pqr(lut, tb["slot_query"], tb["slot_start"], slot_base, q_sq, tau_d, gn.view, idx.codes,
                                      idx.list_start, idx.r_sq, idx.ids, tb["tiles"], gc.view, CAP)
            else:
                cd.ops.ivf_filter_pq(lut, tb["slot_query"], tb["slot_start"], q_sq, tau_d, gn.view, idx.codes, idx.list_start,
                                     idx.r_sq, idx.ids, tb["tiles"], gc.view, CAP)
            torch.cuda.synchronize()
        gc.assert_guards_intact("cand"), gn.assert_guards_intact("cnt")
        cnt = gn.payload().cpu().numpy()
        assert np.array_equal(cnt, counts), np.nonzero(cnt != counts)[0][:10]
        cand = gc.payload().cpu().numpy().reshape(nq, CAP, 2)
        poison = fp.poison_scalar(torch.int32, pattern)
        for i in range(nq):
            m = min(int(cnt[i]), CAP)
            assert (cand[i, m:] == poison).all(), i                       # nothing behind the query's candidates
            got = sorted(zip(cand[i, :m, 1].tolist(), cand[i, :m, 0].tolist()))
            want_id = model[2][model[0][i]:model[0][i + 1]]
            want_d = (model[1][model[0][i]:model[0][i + 1]].astype(np.float64) * c["unit"]).astype(np.float32).view(np.int32)
            want = sorted(zip(want_id.tolist(), want_d.tolist()))
            if cnt[i] <= CAP:
                assert got == want, i                                     # the model's set: ids and the bits of d
            else:
                assert len({g[0] for g in got}) == CAP and set(got) <= set(want), i
