"""Write footprint of the two filter scans of the IVF index (include/cdml_ivf_filter.h) with tests/footprint.py's poisoned,
guarded buffers, under both poison patterns: cnt[q] is the host model's count exactly; the first min(cnt, cap) candidate
slots of a query hold the model's set of (d, id) (any order; a query over its capacity: cap distinct members of the set);
the slots from min(cnt, cap) on, the guard bands and every input keep their bits.  tau is put halfway between two model
distances at least 1e-4 apart, so that fp32 rounding (BOUND below, some 8e-6) cannot flip a compare."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402
import ivf_f16_ref as f16  # noqa: E402
import ivf_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = (0, 1, 127, 130, 5, 300, 0)
NQ, NPROBE, D = 300, 3, 64
CAP = 64
Q_OVER, Q_NONE = 0, 1                    # a query over its capacity; a query with tau = -1
GAP = 1e-4
# s: D fused steps, each within half an ulp of a partial sum <= (1 + 2^-11)^2 (unit rows, fp16 rounding included); d = (q_sq
# + r_sq) - 2 s: the error of s twice, and two roundings of values below 4 (half an ulp = 2^-23 each)
BOUND = 2 * D * 2.0 ** -24 * (1 + 2.0 ** -11) ** 2 + 2 * 2.0 ** -23


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


@pytest.fixture(scope="module")
def case(cd):
    rng = np.random.RandomState(4)
    nlist, n = len(LENS), sum(LENS)
    x = rng.randn(n, D)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = rng.randn(NQ, D)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    assign = np.repeat(np.arange(nlist), LENS)
    rng.shuffle(assign)
    ids, start = ref.lists_from_assign(assign, nlist)
    probe = np.stack([rng.choice(nlist, size=NPROBE, replace=False) for _ in range(NQ)])
    for r in range(200):                                                  # two slot tiles on the 300-row list
        probe[r] = [5] + list(rng.choice([c for c in range(nlist) if c != 5], size=2, replace=False))
    probe[3] = -1
    probe[10:20, 2] = -1
    dev = cd.dev
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)

    class NS:
        pass
    c = NS()
    c.nlist, c.n, c.ids, c.start, c.probe = nlist, n, ids, start, probe
    c.tb = cd.knn.ivf_tables(t(probe, torch.int32), t(np.asarray(LENS), torch.int64))
    c.start_d, c.ids_d = t(start, torch.int32), t(ids, torch.int32)
    c.rows_of = [np.concatenate([ids[start[l]:start[l + 1]] for l in probe[i] if l >= 0] + [np.zeros(0, np.int64)]).astype(np.int64)
                 for i in range(NQ)]
    c.form = {}
    for form in ("f32", "f16"):
        f = NS()
        xv, qv = (f16.quantise(x).astype(np.float32), f16.quantise(q).astype(np.float32)) if form == "f16" else (x, q)
        dt = torch.float16 if form == "f16" else torch.float32
        f.Q, f.rows = t(qv, dt), t(xv[ids], dt)
        # the squared norms the kernel is given (fp32), and the model's distances from exactly those
        f.q_sq = (qv.astype(np.float64) ** 2).sum(1).astype(np.float32)
        r_sq_all = (xv.astype(np.float64) ** 2).sum(1).astype(np.float32)
        f.q_sq_d, f.r_sq_d = t(f.q_sq, torch.float32), t(r_sq_all[ids], torch.float32)
        d = (f.q_sq.astype(np.float64)[:, None] + r_sq_all.astype(np.float64)[None, :]) - 2.0 * qv.astype(np.float64) @ xv.astype(np.float64).T
        f.d = np.maximum(d, 0.0)
        # tau: halfway inside a gap >= GAP of the query's own sorted distances, some tens of rows in
        tau = np.full(NQ, -1.0)
        for i in range(NQ):
            ds = np.sort(f.d[i, c.rows_of[i]])
            want = 200 if i == Q_OVER else 5 + i % 40
            ok = np.nonzero(np.diff(ds) >= GAP)[0]
            ok = ok[ok >= min(want, len(ds) - 2)] if len(ds) > 1 else ok
            if i != Q_NONE and len(ok):
                tau[i] = 0.5 * (ds[ok[0]] + ds[ok[0] + 1])
        f.tau = tau.astype(np.float32)
        f.tau_d = t(f.tau, torch.float32)
        f.model = []
        for i in range(NQ):
            r = c.rows_of[i]
            sel = f.d[i, r] <= np.float64(f.tau[i])
            f.model.append((r[sel], f.d[i, r][sel]))
            # (the float32 image of tau is still well inside the gap)
            assert not len(r) or np.abs(f.d[i, r] - np.float64(f.tau[i])).min() >= GAP / 4
        c.form[form] = f
    return c


@pytest.mark.parametrize("form", ["f32", "f16"])
def test_filter_footprint(cd, case, form):
    c, f = case, case.form[form]
    tb = c.tb
    counts = np.array([len(m[0]) for m in f.model])
    assert counts[Q_OVER] > CAP and counts[Q_NONE] == 0 and counts[3] == 0 and (counts[2:] <= CAP).mean() > 0.9
    assert ((counts > 0) & (counts <= CAP)).sum() > NQ // 2
    gc = fp.Guarded((NQ, 2 * CAP), torch.int32, cd.dev)
    gn = fp.Guarded((NQ,), torch.int32, cd.dev)
    inputs = (f.Q, tb["slot_query"], tb["slot_start"], f.q_sq_d, f.tau_d, f.rows, c.start_d, f.r_sq_d, c.ids_d, tb["tiles"])
    names = ["Q", "slot_query", "slot_start", "q_sq", "tau", "rows", "list_start", "r_sq", "ids", "tiles"]
    launch = cd.ops.ivf_filter_f16 if form == "f16" else cd.ops.ivf_filter_f32
    worst = 0.0
    for pattern in range(fp.N_PATTERNS):
        gc.rearm(pattern), gn.rearm(pattern)
        gn.fill_from(torch.zeros(NQ, dtype=torch.int32))
        with fp.frozen(*inputs, names=names):
            launch(f.Q, tb["slot_query"], tb["slot_start"], f.q_sq_d, f.tau_d, gn.view, f.rows, c.start_d, f.r_sq_d, c.ids_d, tb["tiles"],
                   gc.view, CAP)
            torch.cuda.synchronize()
        gc.assert_guards_intact("cand"), gn.assert_guards_intact("cnt")
        cnt = gn.payload().cpu().numpy()
        assert np.array_equal(cnt, counts), np.nonzero(cnt != counts)[0][:10]
        cand = gc.payload().cpu().numpy().reshape(NQ, CAP, 2)
        poison = fp.poison_scalar(torch.int32, pattern)
        for i in range(NQ):
            m = min(int(cnt[i]), CAP)
            assert (cand[i, m:] == poison).all(), i                       # nothing behind the query's candidates
            got_id = cand[i, :m, 1].astype(np.int64)
            got_d = cand[i, :m, 0].copy().view(np.float32).astype(np.float64)
            want_id, want_d = f.model[i]
            o = np.argsort(got_id)
            if cnt[i] <= CAP:
                ow = np.argsort(want_id)
                assert np.array_equal(got_id[o], want_id[ow]), i
                if m:
                    worst = max(worst, np.abs(got_d[o] - want_d[ow]).max())
            else:
                assert len(set(got_id.tolist())) == CAP and set(got_id.tolist()) <= set(want_id.tolist())
                dist = dict(zip(want_id.tolist(), want_d.tolist()))
                worst = max(worst, max(abs(got_d[j] - dist[int(got_id[j])]) for j in range(m)))
    print("%s: max |d - fp64 model| = %.3g (bound %.3g)" % (form, worst, BOUND))
    assert worst <= BOUND
