"""The data-parallel N-pair loss, host side: the C ABI of include/cdml_npair_dp.h (names, argument checks without a GPU),
the fp64 model of its three phases (tests/npair_dp_ref.py) against the single-batch reference at the global batch, the
hook's collectives over two gloo ranks, and TrainStep's refusals."""
import ctypes as C
import os
import re
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_dp_ref  # noqa: E402
import npair_ref  # noqa: E402


def _header_names(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_dp_abi_names_header_table_and_library():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    names = _header_names(os.path.join(ROOT, "include", "cdml_npair_dp.h"))
    assert len(names) == 7 and all(n.startswith("cdml_npair_dp_") for n in names)
    assert sorted(_lib.SIGNATURES_DP) == names
    lib = _lib.load_library()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES_DP[n][1]
    main = open(os.path.join(ROOT, "include", "cdml.h")).read()
    assert "npair_dp" not in main and not set(names) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_MIXED))
    assert lib.cdml_build_id().decode() == "CDML_BUILD_ID=" + _lib.source_id()
    assert os.path.exists(os.path.join(ROOT, "collaborative-deep-metric-learning_amd", "csrc", "npair_dp.hip"))


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    B, G = 256, 512
    ws = lib.cdml_npair_dp_workspace(B, G)
    assert ws >= 4 * (4 * B + 2 * G) and lib.cdml_npair_dp_workspace(0, G) == 0 and lib.cdml_npair_dp_workspace(B, B - 4) == 0
    p, odd = C.c_void_p(256), C.c_void_p(260)            # never dereferenced: every call below fails its checks first

    def local(S=p, lds=G, ids=p, B=B, G=G, col0=B, t=0.1, sym=1, lse=p, cp=p, w=p, wb=ws):
        return lib.cdml_npair_dp_local_stats, (S, lds, ids, B, G, col0, t, sym, lse, cp, w, wb, None)

    def stats(S=p, lds=G, B=B, G=G, col0=B, t=0.1, sym=1, lc=p, st=p, w=p, wb=ws):
        return lib.cdml_npair_dp_stats, (S, lds, B, G, col0, t, sym, lc, st, w, wb, None)

    def gradx(S=p, lds=G, ids=p, B=B, G=G, col0=B, t=0.1, sym=1, lr=p, lc=p, W=p, ldw=3 * G, plane=G):
        return lib.cdml_npair_dp_grad_x3, (S, lds, ids, B, G, col0, t, sym, lr, lc, W, ldw, plane, None)

    def gradf(S=p, lds=G, ids=p, B=B, G=G, col0=B, t=0.1, sym=1, lr=p, lc=p, W=p, ldw=G):
        return lib.cdml_npair_dp_grad_f32, (S, lds, ids, B, G, col0, t, sym, lr, lc, W, ldw, None)

    def fold(cp=p, world=2, G=G, lc=p):
        return lib.cdml_npair_dp_col_fold, (cp, world, G, lc, None)

    def pos(recv=p, ldr=64, world=2, B=B, D=64, de=p, ldde=64):
        return lib.cdml_npair_dp_pos_fold, (recv, ldr, world, B, D, de, ldde, None)

    cases = [
        (local(S=None), b"null"), (local(lse=None), b"null"), (local(cp=None), b"null"), (local(w=None), b"null"),
        (local(B=0), b"B >= 1"), (local(G=B - 4), b"G >= B"), (local(G=G + 2, lds=G + 4), b"multiple of 4"),
        (local(col0=-4), b"col0"), (local(col0=B + 4), b"col0"), (local(col0=2), b"col0"), (local(t=0.0), b"temperature"),
        (local(t=float("nan")), b"temperature"), (local(lds=G - 4), b"lds"), (local(S=odd), b"aligned"),
        (local(ids=odd), b"aligned"), (local(cp=odd), b"aligned"), (local(wb=ws - 4), b"workspace"),
        (stats(st=None), b"null"), (stats(lc=None), b"null"), (stats(wb=0), b"workspace"), (stats(col0=G), b"col0"),
        (gradx(W=None), b"null"), (gradx(lr=None), b"null"), (gradx(lc=None), b"null"), (gradx(plane=G - 4), b"plane"),
        (gradx(ldw=3 * G - 4), b"ldw"), (gradx(W=C.c_void_p(258)), b"aligned"), (gradx(t=-1.0), b"temperature"),
        (gradf(W=None), b"null"), (gradf(ldw=G - 4), b"ldw"), (gradf(W=odd), b"aligned"), (gradf(lc=odd), b"aligned"),
        (fold(cp=None), b"null"), (fold(world=0), b"world"), (fold(G=0), b"G >= 1"), (fold(cp=odd), b"aligned"),
        (pos(recv=None), b"null"), (pos(D=62), b"multiple of 4"), (pos(ldr=60), b"leading"), (pos(ldde=60), b"leading"),
        (pos(de=odd), b"aligned"), (pos(world=0), b"world"),
    ]
    for (fn, args), msg in cases:
        assert fn(*args) == -1, args                      # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())
    # the asymmetric loss takes no column buffers
    fn, args = local(sym=0, cp=None, wb=0)
    assert fn(*args) == -1 and b"workspace" in lib.cdml_last_error()


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(G, D, seed):
    rng = np.random.default_rng(seed)
    A = _unit(rng.standard_normal((G, D)))
    P = _unit(A + 0.6 * rng.standard_normal((G, D)))
    ids = rng.choice(50 * G, size=2 * G, replace=False).astype(np.int64)
    ids[2 * 1 + 1] = ids[2 * (G - 2) + 1]                # a positive of the first rank again on the last
    ids[2 * 0] = ids[2 * (G - 1) + 1]                    # an anchor of the first rank = a positive of the last
    ids[2 * 3 + 1] = ids[2 * 4 + 1]                      # a duplicate inside one rank
    ids[6] = ids[7]                                      # a pair whose rows are one video
    return A, P, ids


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_three_phase_model_is_the_single_batch_loss_at_G(world, symmetric):
    G, D, t = 12 * world, 8, 0.2
    A, P, ids = _case(G, D, seed=world)
    want = npair_ref.npair(A, P, ids, t, symmetric)
    got = npair_dp_ref.npair_dp(A, P, ids, world, t, symmetric)
    B = G // world
    assert abs(np.mean(got["loss"]) - want["loss"]) < 1e-13
    assert np.abs(np.concatenate(got["lse_row"]) - want["lse_row"]).max() < 1e-13
    if symmetric:
        assert np.abs(got["lse_col"] - want["lse_col"]).max() < 1e-13
    # the local-mean scale: world x the global mean's gradient, which the gradient average over the ranks divides out
    assert np.abs(np.concatenate(got["W"]) - world * want["W"]).max() < 1e-13
    assert np.abs(np.concatenate(got["dA"]) - world * want["dA"]).max() < 1e-12
    assert np.abs(np.concatenate(got["dP"]) - world * want["dP"]).max() < 1e-12
    dead = (~want["m"] & ~want["mc"]) if symmetric else ~want["m"]
    assert int(dead.sum()) > 0 and (np.concatenate(got["W"])[dead] == 0).all()
    for r in range(world):
        m = want["m"][r * B:(r + 1) * B]
        assert abs(got["stats"][r][3] - (m.sum() - B) / (B * (G - 1))) < 1e-15
        assert abs(got["stats"][r][0] - got["loss"][r]) == 0


def test_fold_model_handles_empty_partials():
    cp = np.zeros((3, 4, 2))
    cp[:, :, 0] = [[-np.inf, 0.5, 1.0, -np.inf], [0.25, -np.inf, 2.0, -np.inf], [1.5, 0.75, -np.inf, -np.inf]]
    cp[:, :, 1] = np.where(np.isfinite(cp[:, :, 0]), 1.5, 0.0)
    got = npair_dp_ref.fold(cp)
    want = [np.log(1.5 * np.exp(0.25) + 1.5 * np.exp(1.5)), np.log(1.5 * np.exp(0.5) + 1.5 * np.exp(0.75)),
            np.log(1.5 * np.exp(1.0) + 1.5 * np.exp(2.0))]
    assert np.abs(got[:3] - want).max() < 1e-14 and got[3] == -np.inf and not np.isnan(got).any()


def _sync_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cdml_amd import dist as cdist
        sync = cdist.NPairSync(group=dist.new_group())
        assert (sync.world, sync.rank) == (world, rank)
        B, D = 3, 4
        inp = torch.arange(B * D, dtype=torch.float32).view(B, D) + 100.0 * rank
        out = torch.full((world * B, D), -1.0)
        sync.all_gather(out, inp)
        ids = torch.arange(2 * B, dtype=torch.int32) + 1000 * rank          # an int32 payload survives as bits
        wire = torch.zeros(world * B, 2)
        sync.all_gather(wire, ids.view(B, 2).view(torch.float32))
        cp = torch.full((5, 2), float(rank))
        cp[0, 0] = -float("inf")
        cpa = torch.zeros(world, 5, 2)
        sync.all_gather(cpa, cp)
        send = torch.stack([torch.full((B, D), 10.0 * rank + s) for s in range(world)]).view(world * B, D)   # block s -> rank s
        recv = torch.zeros(world, B, D)
        sync.all_to_all(recv, send)
        q.put((rank, "ok", out.numpy(), wire.view(torch.int32).numpy(), cpa.numpy(), recv.numpy()))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None, None, None, None))
    finally:
        dist.destroy_process_group()


def test_npair_sync_collectives_over_two_gloo_ranks():
    world, B, D = 2, 3, 4
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sync_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in res:
        assert r[1] == "ok", "rank %d: %s" % (r[0], r[1])
    base = np.arange(B * D, dtype=np.float32).reshape(B, D)
    for rank, _, out, wire, cpa, recv in res:
        np.testing.assert_array_equal(out, np.concatenate([base + 100.0 * s for s in range(world)]))
        np.testing.assert_array_equal(wire.reshape(-1), np.concatenate([np.arange(2 * B) + 1000 * s for s in range(world)]))
        for s in range(world):
            assert cpa[s, 0, 0] == -np.inf and (cpa[s, 1:] == s).all() and cpa[s, 0, 1] == s
            assert (recv[s] == 10.0 * s + rank).all()      # block `rank` of rank s's send buffer


def test_train_step_refusals():
    from cdml_amd import train
    table = types.SimpleNamespace(n_rows_global=1000, data=torch.zeros(1), feature_size=8)
    pairs = torch.zeros((4, 2), dtype=torch.int32)
    sync = types.SimpleNamespace(world=2, rank=1, group=None)
    mk = lambda B=256, **kw: train.TrainStep(table, pairs, B, device="cpu", **dict(dict(slot0=B, batch_global=2 * B), **kw))
    for mode in ("uniform", "inbatch", "semihard"):
        with pytest.raises(ValueError, match="npair_sync goes with mode 'npair'"):
            mk(mode=mode, npair_sync=sync)
    with pytest.raises(ValueError, match="memory_size"):
        mk(mode="npair", npair_sync=sync, memory_size=512)
    with pytest.raises(ValueError, match="logq"):
        mk(mode="npair", npair_sync=sync, logq="stream")
    with pytest.raises(ValueError, match="uniform_negatives"):
        mk(mode="npair", npair_sync=sync, uniform_negatives=True)
    with pytest.raises(ValueError, match="train_table"):
        mk(mode="npair", npair_sync=sync, train_table=True)
    with pytest.raises(ValueError, match="batch_global"):
        mk(mode="npair", npair_sync=sync, batch_global=256)
    with pytest.raises(ValueError, match="slot0"):
        mk(mode="npair", npair_sync=sync, slot0=0)
    with pytest.raises(ValueError, match="multiple of 256"):
        mk(B=320, mode="npair", npair_sync=sync, precision="f32x3")
    with pytest.raises(ValueError, match="multiple of 64"):
        mk(B=100, mode="npair", npair_sync=sync)
    # without the hook the loss still refuses data parallelism
    for kw in (dict(exchange=object()), dict(grad_sync=object()), dict(exchange=object(), grad_sync=object())):
        with pytest.raises(ValueError, match="one GPU"):
            mk(mode="npair", **kw)
