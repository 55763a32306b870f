"""Mixed negative sampling of the N-pair loss, host side: the fp64 reference (tests/npair_mixed_ref.py) against autograd
and its two reductions, the C ABI of include/cdml_npair_mixed.h (names, argument checks without a GPU) and the refusals
of TrainStep / TrainConfig / NPairLoss."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_memory_ref  # noqa: E402
import npair_mixed_ref as ref  # noqa: E402
import npair_ref  # noqa: E402


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(rng, B=12, M=16, D=16):
    A, P, N = (_unit(rng.standard_normal((B, D))) for _ in range(3))
    ids3 = rng.choice(1000, size=3 * B, replace=False).astype(np.int64)
    ids3[3 * 2 + 2] = ids3[3 * 5]                        # n_2 is anchor 5's video
    ids3[3 * 4 + 2] = ids3[3 * 7 + 1]                    # n_4 is positive 7's video
    ids3[3 * 1 + 1] = ids3[3 * 3 + 1]                    # an in-batch duplicate
    ids3[3 * 6 + 2] = ids3[3 * 8 + 2]                    # the same video drawn twice: two columns
    mem = _unit(rng.standard_normal((M, D)))
    mem_id = rng.choice(np.arange(2000, 3000), size=M, replace=False)
    mem_id[[1, 5]] = -1
    mem_id[3] = ids3[3 * 9]
    return A, P, N, ids3, mem, mem_id


def _autograd(A, P, N, ids3, mem, mem_id, t, symmetric, bias, lq_u, mem_bias):
    B = A.shape[0]
    tA, tP, tN = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (A, P, N))
    ids2, _ = ref.split_ids(ids3, B)
    m, mc = (torch.as_tensor(x) for x in npair_ref.masks(ids2, B))
    cn = torch.as_tensor(ref.neg_mask(ids3, B))
    b = torch.zeros(B, 2, dtype=torch.float64) if bias is None else torch.as_tensor(bias, dtype=torch.float64).view(B, 2)
    lq_u = lq_u if bias is not None else 0.0
    ninf = -float("inf")
    S = tA @ tP.T / t
    cols = [(S - b[None, :, 1]).masked_fill(~m, ninf), (tA @ tN.T / t - lq_u).masked_fill(~cn, ninf)]
    if mem is not None:
        cm = torch.as_tensor(npair_memory_ref.mem_mask(ids2, mem_id, B))
        mb = torch.zeros(mem.shape[0], dtype=torch.float64) if (mem_bias is None or bias is None) else torch.as_tensor(mem_bias)
        cols.append((tA @ torch.as_tensor(mem).T / t - mb[None, :]).masked_fill(~cm, ninf))
    lr = torch.logsumexp(torch.cat(cols, 1), 1)
    d = torch.diagonal(S)
    loss = (lr - (d - b[:, 1])).mean()
    if symmetric:
        lc = torch.logsumexp((S - b[:, 0:1]).masked_fill(~mc, ninf), 0)
        loss = 0.5 * (loss + (lc - (d - b[:, 0])).mean())
    loss.backward()
    return loss.item(), tA.grad.numpy(), tP.grad.numpy(), tN.grad.numpy()


@pytest.mark.parametrize("with_logq", [False, True])
@pytest.mark.parametrize("with_mem", [False, True])
@pytest.mark.parametrize("symmetric", [True, False])
def test_reference_matches_float64_autograd(symmetric, with_mem, with_logq):
    rng = np.random.default_rng(3)
    A, P, N, ids3, mem, mem_id = _case(rng)
    if not with_mem:
        mem = mem_id = None
    bias = rng.normal(-6, 1, 2 * A.shape[0]) if with_logq else None
    mem_bias = rng.normal(-6, 1, 16) if (with_logq and with_mem) else None
    lq_u = -4.5 if with_logq else 0.0
    for t in (0.1, 1.0):
        r = ref.npair_mixed(A, P, N, ids3, t, symmetric, mem, mem_id, bias, lq_u, mem_bias)
        loss, gA, gP, gN = _autograd(A, P, N, ids3, mem, mem_id, t, symmetric, bias, lq_u, mem_bias)
        assert abs(r["loss"] - loss) < 1e-12
        for got, want in ((r["dA"], gA), (r["dP"], gP), (r["dN"], gN)):
            assert np.abs(got - want).max() < 1e-12
        assert np.abs(r["dN"]).max() > 0
        assert (r["W_n"][~r["cn"]] == 0).all() and int((~r["cn"]).sum()) >= 2
        B, M = A.shape[0], 0 if mem is None else mem.shape[0]
        n = (r["m"] & ~np.eye(B, dtype=bool)).sum() + r["cn"].sum() + (0 if mem is None else r["cm"].sum())
        assert abs(r["stats"][3] - n / (B * (B - 1) + B * B + B * M)) < 1e-15


@pytest.mark.parametrize("symmetric", [True, False])
def test_every_uniform_id_masked_is_the_unmixed_loss(symmetric):
    """n ids equal to the anchors' (every uniform column would be masked only for its own row) -- so give every anchor the
    same video id and every n that id: no uniform column counts anywhere, and the loss is npair_memory_ref's / npair_ref's."""
    rng = np.random.default_rng(5)
    A, P, N, ids3, mem, mem_id = _case(rng)
    B = A.shape[0]
    ids3 = ids3.reshape(B, 3).copy()
    ids3[:, 0] = 7777                                    # one anchor video; the column rule then masks every i != j too
    ids3[:, 2] = 7777                                    # every uniform negative is that video
    ids3 = ids3.reshape(-1)
    ids2, _ = ref.split_ids(ids3, B)
    r = ref.npair_mixed(A, P, N, ids3, 0.2, symmetric, mem, mem_id)
    want = npair_memory_ref.npair_memory(A, P, ids2, mem, mem_id, 0.2, symmetric)
    assert not r["cn"].any() and np.all(r["dN"] == 0) and np.all(r["W_n"] == 0)
    assert abs(r["loss"] - want["loss"]) < 1e-13
    assert np.abs(r["dA"] - want["dA"]).max() < 1e-13 and np.abs(r["dP"] - want["dP"]).max() < 1e-13
    r0 = ref.npair_mixed(A, P, N, ids3, 0.2, symmetric)
    want0 = npair_ref.npair(A, P, ids2, 0.2, symmetric)
    assert abs(r0["loss"] - want0["loss"]) < 1e-13
    assert np.abs(r0["dA"] - want0["dA"]).max() < 1e-13 and np.abs(r0["dP"] - want0["dP"]).max() < 1e-13
    assert np.all(r0["dN"] == 0)


@pytest.mark.parametrize("symmetric", [True, False])
def test_without_memory_the_uniform_rows_are_a_memory(symmetric):
    """M = 0: the uniform block's rule and formula are the memory block's, so the loss and dA equal npair_memory_ref's with
    the uniform rows as its "memory" (ids >= 0)."""
    rng = np.random.default_rng(6)
    A, P, N, ids3, _, _ = _case(rng)
    B = A.shape[0]
    ids2, nid = ref.split_ids(ids3, B)
    r = ref.npair_mixed(A, P, N, ids3, 0.1, symmetric)
    want = npair_memory_ref.npair_memory(A, P, ids2, N, nid, 0.1, symmetric)
    assert abs(r["loss"] - want["loss"]) < 1e-13
    assert np.abs(r["dA"] - want["dA"]).max() < 1e-13 and np.abs(r["dP"] - want["dP"]).max() < 1e-13
    assert np.abs(r["W_n"] - want["W_mem"]).max() < 1e-15
    assert np.abs(r["dN"] - want["W_mem"].T @ A).max() < 1e-13
    assert np.array_equal(r["cn"], want["cm"])


def _header_names(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_mixed_abi_names_header_table_and_library():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    names = _header_names(os.path.join(ROOT, "include", "cdml_npair_mixed.h"))
    assert len(names) == 5 and all(n.startswith("cdml_npair_mixed_") for n in names)
    assert sorted(_lib.SIGNATURES_MIXED) == names
    lib = _lib.load_library()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES_MIXED[n][1]
    main = open(os.path.join(ROOT, "include", "cdml.h")).read()
    assert "npair_mixed" not in main and not set(names) & set(_lib.SIGNATURES)
    assert lib.cdml_version() == 3000
    # the new source and header are part of the library's source id
    sid = _lib.source_id()
    assert lib.cdml_build_id().decode() == "CDML_BUILD_ID=" + sid
    assert os.path.exists(os.path.join(ROOT, "collaborative-deep-metric-learning_amd", "csrc", "npair_mixed.hip"))


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    assert lib.cdml_npair_mixed_workspace(8192, 16384) >= lib.cdml_npair_workspace(8192)
    assert lib.cdml_npair_mixed_workspace(0, 256) == 0 and lib.cdml_npair_mixed_workspace(256, -4) == 0
    p, odd = C.c_void_p(256), C.c_void_p(260)            # never dereferenced: every call below fails its checks first
    B, M = 256, 512
    K = 2 * B + M
    ws = lib.cdml_npair_mixed_workspace(B, M)
    st, gx, gf, sp = (lib.cdml_npair_mixed_stats, lib.cdml_npair_mixed_grad_x3, lib.cdml_npair_mixed_grad_f32,
                      lib.cdml_npair_mixed_split_x3)

    def stats(S=p, lds=K, ids=p, B=B, nc=B, mc=2 * B, mid=p, M=M, bias=None, lq=0.0, mb=None, t=0.1, lse=p, out=p, w=p, wb=ws):
        return st, (S, lds, ids, B, nc, mc, mid, M, bias, lq, mb, t, 1, lse, out, w, wb, None)

    def gradx(W=p, ldw=3 * K, plane=K, **kw):
        a = stats(**kw)[1]
        return gx, a[:14] + (W, ldw, plane, None)

    def gradf(W=p, ldw=K, **kw):
        a = stats(**kw)[1]
        return gf, a[:14] + (W, ldw, None)

    def split(e=p, lde=64, B=B, D=64, A3=p, lda=192, pa=64, R3=p, ldr=192, pr=64, T3=p, ldt=3 * K, pt=K, nr=B):
        return sp, (e, lde, B, D, A3, lda, pa, R3, ldr, pr, T3, ldt, pt, nr, None)

    cases = [
        (stats(S=None), b"null"), (stats(lse=None), b"null"), (stats(out=None), b"null"), (stats(w=None), b"null"),
        (stats(mid=None), b"mem_id"), (stats(B=0), b"B must be"), (stats(B=254), b"B must be"), (stats(M=510), b"memory size"),
        (stats(M=-4), b"memory size"), (stats(t=0.0), b"temperature"), (stats(t=float("nan")), b"temperature"),
        (stats(nc=B - 4), b"neg_col"), (stats(nc=B + 2), b"neg_col"), (stats(mc=2 * B - 4), b"mem_col"),
        (stats(lds=K - 4), b"lds"), (stats(S=odd), b"aligned"), (stats(ids=odd), b"aligned"), (stats(wb=ws - 4), b"workspace"),
        (stats(bias=odd, mb=p), b"bias"), (stats(bias=p, mb=None), b"mem_bias"), (stats(bias=p, mb=p, lq=float("inf")), b"lq_u"),
        (stats(M=0, mid=None, lds=2 * B - 4), b"lds"),
        (gradx(W=None), b"null"), (gradx(plane=K - 4), b"plane"), (gradx(ldw=3 * K - 4), b"ldw"), (gradx(t=-1.0), b"temperature"),
        (gradx(W=C.c_void_p(258)), b"aligned"),
        (gradf(W=None), b"null"), (gradf(ldw=K - 4), b"ldw"), (gradf(W=odd), b"aligned"), (gradf(M=502), b"memory size"),
        (split(e=None), b"null"), (split(T3=None), b"null"), (split(B=250), b"multiples of 4"), (split(D=62), b"multiples of 4"),
        (split(lde=60), b"lde"), (split(e=odd), b"lde"), (split(nr=B - 4), b"neg_row"), (split(pa=60), b"plane"),
        (split(lda=188), b"ld >="), (split(ldr=128), b"ld >="), (split(pt=2 * B - 4), b"plane_t"), (split(ldt=3 * K - 2 * M - 4), b"plane_t"),
        (split(A3=C.c_void_p(258)), b"aligned"),
    ]
    for (fn, args), msg in cases:
        assert fn(*args) == -1, args                      # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())


def test_train_step_config_and_loss_refusals(tmp_path):
    from cdml_amd import losses, train
    from cdml_amd.config import TrainConfig
    table = types.SimpleNamespace(n_rows_global=1000, data=torch.zeros(1), feature_size=8)
    pairs = torch.zeros((4, 2), dtype=torch.int32)
    mk = lambda **kw: train.TrainStep(table, pairs, 256, device="cpu", **kw)
    for mode in ("uniform", "inbatch", "semihard"):
        with pytest.raises(ValueError, match="mode 'npair'"):
            mk(mode=mode, uniform_negatives=True)
    with pytest.raises(ValueError, match="uniform_negatives=True"):
        mk(mode="npair", uniform_logq=-3.0, logq="stream")
    with pytest.raises(ValueError, match="logQ correction"):
        mk(mode="npair", uniform_negatives=True, uniform_logq=-3.0)
    with pytest.raises(ValueError, match="finite"):
        mk(mode="npair", uniform_negatives=True, logq="stream", uniform_logq=float("inf"))
    # everything mode "npair" refuses today is still refused with uniform negatives
    with pytest.raises(ValueError, match="one GPU"):
        mk(mode="npair", uniform_negatives=True, grad_sync=object())
    with pytest.raises(ValueError, match="train_table"):
        mk(mode="npair", uniform_negatives=True, train_table=True)
    with pytest.raises(ValueError, match="multiple of 256"):
        train.TrainStep(table, pairs, 192, device="cpu", mode="npair", precision="f32x3", uniform_negatives=True)
    with pytest.raises(ValueError, match="multiple of the batch"):
        mk(mode="npair", uniform_negatives=True, memory_size=384)
    with pytest.raises(ValueError, match="precision"):
        mk(mode="npair", uniform_negatives=True, precision="f16x2")
    c = TrainConfig(mode="npair", uniform_negatives=True, uniform_logq=-7.5, logq="stream", batch_size=8192)
    back = TrainConfig.from_json(c.to_json())
    assert back == c and back.uniform_negatives is True and back.uniform_logq == -7.5
    path = str(tmp_path / "c.json")
    c.to_json(path)
    assert TrainConfig.from_json(path) == c
    assert TrainConfig().uniform_negatives is False and TrainConfig().uniform_logq is None
    with pytest.raises(ValueError, match="mode 'npair'"):
        TrainConfig(mode="inbatch", uniform_negatives=True, batch_size=256).train_step(table, pairs, device="cpu")
    loss = losses.NPairLoss()
    x = torch.zeros((256, 2, 64))
    with pytest.raises(ValueError, match="go with negatives"):
        loss.calculate_loss(x, negative_ids=torch.zeros(256, dtype=torch.int32))
    with pytest.raises(ValueError, match="go with negatives"):
        loss.calculate_loss(x, negative_logq=-3.0)
    with pytest.raises(ValueError, match=r"\[batch, embedding\]"):
        loss.calculate_loss(x, negatives=torch.zeros((256, 32)))
    with pytest.raises(ValueError, match="multiple of 256"):
        loss.calculate_loss(torch.zeros((100, 2, 64)), negatives=torch.zeros((100, 64)))
    with pytest.raises(ValueError, match="go together"):
        loss.calculate_loss(x, negatives=torch.zeros((256, 64)), ids=torch.zeros((256, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="goes with logq"):
        loss.calculate_loss(x, negatives=torch.zeros((256, 64)), negative_logq=-3.0)


def test_default_uniform_logq():
    from cdml_amd import ops
    est = object.__new__(ops.LogQEstimator)             # (no device buffers: only the initial gap is read)
    est.init_gap = 125.0
    assert abs(ops.uniform_logq(est) - ref.default_uniform_logq(1000, 8, init_gap=125.0)) < 1e-12
    assert abs(ref.default_uniform_logq(1000, 8) + np.log(125.0)) < 1e-12
    tab = types.SimpleNamespace(n_videos=1000)
    assert abs(ops.uniform_logq(tab) - ref.default_uniform_logq(1000, 8, stream=False)) < 1e-12
    assert ops.uniform_logq(tab, -2.5) == -2.5 and ops.uniform_logq(None) == 0.0
    with pytest.raises(ValueError, match="logQ correction"):
        ops.uniform_logq(None, -2.5)
