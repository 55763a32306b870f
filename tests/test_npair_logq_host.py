"""The N-pair loss's sampling-bias (logQ) correction without a GPU: the fp64 reference against float64 autograd (with
and without a cross-batch memory), the softmax's shift invariance, the estimator's host model, the C ABI's argument checks
and the configuration's JSON round trip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_logq_ref as ref  # noqa: E402
import npair_memory_ref  # noqa: E402
import npair_ref  # noqa: E402


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(rng, B=12, M=16, D=16):
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.5 * rng.standard_normal((B, D)))
    ids = rng.choice(10 * B, size=2 * B, replace=False).astype(np.int64)
    ids[1] = ids[5]                                  # in-batch duplicates
    ids[6] = ids[3]
    bias = rng.uniform(-12.0, 0.0, 2 * B)            # heavy skew
    mem = _unit(rng.standard_normal((M, D)))
    mem_id = rng.choice(np.arange(10 * B, 20 * B), size=M, replace=False).astype(np.int64)
    mem_id[[2, 9]] = -1
    mem_id[4] = ids[2 * 3]
    mem_bias = rng.uniform(-12.0, 0.0, M)
    return A, P, ids, bias, mem, mem_id, mem_bias


def _autograd(A, P, ids, bias, t, symmetric, mem=None, mem_id=None, mem_bias=None):
    B = A.shape[0]
    m, mc = (torch.from_numpy(x) for x in npair_ref.masks(ids, B))
    b = torch.as_tensor(bias, dtype=torch.float64).view(B, 2)
    S = A @ P.T / t
    X = (S - b[:, 1][None, :]).masked_fill(~m, -float("inf"))
    dr = torch.diagonal(S) - b[:, 1]
    if mem is not None:
        cm = torch.from_numpy(npair_memory_ref.mem_mask(ids, mem_id, B))
        Xm = (A @ mem.T / t - torch.as_tensor(mem_bias)[None, :]).masked_fill(~cm, -float("inf"))
        X = torch.cat([X, Xm], 1)
    L = (torch.logsumexp(X, 1) - dr).mean()
    if symmetric:
        Xc = (S - b[:, 0][:, None]).masked_fill(~mc, -float("inf"))
        L = 0.5 * (L + (torch.logsumexp(Xc, 0) - (torch.diagonal(S) - b[:, 0])).mean())
    return L


@pytest.mark.parametrize("with_mem", [False, True])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("with_ids", [True, False])
@pytest.mark.parametrize("t", [0.05, 1.0])
def test_reference_matches_float64_autograd(with_mem, symmetric, with_ids, t):
    rng = np.random.default_rng(17)
    A, P, ids, bias, mem, mem_id, mem_bias = _case(rng)
    ids = ids if with_ids else None
    kw = dict(mem=mem, mem_id=mem_id, mem_bias=mem_bias) if with_mem else {}
    r = ref.npair_logq(A, P, ids, bias, t, symmetric, **kw)
    ta, tp = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (A, P))
    tkw = dict(mem=torch.tensor(mem), mem_id=mem_id, mem_bias=mem_bias) if with_mem else {}
    L = _autograd(ta, tp, ids, bias, t, symmetric, **tkw)
    L.backward()
    assert abs(L.item() - r["loss"]) < 1e-12
    np.testing.assert_allclose(r["dA"], ta.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(r["dP"], tp.grad.numpy(), atol=1e-12)
    assert (r["W"][~(r["m"] | r["mc"])] == 0).all()                # the masks are unchanged by the bias


def test_zero_bias_is_the_uncorrected_loss():
    rng = np.random.default_rng(3)
    A, P, ids, bias, mem, mem_id, mem_bias = _case(rng)
    for symmetric in (True, False):
        r = ref.npair_logq(A, P, ids, np.zeros_like(bias), 0.1, symmetric)
        r0 = npair_ref.npair(A, P, ids, 0.1, symmetric)
        assert abs(r["loss"] - r0["loss"]) < 1e-12
        np.testing.assert_allclose(r["dA"], r0["dA"], atol=1e-12)
        rm = ref.npair_logq(A, P, ids, np.zeros_like(bias), 0.1, symmetric, mem, mem_id, np.zeros_like(mem_bias))
        rm0 = npair_memory_ref.npair_memory(A, P, ids, mem, mem_id, 0.1, symmetric)
        assert abs(rm["loss"] - rm0["loss"]) < 1e-12
        np.testing.assert_allclose(rm["dA"], rm0["dA"], atol=1e-12)
        np.testing.assert_allclose(rm["dP"], rm0["dP"], atol=1e-12)


@pytest.mark.parametrize("c", [-7.25, 0.0, 3.0])
def test_constant_lq_changes_nothing(c):
    """softmax shift invariance: the same lq for every candidate leaves loss and gradient as they are"""
    rng = np.random.default_rng(4)
    A, P, ids, bias, mem, mem_id, mem_bias = _case(rng)
    for symmetric in (True, False):
        r = ref.npair_logq(A, P, ids, np.full_like(bias, c), 0.1, symmetric, mem, mem_id, np.full_like(mem_bias, c))
        r0 = npair_memory_ref.npair_memory(A, P, ids, mem, mem_id, 0.1, symmetric)
        assert abs(r["loss"] - r0["loss"]) < 1e-12
        np.testing.assert_allclose(r["dA"], r0["dA"], atol=1e-12)
        np.testing.assert_allclose(r["dP"], r0["dP"], atol=1e-12)
        np.testing.assert_allclose(r["lse_row"], r0["lse_row"] - c, atol=1e-12)


def test_skewed_lq_moves_the_loss():
    rng = np.random.default_rng(5)
    A, P, ids, bias, *_ = _case(rng)
    r, r0 = ref.npair_logq(A, P, ids, bias, 0.1, True), npair_ref.npair(A, P, ids, 0.1, True)
    assert abs(r["loss"] - r0["loss"]) > 1e-3


def test_estimator_host_model():
    n, B, a = 10, 4, 0.25
    g0 = ref.default_gap(n, B)
    assert g0 == 2.5 and ref.default_gap(3, 8) == 1.0
    steps = [[1, 1, 3, 20],                          # a duplicate within the batch, an id outside [0, n)
             [1, 5, 5, 5],
             [3, -1, 9, 1],
             [7, 7, 7, 7]]
    last, gap = ref.estimator_after(steps, n, B, a)
    assert last.dtype == np.int32 and gap.dtype == np.float32
    assert list(last) == [-1, 2, -1, 2, -1, 1, -1, 3, -1, 2]
    f = np.float32
    g1 = f(f(f(0.75) * f(2.5)) + f(f(0.25) * f(1.0)))        # video 1: first seen at 0, then at 1 and 2
    g1 = f(f(f(0.75) * g1) + f(f(0.25) * f(1.0)))
    assert gap[1] == g1
    assert gap[3] == f(f(f(0.75) * f(2.5)) + f(f(0.25) * f(2.0)))   # video 3: steps 0 and 2
    for v in (5, 7, 9):                                       # first sightings keep g0
        assert gap[v] == f(2.5)
    assert gap[0] == f(2.5) and last[0] == -1
    # the rounding rule: each product and sum rounded to float32 on its own (not one rounding of the exact value)
    a = 0.1
    steps = [[0], [0], [0], [0], [0], [0]]
    _, gap = ref.estimator_after(steps, 1, 1, a, g0=3.0)
    g, x = f(3.0), 3.0
    for _ in range(5):
        g = f(f(f(1.0) - f(a)) * g) + f(f(a) * f(1.0))
        x = (1 - float(f(a))) * x + float(f(a))
    assert gap[0] == g and float(gap[0]) != x
    # t0: the host model's step numbers
    last, _ = ref.estimator_after([[2], [2]], 4, 1, 0.5, g0=1.0, t0=10)
    assert last[2] == 11


def test_logq_abi_exported_and_checked_without_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    names = ("cdml_npair_logq_stats", "cdml_npair_logq_grad_x3", "cdml_npair_logq_grad_f32", "cdml_npair_memory_logq_stats",
             "cdml_npair_memory_logq_grad_x3", "cdml_npair_memory_logq_grad_f32", "cdml_logq_table_gather",
             "cdml_logq_stream_gather", "cdml_logq_stream_update", "cdml_logq_stream_reset")
    for name in names:
        assert name in _lib.SIGNATURES
    lib = _lib.load_library()
    assert lib.cdml_version() == 3000
    p, odd = C.c_void_p(256), C.c_void_p(258)           # never dereferenced: every call below fails its checks first
    ws = lib.cdml_npair_workspace(256)
    K = 768
    st, gx, gf = lib.cdml_npair_logq_stats, lib.cdml_npair_logq_grad_x3, lib.cdml_npair_logq_grad_f32
    mst, mgx, mgf = lib.cdml_npair_memory_logq_stats, lib.cdml_npair_memory_logq_grad_x3, lib.cdml_npair_memory_logq_grad_f32
    tg, sg, su, sr = lib.cdml_logq_table_gather, lib.cdml_logq_stream_gather, lib.cdml_logq_stream_update, \
        lib.cdml_logq_stream_reset
    cases = [
        (st, (p, 256, p, 256, None, 0.1, 1, p, p, p, ws, None), b"bias"),
        (st, (p, 256, p, 256, odd, 0.1, 1, p, p, p, ws, None), b"bias"),
        (st, (None, 256, p, 256, p, 0.1, 1, p, p, p, ws, None), b"null"),
        (st, (p, 256, p, 256, p, float("inf"), 1, p, p, p, ws, None), b"temperature"),
        (st, (p, 256, p, 256, p, 0.1, 1, p, p, p, ws - 4, None), b"workspace"),
        (st, (p, 252, p, 256, p, 0.1, 1, p, p, p, ws, None), b"lds"),
        (gx, (p, 256, p, 256, None, 0.1, 1, p, p, 768, 256, None), b"bias"),
        (gx, (p, 256, p, 256, p, 0.1, 1, p, p, 764, 256, None), b"ldw"),
        (gx, (p, 256, p, 256, p, float("nan"), 1, p, p, 768, 256, None), b"temperature"),
        (gf, (p, 256, p, 256, None, 0.1, 1, p, p, 256, None), b"bias"),
        (gf, (p, 256, p, 256, p, 0.1, 1, p, None, 256, None), b"null"),
        (mst, (p, K, p, 256, p, 256, p, None, 512, 0.1, 1, p, p, p, ws, None), b"mem_bias"),
        (mst, (p, K, p, 256, p, 256, p, C.c_void_p(260), 512, 0.1, 1, p, p, p, ws, None), b"mem_bias"),
        (mst, (p, K, p, 256, None, 256, p, p, 512, 0.1, 1, p, p, p, ws, None), b"bias"),
        (mst, (p, K, p, 256, p, 256, p, p, 510, 0.1, 1, p, p, p, ws, None), b"memory size"),
        (mgx, (p, K, p, 256, 256, p, None, 512, 0.1, 1, p, p, 3 * K, K, None), b"mem_bias"),
        (mgx, (p, K, p, 256, 256, p, p, 512, 0.1, 1, p, p, 3 * K, K - 4, None), b"plane"),
        (mgf, (p, K, p, 256, 256, p, None, 512, 0.1, 1, p, p, K, None), b"mem_bias"),
        (mgf, (p, K, p, 256, 256, p, p, 512, -0.1, 1, p, p, K, None), b"temperature"),
        (tg, (None, 100, p, 256, None, 0, p, None, None), b"table"),
        (tg, (p, 0, p, 256, None, 0, p, None, None), b"n_videos"),
        (tg, (p, 2 ** 31, p, 256, None, 0, p, None, None), b"n_videos"),
        (tg, (p, 100, None, 256, None, 0, p, None, None), b"null"),
        (tg, (p, 100, p, 0, None, 0, p, None, None), b"B >= 1"),
        (tg, (p, 100, p, 256, None, 512, p, None, None), b"M > 0"),
        (sg, (p, p, 100, p, 256, None, 0, p, None, None, p, None), b"estimator"),
        (sg, (p, None, 100, p, 256, None, 0, p, None, p, p, None), b"estimator"),
        (sg, (p, p, 100, p, 256, None, 0, None, None, p, p, None), b"null"),
        (su, (p, p, 100, p, 256, p, p, 0.0, 0, None, None), b"alpha"),
        (su, (p, p, 100, p, 256, p, p, 1.5, 0, None, None), b"alpha"),
        (su, (p, p, 100, p, 256, p, p, float("nan"), 0, None, None), b"alpha"),
        (su, (p, p, 0, p, 256, p, p, 0.01, 0, None, None), b"n_videos"),
        (su, (p, p, 100, p, 0, p, p, 0.01, 0, None, None), b"B must be"),
        (su, (p, p, 100, None, 256, p, p, 0.01, 0, None, None), b"null"),
        (sr, (p, p, 100, 0.5, None), b"g0"),
        (sr, (p, p, 100, float("inf"), None), b"g0"),
        (sr, (p, None, 100, 2.0, None), b"null"),
        (sr, (p, p, -1, 2.0, None), b"n_videos"),
    ]
    for fn, args, msg in cases:
        assert fn(*args) == -1, args                      # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())


def test_train_config_logq_round_trip(tmp_path):
    from cdml_amd.config import TrainConfig
    c = TrainConfig(mode="npair", logq="stream", logq_alpha=0.05, memory_size=16384, batch_size=8192)
    back = TrainConfig.from_json(c.to_json())
    assert back == c and back.logq == "stream" and back.logq_alpha == 0.05
    path = str(tmp_path / "c.json")
    c.to_json(path)
    assert TrainConfig.from_json(path) == c
    assert TrainConfig().logq == "" and TrainConfig().logq_alpha == 0.01           # no correction by default
