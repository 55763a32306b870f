"""The N-pair loss's cross-batch memory without a GPU: the fp64 reference against float64 autograd (empty slots, slots of
an anchor's or its positive's video), the ring rule, the C ABI's argument checks and the configuration's JSON round trip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_memory_ref as ref  # noqa: E402
import npair_ref  # noqa: E402


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _case(rng, B=12, M=16, D=16):
    A = _unit(rng.standard_normal((B, D)))
    P = _unit(A + 0.5 * rng.standard_normal((B, D)))
    mem = _unit(rng.standard_normal((M, D)))
    ids = rng.choice(10 * B, size=2 * B, replace=False).astype(np.int64)
    ids[1] = ids[5]                                  # in-batch duplicates, as the N-pair host tests plant them
    ids[6] = ids[3]
    mem_id = rng.choice(np.arange(10 * B, 20 * B), size=M, replace=False).astype(np.int64)
    mem_id[[2, 9]] = -1                              # empty slots
    mem_id[4] = ids[2 * 3]                           # slot 4 is anchor 3's video
    mem_id[7] = ids[2 * 8 + 1]                       # slot 7 is positive 8's video
    mem_id[11] = ids[2 * 0 + 1]                      # slot 11 is positive 0's video (= an in-batch duplicate's, too)
    return A, P, mem, ids, mem_id


def _autograd(A, P, mem, ids, mem_id, t, symmetric):
    B = A.shape[0]
    m, mc = (torch.from_numpy(x) for x in npair_ref.masks(ids, B))
    cm = torch.from_numpy(ref.mem_mask(ids, mem_id, B))
    S, Sm = A @ P.T / t, A @ mem.T / t
    d = torch.diagonal(S)
    X = torch.cat([S.masked_fill(~m, -float("inf")), Sm.masked_fill(~cm, -float("inf"))], 1)
    L = (torch.logsumexp(X, 1) - d).mean()
    if symmetric:
        L = 0.5 * (L + (torch.logsumexp(S.masked_fill(~mc, -float("inf")), 0) - d).mean())
    return L


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("with_ids", [True, False])
@pytest.mark.parametrize("t", [0.05, 1.0])
def test_reference_matches_float64_autograd(symmetric, with_ids, t):
    rng = np.random.default_rng(7)
    A, P, mem, ids, mem_id = _case(rng)
    ids = ids if with_ids else None
    r = ref.npair_memory(A, P, ids, mem, mem_id, t, symmetric)
    ta, tp = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (A, P))
    tm = torch.tensor(mem, dtype=torch.float64, requires_grad=True)
    L = _autograd(ta, tp, tm, ids, mem_id, t, symmetric)
    L.backward()
    assert abs(L.item() - r["loss"]) < 1e-12
    np.testing.assert_allclose(r["dA"], ta.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(r["dP"], tp.grad.numpy(), atol=1e-12)
    # the memory's own gradient is what W_mem^T A would be: the chain does not take it (the ring is not trained)
    np.testing.assert_allclose(r["W_mem"].T @ A, tm.grad.numpy(), atol=1e-12)
    cm = r["cm"]
    assert not cm[:, 2].any() and not cm[:, 9].any()               # empty slots never count
    if with_ids:
        assert not cm[3, 4] and not cm[8, 7] and not cm[0, 11]    # a slot of the anchor's / positive's video does not
        assert cm[0, 4] and cm[3, 7]
    assert (r["W_mem"][~cm] == 0).all()
    B, M = A.shape[0], mem.shape[0]
    assert r["stats"][3] == pytest.approx(((r["m"].sum() - B) + cm.sum()) / (B * (B - 1) + B * M))


def test_empty_memory_is_the_in_batch_loss():
    rng = np.random.default_rng(8)
    A, P, mem, ids, _ = _case(rng)
    for symmetric in (True, False):
        r = ref.npair_memory(A, P, ids, mem, np.full(mem.shape[0], -1), 0.1, symmetric)
        r0 = npair_ref.npair(A, P, ids, 0.1, symmetric)
        assert abs(r["loss"] - r0["loss"]) < 1e-12
        np.testing.assert_allclose(r["dA"], r0["dA"], atol=1e-12)
        np.testing.assert_allclose(r["dP"], r0["dP"], atol=1e-12)


def test_ring_rule():
    B, M = 4, 12
    assert [ref.push_slot(t, 2, M, B) for t in range(7)] == [None, None, 0, 4, 8, 0, 4]
    pos = [np.full((B, 2), t, float) for t in range(7)]
    pid = [np.arange(B) + 100 * t for t in range(7)]
    rows, ids = ref.ring_after(7, 2, M, pos, pid)
    assert list(ids) == list(pid[5]) + list(pid[6]) + list(pid[4])
    assert rows[0, 0] == 5 and rows[4, 0] == 6 and rows[8, 0] == 4


def test_memory_abi_exported_and_checked_without_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    names = ("cdml_npair_memory_workspace", "cdml_npair_memory_stats", "cdml_npair_memory_grad_x3",
             "cdml_npair_memory_grad_f32", "cdml_npair_memory_push")
    for name in names:
        assert name in _lib.SIGNATURES
    lib = _lib.load_library()
    assert lib.cdml_npair_memory_workspace(8192, 32768) >= lib.cdml_npair_workspace(8192)
    assert lib.cdml_npair_memory_workspace(0, 256) == 0
    p = C.c_void_p(256)                                  # never dereferenced: every call below fails its checks first
    ws = lib.cdml_npair_memory_workspace(256, 512)
    K = 768                                              # B + M: the concatenated S / W width
    st = lib.cdml_npair_memory_stats
    gx, gf, push = lib.cdml_npair_memory_grad_x3, lib.cdml_npair_memory_grad_f32, lib.cdml_npair_memory_push
    cases = [
        (st, (None, K, p, 256, 256, p, 512, 0.1, 1, p, p, p, ws, None), b"null"),
        (st, (p, K, p, 256, 256, None, 512, 0.1, 1, p, p, p, ws, None), b"null"),
        (st, (p, K, p, 256, 256, p, 512, 0.1, 1, None, p, p, ws, None), b"null"),
        (st, (p, K, p, 256, 256, p, 512, 0.1, 1, p, None, p, ws, None), b"null"),
        (st, (p, K, p, 0, 256, p, 512, 0.1, 1, p, p, p, ws, None), b"B must be"),
        (st, (p, K, p, 256, 256, p, 0, 0.1, 1, p, p, p, ws, None), b"memory size"),
        (st, (p, K, p, 256, 256, p, 510, 0.1, 1, p, p, p, ws, None), b"memory size"),
        (st, (p, K, p, 256, 256, p, 512, 0.0, 1, p, p, p, ws, None), b"temperature"),
        (st, (p, K, p, 256, 256, p, 512, float("nan"), 1, p, p, p, ws, None), b"temperature"),
        (st, (p, K, p, 256, 128, p, 512, 0.1, 1, p, p, p, ws, None), b"mem_col"),
        (st, (p, K - 4, p, 256, 256, p, 512, 0.1, 1, p, p, p, ws, None), b"lds"),
        (st, (p, K, p, 256, 256, p, 512, 0.1, 1, p, p, p, ws - 4, None), b"workspace"),
        (gx, (p, K, p, 256, 256, p, 512, 0.1, 1, p, None, 3 * K, K, None), b"null"),
        (gx, (p, K, p, 256, 256, p, 512, 0.1, 1, p, p, 3 * K, K - 4, None), b"plane"),
        (gx, (p, K, p, 256, 256, p, 512, 0.1, 1, p, p, 3 * K - 4, K, None), b"ldw"),
        (gx, (p, K, p, 256, 256, p, 512, -1.0, 1, p, p, 3 * K, K, None), b"temperature"),
        (gf, (p, K, p, 256, 256, p, 512, 0.1, 1, p, None, K, None), b"null"),
        (gf, (p, K, p, 256, 256, p, 512, 0.1, 1, p, p, K - 4, None), b"ldw"),
        (gf, (p, K, p, 256, 256, p, 502, 0.1, 1, p, p, K, None), b"memory size"),
        (push, (None, 512, p, 256, 256, 0, None, 0, 512, p, 256, p, None, 0, 0, None, 0, 0, None), b"null"),
        (push, (p, 512, p, 256, 256, 0, None, 0, 512, p, 256, None, None, 0, 0, None, 0, 0, None), b"null"),
        (push, (p, 512, None, 256, 256, 0, None, 0, 512, p, 256, p, None, 0, 0, None, 0, 0, None), b"null"),
        (push, (p, 512, p, 256, 256, 0, None, 0, 640, p, 256, p, None, 0, 0, None, 0, 0, None), b"multiple of B"),
        (push, (p, 512, p, 256, 256, 0, None, 0, 128, p, 256, p, None, 0, 0, None, 0, 0, None), b"multiple of B"),
        (push, (p, 128, p, 256, 256, 0, None, 0, 512, p, 256, p, None, 0, 0, None, 0, 0, None), b"ldp"),
        (push, (p, 512, p, 256, 256, 0, None, -1, 512, p, 256, p, None, 0, 0, None, 0, 0, None), b"start"),
        (push, (p, 512, p, 256, 256, 0, None, 0, 512, p, 256, p, p, 768, 256, None, 0, 0, None), b"together"),
        (push, (p, 512, p, 256, 256, 0, None, 0, 512, p, 256, p, p, 768, 256, p, 3 * K, 256, None), b"plane_t"),
    ]
    for fn, args, msg in cases:
        assert fn(*args) == -1, args                      # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())


def test_train_config_memory_round_trip(tmp_path):
    from cdml_amd.config import TrainConfig
    c = TrainConfig(mode="npair", memory_size=32768, memory_start=100, batch_size=8192)
    back = TrainConfig.from_json(c.to_json())
    assert back == c and back.memory_size == 32768 and back.memory_start == 100
    path = str(tmp_path / "c.json")
    c.to_json(path)
    assert TrainConfig.from_json(path) == c
    assert TrainConfig().memory_size == 0 and TrainConfig().memory_start == 0         # no memory by default
