"""The multi-class N-pair loss without a GPU: the fp64 reference against float64 autograd, the C ABI's argument checks
and the configuration's JSON round trip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npair_ref  # noqa: E402


def _ids_with_duplicates(rng, B):
    ids = rng.choice(10 * B, size=2 * B, replace=False).astype(np.int64)
    ids[1] = ids[5]              # two positives of one video: masked in each other's row term
    ids[6] = ids[3]              # anchor 3 is positive 1: masked in both terms
    ids[9] = ids[8]              # a pair whose two rows are one video
    ids[2 * (B - 1)] = ids[1]    # an anchor that is another pair's positive
    return ids


def _autograd_loss(A, P, ids, t, symmetric):
    B = A.shape[0]
    m, mc = (torch.from_numpy(x) for x in npair_ref.masks(ids, B))
    S = A @ P.T / t
    d = torch.diagonal(S)
    L = (torch.logsumexp(S.masked_fill(~m, -float("inf")), dim=1) - d).mean()
    if symmetric:
        L = 0.5 * (L + (torch.logsumexp(S.masked_fill(~mc, -float("inf")), dim=0) - d).mean())
    return L


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("with_ids", [True, False])
@pytest.mark.parametrize("t", [0.05, 1.0])
def test_reference_matches_float64_autograd(symmetric, with_ids, t):
    rng = np.random.default_rng(3)
    B, D = 12, 16
    A = rng.standard_normal((B, D))
    P = A + 0.5 * rng.standard_normal((B, D))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    ids = _ids_with_duplicates(rng, B) if with_ids else None
    ref = npair_ref.npair(A, P, ids, t, symmetric)
    ta = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    tp = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    L = _autograd_loss(ta, tp, ids, t, symmetric)
    L.backward()
    assert abs(L.item() - ref["loss"]) < 1e-12
    np.testing.assert_allclose(ref["dA"], ta.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(ref["dP"], tp.grad.numpy(), atol=1e-12)
    m, mc = ref["m"], ref["mc"]
    if with_ids:
        assert not m.all() and not mc.all()           # the planted duplicates are masked
        assert not m[0, 2] and not m[2, 0]            # positives 0 and 2 are one video
    dead = ~m & ~mc if symmetric else ~m
    assert (ref["W"][dead] == 0).all()


def test_npair_abi_exported_and_checked_without_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    for name in ("cdml_npair_workspace", "cdml_npair_stats", "cdml_npair_grad_x3", "cdml_npair_grad_f32"):
        assert name in _lib.SIGNATURES
    lib = _lib.load_library()
    assert lib.cdml_npair_workspace(8192) >= 8192 * 5 * 4
    assert lib.cdml_npair_workspace(0) == 0
    p = C.c_void_p(256)                                  # never dereferenced: every call below fails its checks first
    ws = lib.cdml_npair_workspace(256)
    stats = lambda *a: lib.cdml_npair_stats(*a)
    cases = [
        (stats, (None, 256, None, 256, 0.1, 1, p, p, p, ws, None), b"null"),
        (stats, (p, 256, None, 256, 0.1, 1, None, p, p, ws, None), b"null"),
        (stats, (p, 256, None, 256, 0.1, 1, p, None, p, ws, None), b"null"),
        (stats, (p, 256, None, 0, 0.1, 1, p, p, p, ws, None), b"B must be"),
        (stats, (p, 256, None, 256, 0.0, 1, p, p, p, ws, None), b"temperature"),
        (stats, (p, 256, None, 256, -1.0, 1, p, p, p, ws, None), b"temperature"),
        (stats, (p, 256, None, 256, float("nan"), 1, p, p, p, ws, None), b"temperature"),
        (stats, (p, 256, None, 256, float("inf"), 1, p, p, p, ws, None), b"temperature"),
        (stats, (p, 255, None, 256, 0.1, 1, p, p, p, ws, None), b"lds"),
        (stats, (p, 258, None, 256, 0.1, 1, p, p, p, ws, None), b"lds"),
        (stats, (p, 256, None, 256, 0.1, 1, p, p, p, ws - 4, None), b"workspace"),
        (lib.cdml_npair_grad_x3, (p, 256, None, 256, 0.1, 1, p, None, 768, 256, None), b"null"),
        (lib.cdml_npair_grad_x3, (p, 256, None, 256, 0.1, 1, p, p, 700, 256, None), b"ldw"),
        (lib.cdml_npair_grad_x3, (p, 256, None, 256, 0.1, 1, p, p, 768, 200, None), b"plane"),
        (lib.cdml_npair_grad_x3, (p, 256, None, 256, 0.1, 1, p, p, 770, 258, None), b"multiples of 4"),
        (lib.cdml_npair_grad_x3, (p, 256, None, 256, 0.0, 1, p, p, 768, 256, None), b"temperature"),
        (lib.cdml_npair_grad_f32, (p, 256, None, 256, 0.1, 1, p, None, 256, None), b"null"),
        (lib.cdml_npair_grad_f32, (p, 256, None, 256, 0.1, 1, p, p, 128, None), b"ldw"),
        (lib.cdml_npair_grad_f32, (p, 256, None, 256, 0.1, 1, p, p, 258, None), b"ldw"),
        (lib.cdml_npair_grad_f32, (p, 256, None, -3, 0.1, 1, p, p, 256, None), b"B must be"),
        (lib.cdml_npair_grad_f32, (None, 256, None, 256, 0.1, 1, p, p, 256, None), b"null"),
    ]
    for fn, args, msg in cases:
        assert fn(*args) == -1, args                      # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())


def test_train_config_npair_round_trip(tmp_path):
    from cdml_amd.config import TrainConfig
    c = TrainConfig(mode="npair", temperature=0.07, symmetric=False, batch_size=4096)
    back = TrainConfig.from_json(c.to_json())
    assert back == c and back.temperature == 0.07 and back.symmetric is False and back.mode == "npair"
    path = str(tmp_path / "c.json")
    c.to_json(path)
    assert TrainConfig.from_json(path) == c
    assert TrainConfig().temperature == 0.1 and TrainConfig().symmetric is True       # the build-defined defaults


def test_npair_loss_is_a_plugin():
    from cdml_amd import losses, utils
    assert utils.find_class_by_name("NPairLoss", [losses]) is losses.NPairLoss
    assert issubclass(losses.NPairLoss, losses.BaseLoss)
