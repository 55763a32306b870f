"""The N-pair loss on the config-4 precision, host side: the C ABI of include/cdml_npair_bf16.h (names, ctypes prototypes,
argument checks without a GPU) and the refusals of ops.NPairWorkspace / NPairDP / NPairMixed and TrainStep."""
import ctypes as C
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _header_names(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_bf16_abi_names_header_table_and_library():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    names = _header_names(os.path.join(ROOT, "include", "cdml_npair_bf16.h"))
    assert len(names) == 6 and all(n.startswith("cdml_npair_") and n.endswith("_bf16") for n in names)
    assert sorted(_lib.SIGNATURES_BF16) == names
    lib = _lib.load_library()
    for n in names:
        fn = getattr(lib, n)                              # exported
        assert fn.argtypes == _lib.SIGNATURES_BF16[n][1] and fn.restype == _lib.SIGNATURES_BF16[n][0]
    # the main header does not declare them (tests/footprint_table.py accounts every declaration there)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdml.h")).read(), flags=re.S)
    assert not set(names) & set(re.findall(r"\b(cdml_\w+)\s*\(", main)) and not set(names) & set(_lib.SIGNATURES)
    # the new source and header are part of the library's source id
    assert lib.cdml_build_id().decode() == "CDML_BUILD_ID=" + _lib.source_id()
    assert os.path.exists(os.path.join(ROOT, "collaborative-deep-metric-learning_amd", "csrc", "npair_bf16.hip"))


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p, odd4, odd2 = C.c_void_p(256), C.c_void_p(260), C.c_void_p(258)   # never dereferenced: every call fails its checks first
    B, M, D = 256, 512, 64
    K = B + M
    inf, nan = float("inf"), float("nan")

    def operands(e=p, lde=D, B=B, D=D, A=p, lda=D, P=p, ldp=D, PT=p, ldt=B):
        return lib.cdml_npair_operands_bf16, (e, lde, B, D, A, lda, P, ldp, PT, ldt, None)

    def grad(S=p, lds=B, ids=p, B=B, t=0.1, lse=p, W=p, ldw=B):
        return lib.cdml_npair_grad_bf16, (S, lds, ids, B, t, 1, lse, W, ldw, None)

    def lgrad(S=p, lds=B, ids=p, B=B, bias=p, t=0.1, lse=p, W=p, ldw=B):
        return lib.cdml_npair_logq_grad_bf16, (S, lds, ids, B, bias, t, 1, lse, W, ldw, None)

    def mgrad(S=p, lds=K, ids=p, B=B, mc=B, mid=p, M=M, t=0.1, lse=p, W=p, ldw=K):
        return lib.cdml_npair_memory_grad_bf16, (S, lds, ids, B, mc, mid, M, t, 1, lse, W, ldw, None)

    def mlgrad(S=p, lds=K, ids=p, B=B, mc=B, mid=p, mb=p, M=M, t=0.1, lse=p, W=p, ldw=K):
        return lib.cdml_npair_memory_logq_grad_bf16, (S, lds, ids, B, mc, mid, mb, M, t, 1, lse, W, ldw, None)

    def push(P=p, ldp=D, ids=p, B=B, D=D, start=0, M=M, mem=p, ldm=D, mid=p, R=p, ldr=D, T=p, ldt=M):
        return lib.cdml_npair_memory_push_bf16, (P, ldp, ids, B, D, 0, None, start, M, mem, ldm, mid, R, ldr, T, ldt, None)

    cases = [
        (operands(e=None), b"null"), (operands(A=None), b"null"), (operands(P=None), b"null"), (operands(PT=None), b"null"),
        (operands(B=0), b"B >= 1"), (operands(D=0), b"D >= 1"), (operands(lde=D - 4), b"lde"), (operands(lde=D + 2), b"lde"),
        (operands(lda=D - 8), b"lda"), (operands(lda=D + 4), b"lda"), (operands(ldp=D - 8), b"ldp"), (operands(ldp=D + 4), b"ldp"),
        (operands(ldt=B - 8), b"ldt"), (operands(ldt=B + 4), b"ldt"), (operands(e=odd4), b"aligned"), (operands(A=odd4), b"aligned"),
        (operands(P=odd2), b"aligned"), (operands(PT=odd4), b"aligned"),
    ]
    for fn in (grad, lgrad, mgrad, mlgrad):
        span = B if fn in (grad, lgrad) else K
        cases += [
            (fn(S=None), b"null"), (fn(lse=None), b"null"), (fn(W=None), b"null"), (fn(B=0), b"B must be"),
            (fn(t=0.0), b"temperature"), (fn(t=-1.0), b"temperature"), (fn(t=nan), b"temperature"), (fn(t=inf), b"temperature"),
            (fn(lds=span - 4), b"lds"), (fn(lds=span + 2), b"lds"), (fn(S=odd4), b"aligned"),
            (fn(ldw=span - 4), b"ldw"), (fn(ldw=span + 2), b"ldw"), (fn(W=odd4), b"aligned"), (fn(W=odd2), b"aligned"),
        ]
    cases += [
        (lgrad(bias=None), b"bias"), (lgrad(bias=odd4), b"bias"),
        (mgrad(mid=None), b"null"), (mgrad(M=510), b"memory size"), (mgrad(M=0), b"memory size"), (mgrad(mc=B - 4), b"mem_col"),
        (mgrad(mc=B + 2), b"mem_col"), (mgrad(mid=odd4), b"aligned"),
        (mlgrad(mid=None), b"null"), (mlgrad(mb=None), b"mem_bias"), (mlgrad(mb=odd4), b"mem_bias"), (mlgrad(M=510), b"memory size"),
        (push(P=None), b"null"), (push(ids=None), b"null"), (push(mem=None), b"null"), (push(mid=None), b"null"),
        (push(R=None), b"null"), (push(T=None), b"null"), (push(B=0), b"B >= 1"), (push(D=0), b"D >= 1"),
        (push(M=B + 64), b"multiple of B"), (push(M=B // 2), b"multiple of B"), (push(ldp=D - 1), b"ldp"),
        (push(ldm=D - 1), b"ldm"), (push(ldr=D - 1), b"ldr"), (push(ldt=M - 1), b"ldt"), (push(start=-1), b"start"),
    ]
    for (fn, args), msg in cases:
        assert fn(*args) == -1, args                      # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())


def test_workspace_and_chain_refusals():
    from cdml_amd import ops
    assert "bf16" in ops.NPAIR_PRECISIONS and ops.NPAIR_TILE["bf16"] == 256
    with pytest.raises(ValueError, match="multiple of 256"):
        ops.NPairWorkspace(320, 64, "bf16", "cpu")
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.NPairWorkspace(256, 96, "bf16", "cpu")
    with pytest.raises(ValueError, match="multiple of the batch"):
        ops.NPairMemory(384, 256, 64, "bf16", "cpu")
    with pytest.raises(ValueError, match="'bf16'"):
        ops.NPairDP(256, 512, 64, "bf16", "cpu")
    with pytest.raises(ValueError, match="'bf16'"):
        ops.NPairMixed(256, 64, "bf16", "cpu")
    with pytest.raises(ValueError, match="'f16x2'"):
        ops.NPairWorkspace(256, 64, "f16x2", "cpu")


def test_train_step_refusals_and_auto():
    from cdml_amd import train
    pairs = torch.zeros((4, 2), dtype=torch.int32)
    t16 = types.SimpleNamespace(n_rows_global=1000, data=torch.zeros(1, dtype=torch.float16), feature_size=8)
    t32 = types.SimpleNamespace(n_rows_global=1000, data=torch.zeros(1), feature_size=8)
    mk = lambda table, B=256, **kw: train.TrainStep(table, pairs, B, device="cpu", mode="npair", **kw)
    sync = types.SimpleNamespace(world=1, rank=0)
    for kw in ({}, {"precision": "bf16"}):                # "auto" on an fp16 catalogue is "bf16"
        with pytest.raises(ValueError, match="uniform_negatives"):
            mk(t16, uniform_negatives=True, **kw)
        with pytest.raises(ValueError, match="npair_sync"):
            mk(t16, npair_sync=sync, **kw)
        with pytest.raises(ValueError, match="train_table"):
            mk(t16, train_table=True, **kw)
        with pytest.raises(ValueError, match="multiple of 256"):
            mk(t16, B=320, **kw)
        with pytest.raises(ValueError, match="multiple of the batch"):
            mk(t16, memory_size=384, **kw)
    with pytest.raises(ValueError, match="FeatureTableF16.*f32x3"):       # "bf16" on an fp32 catalogue: the table check
        mk(t32, precision="bf16")
    with pytest.raises(ValueError, match="f32x3"):
        mk(t16, precision="f16x2")
