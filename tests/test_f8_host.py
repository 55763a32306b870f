"""The fp8 catalogue (include/cdml_f8.h) on the host: the package's host quantiser against the numpy reference of
tests/f8_ref.py bit for bit, the format's error bound, the exactness of e4m3 -> fp16, the header / binding table / library
agreement, every new entry point's refusals (placeholder pointers that nothing dereferences: every check returns before a
HIP call, as tests/test_gather_plan_host.py describes) and TrainStep's argument rules for an fp8 table.  No GPU."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f8_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [7, 520, 1500]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    return _lib.load_library()


# ---- the quantiser rule ----
@pytest.mark.parametrize("F", SIZES)
def test_host_quantiser_is_the_reference_bit_for_bit(F):
    from cdml_amd import engine_bf16
    x = ref.sample_rows(F)
    codes, scale = engine_bf16.quantize_f8_host(x)
    want_codes, want_scale = ref.quantize(x)
    assert codes.dtype == np.uint8 and scale.dtype == np.float32 and codes.shape == x.shape
    assert np.array_equal(scale.view(np.uint32), want_scale.view(np.uint32))
    assert np.array_equal(codes, want_codes)
    # the rule's landmarks: powers of two; zero rows scale 1; the row just below a power of two rounds up to code 256
    m, e = np.frexp(scale.astype(np.float64))
    assert np.all(m == 0.5)
    assert scale[3] == 1 and not codes[3].any()
    assert scale[5] == 2.0 ** -5 and codes[5, 1 % F] == 0x70                # 4 / 2^-5 = 128
    assert scale[6] == 2.0 ** -6 and codes[6, 2 % F] == 0x78                # 3.9999998 / 2^-6 -> 256
    assert scale[11] == 2.0 ** -126                                          # the clamp: fp32 denormals
    assert codes[13, F - 1] == 0xF0 and scale[13] == 2.0 ** -7              # -1 = -128 x 2^-7
    assert list(codes[10, [0, 1, 3, 4]]) == [0x7F, 0x7F, 0xFF, 0xFF]       # +Inf, +NaN, -Inf, -NaN
    # nothing saturates, every non-zero finite row above the clamp uses the top binade
    mag = codes & 0x7F
    finite_rows = np.isfinite(x).all(1) & (np.abs(x).max(1) >= 2.0 ** -119)
    assert mag[finite_rows].max(1).min() >= 0x70 and mag[mag != 0x7F].max() <= 0x78


@pytest.mark.parametrize("F", SIZES)
def test_error_bound_of_the_format(F):
    x = ref.sample_rows(F)
    codes, scale = ref.quantize(x)
    fin = np.isfinite(x)
    assert np.array_equal(np.isnan(ref.decode(codes)), ~fin)
    deq = np.where(fin, ref.decode(codes), 0.0) * scale.astype(np.float64)[:, None]
    x0 = np.where(fin, x, 0).astype(np.float64)
    err = np.linalg.norm(deq - x0, axis=1)
    assert np.all(err <= ref.error_bound(x0, scale))
    # per element: half an ulp of three mantissa bits, or half a subnormal step of the code
    assert np.all(np.abs(deq - x0) <= np.maximum(2.0 ** -4 * np.abs(x0), 2.0 ** -10 * scale.astype(np.float64)[:, None]))
    if F == 1500:                                             # the typical rows: well inside the bound
        rel = err[14:] / np.linalg.norm(x0[14:], axis=1)
        cos = (deq[14:] * x0[14:]).sum(1) / (np.linalg.norm(deq[14:], axis=1) * np.linalg.norm(x0[14:], axis=1))
        print("relative L2 error: max %.4f; min cosine %.5f" % (rel.max(), cos.min()))
        assert rel.max() <= 0.0625 and cos.min() >= 0.998           # (a relative error e leaves a cosine >= sqrt(1 - e^2))


def test_every_code_is_exactly_an_fp16_value():
    codes = torch.arange(256, dtype=torch.uint8)
    h = codes.view(torch.float8_e4m3fn).to(torch.float16)
    nan = torch.isnan(h)
    assert nan.nonzero().view(-1).tolist() == [0x7F, 0xFF]
    back = h.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(back[~nan], codes[~nan])
    want = ref.decode(codes.numpy())
    assert np.array_equal(h.double().numpy()[~nan.numpy()], want[~nan.numpy()]) and np.isnan(want[[0x7F, 0xFF]]).all()
    assert np.array_equal(ref.encode(want), codes.numpy())              # (-0 included: code 0x80)


# ---- header, binding table, library ----
def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cdml_f8.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_table_and_library_agree(lib):
    from cdml_amd import _lib
    syms = _header_symbols()
    assert syms == sorted(_lib.SIGNATURES_F8) and len(syms) == 6
    for s in syms:
        assert hasattr(lib, s), s
    others = (_lib.SIGNATURES, _lib.SIGNATURES_HARDNEG, _lib.SIGNATURES_NEGW, _lib.SIGNATURES_MIXED, _lib.SIGNATURES_BF16)
    assert not any(set(syms) & set(o) for o in others)
    assert "cdml_f8" not in open(os.path.join(ROOT, "include", "cdml.h")).read()


# ---- argument checks: all before any HIP call ----
P = 0x10000                                    # a 16-B aligned placeholder address, never dereferenced


def _fused(name, **kw):
    a = dict(mode=0, pairs=P, table=P, idx=P, shift=P, x=P, row_stride=1536, F=1500, out_stride=1536, n_steps=2, lists=P,
             start=P, coarse=P, batch=32)
    a.update(kw)
    p = lambda v: C.c_void_p(v) if v else None
    head = (p(a["pairs"]), 64, 1, 0, None, a["batch"], 0, a["batch"], p(a["table"]), 1000, a["row_stride"], a["F"])
    tail = (p(a["x"]), a["out_stride"], a["n_steps"], 96 * a["out_stride"], 96)
    if name == "cdml_sample_gather_f8":
        return (a["mode"],) + head + (p(a["idx"]), p(a["shift"])) + tail + (None, None)
    mid = (p(a["lists"]), 8, 8, 1 << 31) if "listed" in name else (p(a["start"]), 1000, p(a["coarse"]), 16)
    return head + mid + (p(a["idx"]), None) + tail + (32, None, None)


def _rows(**kw):
    a = dict(table=P, idx=P, x=P, row_stride=1536, F=1500, out_stride=1536)
    a.update(kw)
    p = lambda v: C.c_void_p(v) if v else None
    return (p(a["table"]), 0, 1000, a["row_stride"], p(a["idx"]), 130, a["F"], p(a["x"]), a["out_stride"], None, None)


def _quant(**kw):
    a = dict(src=P, codes=P, scale=P, src_stride=1536, F=1500, code_stride=1536, width=1536)
    a.update(kw)
    p = lambda v: C.c_void_p(v) if v else None
    return (p(a["src"]), 300, a["src_stride"], a["F"], p(a["codes"]), a["code_stride"], a["width"], p(a["scale"]), None)


FUSED = ["cdml_sample_gather_f8", "cdml_sample_gather_listed_f8", "cdml_sample_gather_weighted_f8"]
QUANT = ["cdml_quantize_rows_f8_f32", "cdml_quantize_rows_f8_f16"]
E_BADARG, E_ALIGN, E_UNSUPPORTED = -1, -3, -4


def test_argument_errors_need_no_gpu(lib):
    cases = []
    for name in FUSED:
        layout = b"sample_gather_f8: row_stride must be >= F and a multiple of 16, out_stride >= F and a multiple of 8, bases 16-B aligned"
        cases += [(name, _fused(name, pairs=0), E_BADARG, b"sample_gather_f8: bad argument"),
                  (name, _fused(name, table=0), E_BADARG, b"sample_gather_f8: bad argument"),
                  (name, _fused(name, idx=0), E_BADARG, b"sample_gather_f8: bad argument"),
                  (name, _fused(name, x=0), E_BADARG, b"sample_gather_f8: bad argument"),
                  (name, _fused(name, F=0), E_UNSUPPORTED, b"sample_gather_f8: F = 0 outside (0, 4096]"),
                  (name, _fused(name, F=4097, row_stride=4112, out_stride=4104), E_UNSUPPORTED, b"F = 4097 outside (0, 4096]"),
                  (name, _fused(name, row_stride=1528), E_ALIGN, layout),            # a multiple of 8, not of 16
                  (name, _fused(name, row_stride=1496), E_ALIGN, layout),            # < F
                  (name, _fused(name, out_stride=1508), E_ALIGN, layout),            # a multiple of 4, not of 8
                  (name, _fused(name, out_stride=1496), E_ALIGN, layout),
                  (name, _fused(name, table=P + 8), E_ALIGN, layout),
                  (name, _fused(name, x=P + 8), E_ALIGN, layout),
                  (name, _fused(name, n_steps=65), E_BADARG, b"sample_gather_f8: n_steps must be in [1, 64]"),
                  (name, _fused(name, n_steps=0), E_BADARG, b"sample_gather_f8: n_steps must be in [1, 64]"),
                  (name, _fused(name, batch=0), E_BADARG, b"sample_gather_f8: batch too small")]
    name = FUSED[0]
    cases += [(name, _fused(name, mode=m), E_BADARG, b"sample_gather_f8: mode must be 0 or 1") for m in (-1, 2, 3, 4)]
    cases += [(name, _fused(name, mode=1, shift=0), E_BADARG, b"sample_gather_f8: shift_out required in mode 1"),
              (FUSED[1], _fused(FUSED[1], lists=0), E_BADARG, b"sample_gather_listed_f8: lists is null"),
              (FUSED[2], _fused(FUSED[2], start=0), E_BADARG, b"sample_gather_weighted_f8: the start / coarse tables are null"),
              (FUSED[2], _fused(FUSED[2], coarse=0), E_BADARG, b"sample_gather_weighted_f8: the start / coarse tables are null")]
    name = "cdml_gather_rows_f8"
    layout = b"gather_rows_f8: row_stride must be >= F and a multiple of 16, out_stride >= F and a multiple of 8, bases 16-B aligned"
    cases += [(name, _rows(table=0), E_BADARG, b"gather_rows_f8: bad argument"),
              (name, _rows(idx=0), E_BADARG, b"gather_rows_f8: bad argument"),
              (name, _rows(x=0), E_BADARG, b"gather_rows_f8: bad argument"),
              (name, _rows(F=0), E_UNSUPPORTED, b"gather_rows_f8: F = 0 outside (0, 4096]"),
              (name, _rows(F=4097, row_stride=4112, out_stride=4104), E_UNSUPPORTED, b"F = 4097 outside (0, 4096]"),
              (name, _rows(row_stride=1528), E_ALIGN, layout), (name, _rows(out_stride=1508), E_ALIGN, layout),
              (name, _rows(table=P + 8), E_ALIGN, layout), (name, _rows(x=P + 8), E_ALIGN, layout)]
    for name in QUANT:
        who = name[5:].encode()
        cases += [(name, _quant(src=0), E_BADARG, who + b": bad argument"),
                  (name, _quant(codes=0), E_BADARG, who + b": bad argument"),
                  (name, _quant(scale=0), E_BADARG, who + b": bad argument"),
                  (name, _quant(F=0), E_UNSUPPORTED, who + b": F = 0 outside (0, 4096]"),
                  (name, _quant(F=4097, src_stride=4104, code_stride=4224, width=4224), E_UNSUPPORTED, b"F = 4097 outside"),
                  (name, _quant(src_stride=1508), E_ALIGN, who + b": src_stride must be >= F and a multiple of 8"),
                  (name, _quant(src_stride=1496), E_ALIGN, who + b": src_stride must be >= F and a multiple of 8"),
                  (name, _quant(src=P + 8), E_ALIGN, who + b": src_stride must be >= F"),
                  (name, _quant(width=1508), E_ALIGN, who + b": width must be >= F, a multiple of 8"),
                  (name, _quant(width=1496), E_ALIGN, who + b": width must be >= F, a multiple of 8"),
                  (name, _quant(width=1544), E_ALIGN, who + b": width must be >= F, a multiple of 8 and <= code_stride"),
                  (name, _quant(code_stride=1540, width=1504), E_ALIGN, who + b": width must be"),
                  (name, _quant(codes=P + 4), E_ALIGN, who + b": width must be")]
    assert len(cases) == 88
    for name, args, status, text in cases:
        rc = getattr(lib, name)(*args)
        msg = lib.cdml_last_error()
        assert rc == status and text in msg, (name, args, rc, msg)


def test_wrapper_refusals():
    from cdml_amd import engine_bf16, ops
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops._mat8(torch.zeros((4, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="fp32 or fp16 source"):
        ops.quantize_rows_f8(torch.zeros((4, 16), dtype=torch.float64), 16, None, None)
    codes = torch.zeros((4, 128), dtype=torch.float8_e4m3fn)
    assert ops._gather_format(codes, torch.zeros(1, dtype=torch.bfloat16)) == "_f8"
    with pytest.raises(ValueError, match="device tensor"):
        engine_bf16.FeatureTableF8(codes, 16)
    T = engine_bf16.FeatureTableF8
    assert (T.DTYPE, T.KIND) == (torch.float8_e4m3fn, "fp8") and [T.padded_stride(f) for f in (1, 128, 1500)] == [128, 128, 1536]


# ---- TrainStep's argument rules ----
N = 1000
HOOK = types.SimpleNamespace(world=2, rank=1)


def _table(dtype=torch.float8_e4m3fn):
    return types.SimpleNamespace(n_rows_global=N, n_rows=N, feature_size=8, data=torch.zeros((1, 8), dtype=torch.uint8).view(dtype)
                                 if dtype == torch.float8_e4m3fn else torch.zeros((1, 8), dtype=dtype))


def _validate(batch, use_graph=False, **kw):
    from cdml_amd import train
    tab = _table()
    a = train.validate_args(tab, batch, **kw)
    rows = batch * (3 if a.uniform_negatives or kw.get("mode", "uniform") == "uniform" else 2)
    return train.resolve_precision(tab, rows, a.precision, use_graph, kw.get("exchange"), kw.get("grad_sync"))


def test_train_step_arguments_for_an_fp8_table():
    from cdml_amd import engine
    mismatch = "precision 'bf16' goes with an fp16 FeatureTableF16, 'f32' / 'f32x3' with an fp32 table"
    for p in ("f32x3", "f32", "f16x2", "f32x3-3"):
        with pytest.raises(ValueError, match=mismatch):
            _validate(128, precision=p)
    with pytest.raises(ValueError, match="an fp8 catalogue is read-only"):
        _validate(128, train_table=True)
    with pytest.raises(ValueError, match="exchange does not go with an fp8 catalogue"):
        _validate(128, exchange=HOOK)
    with pytest.raises(ValueError, match="grad_sync does not go with an fp8 catalogue"):
        _validate(128, grad_sync=HOOK)
    assert engine.auto_precision(torch.float8_e4m3fn, 384) == "bf16" and engine.auto_precision(torch.float8_e4m3fn, 100) == "bf16"
    for mode, batch in (("uniform", 128), ("inbatch", 64), ("semihard", 96), ("npair", 256)):
        for auto in ("auto", None, "bf16"):
            assert _validate(batch, mode=mode, precision=auto) == "bf16"
    assert _validate(256, mode="npair", memory_size=256, logq="stream") == "bf16"
    assert _validate(128, negative_weights=np.ones(N)) == "bf16" and _validate(128, use_graph=True) == "bf16"
    with pytest.raises(ValueError, match="mode 'npair' on precision 'bf16' does not take uniform_negatives"):
        _validate(256, mode="npair", uniform_negatives=True)
    E = engine.get_engine("bf16")
    assert E.table_dtype == torch.float16 and set(E.table_dtypes) == {torch.float16, torch.float8_e4m3fn}
    assert engine.get_engine("f32x3").table_dtypes == (torch.float32,)
