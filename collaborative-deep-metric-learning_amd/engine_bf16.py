"""Reduced-precision tower for BASELINE config 4: fp16 catalogue, bf16 MFMA
projection, fp32 accumulation, fp32 master weights and optimizer.

Build-defined precision (the reference computes in fp32): same layers and the
same fp32 loss / normalisation kernels as ``engine``, but the four projection
GEMMs and the data gradient run on ``v_mfma_f32_32x32x16_bf16`` through the one
k-contiguous form ``C = A . B^T`` (``ops.gemm_bf16_nt``).  Operands that are
k-strided in memory (the weight gradients contract over batch rows) are fed
from transposed bf16 copies.  Tolerance stated in the tests: 5e-3 absolute on the
unit-norm embeddings, 2e-2 on the loss.
"""
import os

import numpy as np
import torch

from . import ops
from .engine import EngineWorkspace, FeatureTable, TowerLayout, dw1_in_blocks, round_up


class FeatureTableF16(FeatureTable):
    """fp16 catalogue shard [n_rows, row_stride] (3 KB rows at F=1500)."""
    DTYPE, NP_DTYPE, KIND = torch.float16, np.float16, "fp16"
    _fill = staticmethod(ops.fill_uniform_table_f16)


def quantize_f8_host(features):
    """(codes uint8 [n, F], scale fp32 [n]) of a float [n, F] array by the rule of include/cdml_f8.h, on the host: per row
    scale = 2^(max(floor(log2 m), -119) - 7) for the largest finite |x| m (1 for m = 0), code = RNE_e4m3(x / scale) by
    torch's CPU conversion, an Inf / NaN element -> the NaN code of its sign.  Exact exponent arithmetic (frexp / ldexp)."""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(features, dtype=np.float32)))
    finite = torch.isfinite(x)
    m = torch.where(finite, x.abs(), torch.zeros_like(x)).amax(dim=1) if x.shape[1] else x.new_zeros(x.shape[0])
    e = torch.frexp(m).exponent                                  # m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    k = torch.where(m > 0, (e - 1).clamp(min=-119) - 7, torch.zeros_like(e))
    one = torch.ones_like(m)
    scale = torch.ldexp(one, k)
    y = x * torch.ldexp(one, -k)[:, None]                        # exact: a power of two, |y| < 256
    codes = torch.where(finite, y, torch.zeros_like(y)).to(torch.float8_e4m3fn).view(torch.uint8)
    nan_code = (0x7F | ((x.view(torch.int32) >> 24) & 0x80)).to(torch.uint8)
    return torch.where(finite, codes, nan_code).numpy(), scale.numpy()


class FeatureTableF8(FeatureTable):
    """fp8 catalogue shard (include/cdml_f8.h): OCP e4m3 codes [n_rows, row_stride] (1.5 KB rows at F=1500, rows on 128-B
    lines, pad columns code 0) and ``scale`` fp32 [n_rows], one power of two per row, value = code x scale.  Precision "bf16"
    gathers the codes (the scale cancels in the input l2-normalisation); read-only."""
    DTYPE, NP_DTYPE, KIND = torch.float8_e4m3fn, np.float32, "fp8"

    def __init__(self, data, feature_size, row0=0, n_rows_global=None, scale=None):
        super().__init__(data, feature_size, row0, n_rows_global)
        if scale is None:
            scale = torch.ones(self.n_rows, dtype=torch.float32, device=data.device)
        if scale.dtype != torch.float32 or scale.shape != (self.n_rows,) or scale.device != data.device:
            raise ValueError("FeatureTableF8 needs one fp32 scale per row on the codes' device")
        self.scale = scale

    @staticmethod
    def padded_stride(feature_size):
        return round_up(feature_size, 128)

    @classmethod
    def from_numpy(cls, features, device, row0=0, n_rows_global=None):
        """features.npy contents (float [N,F]) quantised on the host, codes and scales -> HBM."""
        codes, scale = quantize_f8_host(features)
        n, F = codes.shape
        data = torch.zeros((n, cls.padded_stride(F)), dtype=torch.uint8, device=device)
        data[:, :F] = torch.from_numpy(codes).to(device)
        return cls(data.view(cls.DTYPE), F, row0, n_rows_global, torch.from_numpy(scale).to(device))

    @classmethod
    def _empty(cls, n_rows, feature_size, device):
        return (torch.empty((n_rows, cls.padded_stride(feature_size)), dtype=cls.DTYPE, device=device),
                torch.empty(n_rows, dtype=torch.float32, device=device))

    @classmethod
    def from_table(cls, table, chunk_rows=65536):
        """A device FeatureTable (fp32) or FeatureTableF16 quantised by the HIP quantiser, ``chunk_rows`` rows per launch."""
        F = table.feature_size
        data, scale = cls._empty(table.n_rows, F, table.data.device)
        for lo in range(0, table.n_rows, int(chunk_rows)):
            hi = min(lo + int(chunk_rows), table.n_rows)
            ops.quantize_rows_f8(table.data[lo:hi], F, data[lo:hi], scale[lo:hi])
        return cls(data, F, table.row0, table.n_rows_global, scale)

    @classmethod
    def synthetic(cls, n_rows, feature_size, seed, device, row0=0, n_rows_global=None, chunk_rows=65536):
        """The U[0,1) table of FeatureTableF16.synthetic, quantised: fp16 chunks from the fill kernel (its ``row0``) go
        through the quantiser one after the other, so the content is from_table(FeatureTableF16.synthetic(...))'s and no
        whole fp16 table ever exists."""
        data, scale = cls._empty(n_rows, feature_size, device)
        chunk = min(int(chunk_rows), n_rows)
        tmp = torch.empty((chunk, FeatureTableF16.padded_stride(feature_size)), dtype=torch.float16, device=device)
        for lo in range(0, n_rows, chunk):
            hi = min(lo + chunk, n_rows)
            ops.fill_uniform_table_f16(tmp[:hi - lo], row0 + lo, feature_size, seed)
            ops.quantize_rows_f8(tmp[:hi - lo], feature_size, data[lo:hi], scale[lo:hi])
        return cls(data, feature_size, row0, n_rows_global, scale)

    def codes(self, idx=None):
        """The codes as uint8 [n, F] (of the given LOCAL rows)."""
        u = self.data.view(torch.uint8)
        return (u if idx is None else u[idx])[:, :self.feature_size]

    def rows(self, idx):
        return self.dequantize(idx)

    def dequantize(self, idx=None):
        """fp32 rows code x scale, unpadded (of the given LOCAL rows)."""
        c = self.codes(idx).contiguous().view(self.DTYPE).to(torch.float32)
        return c * (self.scale if idx is None else self.scale[idx])[:, None]

    def as_f16(self, chunk_rows=65536):
        """The FeatureTableF16 holding the codes' values (every e4m3 value is an fp16 value: exact) -- what the fp8 gather is
        bit-identical to the fp16 gather of."""
        F = self.feature_size
        data = torch.zeros((self.n_rows, FeatureTableF16.padded_stride(F)), dtype=torch.float16, device=self.data.device)
        for lo in range(0, self.n_rows, int(chunk_rows)):
            hi = min(lo + int(chunk_rows), self.n_rows)
            data[lo:hi, :F] = self.data[lo:hi, :F].to(torch.float16)
        return FeatureTableF16(data, F, self.row0, self.n_rows_global)


def layout_bf16(feature_size, hidden=5000, output_size=256):
    """TowerLayout whose padded sizes satisfy the bf16 GEMM (N % 128, K % 64)."""
    return TowerLayout(feature_size, hidden, output_size, pad=(64, 128, 128))


class TowerWorkspaceBF16(EngineWorkspace):
    ROWS, TABLE_DTYPE, INFERENCE = 64, torch.float16, "bf16"
    TABLE_DTYPES = (torch.float16, torch.float8_e4m3fn)       # FeatureTableF16, or the codes of a FeatureTableF8

    def __init__(self, layout, n_rows, device, backward=True, **plane_options):
        L, R = layout, int(n_rows)
        if R % 64:
            raise ValueError("the bf16 path needs a row count that is a multiple of 64 (got %d)" % R)
        self.layout, self.R = L, R
        bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=device)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        self.x_hat, self.h1 = bf(R, L.Fp), bf(R, L.Hp)
        self.z, self.e = f32(R, L.Dp), f32(R, L.Dp)
        self.W1T, self.W2T, self.W2 = bf(L.Hp, L.Fp), bf(L.Dp, L.Hp), bf(L.Hp, L.Dp)
        if not backward:                                   # catalogue inference: forward buffers only
            self.gemm_ws = torch.empty(max(ops.gemm_bf16_workspace(R, L.Dp, L.Hp), 16) // 4, dtype=torch.float32,
                                       device=device)
            return
        # weight gradients straight from the activations as stored (k-strided GEMM with
        # transposed LDS reads) when the shapes allow; otherwise transposed bf16 copies
        self.tn1 = ops.gemm_bf16_tn_supported(L.Fp, L.Hp, R, L.Fp, L.Hp)
        self.tn2 = ops.gemm_bf16_tn_supported(L.Hp, L.Dp, R, L.Hp, L.Dp)
        self.dz1 = bf(R, L.Hp)
        # leaky-relu' of the hidden layer as ONE BIT per element, written by FC1's epilogue and read by
        # the data gradient instead of the 2-byte activations (epilogues 4 / 5).  OFF by default: measured
        # on one box in the config-4 step (profiles/r03_bf16_maskbits_ab.txt) the byte stores cost FC1's
        # epilogue 23 us and the data gradient did not get faster -- it is not bound by the mask bytes
        # (tools/experiments/k256_ablate.sh: without any mask traffic 86 us of its 119)
        self.h1_bits = None
        if (os.environ.get("CDML_BF16_MASKBITS") == "1"
                and ops.gemm_bf16_epilogue_supported(ops.BE_BIAS_LRELU_BF16_BITS, R, L.Hp, L.Fp, L.Fp, L.Fp, L.Hp, L.Hp // 8)
                and ops.gemm_bf16_epilogue_supported(ops.BE_MASKBITS_BF16, R, L.Hp, L.Dp, L.Dp, L.Dp, L.Hp, L.Hp // 8)):
            self.h1_bits = torch.zeros((R, L.Hp // 8), dtype=torch.uint8, device=device)
        self.de, self.dz2 = f32(R, L.Dp), f32(R, L.Dp)
        self.dz2_bf = bf(R, L.Dp)
        if not self.tn1:
            self.xT, self.dz1T = bf(L.Fp, R), bf(L.Hp, R)
        if not self.tn2:
            self.h1T, self.dz2T = bf(L.Hp, R), bf(L.Dp, R)
        # both weight gradients in one stream-K launch when the shapes allow (0 = they do not)
        self.tn2_bytes = ops.gemm_bf16_tn2_workspace(L.Fp, L.Hp, L.Hp, L.Dp, R) if (self.tn1 and self.tn2) else 0
        nb = max(self.tn2_bytes,
                 ops.gemm_bf16_workspace(L.Hp, L.Dp, R), ops.gemm_bf16_workspace(L.Fp, L.Hp, R),
                 ops.gemm_bf16_workspace(R, L.Dp, L.Hp),
                 ops.gemm_bf16_tn_workspace(L.Hp, L.Dp, R), ops.gemm_bf16_tn_workspace(L.Fp, L.Hp, R),
                 ops.gemm_bf16_tn_workspace(L.Fp // 2, L.Hp, R), 16)      # dW1 in two row blocks (data-parallel)
        self.gemm_ws = torch.empty(nb // 4, dtype=torch.float32, device=device)
        self.colsum_ws = f32(max(ops.colsum_workspace_floats(R, L.Hp), ops.colsum_workspace_floats(R, L.Dp)))

    def tail_operands(self, indexed=False):
        return {"dz2_bf16": self.dz2_bf}, False            # (the bf16 copy of dz2: both tails write it)

    def optimizer_operands(self):
        return {"wt": self.W1T}, {"wt": self.W2T, "wc": self.W2}


def refresh_weights(p, ws):
    """bf16 operand copies of the fp32 master weights (after every optimizer step)."""
    L = p.layout
    ops.transpose_to_bf16(p.W1, ws.W1T, L.Fp, L.Hp)
    ops.transpose_to_bf16(p.W2, ws.W2T, L.Hp, L.Dp)
    ops.cast_f32_bf16(p.W2, ws.W2, L.Hp, L.Dp)


def tower_forward(p, ws, normalize=True):
    """x_hat (bf16, l2-normalised) -> h1 (bf16) -> z (fp32) -> e (fp32).  models.py:59-61.
    ``normalize=False``: stop at z (the fused tail of the training step takes over)."""
    L, R = p.layout, ws.R
    bits = ws.h1_bits
    if bits is not None:
        ops.gemm_bf16_nt(ops.BE_BIAS_LRELU_BF16_BITS, ws.x_hat, ws.W1T, ws.h1, R, L.Hp, L.Fp, bias=p.b1, aux=bits)
    else:
        ops.gemm_bf16_nt(ops.BE_BIAS_LRELU_BF16, ws.x_hat, ws.W1T, ws.h1, R, L.Hp, L.Fp, bias=p.b1)
    ops.gemm_bf16_nt(ops.BE_BIAS_LRELU_F32, ws.h1, ws.W2T, ws.z, R, L.Dp, L.Hp, bias=p.b2, workspace=ws.gemm_ws)
    ws.tail_done = False
    if normalize:
        ops.l2norm_fwd(ws.z, L.Dp, ws.e)
    return ws.e


def tower_backward(p, ws, after_w1=None, w1_chunks=1, after_w1_chunk=None):
    """ws.de -> p.grad (fp32).  train.py:141; no dX.  As in the fp32 engine the first layer's
    gradient (85 % of the bytes) is produced BEFORE the second layer's, so that ``after_w1`` --
    the data-parallel all-reduce of [dW1|db1] -- runs under the dW2 GEMM and the db2 sums;
    with ``w1_chunks`` > 1 dW1 comes in row blocks of W1 and ``after_w1_chunk(lo, hi)`` fires
    after each (flat-gradient ranges; the last one ends after db1), as in engine.tower_backward.
    Without those hooks (one GPU) the second layer's gradient goes FIRST: it and the data gradient
    that follows both stream h1 (252 MB at the config-4 shape), and back to back the second pass
    finds part of it in the Infinity Cache (1.087 -> 1.070 ms per step, measured)."""
    L, R = p.layout, ws.R
    if not ws.tail_done:                             # the fused tail writes dz2 and its bf16 copy
        ops.l2norm_bwd(ws.z, ws.de, L.Dp, ws.dz2, lrelu_alpha=ops.LRELU_ALPHA)
        ops.cast_f32_bf16(ws.dz2, ws.dz2_bf, R, L.Dp)
    single = after_w1 is None and after_w1_chunk is None
    how = os.environ.get("CDML_BF16_DW", "split")                        # (the switch: A/B runs)
    joint = single and ws.tn2_bytes and how == "joint"
    w2_first = single and not joint and ws.tn2 and not os.environ.get("CDML_BF16_W2_LAST")
    if joint:
        # NOT the default (profiles/r03_bf16_joint_dw.txt): data gradient first, then BOTH weight gradients and
        # both bias gradients in one stream-K launch + fix-up pass.  Every block gets the same number of K-tiles,
        # but blocks that sit at different k share no operand panels in L2 and the launch runs 29 % slower than
        # the two split-K launches (the same finding as the fp32 pure stream-K of round 2).  Running dW2 on a
        # side stream beside dW1 was measured too: the two finish 23 us sooner, the fork/join costs 34.
        if ws.h1_bits is not None:
            ops.gemm_bf16_nt(ops.BE_MASKBITS_BF16, ws.dz2_bf, ws.W2, ws.dz1, R, L.Hp, L.Dp, aux=ws.h1_bits)
        else:
            ops.gemm_bf16_nt(ops.BE_MASK_BF16, ws.dz2_bf, ws.W2, ws.dz1, R, L.Hp, L.Dp, aux=ws.h1)
        ops.gemm_bf16_tn2(ws.x_hat, ws.dz1, p.gW1, L.Fp, L.Hp, ws.h1, ws.dz2_bf, p.gW2, L.Hp, L.Dp, R, ws.gemm_ws,
                          colsum1=p.gb1, colsum2=p.gb2)
        return p.grad
    if w2_first:
        # db2 = column sums of the bf16 dz2 the two products consume, from the LDS tiles of the same GEMM
        ops.gemm_bf16_tn(ws.h1, ws.dz2_bf, p.gW2, L.Hp, L.Dp, R, workspace=ws.gemm_ws, colsum=p.gb2)
    if ws.h1_bits is not None:
        ops.gemm_bf16_nt(ops.BE_MASKBITS_BF16, ws.dz2_bf, ws.W2, ws.dz1, R, L.Hp, L.Dp, aux=ws.h1_bits)
    else:
        ops.gemm_bf16_nt(ops.BE_MASK_BF16, ws.dz2_bf, ws.W2, ws.dz1, R, L.Hp, L.Dp, aux=ws.h1)
    def dw1(lo, hi, db):
        if ws.tn1:   # db1 = column sums of dz1, taken from the LDS tiles of the same GEMM
            ops.gemm_bf16_tn(ws.x_hat[:, lo:hi], ws.dz1, p.gW1[lo:hi], hi - lo, L.Hp, R, workspace=ws.gemm_ws, colsum=db)
        else:        # (whole only: the row blocks need the k-strided form)
            ops.colsum(ws.dz1, R, L.Hp, p.gb1, ws.colsum_ws)
            ops.transpose_to_bf16(ws.dz1, ws.dz1T, R, L.Hp)
            ops.transpose_to_bf16(ws.x_hat, ws.xT, R, L.Fp)
            ops.gemm_bf16_nt(ops.BE_F32, ws.xT, ws.dz1T, p.gW1, L.Fp, L.Hp, R, workspace=ws.gemm_ws)
    dw1_in_blocks(p, dw1, w1_chunks, after_w1_chunk,
                  lambda rows: ws.tn1 and ops.gemm_bf16_tn_supported(rows, L.Hp, R, L.Fp, L.Hp))
    if after_w1 is not None:
        after_w1()
    if w2_first:
        return p.grad
    if ws.tn2:
        ops.gemm_bf16_tn(ws.h1, ws.dz2_bf, p.gW2, L.Hp, L.Dp, R, workspace=ws.gemm_ws, colsum=p.gb2)
    else:
        ops.colsum(ws.dz2, R, L.Dp, p.gb2, ws.colsum_ws)
        ops.transpose_to_bf16(ws.dz2, ws.dz2T, R, L.Dp)
        ops.transpose_to_bf16(ws.h1, ws.h1T, R, L.Hp)
        ops.gemm_bf16_nt(ops.BE_F32, ws.h1T, ws.dz2T, p.gW2, L.Hp, L.Dp, R, workspace=ws.gemm_ws)
    return p.grad
