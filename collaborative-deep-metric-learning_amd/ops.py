"""Tensor-level wrappers over the C ABI: pointer/stride plumbing only.

Each function hands raw device pointers, sizes and the current torch stream to
libcdml_hip.so.  Nothing here computes; a CPU tensor is an error.
"""
import ctypes as C

import torch

from ._lib import call, load_library

LRELU_ALPHA = 0.2     # tf.nn.leaky_relu default (reference models.py:21)


def _stream():
    # the caller selects the device (TrainStep asserts it); the stream is that device's current one
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, dtype=None):
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise ValueError("cdml ops need device tensors (there is no CPU path)")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"expected {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def _mat(t, dtype=torch.float32):
    """(pointer, leading dimension) of a 2-D row-major view."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("expected a 2-D tensor with unit inner stride")
    return _p(t, dtype), t.stride(0)


def version():
    return load_library().cdml_version()


# ------------------------------------------------------------------ data ------
def fill_uniform_table(table, row0, feature_size, seed):
    ptr, ld = _mat(table)
    call("cdml_fill_uniform_table", ptr, row0, table.shape[0], feature_size, ld, seed, _stream())
    return table


def sample_uniform(pairs, n_rows, seed, step, batch, idx_out, slot0=0, batch_global=None,
                   step_dev=None):
    bg = batch if batch_global is None else batch_global
    call("cdml_sample_uniform", _p(pairs, torch.int32), pairs.shape[0], n_rows, seed,
         0 if step is None else step, _p(step_dev, torch.int64), batch, slot0, bg,
         _p(idx_out, torch.int32), _stream())
    return idx_out


def sample_inbatch(pairs, seed, step, batch, rows_out, shift_out, slot0=0, batch_global=None,
                   step_dev=None):
    bg = batch if batch_global is None else batch_global
    call("cdml_sample_inbatch", _p(pairs, torch.int32), pairs.shape[0], seed,
         0 if step is None else step, _p(step_dev, torch.int64), batch, slot0, bg,
         _p(rows_out, torch.int32), _p(shift_out, torch.int32), _stream())
    return rows_out, shift_out


def step_advance(step_dev):
    call("cdml_step_advance", _p(step_dev, torch.int64), _stream())


def gather_rows(table, row0, idx, feature_size, x_out, normalize=True, inv_norm_out=None,
                oob_flag=None, nan_missing=False):
    """nan_missing: an idx of -1 is a request that got no row (exchange overflow) -> that output row
    becomes NaN; otherwise -1 marks a padding slot and the output row is left untouched."""
    tp, tld = _mat(table)
    xp, xld = _mat(x_out)
    call("cdml_gather_rows", tp, row0, table.shape[0], tld, _p(idx, torch.int32), idx.numel(),
         feature_size, (1 if normalize else 0) | (2 if nan_missing else 0), xp, xld, _p(inv_norm_out),
         _p(oob_flag, torch.int32), _stream())
    return x_out


def gather_rows_x3(src, idx, feature_size, x_out_planes, nan_missing=False, oob_flag=None):
    """x_out_planes[r] = the three bf16 planes of the fp32 row src[idx[r]] as stored (the row exchange's last step on the
    split-fp32 path: request order and operand form in one pass)."""
    sp, sld = _mat(src)
    xp, xld = _mat16(x_out_planes)
    call("cdml_gather_rows_x3", sp, src.shape[0], sld, _p(idx, torch.int32), idx.numel(), feature_size, 2 if nan_missing else 0,
         xp, xld, _p(oob_flag, torch.int32), _stream())
    return x_out_planes


def _gather_format(table, x_out):
    """The suffix of the row format's entry points, from the types: fp16 table -> bf16 rows ("_f16", config 4), fp8 (e4m3)
    table -> bf16 rows ("_f8", include/cdml_f8.h); fp32 table -> fp32 rows (""), rows as three bf16 planes ("_x3", precision
    f32x3) or as two fp16 planes of x_hat * 2^14 ("_h2", f16x2)."""
    if table.dtype == torch.float16:
        return "_f16"
    if table.dtype == torch.float8_e4m3fn:
        return "_f8"
    return {torch.bfloat16: "_x3", torch.float16: "_h2"}.get(x_out.dtype, "")


def _gather_io(fmt, table, x_out, idx_out, n_steps, x_ki, x_ki_errors, kind_out=None, batch=0, lists=None):
    """What a fused sampler + gather launch derives from its tensors: (table pointer and leading dimension, x_out pointer and
    leading dimension, the per-step strides of x_out / idx_out / kind_out / x_ki, the listed draw's arguments or None).
    x_ki_errors: the caller's words for (x_ki with a format that has none, x_ki that is no contiguous bf16 buffer);
    lists: (lists, hard_fraction) of a listed launch, checked where that launch has always checked them."""
    tp, tld = {"_f16": _mat16, "_f8": _mat8}.get(fmt, _mat)(table)
    listed = None if lists is None else _lists_args(lists[0], table.shape[0], lists[1])
    omat = _mat16 if fmt else _mat
    if n_steps > 1:
        if x_out.dim() != 3 or idx_out.dim() != 2 or x_out.shape[0] != n_steps or idx_out.shape[0] != n_steps:
            raise ValueError("n_steps > 1 needs x_out [n_steps, rows, stride] and idx_out [n_steps, rows]")
        if kind_out is not None and (kind_out.dim() != 2 or kind_out.shape[0] != n_steps or kind_out.stride(1) != 1):
            raise ValueError("n_steps > 1 needs kind_out [n_steps, batch]")
        xp, xld = omat(x_out[0])
        xss, iss = x_out.stride(0), idx_out.stride(0)
        kss = kind_out.stride(0) if kind_out is not None else 0
    else:
        xp, xld = omat(x_out)
        xss = iss = kss = 0
    if kind_out is not None and kind_out.numel() < n_steps * batch:
        raise ValueError("kind_out needs one int32 per triplet")
    kis = 0
    if x_ki is not None:
        if fmt != "_x3":
            raise ValueError(x_ki_errors[0])
        if x_ki.dtype != torch.bfloat16 or not x_ki.is_contiguous():
            raise ValueError(x_ki_errors[1])
        kis = x_ki.stride(0) if (n_steps > 1 and x_ki.dim() > 1) else 0
    return (tp, tld), (xp, xld), (xss, iss, kss, kis), listed


def sample_gather(mode, pairs, seed, step, batch, table, feature_size, idx_out, x_out,
                  shift_out=None, slot0=0, batch_global=None, step_dev=None, n_steps=1, oob_flag=None, x_ki=None):
    """n_steps > 1: x_out is [n_steps, rows, stride], idx_out [n_steps, rows], shift_out [n_steps]
    (steps step, step+1, ... in one launch).  oob_flag (int32[1]): bit 0 set when a pair id lies
    outside the catalogue (the reference's IndexError, inputs.py:158).  x_ki (three-plane output only): a contiguous
    bf16 buffer [n_steps, 3 * rows * plane] that also receives every step's rows k8-interleaved."""
    bg = batch if batch_global is None else batch_global
    fmt = _gather_format(table, x_out)
    (tp, tld), (xp, xld), (xss, iss, _, kis), _ = _gather_io(
        fmt, table, x_out, idx_out, n_steps, x_ki, ("x_ki goes with the three-plane output and must be a contiguous bf16 buffer",) * 2)
    ki = () if x_ki is None else (C.c_void_p(x_ki.data_ptr()), kis)
    call("cdml_sample_gather" + (fmt if x_ki is None else "_x3k"), mode, _p(pairs, torch.int32), pairs.shape[0], seed,
         0 if step is None else step, _p(step_dev, torch.int64), batch, slot0, bg, tp,
         table.shape[0], tld, feature_size, _p(idx_out, torch.int32), _p(shift_out, torch.int32),
         xp, xld, n_steps, xss, iss, _p(oob_flag, torch.int32), *ki, _stream())
    return x_out


def hard_threshold(hard_fraction):
    """round(hard_fraction * 2^32): the listed draw's integer threshold (include/cdml_hardneg.h)."""
    h = float(hard_fraction)
    if not 0.0 <= h <= 1.0:
        raise ValueError("hard_fraction must be in [0, 1], got %r" % (hard_fraction,))
    return int(round(h * 4294967296.0))


def _lists_args(lists, n_rows, hard_fraction):
    """(pointer, ldl, L, hard_thresh) of a listed draw: lists int32 [n_rows, L] (unit inner stride), one row per video."""
    if lists.dim() != 2 or lists.stride(1) != 1 or lists.shape[0] != n_rows or lists.shape[1] < 1:
        raise ValueError("negative lists must be an int32 [n_rows = %d, L >= 1] tensor with unit inner stride, got %s"
                         % (n_rows, tuple(lists.shape)))
    return _p(lists, torch.int32), lists.stride(0), lists.shape[1], hard_threshold(hard_fraction)


def sample_listed(pairs, n_rows, seed, step, batch, lists, hard_fraction, idx_out, kind_out=None, slot0=0, batch_global=None,
                  step_dev=None):
    """The ids of the listed ("hard") negative draw, the twin of sample_uniform: idx_out int32 [3 * batch]; kind_out (int32
    [batch] or None) = 1 where the negative came from the anchor's list."""
    bg = batch if batch_global is None else batch_global
    lp, ldl, L, thresh = _lists_args(lists, n_rows, hard_fraction)
    call("cdml_sample_listed", _p(pairs, torch.int32), pairs.shape[0], n_rows, seed, 0 if step is None else step,
         _p(step_dev, torch.int64), batch, slot0, bg, lp, ldl, L, thresh, _p(idx_out, torch.int32), _p(kind_out, torch.int32),
         _stream())
    return idx_out


def sample_gather_listed(pairs, seed, step, batch, table, feature_size, lists, hard_fraction, idx_out, x_out, kind_out=None,
                         slot0=0, batch_global=None, step_dev=None, n_steps=1, oob_flag=None, x_ki=None):
    """sample_gather in sampler mode 2 (listed negatives, three rows per triplet): the row format follows the table's and
    x_out's types as there (fp32 rows, three bf16 planes with or without x_ki, fp16 table -> bf16 rows; the two-fp16-plane
    output has no listed form).  kind_out: int32 [batch], or [n_steps, batch] with n_steps > 1."""
    bg = batch if batch_global is None else batch_global
    fmt = _gather_format(table, x_out)
    if fmt == "_h2":
        raise ValueError("the two-fp16-plane rows (precision 'f16x2') have no listed form")
    (tp, tld), (xp, xld), (xss, iss, kss, kis), (lp, ldl, L, thresh) = _gather_io(
        fmt, table, x_out, idx_out, n_steps, x_ki, ("x_ki goes with the three-plane output", "x_ki must be a contiguous bf16 buffer"),
        kind_out, batch, (lists, hard_fraction))
    ki = (_p(x_ki), kis) if fmt == "_x3" else ()
    call("cdml_sample_gather_listed" + fmt, _p(pairs, torch.int32), pairs.shape[0], seed, 0 if step is None else step,
         _p(step_dev, torch.int64), batch, slot0, bg, tp, table.shape[0], tld, feature_size, lp, ldl, L, thresh,
         _p(idx_out, torch.int32), _p(kind_out, torch.int32), xp, xld, n_steps, xss, iss, kss, _p(oob_flag, torch.int32), *ki,
         _stream())
    return x_out


# ---- weighted negatives (sampler mode 3; include/cdml_negweights.h, the tables: negweights.NegativeWeights.tables) ----
def _weighted_args(tables, n_rows):
    """(start pointer, n_live, coarse pointer, bits) of a weighted draw; ``tables``: anything with device tensors ``start``
    (int32, uint32 bits) and ``coarse`` (int32 [2^bits + 1]), ``bits`` and ``n_live`` (negweights.NegTables)."""
    start, coarse, bits, n_live = tables.start, tables.coarse, int(tables.bits), int(tables.n_live)
    if not 8 <= bits <= 24:
        raise ValueError("bits must be in [8, 24], got %d" % bits)
    if coarse.dim() != 1 or coarse.numel() != (1 << bits) + 1 or not coarse.is_contiguous():
        raise ValueError("the coarse table holds 2^bits + 1 = %d int32 entries, got %s" % ((1 << bits) + 1, tuple(coarse.shape)))
    if start.dim() != 1 or not start.is_contiguous() or not 3 <= n_live <= start.numel() or n_live > n_rows:
        raise ValueError("the start table holds n_live int32 entries, 3 <= n_live <= n_rows = %d (got n_live = %d, %d entries)"
                         % (n_rows, n_live, start.numel()))
    return _p(start, torch.int32), n_live, _p(coarse, torch.int32), bits


def sample_weighted(pairs, n_rows, seed, step, batch, tables, idx_out, kind_out=None, slot0=0, batch_global=None, step_dev=None):
    """The ids of the weighted negative draw, the twin of sample_listed: idx_out int32 [3 * batch]; kind_out (int32 [batch]
    or None) = 1 where the negative came from the weighted draw, 0 where the uniform fall-back drew it."""
    bg = batch if batch_global is None else batch_global
    sp, n_live, cp, bits = _weighted_args(tables, n_rows)
    if kind_out is not None and kind_out.numel() < batch:
        raise ValueError("kind_out needs one int32 per triplet")
    call("cdml_sample_weighted", _p(pairs, torch.int32), pairs.shape[0], n_rows, seed, 0 if step is None else step,
         _p(step_dev, torch.int64), batch, slot0, bg, sp, n_live, cp, bits, _p(idx_out, torch.int32), _p(kind_out, torch.int32),
         _stream())
    return idx_out


def sample_gather_weighted(pairs, seed, step, batch, table, feature_size, tables, idx_out, x_out, kind_out=None,
                           slot0=0, batch_global=None, step_dev=None, n_steps=1, oob_flag=None, x_ki=None):
    """sample_gather in sampler mode 3 (weighted negatives, three rows per triplet): the row formats, x_ki and kind_out of
    sample_gather_listed (the two-fp16-plane output has no weighted form)."""
    bg = batch if batch_global is None else batch_global
    fmt = _gather_format(table, x_out)
    if fmt == "_h2":
        raise ValueError("the two-fp16-plane rows (precision 'f16x2') have no weighted form")
    (tp, tld), (xp, xld), (xss, iss, kss, kis), _ = _gather_io(
        fmt, table, x_out, idx_out, n_steps, x_ki, ("x_ki goes with the three-plane output", "x_ki must be a contiguous bf16 buffer"),
        kind_out, batch)
    sp, n_live, cp, bits = _weighted_args(tables, table.shape[0])
    ki = (_p(x_ki), kis) if fmt == "_x3" else ()
    call("cdml_sample_gather_weighted" + fmt, _p(pairs, torch.int32), pairs.shape[0], seed, 0 if step is None else step,
         _p(step_dev, torch.int64), batch, slot0, bg, tp, table.shape[0], tld, feature_size, sp, n_live, cp, bits,
         _p(idx_out, torch.int32), _p(kind_out, torch.int32), xp, xld, n_steps, xss, iss, kss, _p(oob_flag, torch.int32), *ki,
         _stream())
    return x_out


def negw_bias(lq, rows3, B, offset, neg_bias):
    """neg_bias[j] = lq[rows3[3j + 2]] + offset for j < B: the per-negative logQ of the drawn negatives (lq fp32 [n_rows],
    e.g. NegativeWeights' ``lq``); an id outside the catalogue gives 0."""
    if rows3.numel() < 3 * B or neg_bias.numel() < B:
        raise ValueError("negw_bias needs 3 B ids and B outputs")
    call("cdml_negw_bias", _p(lq, torch.float32), lq.numel(), _p(rows3, torch.int32), int(B), float(offset),
         _p(neg_bias, torch.float32), _stream())
    return neg_bias


def route_rows(ids, rows_per_shard, world, capacity, send_ids, slot_out, overflow_flag):
    call("cdml_route_rows", _p(ids, torch.int32), ids.numel(), rows_per_shard, world, capacity,
         _p(send_ids, torch.int32), _p(slot_out, torch.int32), _p(overflow_flag, torch.int32), _stream())


def scatter_rows(src, slot, dst, width):
    sp, sld = _mat(src)
    dp, dld = _mat(dst)
    call("cdml_scatter_rows", sp, sld, _p(slot, torch.int32), slot.numel(), width, dp, dld, _stream())
    return dst


# ----------------------------------------------------------------- tower ------
def l2norm_fwd(x, n_cols, y, inv_out=None):
    xp, xld = _mat(x)
    yp, yld = _mat(y)
    call("cdml_l2norm_fwd", xp, xld, x.shape[0], n_cols, yp, yld, _p(inv_out), _stream())
    return y


def l2norm_bwd(z, g, n_cols, dz, lrelu_alpha=-1.0):
    zp, zld = _mat(z)
    gp, gld = _mat(g)
    dp, dld = _mat(dz)
    call("cdml_l2norm_bwd", zp, zld, gp, gld, z.shape[0], n_cols, lrelu_alpha, dp, dld, _stream())
    return dz


def fc_lrelu_fwd(x, W, b, y, M, K, N, alpha=LRELU_ALPHA):
    xp, xld = _mat(x)
    wp, wld = _mat(W)
    yp, yld = _mat(y)
    call("cdml_fc_lrelu_fwd", xp, xld, wp, wld, _p(b, torch.float32), alpha, M, K, N, yp, yld,
         _stream())
    return y


def fc_bwd_data(dy, W, x_post, dx, M, K, N, alpha=LRELU_ALPHA):
    dyp, dyld = _mat(dy)
    wp, wld = _mat(W)
    dxp, dxld = _mat(dx)
    if x_post is None:
        xpp, xpld = C.c_void_p(0), 0
    else:
        xpp, xpld = _mat(x_post)
    call("cdml_fc_bwd_data", dyp, dyld, wp, wld, xpp, xpld, alpha, M, K, N, dxp, dxld, _stream())
    return dx


def fc_bwd_weight_workspace(M, K, N):
    return int(load_library().cdml_fc_bwd_weight_workspace(M, K, N))


def fc_bwd_weight(x, dy, dW, db, workspace, M, K, N):
    xp, xld = _mat(x)
    dyp, dyld = _mat(dy)
    wp, wld = _mat(dW)
    call("cdml_fc_bwd_weight", xp, xld, dyp, dyld, M, K, N, wp, wld, _p(db, torch.float32),
         _p(workspace), workspace.numel() * workspace.element_size(), _stream())
    return dW, db


def fc_bwd_weight2_workspace(M, K1, N1, K2, N2):
    """0 = shapes the stream-K launch does not take (use fc_bwd_weight per layer)."""
    return int(load_library().cdml_fc_bwd_weight2_workspace(M, K1, N1, K2, N2))


def fc_bwd_weight2(x1, dy1, dW1, db1, K1, N1, x2, dy2, dW2, db2, K2, N2, M, workspace):
    """Both weight gradients (and bias gradients) of the two-layer tower in one stream-K launch."""
    a1, lda1 = _mat(x1)
    b1, ldb1 = _mat(dy1)
    c1, ldc1 = _mat(dW1)
    a2, lda2 = _mat(x2)
    b2, ldb2 = _mat(dy2)
    c2, ldc2 = _mat(dW2)
    call("cdml_fc_bwd_weight2", a1, lda1, b1, ldb1, K1, N1, c1, ldc1, _p(db1, torch.float32), a2, lda2, b2, ldb2,
         K2, N2, c2, ldc2, _p(db2, torch.float32), M, _p(workspace), workspace.numel() * workspace.element_size(),
         _stream())


# ------------------------------------------------------------------ loss ------
def triplet_hinge(e, B, D, margin, pos, neg, hinge, stats=None, de=None):
    ep, eld = _mat(e)
    dep, deld = (C.c_void_p(0), 0) if de is None else _mat(de)
    call("cdml_triplet_hinge", ep, eld, B, D, margin, _p(pos), _p(neg), _p(hinge), _p(stats), dep,
         deld, _stream())


def triplet_hinge_inbatch(e, rows, shift, B, D, margin, pos, neg, hinge, valid=None, stats=None,
                          de=None):
    ep, eld = _mat(e)
    dep, deld = (C.c_void_p(0), 0) if de is None else _mat(de)
    call("cdml_triplet_hinge_inbatch", ep, eld, _p(rows, torch.int32), _p(shift, torch.int32), B, D,
         margin, _p(pos), _p(neg), _p(hinge), _p(valid, torch.uint8), _p(stats), dep, deld, _stream())


TICKET_WORDS = 128    # CDML_TICKET_WORDS (include/cdml.h)


def new_tickets(device):
    """Zeroed ticket words for cdml_adam_step's advance_step (its last block advances the counter)."""
    return torch.zeros(TICKET_WORDS, dtype=torch.int32, device=device)


def vnet_tail_workspace_floats(B, D):
    return int(load_library().cdml_vnet_tail_workspace(B, D)) // 4


def vnet_tail(mode, z, rows, shift, B, D, margin, e, pos, neg, hinge, dz2, valid=None, stats=None,
              dz2_bf16=None, var_ws=None, alpha=LRELU_ALPHA, plane_bf=0, h2_scale=0.0):
    """l2norm -> hinge loss -> its gradient -> l2norm backward -> lrelu' in one launch
    (mode 0: rows a,p,n per triplet; 1: in-batch negatives).  h2_scale > 0: dz2_bf16 receives the two fp16 planes of
    dz2 * h2_scale (precision f16x2), ``plane_bf`` apart."""
    zp, zld = _mat(z)
    ep, eld = _mat(e)
    dp, dld = _mat(dz2)
    bp, bld = (C.c_void_p(0), 0) if dz2_bf16 is None else _mat16(dz2_bf16)
    if h2_scale:
        call("cdml_vnet_tail_h2", mode, zp, zld, _p(rows, torch.int32), _p(shift, torch.int32), B, D, margin, alpha,
             ep, eld, _p(pos), _p(neg), _p(hinge), _p(valid, torch.uint8), dp, dld, bp, bld, plane_bf, float(h2_scale), _p(stats),
             _p(var_ws), _stream())
        return
    if plane_bf:                                     # dz2 also as its three bf16 planes (precision f32x3)
        call("cdml_vnet_tail_planes", mode, zp, zld, _p(rows, torch.int32), _p(shift, torch.int32), B, D, margin, alpha,
             ep, eld, _p(pos), _p(neg), _p(hinge), _p(valid, torch.uint8), dp, dld, bp, bld, plane_bf, _p(stats),
             _p(var_ws), _stream())
        return
    call("cdml_vnet_tail", mode, zp, zld, _p(rows, torch.int32), _p(shift, torch.int32), B, D, margin, alpha,
         ep, eld, _p(pos), _p(neg), _p(hinge), _p(valid, torch.uint8), dp, dld, bp, bld, _p(stats), _p(var_ws),
         _stream())


def semihard_select(S, e, rows, B, D, sqn_scratch, neg_row_out):
    sp, sld = _mat(S)
    ep, eld = _mat(e)
    call("cdml_semihard_select", sp, sld, ep, eld, _p(rows, torch.int32), B, D, _p(sqn_scratch),
         _p(neg_row_out, torch.int32), _stream())
    return neg_row_out


def semihard_mine_x3_workspace(B):
    return int(load_library().cdml_semihard_mine_x3_workspace(B))


def semihard_mine_x3(e, rows, B, D, e_planes, plane, sqn, dp, workspace, neg_row_out, z=None, h2_scale=0.0):
    """cdml_semihard_select's result without the score matrix: the B x 2B product on the plane kernels, the selection
    as its epilogue (csrc/gemm_bf16x3.hip).  e_planes bf16 [2B, >= 3 plane], sqn f32[2B], dp f32[B], workspace f32.
    ``z`` given: the un-normalised output rows -- the prep launch normalises them and WRITES ``e`` (cdml_semihard_mine_x3_z).
    ``h2_scale`` > 0: the score product on two fp16 planes of e * h2_scale (e_planes fp16 [2B, >= 2 plane]; cdml_semihard_mine_h2)."""
    ep, eld = _mat(e)
    pp, pld = _mat16(e_planes)
    if h2_scale:
        zp, zld = (C.c_void_p(0), 0) if z is None else _mat(z)
        call("cdml_semihard_mine_h2", zp, zld, ep, eld, _p(rows, torch.int32), B, D, pp, pld, plane, float(h2_scale), _p(sqn), _p(dp),
             _p(workspace), workspace.numel() * workspace.element_size(), _p(neg_row_out, torch.int32), _stream())
        return neg_row_out
    if z is not None:
        zp, zld = _mat(z)
        call("cdml_semihard_mine_x3_z", zp, zld, ep, eld, _p(rows, torch.int32), B, D, pp, pld, plane, _p(sqn), _p(dp),
             _p(workspace), workspace.numel() * workspace.element_size(), _p(neg_row_out, torch.int32), _stream())
        return neg_row_out
    call("cdml_semihard_mine_x3", ep, eld, _p(rows, torch.int32), B, D, pp, pld, plane, _p(sqn), _p(dp),
         _p(workspace), workspace.numel() * workspace.element_size(), _p(neg_row_out, torch.int32), _stream())
    return neg_row_out


def triplet_hinge_indexed(e, neg_row, B, D, margin, pos, neg, hinge, scale_scratch, stats=None, de=None, z=None, dz2=None,
                          dz2_bf16=None, plane_bf=0, lrelu_alpha=LRELU_ALPHA):
    """Hinge loss + gradient over (row 2i, row 2i+1, row neg_row[i]).  ``z`` and ``dz2`` given: the finished row gradients
    also go through l2norm_bwd (+ leaky-relu') into dz2 -- and into its bf16 copy / three planes (``dz2_bf16``,
    ``plane_bf``) -- inside the same launch (cdml_triplet_hinge_indexed_tail)."""
    ep, eld = _mat(e)
    dep, deld = (C.c_void_p(0), 0) if de is None else _mat(de)
    if z is None:
        call("cdml_triplet_hinge_indexed", ep, eld, _p(neg_row, torch.int32), B, D, margin, _p(pos), _p(neg),
             _p(hinge), _p(stats), _p(scale_scratch), dep, deld, _stream())
        return
    zp, zld = _mat(z)
    dzp, dzld = _mat(dz2)
    bp, bld = (C.c_void_p(0), 0) if dz2_bf16 is None else _mat16(dz2_bf16)
    call("cdml_triplet_hinge_indexed_tail", ep, eld, _p(neg_row, torch.int32), B, D, margin, _p(pos), _p(neg),
         _p(hinge), _p(stats), _p(scale_scratch), dep, deld, zp, zld, lrelu_alpha, dzp, dzld, bp, bld, plane_bf, _stream())


# ---- multi-class N-pair loss (in-batch softmax, csrc/npair.hip; build-defined) ----
NPAIR_PRECISIONS = ("f32x3", "f32", "bf16")
# (the mixed-negatives and data-parallel chains have no one-plane form yet: NPairMixed / NPairDP)
NPAIR_FP32_PRECISIONS = ("f32x3", "f32")
# pairs per batch must be a multiple of: f32x3 -- the plane GEMMs' 256 x 256 tiles (S is B x B, the two gradient products
# contract over B); f32 -- the fp32 GEMMs' 64-wide K tiles (fc_bwd_data / fc_bwd_weight contract over B); bf16 -- the bf16
# GEMMs' 256 x 256 tiles (dP = W^T A on gemm_bf16_tn: M and N multiples of 256, K of 128)
NPAIR_TILE = {"f32x3": 256, "f32": 64, "bf16": 256}
_NPAIR_PRECISION_MSG = "the N-pair loss runs on precision 'f32x3', 'f32' or 'bf16', not %r"


def npair_workspace(B):
    return int(load_library().cdml_npair_workspace(int(B)))


def npair_stats(S, rows, B, temperature, symmetric, lse, stats, workspace):
    """lse[:B] (and lse[B:2B] with ``symmetric``) and stats[0..3] from the score matrix S [>= B, >= B] (cdml_npair_stats).
    rows: int32 [2B] video ids (row 2i = anchor i, 2i+1 = positive i) or None (no duplicates)."""
    sp, sld = _mat(S)
    call("cdml_npair_stats", sp, sld, _p(rows, torch.int32), int(B), float(temperature), 1 if symmetric else 0, _p(lse),
         _p(stats), _p(workspace), workspace.numel() * workspace.element_size(), _stream())
    return lse, stats


def npair_grad_x3(S, rows, B, temperature, symmetric, lse, W_planes, plane):
    """W_planes bf16 [>= B, >= 2 plane + B] <- the three bf16 planes of the gradient weights (cdml_npair_grad_x3)."""
    sp, sld = _mat(S)
    wp, wld = _mat16(W_planes)
    call("cdml_npair_grad_x3", sp, sld, _p(rows, torch.int32), int(B), float(temperature), 1 if symmetric else 0, _p(lse),
         wp, wld, int(plane), _stream())
    return W_planes


def npair_grad_f32(S, rows, B, temperature, symmetric, lse, W):
    """W fp32 [>= B, >= B] <- the gradient weights (cdml_npair_grad_f32)."""
    sp, sld = _mat(S)
    wp, wld = _mat(W)
    call("cdml_npair_grad_f32", sp, sld, _p(rows, torch.int32), int(B), float(temperature), 1 if symmetric else 0, _p(lse),
         wp, wld, _stream())
    return W


# ---- the config-4 precision (fp16 catalogue, bf16 MFMA): one bf16 plane of every operand and of W (csrc/npair_bf16.hip,
# include/cdml_npair_bf16.h) ----
def npair_operands_bf16(e, B, D, A, P, PT):
    """cdml_npair_operands_bf16: A, P bf16 [>= B, >= D] <- the rounded rows e[0::2] / e[1::2] (e fp32 [>= 2B, >= D]) and
    PT bf16 [>= D, >= B] <- P^T, in one launch; nothing else of the three images is written."""
    ep, eld = _mat(e)
    ap, ald = _mat16(A)
    pp, pld = _mat16(P)
    tp, tld = _mat16(PT)
    call("cdml_npair_operands_bf16", ep, eld, int(B), int(D), ap, ald, pp, pld, tp, tld, _stream())


def npair_grad_bf16(S, rows, B, temperature, symmetric, lse, W, bias=None):
    """W bf16 [>= B, >= B] <- the gradient weights npair_grad_f32 (bias: npair_logq_grad_f32) writes, rounded to nearest even."""
    sp, sld = _mat(S)
    wp, wld = _mat16(W)
    if bias is None:
        call("cdml_npair_grad_bf16", sp, sld, _p(rows, torch.int32), int(B), float(temperature), 1 if symmetric else 0,
             _p(lse), wp, wld, _stream())
    else:
        call("cdml_npair_logq_grad_bf16", sp, sld, _p(rows, torch.int32), int(B), _p(bias, torch.float32), float(temperature),
             1 if symmetric else 0, _p(lse), wp, wld, _stream())
    return W


def npair_memory_grad_bf16(S, rows, B, mem_col, mem_id, temperature, symmetric, lse, W, mem_bias=None):
    """W's memory block (columns mem_col .. mem_col + M - 1) <- npair_memory_grad_f32's (mem_bias: _logq_grad_f32's) values,
    rounded to nearest even."""
    sp, sld = _mat(S)
    wp, wld = _mat16(W)
    if mem_bias is None:
        call("cdml_npair_memory_grad_bf16", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
             mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), wp, wld, _stream())
    else:
        call("cdml_npair_memory_logq_grad_bf16", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
             _p(mem_bias, torch.float32), mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), wp, wld,
             _stream())
    return W


def npair_memory_push_bf16(P, rows, B, D, step, step_dev, start, mem, mem_id, R, T):
    """cdml_npair_memory_push_bf16: npair_memory_push with the slots' one-plane images R bf16 [M, >= D], T bf16 [>= D, >= M]."""
    pp, pld = _mat(P)
    mp, mld = _mat(mem)
    rp, rld = _mat16(R)
    tp, tld = _mat16(T)
    call("cdml_npair_memory_push_bf16", pp, pld, _p(rows, torch.int32), int(B), int(D), 0 if step is None else int(step),
         _p(step_dev, torch.int64), int(start), mem_id.numel(), mp, mld, _p(mem_id, torch.int32), rp, rld, tp, tld, _stream())


def _npair_bf16_gemm_ws(Bp, K, Dq, device):
    """The split-K workspace of the chain's three bf16 products: S = A [P; Mem]^T (Bp x K over Dq), dA = W [P; Mem]
    (Bp x Dq over K), dP = W^T A (Bp x Dq over Bp)."""
    if not gemm_bf16_tn_supported(Bp, Dq, Bp, K, Dq):
        raise ValueError("precision 'bf16': dP = W^T A (%d x %d over %d, W's leading dimension %d) does not fit gemm_bf16_tn"
                         % (Bp, Dq, Bp, K))
    nb = max(gemm_bf16_workspace(Bp, K, Dq), gemm_bf16_workspace(Bp, Dq, K), gemm_bf16_tn_workspace(Bp, Dq, Bp), 16)
    return torch.zeros(nb // 4, dtype=torch.float32, device=device)


class NPairWorkspace:
    """Every buffer of the N-pair chain for Bp pairs of Dp-wide rows (Bp a multiple of NPAIR_TILE[precision]), allocated
    once: ``npair_loss`` then allocates nothing (hipGraph-capturable).  Pad rows and columns of W stay zero.
    ``in_batch=False``: without the in-batch chain's S, W and positive planes (a chain that always runs with an NPairMemory,
    which holds its own concatenated ones)."""

    def __init__(self, Bp, Dp, precision, device, in_batch=True):
        if precision not in NPAIR_PRECISIONS:
            raise ValueError(_NPAIR_PRECISION_MSG % (precision,))
        tile = NPAIR_TILE[precision]
        if Bp < tile or Bp % tile:
            raise ValueError("precision %r: the N-pair loss needs a batch that is a multiple of %d pairs (got %d)"
                             % (precision, tile, Bp))
        if Dp % 64:
            raise ValueError("the N-pair loss needs an embedding width that is a multiple of 64 (got %d)" % Dp)
        self.Bp, self.Dp, self.precision, self.in_batch = int(Bp), int(Dp), precision, bool(in_batch)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=device)
        self.S = f32(Bp, Bp) if in_batch else None
        self.lse = f32(2 * Bp)
        self.bias = f32(2 * Bp)                             # logQ correction: lq of every row, laid out like the ids
        self.ws = torch.zeros(npair_workspace(Bp) // 4, dtype=torch.float32, device=device)
        if precision == "f32x3":
            self.Dq = Dq = (Dp + 255) // 256 * 256          # the plane GEMMs' N tile: narrower rows are zero-padded
            self.A3 = bf(Bp, 3 * Dq)
            if in_batch:
                self.P3 = bf(Bp, 3 * Dq)
                self.PT3 = bf(Dq, 3 * Bp)                   # the positives transposed: dA = W . P's k-contiguous operand
                self.W3 = bf(Bp, 3 * Bp)
                nb = max(gemm_bf16x3_workspace(False, Bp, Bp, Dq), gemm_bf16x3_workspace(False, Bp, Dq, Bp),
                         gemm_bf16x3_workspace(True, Bp, Dq, Bp), 16)
                self.gemm_ws = torch.zeros(nb // 4, dtype=torch.float32, device=device)
            self.dA = f32(Bp, Dq) if Dq != Dp else None     # (rows narrower than the tile: the products land here first)
            self.dP = f32(Bp, Dq) if Dq != Dp else None
        elif precision == "bf16":                           # one bf16 plane of every operand (include/cdml_npair_bf16.h)
            self.Dq = Dq = (Dp + 255) // 256 * 256          # gemm_bf16_tn's N tile: narrower rows are zero-padded
            self.A16 = bf(Bp, Dq)
            if in_batch:
                self.P16 = bf(Bp, Dq)
                self.PT16 = bf(Dq, Bp)                      # the positives transposed: dA = W . P's k-contiguous operand
                self.W16 = bf(Bp, Bp)
                self.gemm_ws = _npair_bf16_gemm_ws(Bp, Bp, Dq, device)
            self.dA = f32(Bp, Dq) if Dq != Dp else None
            self.dP = f32(Bp, Dq) if Dq != Dp else None
        else:
            self.Wf = f32(Bp, Bp) if in_batch else None
            self.zero_bias = f32(Dp)
            self.bw = torch.zeros(max(fc_bwd_weight_workspace(Bp, Bp, Dp), 16) // 4, dtype=torch.float32, device=device)

    def W(self):
        """the gradient weights as one fp32 tensor [Bp, Bp] (tests, debugging)"""
        if self.precision == "f32":
            return self.Wf
        if self.precision == "bf16":
            return self.W16.float()
        Bp = self.Bp
        return self.W3[:, :Bp].float() + self.W3[:, Bp:2 * Bp].float() + self.W3[:, 2 * Bp:].float()


def npair_memory_workspace(B, M):
    return int(load_library().cdml_npair_memory_workspace(int(B), int(M)))


def npair_memory_stats(S, rows, B, mem_col, mem_id, temperature, symmetric, lse, stats, workspace):
    """cdml_npair_memory_stats: npair_stats over S = A [P; Mem]^T, the memory's M = mem_id.numel() columns at mem_col."""
    sp, sld = _mat(S)
    call("cdml_npair_memory_stats", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
         mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), _p(stats), _p(workspace),
         workspace.numel() * workspace.element_size(), _stream())
    return lse, stats


def npair_memory_grad_x3(S, rows, B, mem_col, mem_id, temperature, symmetric, lse, W_planes, plane):
    """W_planes' memory block (columns mem_col .. mem_col + M - 1 of each plane) <- cdml_npair_memory_grad_x3."""
    sp, sld = _mat(S)
    wp, wld = _mat16(W_planes)
    call("cdml_npair_memory_grad_x3", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
         mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), wp, wld, int(plane), _stream())
    return W_planes


def npair_memory_grad_f32(S, rows, B, mem_col, mem_id, temperature, symmetric, lse, W):
    """W's memory block (columns mem_col .. mem_col + M - 1) <- cdml_npair_memory_grad_f32."""
    sp, sld = _mat(S)
    wp, wld = _mat(W)
    call("cdml_npair_memory_grad_f32", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
         mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), wp, wld, _stream())
    return W


def npair_memory_push(P, rows, B, D, step, step_dev, start, mem, mem_id, R3=None, plane_r=0, T3=None, plane_t=0):
    """cdml_npair_memory_push: the positives P [>= B, >= D] and their ids rows[1::2] into the ring slots of step
    ``step`` + *step_dev (mem fp32 [M, >= D], mem_id int32 [M]); R3 / T3: the slots' plane images (precision f32x3)."""
    pp, pld = _mat(P)
    mp, mld = _mat(mem)
    rp, rld = (C.c_void_p(0), 0) if R3 is None else _mat16(R3)
    tp, tld = (C.c_void_p(0), 0) if T3 is None else _mat16(T3)
    call("cdml_npair_memory_push", pp, pld, _p(rows, torch.int32), int(B), int(D), 0 if step is None else int(step),
         _p(step_dev, torch.int64), int(start), mem_id.numel(), mp, mld, _p(mem_id, torch.int32), rp, rld, int(plane_r),
         tp, tld, int(plane_t), _stream())


class NPairMemory:
    """The cross-batch memory of the N-pair loss (XBM, Wang et al. 2020; build-defined): a FIFO ring of the last M
    positives (fp32 unit rows ``rows`` [M, Dp] and video ids ``ids`` [M], -1 = empty) that ``npair_loss(memory=...)``
    uses as M more negatives of every anchor, without a gradient.  It owns the chain's concatenated buffers, allocated once
    (hipGraph-capturable): S [Bp, Bp + M] and W over K = Bp + M, and the operand [P; Mem] -- f32x3: its row planes
    ``PM3`` [Bp + M, 3 Dq] and transposed planes ``PMT3`` [Dq, 3 (Bp + M)], the ring's part written by the push (never
    re-split); f32: fp32 ``PM`` [Bp + M, Dp], whose last M rows ARE ``rows``.  Step t pushes its Bp positives into slots
    ((t - start) mod (M / Bp)) Bp ..; steps before ``start`` push nothing.  M: a multiple of Bp and of
    NPAIR_TILE[precision]."""

    def __init__(self, size, Bp, Dp, precision, device, start=0):
        if precision not in NPAIR_PRECISIONS:
            raise ValueError(_NPAIR_PRECISION_MSG % (precision,))
        M, tile = int(size), NPAIR_TILE[precision]
        if M < 1 or M % int(Bp) or M % tile:
            raise ValueError("precision %r: the memory size must be a positive multiple of the batch (%d pairs) and of %d "
                             "(got %d)" % (precision, Bp, tile, M))
        if int(start) < 0:
            raise ValueError("memory_start must be >= 0, got %r" % (start,))
        self.M, self.Bp, self.Dp, self.precision, self.start = M, int(Bp), int(Dp), precision, int(start)
        self.K = K = self.Bp + M                            # the contraction of dA = W [P; Mem]
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=device)
        self.ids = torch.full((M,), -1, dtype=torch.int32, device=device)
        self.bias = f32(M)                                  # logQ correction: lq of every slot's video
        self.S = f32(Bp, K)
        if precision == "f32x3":
            self.Dq = Dq = (Dp + 255) // 256 * 256
            self.rows = f32(M, Dp)
            self.PM3, self.PMT3 = bf(K, 3 * Dq), bf(Dq, 3 * K)
            self.W3 = bf(Bp, 3 * K)
            nb = max(gemm_bf16x3_workspace(False, Bp, K, Dq), gemm_bf16x3_workspace(False, Bp, Dq, K),
                     gemm_bf16x3_workspace(True, Bp, Dq, Bp), 16)
            self.gemm_ws = torch.zeros(nb // 4, dtype=torch.float32, device=device)
        elif precision == "bf16":                           # [P; Mem] and its transpose in one bf16 plane each
            self.Dq = Dq = (Dp + 255) // 256 * 256
            self.rows = f32(M, Dp)
            self.PM16, self.PMT16 = bf(K, Dq), bf(Dq, K)
            self.W16 = bf(Bp, K)
            self.gemm_ws = _npair_bf16_gemm_ws(Bp, K, Dq, device)
        else:
            self.PM = f32(K, Dp)
            self.rows = self.PM[Bp:]
            self.Wf = f32(Bp, K)

    def load(self, rows, ids):
        """Set the ring: rows fp32 [M, Dp], ids int [M] (-1 = empty); the f32x3 planes are re-derived (hi + mid + lo is
        exactly the fp32 value, so they are the bits the pushes would have written), and so are the bf16 images (the
        round-to-nearest-even of the fp32 rows, as the push writes them)."""
        if tuple(rows.shape) != (self.M, self.Dp) or tuple(ids.shape) != (self.M,):
            raise ValueError("a ring of %d rows x %d columns and %d ids, got %s and %s"
                             % (self.M, self.Dp, self.M, tuple(rows.shape), tuple(ids.shape)))
        self.rows.copy_(rows.to(device=self.rows.device, dtype=torch.float32))
        self.ids.copy_(ids.to(device=self.ids.device, dtype=torch.int32))
        if self.precision == "f32x3":
            split_f32_bf16x3(self.rows, self.PM3[self.Bp:], self.Dq)
            split_f32_bf16x3(self.rows, self.PMT3[:, self.Bp:], self.K, transpose=True)
        elif self.precision == "bf16":
            cast_f32_bf16(self.rows, self.PM16[self.Bp:], self.M, self.Dp)
            transpose_to_bf16(self.rows, self.PMT16[:, self.Bp:], self.M, self.Dp)

    def clear(self):
        self.load(torch.zeros_like(self.rows), torch.full_like(self.ids, -1))

    def W(self):
        """the gradient weights as one fp32 tensor [Bp, Bp + M] (tests, debugging)"""
        if self.precision == "f32":
            return self.Wf
        if self.precision == "bf16":
            return self.W16.float()
        K = self.K
        return self.W3[:, :K].float() + self.W3[:, K:2 * K].float() + self.W3[:, 2 * K:].float()

    def state_dict(self):
        return {"size": self.M, "rows": self.rows.detach().cpu().clone(), "ids": self.ids.detach().cpu().clone()}


# ---- sampling-bias (logQ) correction of the N-pair loss (Yi et al. 2019; csrc/npair_logq.hip; build-defined) ----
def npair_logq_stats(S, rows, B, bias, temperature, symmetric, lse, stats, workspace):
    """npair_stats with every logit less its candidate's lq (bias fp32 [>= 2B], laid out like rows)."""
    sp, sld = _mat(S)
    call("cdml_npair_logq_stats", sp, sld, _p(rows, torch.int32), int(B), _p(bias, torch.float32), float(temperature),
         1 if symmetric else 0, _p(lse), _p(stats), _p(workspace), workspace.numel() * workspace.element_size(), _stream())
    return lse, stats


def npair_logq_grad_x3(S, rows, B, bias, temperature, symmetric, lse, W_planes, plane):
    sp, sld = _mat(S)
    wp, wld = _mat16(W_planes)
    call("cdml_npair_logq_grad_x3", sp, sld, _p(rows, torch.int32), int(B), _p(bias, torch.float32), float(temperature),
         1 if symmetric else 0, _p(lse), wp, wld, int(plane), _stream())
    return W_planes


def npair_logq_grad_f32(S, rows, B, bias, temperature, symmetric, lse, W):
    sp, sld = _mat(S)
    wp, wld = _mat(W)
    call("cdml_npair_logq_grad_f32", sp, sld, _p(rows, torch.int32), int(B), _p(bias, torch.float32), float(temperature),
         1 if symmetric else 0, _p(lse), wp, wld, _stream())
    return W


def npair_memory_logq_stats(S, rows, B, bias, mem_col, mem_id, mem_bias, temperature, symmetric, lse, stats, workspace):
    sp, sld = _mat(S)
    call("cdml_npair_memory_logq_stats", sp, sld, _p(rows, torch.int32), int(B), _p(bias, torch.float32), int(mem_col),
         _p(mem_id, torch.int32), _p(mem_bias, torch.float32), mem_id.numel(), float(temperature), 1 if symmetric else 0,
         _p(lse), _p(stats), _p(workspace), workspace.numel() * workspace.element_size(), _stream())
    return lse, stats


def npair_memory_logq_grad_x3(S, rows, B, mem_col, mem_id, mem_bias, temperature, symmetric, lse, W_planes, plane):
    sp, sld = _mat(S)
    wp, wld = _mat16(W_planes)
    call("cdml_npair_memory_logq_grad_x3", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
         _p(mem_bias, torch.float32), mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), wp, wld, int(plane),
         _stream())
    return W_planes


def npair_memory_logq_grad_f32(S, rows, B, mem_col, mem_id, mem_bias, temperature, symmetric, lse, W):
    sp, sld = _mat(S)
    wp, wld = _mat(W)
    call("cdml_npair_memory_logq_grad_f32", sp, sld, _p(rows, torch.int32), int(B), int(mem_col), _p(mem_id, torch.int32),
         _p(mem_bias, torch.float32), mem_id.numel(), float(temperature), 1 if symmetric else 0, _p(lse), wp, wld, _stream())
    return W


def logq_table_gather(table, rows, B, mem_id, bias, mem_bias):
    """bias[:2B] <- table[rows[:2B]], mem_bias <- table[mem_id] (0 for -1 and for ids outside the table)."""
    call("cdml_logq_table_gather", _p(table, torch.float32), table.numel(), _p(rows, torch.int32), int(B),
         _p(mem_id, torch.int32), 0 if mem_id is None else mem_id.numel(), _p(bias, torch.float32),
         _p(mem_bias, torch.float32), _stream())


def logq_stream_gather(last, gap, rows, B, mem_id, bias, mem_bias, snap_last, snap_gap):
    call("cdml_logq_stream_gather", _p(last, torch.int32), _p(gap, torch.float32), gap.numel(), _p(rows, torch.int32),
         int(B), _p(mem_id, torch.int32), 0 if mem_id is None else mem_id.numel(), _p(bias, torch.float32),
         _p(mem_bias, torch.float32), _p(snap_last, torch.int32), _p(snap_gap, torch.float32), _stream())


def logq_stream_update(last, gap, rows, B, snap_last, snap_gap, alpha, step, step_dev):
    call("cdml_logq_stream_update", _p(last, torch.int32), _p(gap, torch.float32), gap.numel(), _p(rows, torch.int32),
         int(B), _p(snap_last, torch.int32), _p(snap_gap, torch.float32), float(alpha), 0 if step is None else int(step),
         _p(step_dev, torch.int64), _stream())


def logq_stream_reset(last, gap, g0):
    call("cdml_logq_stream_reset", _p(last, torch.int32), _p(gap, torch.float32), gap.numel(), float(g0), _stream())


class LogQTable:
    """A fixed per-video log sampling probability lq(v) = logq[v] (fp32 [n_videos], every entry finite) as the source of
    ``npair_loss(logq=...)``'s correction -- e.g. the log of each video's share of the co-watch degrees."""

    def __init__(self, logq, device):
        t = torch.as_tensor(logq).detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        if t.numel() < 1:
            raise ValueError("a logQ table needs at least one entry")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("every entry of the logQ table must be finite")
        self.table, self.n_videos = t, t.numel()

    def logq(self):
        return self.table

    def gather(self, rows, B, mem_id, bias, mem_bias):
        logq_table_gather(self.table, rows, B, mem_id, bias, mem_bias)

    def update(self, rows, B, step, step_dev):
        pass                                                # a fixed table does not learn

    def state_dict(self):
        return {"logq": self.table.detach().cpu().clone()}

    def load(self, state):
        t = torch.as_tensor(state["logq"]).reshape(-1)
        if t.numel() != self.n_videos or not bool(torch.isfinite(t).all()):
            raise ValueError("a logQ table of %d finite entries, got %d" % (self.n_videos, t.numel()))
        self.table.copy_(t.to(device=self.table.device, dtype=torch.float32))


class LogQEstimator:
    """Yi et al.'s streaming estimate of each video's sampling probability, indexed by video id: ``last`` int32
    [n_videos] (the step the video was last drawn as a positive, -1 = unseen) and ``gap`` fp32 [n_videos] (the smoothed
    steps between draws, initially g0 = ``init_gap`` or max(1, n_videos / Bp)); lq(v) = -log(gap[v]).  Step t updates every
    positive video of its batch once, after the products that read the bias: gap = (1 - alpha) gap + alpha (t - last)
    when seen before, last = t (csrc/npair_logq.hip).  Bp: the batch's pairs (the snapshot buffers)."""

    def __init__(self, n_videos, Bp, alpha=0.01, init_gap=None, device="cuda"):
        n, Bp, alpha = int(n_videos), int(Bp), float(alpha)
        if n < 1 or n > 2 ** 31 - 1:
            raise ValueError("n_videos must be in [1, 2^31 - 1], got %d" % n)
        if not 0.0 < alpha <= 1.0:
            raise ValueError("logq_alpha must be in (0, 1], got %r" % (alpha,))
        g0 = max(1.0, n / Bp) if init_gap is None else float(init_gap)
        if not (1.0 <= g0 < float("inf")):
            raise ValueError("logq_init_gap must be finite and >= 1, got %r" % (init_gap,))
        self.n_videos, self.Bp, self.alpha, self.init_gap = n, Bp, alpha, g0
        self.last = torch.empty(n, dtype=torch.int32, device=device)
        self.gap = torch.empty(n, dtype=torch.float32, device=device)
        self.snap_last = torch.zeros(Bp, dtype=torch.int32, device=device)
        self.snap_gap = torch.zeros(Bp, dtype=torch.float32, device=device)
        self.reset()

    def reset(self):
        logq_stream_reset(self.last, self.gap, self.init_gap)

    def logq(self):
        return -torch.log(self.gap)

    def gather(self, rows, B, mem_id, bias, mem_bias):
        logq_stream_gather(self.last, self.gap, rows, B, mem_id, bias, mem_bias, self.snap_last, self.snap_gap)

    def update(self, rows, B, step, step_dev):
        logq_stream_update(self.last, self.gap, rows, B, self.snap_last, self.snap_gap, self.alpha, step, step_dev)

    def state_dict(self):
        return {"last": self.last.detach().cpu().clone(), "gap": self.gap.detach().cpu().clone(), "alpha": self.alpha,
                "init_gap": self.init_gap}

    def load(self, state):
        if tuple(state["last"].shape) != (self.n_videos,) or tuple(state["gap"].shape) != (self.n_videos,):
            raise ValueError("a logQ estimator of %d videos, got %s / %s"
                             % (self.n_videos, tuple(state["last"].shape), tuple(state["gap"].shape)))
        self.alpha, self.init_gap = float(state["alpha"]), float(state["init_gap"])
        self.last.copy_(state["last"].to(device=self.last.device, dtype=torch.int32))
        self.gap.copy_(state["gap"].to(device=self.gap.device, dtype=torch.float32))


def npair_loss(e, rows, B, Dp, temperature=0.1, symmetric=True, precision="f32x3", de=None, stats=None, ws=None,
               memory=None, step=0, step_dev=None, logq=None):
    """The multi-class N-pair loss of B pairs and its gradient (include/cdml.h, "multi-class N-pair loss").
    e: fp32 [2 Bp, Dp] unit rows, row 2i = anchor i, row 2i+1 = positive i (rows >= 2B zero: padding); rows: int32 [2 Bp]
    video ids or None.  The chain: S = A P^T -> row (and column) log-sum-exp + step scalars -> W -> dA = W P, dP = W^T A,
    written into de[0::2] / de[1::2] (fp32 [2 Bp, Dp]; None: loss only).  Precision "f32x3": fp32 operands as three
    bf16 planes on the plane GEMMs; "f32": the fp32-MFMA GEMMs; "bf16": the config-4 precision -- the rows rounded to ONE
    bf16 plane, W in one bf16 plane, each product one pass of the bf16 GEMMs with fp32 accumulation (S, the statistics and
    the gradient stay fp32).  stats: fp32 [>= 4] (loss, mean positive distance,
    mean counted-negative distance, fraction of counted negatives).  ws: an NPairWorkspace (allocated here if None).
    memory: an NPairMemory (B == Bp, video ids given): its ring adds M negatives to every anchor's row term -- S = A [P;
    Mem]^T -> statistics -> W (the in-batch block + the memory block) -> dA = W [P; Mem] over K = Bp + M, dP = W^T A ->
    with ``de``, the push of this step's positives (step number ``step`` + *step_dev, the sampler's convention).
    logq: the sampling-bias correction (Yi et al. 2019) -- every logit less its candidate's log sampling probability lq.
    A LogQTable or LogQEstimator (video ids ``rows`` required): one gather launch fills ws.bias (and the memory's bias)
    before the statistics, and with ``de`` an estimator's update follows the gradient weights (before the push); or a
    fp32 tensor [>= 2B] of each row's lq, laid out like ``rows`` (no memory).  None: the uncorrected chain, launch for launch.
    Returns (stats, lse): lse[:B] the rows', lse[B:2B] the columns' (symmetric)."""
    if not (temperature > 0.0) or temperature == float("inf"):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    Bp = e.shape[0] // 2
    if e.shape[0] != 2 * Bp or not 1 <= B <= Bp:
        raise ValueError("e must hold 2 Bp rows with 1 <= B <= Bp")
    if ws is None:
        ws = NPairWorkspace(Bp, Dp, precision, e.device)
    elif (ws.Bp, ws.Dp, ws.precision) != (Bp, Dp, precision):
        raise ValueError("NPairWorkspace is for %d pairs x %d columns on %s" % (ws.Bp, ws.Dp, ws.precision))
    if stats is None:
        stats = torch.zeros(4, dtype=torch.float32, device=e.device)
    if memory is None and not ws.in_batch:
        raise ValueError("this NPairWorkspace was allocated for the cross-batch memory's chain only (in_batch=False)")
    if logq is not None:
        if isinstance(logq, torch.Tensor):
            if memory is not None:
                raise ValueError("a per-row logQ tensor has no memory part: give a LogQTable / LogQEstimator with a memory")
            if logq.numel() < 2 * B:
                raise ValueError("a per-row logQ tensor needs 2B = %d entries, got %d" % (2 * B, logq.numel()))
        elif rows is None:
            raise ValueError("the logQ correction needs the rows' video ids")
    return _npair_chain(e, rows, B, Dp, temperature, symmetric, precision, de, stats, ws, memory, step, step_dev, logq)


def _npair_buffers(precision, ws, mem):
    """(K, S, W, the row image of [P; Mem], its transposed image, the GEMM workspace): the in-batch chain's (K = Bp, from
    the NPairWorkspace) or, with a memory, the concatenated ones it owns (K = Bp + M).  f32 has no images: None."""
    if precision == "f32x3":
        return (ws.Bp, ws.S, ws.W3, ws.P3, ws.PT3, ws.gemm_ws) if mem is None else \
            (mem.K, mem.S, mem.W3, mem.PM3, mem.PMT3, mem.gemm_ws)
    if precision == "bf16":
        return (ws.Bp, ws.S, ws.W16, ws.P16, ws.PT16, ws.gemm_ws) if mem is None else \
            (mem.K, mem.S, mem.W16, mem.PM16, mem.PMT16, mem.gemm_ws)
    return (ws.Bp, ws.S, ws.Wf, None, None, None) if mem is None else (mem.K, mem.S, mem.Wf, mem.PM, None, None)


def _npair_scores(precision, e, ws, K, S, PM, PMT, gws):
    """The operands of the batch (the batch's part of both images of [P; Mem]) and S = A [P; Mem]^T.  Returns [P; Mem] as
    the dA product reads it on f32 (fp32 rows)."""
    Bp, Dp = ws.Bp, ws.Dp
    A, P = e[0::2, :Dp], e[1::2, :Dp]
    if precision == "f32x3":
        Dq = ws.Dq
        split_f32_bf16x3(A, ws.A3, Dq)
        split_f32_bf16x3(P, PM[:Bp], Dq)
        split_f32_bf16x3(P, PMT, K, transpose=True)
        gemm_bf16x3_nt(BE_F32, ws.A3, Dq, PM, Dq, S, Bp, K, Dq, workspace=gws)
    elif precision == "bf16":
        npair_operands_bf16(e, Bp, Dp, ws.A16, PM, PMT)
        gemm_bf16_nt(BE_F32, ws.A16, PM, S, Bp, K, ws.Dq, workspace=gws)
    else:
        if PM is None:
            PM = P
        else:
            PM[:Bp].copy_(P)
        fc_bwd_data(A, PM, None, S, Bp, K, Dp)                # S[i][j] = <a_i, [p; mem]_j>
    return PM


def _npair_any_stats(S, rows, B, bias, mem, mem_bias, temperature, symmetric, lse, stats, workspace):
    if mem is None and bias is None:
        npair_stats(S, rows, B, temperature, symmetric, lse, stats, workspace)
    elif mem is None:
        npair_logq_stats(S, rows, B, bias, temperature, symmetric, lse, stats, workspace)
    elif bias is None:
        npair_memory_stats(S, rows, B, mem.Bp, mem.ids, temperature, symmetric, lse, stats, workspace)
    else:
        npair_memory_logq_stats(S, rows, B, bias, mem.Bp, mem.ids, mem_bias, temperature, symmetric, lse, stats, workspace)


def _npair_weights(precision, S, rows, B, bias, mem, mem_bias, temperature, symmetric, lse, W, K):
    """W: the in-batch block, then the memory block."""
    if precision == "bf16":
        npair_grad_bf16(S, rows, B, temperature, symmetric, lse, W, bias=bias)
        if mem is not None:
            npair_memory_grad_bf16(S, rows, B, mem.Bp, mem.ids, temperature, symmetric, lse, W, mem_bias=mem_bias)
        return
    x3 = precision == "f32x3"
    plane = (K,) if x3 else ()
    if bias is None:
        (npair_grad_x3 if x3 else npair_grad_f32)(S, rows, B, temperature, symmetric, lse, W, *plane)
    else:
        (npair_logq_grad_x3 if x3 else npair_logq_grad_f32)(S, rows, B, bias, temperature, symmetric, lse, W, *plane)
    if mem is None:
        return
    if mem_bias is None:
        (npair_memory_grad_x3 if x3 else npair_memory_grad_f32)(S, rows, B, mem.Bp, mem.ids, temperature, symmetric, lse, W,
                                                                *plane)
    else:
        (npair_memory_logq_grad_x3 if x3 else npair_memory_logq_grad_f32)(S, rows, B, mem.Bp, mem.ids, mem_bias, temperature,
                                                                          symmetric, lse, W, *plane)


def _npair_products(precision, e, ws, K, W, PM, PMT, gws, de):
    """dA = W [P; Mem] over K, dP = W^T A over the in-batch block of W, into de[0::2] / de[1::2]."""
    Bp, Dp = ws.Bp, ws.Dp
    dA, dP = de[0::2], de[1::2]
    if precision == "f32":
        fc_lrelu_fwd(W, PM, ws.zero_bias, dA, Bp, K, Dp, alpha=1.0)          # (x W form, identity activation)
        fc_bwd_weight(W[:, :Bp], e[0::2, :Dp], dP, None, ws.bw, Bp, Bp, Dp)  # (x^T dy form)
        return
    Dq = ws.Dq
    oA = dA if ws.dA is None else ws.dA                     # (rows narrower than the tile: the products land here first)
    oP = dP if ws.dP is None else ws.dP
    if precision == "f32x3":
        gemm_bf16x3_nt(BE_F32, W, K, PMT, K, oA, Bp, Dq, K, workspace=gws)
        gemm_bf16x3_tn(W, K, ws.A3, Dq, oP, Bp, Dq, Bp, workspace=gws)
    else:
        gemm_bf16_nt(BE_F32, W, PMT, oA, Bp, Dq, K, workspace=gws)
        gemm_bf16_tn(W, ws.A16, oP, Bp, Dq, Bp, workspace=gws)
    if ws.dA is not None:
        dA.copy_(ws.dA[:, :Dp])
        dP.copy_(ws.dP[:, :Dp])


def _npair_push(precision, P, rows, ws, mem, step, step_dev):
    """This step's positives into the ring, with the slots' part of the operand images the precision keeps."""
    Bp, Dp = ws.Bp, ws.Dp
    if precision == "f32x3":
        npair_memory_push(P, rows, Bp, Dp, step, step_dev, mem.start, mem.rows, mem.ids, R3=mem.PM3[Bp:], plane_r=ws.Dq,
                          T3=mem.PMT3[:, Bp:], plane_t=mem.K)
    elif precision == "bf16":
        npair_memory_push_bf16(P, rows, Bp, Dp, step, step_dev, mem.start, mem.rows, mem.ids, mem.PM16[Bp:], mem.PMT16[:, Bp:])
    else:                                                   # (the ring's rows ARE the last M rows of [P; Mem])
        npair_memory_push(P, rows, Bp, Dp, step, step_dev, mem.start, mem.rows, mem.ids)


def _npair_chain(e, rows, B, Dp, temperature, symmetric, precision, de, stats, ws, mem, step, step_dev, logq):
    """npair_loss's one chain, for every precision, with or without a memory and a logQ correction: the logQ gather, the
    operands, S = A [P; Mem]^T, the statistics, W (the in-batch block, the memory block), the estimator's update, dA and dP,
    the ring push -- in that order (the gather reads the ring's ids before this step's push; the update follows the
    launches that read the bias)."""
    Bp, lse = ws.Bp, ws.lse
    if mem is not None:
        if (mem.Bp, mem.Dp, mem.precision) != (Bp, Dp, precision):
            raise ValueError("NPairMemory is for %d pairs x %d columns on %s" % (mem.Bp, mem.Dp, mem.precision))
        if B != Bp or rows is None:
            raise ValueError("the cross-batch memory needs an unpadded batch (B == Bp) and the rows' video ids")
    K, S, W, PM, PMT, gws = _npair_buffers(precision, ws, mem)
    bias = None if logq is None else ws.bias
    mem_bias = None if logq is None or mem is None else mem.bias
    # (the plane and fp32 chains with a memory gather after S, the others before the operands: the order they were built in)
    late = mem is not None and precision != "bf16"

    def gather():
        if isinstance(logq, torch.Tensor):
            bias[:2 * B].copy_(logq.reshape(-1)[:2 * B])
        elif logq is not None:
            logq.gather(rows, B, None if mem is None else mem.ids, bias, mem_bias)

    if not late:
        gather()
    PM = _npair_scores(precision, e, ws, K, S, PM, PMT, gws)
    if late:
        gather()
    _npair_any_stats(S, rows, B, bias, mem, mem_bias, temperature, symmetric, lse, stats, ws.ws)
    if de is None:
        return stats, lse
    _npair_weights(precision, S, rows, B, bias, mem, mem_bias, temperature, symmetric, lse, W, K)
    if logq is not None and not isinstance(logq, torch.Tensor):
        logq.update(rows, B, step, step_dev)
    _npair_products(precision, e, ws, K, W, PM, PMT, gws, de)
    if mem is not None:
        _npair_push(precision, e[1::2, :Dp], rows, ws, mem, step, step_dev)
    return stats, lse


# ---- mixed negative sampling for the N-pair loss (Yang et al. 2020; csrc/npair_mixed.hip, include/cdml_npair_mixed.h) ----
def npair_mixed_workspace(B, M):
    return int(load_library().cdml_npair_mixed_workspace(int(B), int(M)))


def _mixed_args(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric):
    """(suffix of the entry point, its leading arguments): ``lq_u`` a float -- the uniform block's scalar -- or a fp32 tensor
    [B], the per-negative bias of the "_nb" entry points (include/cdml_negweights.h)."""
    sp, sld = _mat(S)
    nb = isinstance(lq_u, torch.Tensor)
    if nb and (lq_u.dim() != 1 or lq_u.numel() != int(B) or not lq_u.is_contiguous()):
        raise ValueError("neg_bias must be a contiguous fp32 tensor [B = %d], got %s" % (int(B), tuple(lq_u.shape)))
    return "_nb" if nb else "", (sp, sld, _p(rows3, torch.int32), int(B), int(neg_col), int(mem_col), _p(mem_id, torch.int32),
                                 0 if mem_id is None else mem_id.numel(), _p(bias, torch.float32),
                                 _p(lq_u, torch.float32) if nb else float(lq_u), _p(mem_bias, torch.float32),
                                 float(temperature), 1 if symmetric else 0)


def npair_mixed_stats(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric, lse, stats,
                      workspace):
    """cdml_npair_mixed_stats: lse and stats[0..3] over S = A [P; N; Mem]^T (blocks at columns 0, neg_col, mem_col), the
    ids rows3 int32 [3B] in the uniform sampler's layout (a, p, n per triplet) or None.  bias None: uncorrected.
    lq_u: the uniform block's scalar, or a fp32 tensor [B] -- one bias per drawn negative (cdml_npair_mixed_stats_nb)."""
    nb, args = _mixed_args(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric)
    call("cdml_npair_mixed_stats" + nb, *args, _p(lse), _p(stats), _p(workspace),
         workspace.numel() * workspace.element_size(), _stream())
    return lse, stats


def npair_mixed_grad_x3(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric, lse, W_planes,
                        plane):
    """W_planes bf16 [>= B, >= 2 plane + span] <- the gradient weights of all blocks as three planes, one launch."""
    wp, wld = _mat16(W_planes)
    nb, args = _mixed_args(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric)
    call("cdml_npair_mixed_grad_x3" + nb, *args, _p(lse), wp, wld, int(plane), _stream())
    return W_planes


def npair_mixed_grad_f32(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric, lse, W):
    wp, wld = _mat(W)
    nb, args = _mixed_args(S, rows3, B, neg_col, mem_col, mem_id, bias, lq_u, mem_bias, temperature, symmetric)
    call("cdml_npair_mixed_grad_f32" + nb, *args, _p(lse), wp, wld, _stream())
    return W


def npair_mixed_split_x3(e3, B, D, A3, plane_a, R3, plane_r, T3, plane_t, neg_row):
    """cdml_npair_mixed_split_x3: the plane images of A, P, N from the stride-3 rows of e3 fp32 [3B, >= D] -- A3 [B, ..],
    the row image R3 (P at rows 0.., N at rows neg_row..) and the transposed image T3 (the same columns)."""
    ep, eld = _mat(e3)
    ap, ald = _mat16(A3)
    rp, rld = _mat16(R3)
    tp, tld = _mat16(T3)
    call("cdml_npair_mixed_split_x3", ep, eld, int(B), int(D), ap, ald, int(plane_a), rp, rld, int(plane_r), tp, tld,
         int(plane_t), int(neg_row), _stream())


class _MixedRing(NPairMemory):
    """The NPairMemory ring of an NPairMixed: the ring itself (``rows``, ``ids``, ``bias``; push slots, ``state_dict`` and
    ``load`` are NPairMemory's) without NPairMemory's own S, W and [P; Mem] buffers -- the ring's operand images are the
    last M rows / columns of the owner's [P; N; Mem] ones."""

    def __init__(self, size, owner, device, start=0):
        Bp, Dp, precision = owner.Bp, owner.Dp, owner.precision
        M, tile = int(size), NPAIR_TILE[precision]
        if M < 1 or M % Bp or M % tile:
            raise ValueError("precision %r: the memory size must be a positive multiple of the batch (%d pairs) and of %d "
                             "(got %d)" % (precision, Bp, tile, M))
        if int(start) < 0:
            raise ValueError("memory_start must be >= 0, got %r" % (start,))
        self.M, self.Bp, self.Dp, self.precision, self.start = M, Bp, Dp, precision, int(start)
        self.K = 2 * Bp + M
        self.ids = torch.full((M,), -1, dtype=torch.int32, device=device)
        self.bias = torch.zeros(M, dtype=torch.float32, device=device)
        self.owner = owner
        self.rows = None                                    # set by the owner (f32: a view of its [P; N; Mem] operand)

    def load(self, rows, ids):
        if tuple(rows.shape) != (self.M, self.Dp) or tuple(ids.shape) != (self.M,):
            raise ValueError("a ring of %d rows x %d columns and %d ids, got %s and %s"
                             % (self.M, self.Dp, self.M, tuple(rows.shape), tuple(ids.shape)))
        self.rows.copy_(rows.to(device=self.rows.device, dtype=torch.float32))
        self.ids.copy_(ids.to(device=self.ids.device, dtype=torch.int32))
        if self.precision == "f32x3":
            o = self.owner
            split_f32_bf16x3(self.rows, o.R3[2 * self.Bp:], o.Dq)
            split_f32_bf16x3(self.rows, o.T3[:, 2 * self.Bp:], o.K, transpose=True)

    def W(self):
        return self.owner.W()


class NPairMixed:
    """Every buffer of the N-pair chain with mixed negative sampling (``npair_mixed_loss``) for Bp triplets of Dp-wide rows,
    allocated once (hipGraph-capturable): S fp32 [Bp, K] and W over the column set [P | N | Mem], K = 2 Bp + M, with the
    uniform block at column ``neg_col`` = Bp and the memory block at ``mem_col`` = 2 Bp; the operand [P; N; Mem] -- f32x3:
    its row planes ``R3`` [K, 3 Dq] and transposed planes ``T3`` [Dq, 3 K] (the batch's part written by the split launch,
    the ring's by the push), and the anchors' planes ``A3``; f32: fp32 ``PNM`` [K, Dp].  ``memory_size`` > 0: ``ring``, an
    NPairMemory ring of M positives (a multiple of Bp and of NPAIR_TILE[precision])."""

    def __init__(self, Bp, Dp, precision, device, memory_size=0, memory_start=0):
        if precision not in NPAIR_FP32_PRECISIONS:
            raise ValueError("the N-pair loss with mixed negatives runs on precision 'f32x3' or 'f32', not %r" % (precision,))
        tile = NPAIR_TILE[precision]
        if Bp < tile or Bp % tile:
            raise ValueError("precision %r: the N-pair loss needs a batch that is a multiple of %d pairs (got %d)"
                             % (precision, tile, Bp))
        if Dp % 64:
            raise ValueError("the N-pair loss needs an embedding width that is a multiple of 64 (got %d)" % Dp)
        self.Bp, self.Dp, self.precision = int(Bp), int(Dp), precision
        self.ring = _MixedRing(memory_size, self, device, memory_start) if int(memory_size) else None
        self.M = M = self.ring.M if self.ring is not None else 0
        self.K = K = 2 * self.Bp + M
        self.neg_col, self.mem_col = self.Bp, 2 * self.Bp
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=device)
        self.S = f32(Bp, K)
        self.lse = f32(2 * Bp)
        self.bias = f32(2 * Bp)                              # logQ correction: lq(a_i), lq(p_i), the [2B] layout
        self.rows2 = torch.zeros(2 * Bp, dtype=torch.int32, device=device)   # (a, p) ids for the ring push / the estimator
        self.ws = torch.zeros(npair_mixed_workspace(Bp, M) // 4, dtype=torch.float32, device=device)
        if precision == "f32x3":
            self.Dq = Dq = (Dp + 255) // 256 * 256
            self.A3 = bf(Bp, 3 * Dq)
            self.R3, self.T3 = bf(K, 3 * Dq), bf(Dq, 3 * K)
            self.W3 = bf(Bp, 3 * K)
            nb = max(gemm_bf16x3_workspace(False, Bp, K, Dq), gemm_bf16x3_workspace(False, Bp, Dq, K),
                     gemm_bf16x3_workspace(True, Bp, Dq, Bp), 16)
            self.gemm_ws = torch.zeros(nb // 4, dtype=torch.float32, device=device)
            self.dA, self.dP, self.dN = (f32(Bp, Dq), f32(Bp, Dq), f32(Bp, Dq)) if Dq != Dp else (None, None, None)
            if self.ring is not None:
                self.ring.rows = f32(M, Dp)
        else:
            self.PNM = f32(K, Dp)
            self.Wf = f32(Bp, K)
            self.zero_bias = f32(Dp)
            self.bw = torch.zeros(max(fc_bwd_weight_workspace(Bp, Bp, Dp), 16) // 4, dtype=torch.float32, device=device)
            if self.ring is not None:
                self.ring.rows = self.PNM[2 * Bp:]

    def W(self):
        """the gradient weights as one fp32 tensor [Bp, 2 Bp + M] = [W_p | W_n | W_mem] (tests, debugging)"""
        if self.precision == "f32":
            return self.Wf
        K = self.K
        return self.W3[:, :K].float() + self.W3[:, K:2 * K].float() + self.W3[:, 2 * K:].float()


def uniform_logq(logq, value=None):
    """lq_u, the one log sampling probability of the uniform block: ``value`` when given (a finite float); else, for a
    LogQEstimator, -log(g0) -- exactly the lq an unseen video has in the other blocks --, for a LogQTable (per-draw
    shares) -log(n_videos); 0 without a correction."""
    import math
    if logq is None:
        if value is not None:
            raise ValueError("uniform_logq goes with a logQ correction (logq=...)")
        return 0.0
    if value is not None:
        value = float(value)
        if not math.isfinite(value):
            raise ValueError("uniform_logq must be a finite float, got %r" % (value,))
        return value
    if isinstance(logq, LogQEstimator):
        return -math.log(logq.init_gap)
    return -math.log(logq.n_videos)


def npair_mixed_loss(e3, rows3, B, Dp, temperature=0.1, symmetric=True, precision="f32x3", de=None, stats=None, ws=None,
                     step=0, step_dev=None, logq=None, lq_u=0.0, neg_bias=None):
    """The N-pair loss with mixed negative sampling (include/cdml_npair_mixed.h) of B triplets and its gradient.
    e3: fp32 [3 B, >= Dp] unit rows in the uniform sampler's layout (row 3i = anchor, 3i+1 = positive, 3i+2 = uniform
    negative); rows3: int32 [3 B] video ids laid out the same, or None (no ring, no correction).  The chain: the plane
    split of A, P, N from the stride-3 rows -> S = A [P; N; Mem]^T -> statistics -> W (one launch) -> dA = W [P; N; Mem]
    over K = 2 B + M into de[0::3], dP = W_p^T A into de[1::3], dN = W_n^T A into de[2::3] (de fp32 [3 B, Dp]; None: loss
    only) -> with a ring, the push of the step's positives.  ws: an NPairMixed (B == ws.Bp).  logq: a LogQTable /
    LogQEstimator (bias of the in-batch and memory blocks; an estimator is updated by the positives after W), or a fp32
    tensor [2 B] of lq(a_i), lq(p_i) per pair (no ring), with the uniform block's scalar ``lq_u`` (``uniform_logq``) or
    ``neg_bias``, a fp32 tensor [B] of one log sampling probability per drawn negative (``negw_bias``; the "_nb" entry
    points of include/cdml_negweights.h; not together with a non-zero ``lq_u``; not read without a correction).
    Returns (stats, lse)."""
    if not (temperature > 0.0) or temperature == float("inf"):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    if ws is None:
        ws = NPairMixed(B, Dp, precision, e3.device)
    if (ws.Bp, ws.Dp, ws.precision) != (B, Dp, precision) or e3.shape[0] != 3 * B:
        raise ValueError("NPairMixed is for %d triplets x %d columns on %s and needs e3 of 3 B rows (unpadded)"
                         % (ws.Bp, ws.Dp, ws.precision))
    ring = ws.ring
    row_logq = logq if isinstance(logq, torch.Tensor) else None
    if row_logq is not None:
        if ring is not None or row_logq.numel() != 2 * B:
            raise ValueError("a per-row logQ tensor holds 2B = %d entries (a_i, p_i per pair) and has no memory part" % (2 * B))
        logq = None
    if rows3 is None and (ring is not None or logq is not None):
        raise ValueError("the cross-batch memory and the logQ correction need the rows' video ids")
    if logq is None and row_logq is None and lq_u:
        raise ValueError("lq_u goes with a logQ correction (logq=...)")
    if neg_bias is not None:
        if lq_u:
            raise ValueError("neg_bias (one log-probability per negative) and a non-zero lq_u (one for the block) exclude each other")
        if not isinstance(neg_bias, torch.Tensor) or neg_bias.dtype != torch.float32 or neg_bias.numel() != B:
            raise ValueError("neg_bias must be a fp32 tensor [B = %d]" % B)
        lq_u = neg_bias.reshape(-1)                         # (a tensor in lq_u's place routes the launches to the _nb entry points)
    if stats is None:
        stats = torch.zeros(4, dtype=torch.float32, device=e3.device)
    Bp, K, nc, mc = ws.Bp, ws.K, ws.neg_col, ws.mem_col
    A, P, N = e3[0::3, :Dp], e3[1::3, :Dp], e3[2::3, :Dp]
    mem_id = ring.ids if ring is not None else None
    rows2 = None
    if ring is not None or logq is not None:                # the ring push and the estimator take ids laid out [2B]: (a, p)
        rows2 = ws.rows2
        rows2.view(Bp, 2).copy_(rows3.view(Bp, 3)[:, :2])
    bias = mem_bias = None
    if logq is not None:                                    # (the gather reads the ring's ids before this step's push)
        bias, mem_bias = ws.bias, (ring.bias if ring is not None else None)
        logq.gather(rows2, B, mem_id, bias, mem_bias)
    elif row_logq is not None:
        bias = ws.bias
        bias.copy_(row_logq.reshape(-1))
    lse = ws.lse
    if precision == "f32x3":
        Dq = ws.Dq
        npair_mixed_split_x3(e3, B, Dp, ws.A3, Dq, ws.R3, Dq, ws.T3, K, nc)
        gemm_bf16x3_nt(BE_F32, ws.A3, Dq, ws.R3, Dq, ws.S, Bp, K, Dq, workspace=ws.gemm_ws)        # S = A [P; N; Mem]^T
    else:
        ws.PNM[:2 * Bp].view(2, Bp, Dp).copy_(e3.unflatten(0, (Bp, 3))[:, 1:, :Dp].transpose(0, 1))
        fc_bwd_data(A, ws.PNM, None, ws.S, Bp, K, Dp)
    npair_mixed_stats(ws.S, rows3, B, nc, mc, mem_id, bias, lq_u, mem_bias, temperature, symmetric, lse, stats, ws.ws)
    if de is None:
        return stats, lse
    dA, dP, dN = de[0::3], de[1::3], de[2::3]
    if precision == "f32x3":
        npair_mixed_grad_x3(ws.S, rows3, B, nc, mc, mem_id, bias, lq_u, mem_bias, temperature, symmetric, lse, ws.W3, K)
        if logq is not None:
            logq.update(rows2, B, step, step_dev)
        oA, oP, oN = (dA, dP, dN) if ws.dA is None else (ws.dA, ws.dP, ws.dN)
        gemm_bf16x3_nt(BE_F32, ws.W3, K, ws.T3, K, oA, Bp, Dq, K, workspace=ws.gemm_ws)            # dA = W . [P; N; Mem]
        gemm_bf16x3_tn(ws.W3, K, ws.A3, Dq, oP, Bp, Dq, Bp, workspace=ws.gemm_ws)                  # dP = W_p^T . A
        gemm_bf16x3_tn(ws.W3[:, nc:], K, ws.A3, Dq, oN, Bp, Dq, Bp, workspace=ws.gemm_ws)          # dN = W_n^T . A
        if ws.dA is not None:
            dA.copy_(ws.dA[:, :Dp])
            dP.copy_(ws.dP[:, :Dp])
            dN.copy_(ws.dN[:, :Dp])
        if ring is not None:
            npair_memory_push(P, rows2, Bp, Dp, step, step_dev, ring.start, ring.rows, ring.ids, R3=ws.R3[mc:], plane_r=Dq,
                              T3=ws.T3[:, mc:], plane_t=K)
    else:
        npair_mixed_grad_f32(ws.S, rows3, B, nc, mc, mem_id, bias, lq_u, mem_bias, temperature, symmetric, lse, ws.Wf)
        if logq is not None:
            logq.update(rows2, B, step, step_dev)
        fc_lrelu_fwd(ws.Wf, ws.PNM, ws.zero_bias, dA, Bp, K, Dp, alpha=1.0)          # dA = W . [P; N; Mem]
        fc_bwd_weight(ws.Wf[:, :Bp], A, dP, None, ws.bw, Bp, Bp, Dp)                 # dP = W_p^T . A
        fc_bwd_weight(ws.Wf[:, nc:nc + Bp], A, dN, None, ws.bw, Bp, Bp, Dp)          # dN = W_n^T . A
        if ring is not None:
            npair_memory_push(P, rows2, Bp, Dp, step, step_dev, ring.start, ring.rows, ring.ids)
    return stats, lse


# ---- the data-parallel N-pair loss: one softmax over every rank's positives (csrc/npair_dp.hip, include/cdml_npair_dp.h) ----
def npair_dp_workspace(B, G):
    return int(load_library().cdml_npair_dp_workspace(int(B), int(G)))


def npair_dp_local_stats(S, ids_all, B, G, col0, temperature, symmetric, lse_row, colpart, workspace):
    """cdml_npair_dp_local_stats: lse_row [B] over all G columns of this rank's row block S [B, >= G], the rows' partials
    into ``workspace`` (npair_dp_stats reads them) and, with ``symmetric``, colpart [G, 2] = every global column's (max,
    sum-exp) over this rank's rows.  ids_all: int32 [2G], the global batch's ids laid out like npair_stats' rows."""
    sp, sld = _mat(S)
    call("cdml_npair_dp_local_stats", sp, sld, _p(ids_all, torch.int32), int(B), int(G), int(col0), float(temperature),
         1 if symmetric else 0, _p(lse_row, torch.float32), _p(colpart if symmetric else None), _p(workspace),
         workspace.numel() * workspace.element_size(), _stream())
    return lse_row, colpart


def npair_dp_col_fold(colpart_all, lse_col):
    """cdml_npair_dp_col_fold: lse_col [G] from the gathered partials colpart_all [world, G, 2] (contiguous), the ranks
    folded in the order 0 .. world - 1."""
    if colpart_all.dim() != 3 or colpart_all.shape[2] != 2 or not colpart_all.is_contiguous():
        raise ValueError("colpart_all must be a contiguous [world, G, 2] tensor")
    world, G = colpart_all.shape[0], colpart_all.shape[1]
    if lse_col.numel() < G:
        raise ValueError("lse_col needs G = %d entries, got %d" % (G, lse_col.numel()))
    call("cdml_npair_dp_col_fold", _p(colpart_all, torch.float32), int(world), int(G), _p(lse_col, torch.float32), _stream())
    return lse_col


def npair_dp_stats(S, B, G, col0, temperature, symmetric, lse_col, stats, workspace):
    """cdml_npair_dp_stats: this rank's stats[0..3] from the partials npair_dp_local_stats left in ``workspace`` (and,
    with ``symmetric``, the column term of the columns col0 .. col0 + B - 1 it owns)."""
    sp, sld = _mat(S)
    call("cdml_npair_dp_stats", sp, sld, int(B), int(G), int(col0), float(temperature), 1 if symmetric else 0,
         _p(lse_col if symmetric else None), _p(stats, torch.float32), _p(workspace),
         workspace.numel() * workspace.element_size(), _stream())
    return stats


def npair_dp_grad_x3(S, ids_all, B, G, col0, temperature, symmetric, lse_row, lse_col, W_planes, plane):
    """W_planes bf16 [>= B, >= 2 plane + G] <- the three bf16 planes of this rank's gradient weights (cdml_npair_dp_grad_x3)."""
    sp, sld = _mat(S)
    wp, wld = _mat16(W_planes)
    call("cdml_npair_dp_grad_x3", sp, sld, _p(ids_all, torch.int32), int(B), int(G), int(col0), float(temperature),
         1 if symmetric else 0, _p(lse_row), _p(lse_col if symmetric else None), wp, wld, int(plane), _stream())
    return W_planes


def npair_dp_grad_f32(S, ids_all, B, G, col0, temperature, symmetric, lse_row, lse_col, W):
    """W fp32 [>= B, >= G] <- this rank's gradient weights (cdml_npair_dp_grad_f32)."""
    sp, sld = _mat(S)
    wp, wld = _mat(W)
    call("cdml_npair_dp_grad_f32", sp, sld, _p(ids_all, torch.int32), int(B), int(G), int(col0), float(temperature),
         1 if symmetric else 0, _p(lse_row), _p(lse_col if symmetric else None), wp, wld, _stream())
    return W


def npair_dp_pos_fold(recv, B, D, de):
    """de[2i + 1, :D] = recv[0, i] + recv[1, i] + ... (fp32, in rank order): recv [world, B, >= D] contiguous blocks of the
    partial positive gradients, de fp32 [>= 2B, >= D] (cdml_npair_dp_pos_fold).  Rows 2i of de are not touched."""
    if recv.dim() != 3 or recv.shape[1] != B or recv.stride(2) != 1 or recv.stride(0) != B * recv.stride(1):
        raise ValueError("recv must be [world, B, >= D] with the ranks' blocks back to back")
    if de.shape[0] < 2 * B:
        raise ValueError("de needs 2B = %d rows, got %d" % (2 * B, de.shape[0]))
    dp, dld = _mat(de)
    call("cdml_npair_dp_pos_fold", _p(recv, torch.float32), recv.stride(1), recv.shape[0], int(B), int(D), dp, dld, _stream())
    return de


NPAIR_DP_WIRE_PAD = 4      # words behind a positive's fp32 row on the wire: its pair's two video ids (bits), two zero words


class NPairDP:
    """Every buffer of the data-parallel N-pair chain of one rank, allocated once: B local pairs against the G = world B
    global positives, Dp-wide rows (B == Bp: no padding; B a multiple of NPAIR_TILE[precision], Dp of 64).
    ``send`` [B, Dp + 4] / ``wire`` [G, Dp + 4]: the positives as they cross the wire (all-gather) -- the fp32 row, then the
    pair's two video ids as bit patterns -- so rows and ids travel in ONE collective; ``ids_all`` int32 [2G] and the plane
    images are derived on arrival.  ``colpart`` [G, 2] / ``colpart_all`` [world, G, 2]: the column statistics (all-gather).
    ``dP_part`` [G, Dw] / ``recv`` [world, B, Dw]: this rank's partial gradient of every positive and the blocks it
    receives for its own (all-to-all; Dw = Dp, on f32x3 the plane GEMMs' 256-column tile)."""

    def __init__(self, B, G, Dp, precision, device):
        if precision not in NPAIR_FP32_PRECISIONS:
            raise ValueError("the data-parallel N-pair loss runs on precision 'f32x3' or 'f32', not %r" % (precision,))
        B, G, Dp = int(B), int(G), int(Dp)
        tile = NPAIR_TILE[precision]
        if B < tile or B % tile:
            raise ValueError("precision %r: the data-parallel N-pair loss needs a local batch that is a multiple of %d pairs "
                             "(got %d)" % (precision, tile, B))
        if G < B or G % B:
            raise ValueError("the global batch must be a multiple of the local batch (%d pairs), got %d" % (B, G))
        if Dp % 64:
            raise ValueError("the N-pair loss needs an embedding width that is a multiple of 64 (got %d)" % Dp)
        # the GEMMs address an operand through one 2 GiB buffer descriptor: W_r's planes [B + a 256-row tile, 3 G] bf16 on
        # f32x3, W_r [B, G] fp32 on f32 (at B = 8192: G <= 40 960 pairs on f32x3; a blocked gradient product is later work)
        wbytes = (B + 256) * 3 * G * 2 if precision == "f32x3" else B * G * 4
        if wbytes >= 1 << 31:
            raise ValueError("precision %r: the gradient weights of %d x %d pairs exceed the GEMMs' 2 GiB operand range "
                             "(use a smaller local batch or fewer ranks)" % (precision, B, G))
        self.B, self.G, self.Dp, self.precision, self.world = B, G, Dp, precision, G // B
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=device)
        Dw = Dp + NPAIR_DP_WIRE_PAD
        self.send, self.wire = f32(B, Dw), f32(G, Dw)
        self.ids_all = torch.zeros(2 * G, dtype=torch.int32, device=device)
        self.S = f32(B, G)
        self.lse_row, self.lse_col = f32(B), f32(G)
        self.colpart, self.colpart_all = f32(G, 2), f32(self.world, G, 2)
        self.ws = torch.zeros(npair_dp_workspace(B, G) // 4, dtype=torch.float32, device=device)
        if precision == "f32x3":
            self.Dq = Dq = (Dp + 255) // 256 * 256          # the plane GEMMs' N tile: narrower rows are zero-padded
            self.A3 = bf(B, 3 * Dq)
            self.PA3, self.PAT3 = bf(G, 3 * Dq), bf(Dq, 3 * G)   # every rank's positives: row planes and transposed planes
            self.W3 = bf(B, 3 * G)
            nb = max(gemm_bf16x3_workspace(False, B, G, Dq), gemm_bf16x3_workspace(False, B, Dq, G),
                     gemm_bf16x3_workspace(True, G, Dq, B), 16)
            self.gemm_ws = torch.zeros(nb // 4, dtype=torch.float32, device=device)
            self.dA = f32(B, Dq) if Dq != Dp else None
            self.dP_part, self.recv = f32(G, Dq), f32(self.world, B, Dq)
        else:
            self.Wf = f32(B, G)
            self.zero_bias = f32(Dp)
            self.bw = torch.zeros(max(fc_bwd_weight_workspace(B, G, Dp), 16) // 4, dtype=torch.float32, device=device)
            self.dP_part, self.recv = f32(G, Dp), f32(self.world, B, Dp)

    def P_all(self):
        """every rank's positives, fp32 [G, Dp] (a view of ``wire``)"""
        return self.wire[:, :self.Dp]

    def W(self):
        """this rank's gradient weights as one fp32 tensor [B, G] (tests, debugging)"""
        if self.precision == "f32":
            return self.Wf
        G = self.G
        return self.W3[:, :G].float() + self.W3[:, G:2 * G].float() + self.W3[:, 2 * G:].float()


def _npair_dp_args(e, B, ws, rank):
    if e.shape[0] != 2 * B or B != ws.B:
        raise ValueError("the data-parallel N-pair loss needs an unpadded batch: e must hold exactly 2 B = %d rows (got %d)"
                         % (2 * ws.B, e.shape[0]))
    if not 0 <= int(rank) < ws.world:
        raise ValueError("rank %r outside the world of %d" % (rank, ws.world))
    return int(rank) * B


def npair_dp_pack(e, rows, ws):
    """ws.send <- this rank's positives (rows 2i + 1 of e) and its pairs' video ids (rows int32 [2B]) in wire form."""
    B, Dp = ws.B, ws.Dp
    if rows is None:
        raise ValueError("the data-parallel N-pair loss needs the rows' video ids")
    ws.send[:, :Dp].copy_(e[1::2, :Dp])
    ws.send.view(torch.int32)[:, Dp:Dp + 2].copy_(rows.view(B, 2))
    return ws.send


def npair_dp_phase1(e, rank, ws, temperature=0.1, symmetric=True):
    """From this rank's embedded rows e [2B, Dp] and the gathered positives in ``ws.wire``: ws.ids_all, the operand planes,
    S_r = A_r P_all^T, ws.lse_row and (symmetric) ws.colpart.  No communication."""
    B, G, Dp = ws.B, ws.G, ws.Dp
    col0 = _npair_dp_args(e, B, ws, rank)
    ws.ids_all.view(G, 2).copy_(ws.wire.view(torch.int32)[:, Dp:Dp + 2])
    A, P = e[0::2, :Dp], ws.P_all()
    if ws.precision == "f32x3":
        Dq = ws.Dq
        split_f32_bf16x3(A, ws.A3, Dq)
        split_f32_bf16x3(P, ws.PA3, Dq)
        split_f32_bf16x3(P, ws.PAT3, G, transpose=True)
        gemm_bf16x3_nt(BE_F32, ws.A3, Dq, ws.PA3, Dq, ws.S, B, G, Dq, workspace=ws.gemm_ws)
    else:
        fc_bwd_data(A, P, None, ws.S, B, G, Dp)                 # S[i][j] = <a_i, p_j>
    npair_dp_local_stats(ws.S, ws.ids_all, B, G, col0, temperature, symmetric, ws.lse_row, ws.colpart, ws.ws)
    return ws.lse_row, ws.colpart


def npair_dp_phase2(e, rank, ws, temperature=0.1, symmetric=True, de=None, stats=None):
    """From the gathered column partials in ``ws.colpart_all``: ws.lse_col, this rank's stats, and with ``de`` (fp32 [2B,
    Dp]) W_r, dA = W_r P_all into rows 2i of de and the partial positive gradient ws.dP_part = W_r^T A_r [G, .].  No
    communication."""
    B, G, Dp = ws.B, ws.G, ws.Dp
    col0 = _npair_dp_args(e, B, ws, rank)
    if stats is None:
        stats = torch.zeros(4, dtype=torch.float32, device=e.device)
    if symmetric:
        npair_dp_col_fold(ws.colpart_all, ws.lse_col)
    npair_dp_stats(ws.S, B, G, col0, temperature, symmetric, ws.lse_col, stats, ws.ws)
    if de is None:
        return stats
    A, dA = e[0::2, :Dp], de[0::2]
    if ws.precision == "f32x3":
        Dq = ws.Dq
        npair_dp_grad_x3(ws.S, ws.ids_all, B, G, col0, temperature, symmetric, ws.lse_row, ws.lse_col, ws.W3, G)
        oA = dA if ws.dA is None else ws.dA
        gemm_bf16x3_nt(BE_F32, ws.W3, G, ws.PAT3, G, oA, B, Dq, G, workspace=ws.gemm_ws)             # dA = W . P_all
        gemm_bf16x3_tn(ws.W3, G, ws.A3, Dq, ws.dP_part, G, Dq, B, workspace=ws.gemm_ws)              # W^T . A, all G rows
        if ws.dA is not None:
            dA.copy_(ws.dA[:, :Dp])
    else:
        npair_dp_grad_f32(ws.S, ws.ids_all, B, G, col0, temperature, symmetric, ws.lse_row, ws.lse_col, ws.Wf)
        fc_lrelu_fwd(ws.Wf, ws.P_all(), ws.zero_bias, dA, B, G, Dp, alpha=1.0)
        fc_bwd_weight(ws.Wf, A, ws.dP_part, None, ws.bw, B, G, Dp)
    return stats


def npair_dp_phase3(ws, de):
    """rows 2i + 1 of de <- the received partial positive gradients ``ws.recv`` summed in rank order.  No communication."""
    return npair_dp_pos_fold(ws.recv, ws.B, ws.Dp, de)


def npair_dp_loss(e, rows, B, Dp, temperature=0.1, symmetric=True, precision="f32x3", de=None, stats=None, ws=None, sync=None):
    """The N-pair loss of the GLOBAL batch -- ``sync.world`` ranks of B pairs, one softmax over all of their positives --
    and this rank's part of its gradient (include/cdml_npair_dp.h).  e: this rank's fp32 [2B, Dp] unit rows (B == Bp, no
    padding), rows: its int32 [2B] video ids; sync: a dist.NPairSync.  Three phases with the hook's collectives between
    them: all-gather of the positives' rows + ids -> S_r, row statistics, column partials -> (symmetric) all-gather of the
    column partials -> column fold, stats, W_r, dA, partial dP -> (with ``de``) all-to-all of the dP blocks -> their
    rank-order sum into de[1::2].  W_r carries 1 / (B t): averaging the ranks' parameter gradients (GradSync) gives the
    global mean's.  stats[0] is this rank's share (the mean over the ranks is the global loss).  Returns (stats, lse_row
    [B], lse_col [G])."""
    if sync is None:
        raise ValueError("npair_dp_loss needs the NPairSync hook that carries the positives between the ranks")
    if not (temperature > 0.0) or temperature == float("inf"):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    G = int(B) * sync.world
    if ws is None:
        ws = NPairDP(B, G, Dp, precision, e.device)
    elif (ws.B, ws.G, ws.Dp, ws.precision) != (B, G, Dp, precision):
        raise ValueError("NPairDP is for %d of %d pairs x %d columns on %s" % (ws.B, ws.G, ws.Dp, ws.precision))
    if stats is None:
        stats = torch.zeros(4, dtype=torch.float32, device=e.device)
    _npair_dp_args(e, B, ws, sync.rank)
    npair_dp_pack(e, rows, ws)
    sync.all_gather(ws.wire, ws.send)
    npair_dp_phase1(e, sync.rank, ws, temperature, symmetric)
    if symmetric:
        sync.all_gather(ws.colpart_all, ws.colpart)
    npair_dp_phase2(e, sync.rank, ws, temperature, symmetric, de=de, stats=stats)
    if de is not None:
        sync.all_to_all(ws.recv, ws.dP_part)
        npair_dp_phase3(ws, de)
    return stats, ws.lse_row, ws.lse_col


def pair_dist(e, pairs, D, sqdist, dot, means=None):
    ep, eld = _mat(e)
    call("cdml_pair_dist", ep, eld, e.shape[0], _p(pairs, torch.int32), pairs.shape[0], D, _p(sqdist),
         _p(dot), _p(means), _stream())


# ------------------------------------------------- co-watch graph (N3) --------
def _cowatch_ws(P, device):
    nbytes = int(load_library().cdml_cowatch_workspace(P))
    return torch.empty(nbytes + 256, dtype=torch.uint8, device=device)   # torch allocations are 256-B aligned


def cowatch_graph(pairs):
    P = pairs.shape[0]
    dev = pairs.device
    ws = _cowatch_ws(P, dev)
    edges = torch.empty((P, 2), dtype=torch.int32, device=dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    n_edges = torch.zeros(1, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    call("cdml_cowatch_graph", _p(pairs, torch.int32), P, _p(edges), _p(counts), _p(n_edges), _p(flag), _p(ws),
         ws.numel(), _stream())
    return edges, counts, n_edges, flag


def cowatch_select(pairs, threshold, unique):
    P = pairs.shape[0]
    dev = pairs.device
    ws = _cowatch_ws(P, dev)
    out = torch.empty((P, 2), dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    call("cdml_cowatch_select", _p(pairs, torch.int32), P, threshold, 1 if unique else 0, _p(out), _p(n), _p(flag),
         _p(ws), ws.numel(), _stream())
    return out, n, flag


# ------------------------------------------------- exact kNN export (N4) ------
def knn_list_capacity():
    return int(load_library().cdml_knn_list_capacity())


def row_sqnorm(x, D, out):
    xp, xld = _mat(x)
    call("cdml_row_sqnorm", xp, xld, x.shape[0], D, _p(out), _stream())
    return out


def knn_merge(scores, nq, nb, col0, n_valid, q_sq, b_sq, k, best_d, best_i, first):
    sp, sld = _mat(scores)
    call("cdml_knn_merge", sp, sld, nq, nb, col0, n_valid, _p(q_sq), _p(b_sq), k, _p(best_d),
         _p(best_i, torch.int32), int(bool(first)), _stream())


def knn_filter_x3(Q3, plane_q, B3, plane_b, nq, n_cols, D, q_sq, b_sq, tau, col0, n_valid, cnt, cand, cap):
    """The query x catalogue-block inner products on the plane kernels with the threshold filter as their epilogue: every
    element with d <= tau[query] is appended to the query's candidate list (cand int32 [nq, cap, 2]: float bits of d, id)."""
    qp, qld = _mat16(Q3)
    bp, bld = _mat16(B3)
    if cand.dtype != torch.int32 or not cand.is_contiguous() or cand.numel() < nq * cap * 2:
        raise ValueError("cand must be a contiguous int32 buffer of nq * cap * 2 words")
    call("cdml_knn_filter_x3", qp, qld, plane_q, bp, bld, plane_b, nq, n_cols, D, _p(q_sq), _p(b_sq), _p(tau), col0, n_valid,
         _p(cnt, torch.int32), _p(cand, torch.int32), cap, _stream())


def knn_filter_h2(Q2, plane_q, B2, plane_b, nq, n_cols, D, out_scale, q_sq, b_sq, tau, col0, n_valid, cnt, cand, cap):
    """knn_filter_x3 on two fp16 planes per row (split_f32_f16x2 at scales sq / sb; out_scale = 1 / (sq sb))."""
    qp, qld = _mat16(Q2)
    bp, bld = _mat16(B2)
    if cand.dtype != torch.int32 or not cand.is_contiguous() or cand.numel() < nq * cap * 2:
        raise ValueError("cand must be a contiguous int32 buffer of nq * cap * 2 words")
    call("cdml_knn_filter_h2", qp, qld, plane_q, bp, bld, plane_b, nq, n_cols, D, float(out_scale), _p(q_sq), _p(b_sq), _p(tau), col0,
         n_valid, _p(cnt, torch.int32), _p(cand, torch.int32), cap, _stream())


def rank_tau_x3(Q3, plane_q, P3, plane_p, nq, D, q_sq, p_sq, tau_out):
    """tau_out[i] = d(anchor i, partner i) on the plane kernels, in the arithmetic of rank_count_x3 (the product's diagonal):
    Q3 = the anchors' planes [nq, >= 3 plane], P3 = the partners' planes, rows rounded up to a multiple of 256."""
    qp, qld = _mat16(Q3)
    pp, pld = _mat16(P3)
    if P3.shape[0] < (nq + 255) // 256 * 256 or p_sq.numel() < P3.shape[0]:
        raise ValueError("the partners' planes and norms need nq rounded up to 256 rows")
    call("cdml_rank_tau_x3", qp, qld, plane_q, pp, pld, plane_p, nq, D, _p(q_sq), _p(p_sq), _p(tau_out), _stream())


def rank_tau_h2(Q2, plane_q, P2, plane_p, nq, D, out_scale, q_sq, p_sq, tau_out):
    """rank_tau_x3 on two fp16 planes per row (one scale s for both operands; out_scale = 1 / s^2)."""
    qp, qld = _mat16(Q2)
    pp, pld = _mat16(P2)
    if P2.shape[0] < (nq + 255) // 256 * 256 or p_sq.numel() < P2.shape[0]:
        raise ValueError("the partners' planes and norms need nq rounded up to 256 rows")
    call("cdml_rank_tau_h2", qp, qld, plane_q, pp, pld, plane_p, nq, D, float(out_scale), _p(q_sq), _p(p_sq), _p(tau_out),
         _stream())


def rank_count_x3(Q3, plane_q, B3, plane_b, nq, n_cols, D, q_sq, b_sq, tau, pos_id, self_id, col0, n_valid, count):
    """The query x catalogue-block inner products on the plane kernels with the rank count as their epilogue: count[i] (int32,
    accumulated) += the catalogue rows col0 .. col0 + n_cols - 1 ranked ahead of pos_id[i] in self_id[i]'s list."""
    qp, qld = _mat16(Q3)
    bp, bld = _mat16(B3)
    call("cdml_rank_count_x3", qp, qld, plane_q, bp, bld, plane_b, nq, n_cols, D, _p(q_sq), _p(b_sq), _p(tau),
         _p(pos_id, torch.int32), _p(self_id, torch.int32), col0, n_valid, _p(count, torch.int32), _stream())


def rank_count_h2(Q2, plane_q, B2, plane_b, nq, n_cols, D, out_scale, q_sq, b_sq, tau, pos_id, self_id, col0, n_valid, count):
    """rank_count_x3 on two fp16 planes per row (one scale s for queries and catalogue; out_scale = 1 / s^2)."""
    qp, qld = _mat16(Q2)
    bp, bld = _mat16(B2)
    call("cdml_rank_count_h2", qp, qld, plane_q, bp, bld, plane_b, nq, n_cols, D, float(out_scale), _p(q_sq), _p(b_sq), _p(tau),
         _p(pos_id, torch.int32), _p(self_id, torch.int32), col0, n_valid, _p(count, torch.int32), _stream())


def knn_merge_list(cand, cnt, cap, nq, k, best_d, best_i, overflow):
    call("cdml_knn_merge_list", _p(cand, torch.int32), _p(cnt, torch.int32), cap, nq, k, _p(best_d), _p(best_i, torch.int32),
         _p(overflow, torch.int32), _stream())


# ---------------------------------------- IVF index of the kNN (include/cdml_ivf.h) ------
def _vec(t, dtype, n, what):
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < n:
        raise ValueError("%s must be a contiguous %s tensor of at least %d elements" % (what, dtype, n))
    return _p(t, dtype)


def ivf_centroid_sums(x, order, list_start, centroids, D):
    """Every non-empty list's column means over columns [0, D): centroids[c] = mean of x[order[list_start[c]:list_start[c+1]]];
    an empty list's row is not written.  order: int32 row ids of x sorted by (list, id); list_start: int32 [nlist + 1]."""
    xp, xld = _mat(x)
    cp, cld = _mat(centroids)
    nlist = centroids.shape[0]
    call("cdml_ivf_centroid_sums", xp, xld, _vec(order, torch.int32, 0, "order"),
         _vec(list_start, torch.int32, nlist + 1, "list_start"), nlist, D, cp, cld, _stream())
    return centroids


def ivf_scan_f32(Q, slot_query, slot_start, slot_off, rows, list_start, tiles, scores):
    """The grouped score product over probed lists: for every tile (list c, slot tile, row tile) of ``tiles`` (int32
    [n_tiles, 4]) the inner products of the queries Q[slot_query[...]] with the list's rows, into the ragged score buffer
    (slot s owns the floats from scores[slot_off[s]])."""
    qp, qld = _mat(Q)
    rp, rld = _mat(rows)
    if Q.shape[1] != rows.shape[1]:
        raise ValueError("queries and list rows of one padded width")
    nlist = list_start.numel() - 1
    n_slots = slot_query.numel()
    if tiles.dim() != 2 or tiles.shape[1] != 4:
        raise ValueError("tiles must be int32 [n_tiles, 4]")
    call("cdml_ivf_scan_f32", qp, qld, Q.shape[0], _vec(slot_query, torch.int32, 0, "slot_query"),
         _vec(slot_start, torch.int32, nlist + 1, "slot_start"), _vec(slot_off, torch.int64, n_slots, "slot_off"), rp, rld,
         _vec(list_start, torch.int32, nlist + 1, "list_start"), Q.shape[1], _vec(tiles, torch.int32, 4, "tiles"),
         tiles.shape[0], _p(scores, torch.float32), _stream())
    return scores


def ivf_merge(scores, slot_off, slot_of, probe, list_start, ids, r_sq, q_sq, k, best_d, best_i):
    """One wave per query: the k best (d, id) keys over the query's probed score segments; writes the query's whole sorted list
    best_d / best_i [nq, knn_list_capacity()] (+inf / 0x7fffffff = empty)."""
    nq, nprobe = probe.shape
    cap = knn_list_capacity()
    if tuple(slot_of.shape) != (nq, nprobe) or tuple(best_d.shape) != (nq, cap) or tuple(best_i.shape) != (nq, cap):
        raise ValueError("slot_of [nq, nprobe] and best_d / best_i [nq, %d]" % cap)
    call("cdml_ivf_merge", _p(scores, torch.float32), _vec(slot_off, torch.int64, 0, "slot_off"),
         _vec(slot_of, torch.int32, nq * nprobe, "slot_of"), _vec(probe, torch.int32, nq * nprobe, "probe"), nq, nprobe,
         _vec(list_start, torch.int32, 2, "list_start"), _vec(ids, torch.int32, 0, "ids"), _vec(r_sq, torch.float32, 0, "r_sq"),
         _vec(q_sq, torch.float32, nq, "q_sq"), k, _vec(best_d, torch.float32, nq * cap, "best_d"),
         _vec(best_i, torch.int32, nq * cap, "best_i"), _stream())


# ---------------------------------------- fp16 lists of the IVF index (include/cdml_ivf_f16.h) ------
def ivf_scan_f16(Q, slot_query, slot_start, slot_off, rows, list_start, tiles, scores):
    """``ivf_scan_f32`` with fp16 queries and list rows (torch.float16), fp32 scores: the grouped score product on the fp16
    MFMA, same tables and score buffer."""
    if Q.dtype != torch.float16 or rows.dtype != torch.float16:
        raise ValueError("ivf_scan_f16 takes float16 queries and list rows")
    if Q.dim() != 2 or rows.dim() != 2 or Q.stride(1) != 1 or rows.stride(1) != 1 or Q.shape[1] != rows.shape[1]:
        raise ValueError("queries and list rows: 2-D, unit inner stride, one padded width")
    nlist = list_start.numel() - 1
    n_slots = slot_query.numel()
    if tiles.dim() != 2 or tiles.shape[1] != 4:
        raise ValueError("tiles must be int32 [n_tiles, 4]")
    call("cdml_ivf_scan_f16", _p(Q), Q.stride(0), Q.shape[0], _vec(slot_query, torch.int32, 0, "slot_query"),
         _vec(slot_start, torch.int32, nlist + 1, "slot_start"), _vec(slot_off, torch.int64, n_slots, "slot_off"), _p(rows),
         rows.stride(0), _vec(list_start, torch.int32, nlist + 1, "list_start"), Q.shape[1],
         _vec(tiles, torch.int32, 4, "tiles"), tiles.shape[0], _p(scores, torch.float32), _stream())
    return scores


def ivf_refine(Q, base, cand, r, k, best_d, best_i):
    """One wave per query: the direct fp32 distances sum_j (q_j - x_j)^2 of the first ``r`` candidates of ``cand`` (int32
    [nq, knn_list_capacity()], ``ivf_merge``'s best_i; 0x7fffffff = none) against the rows of ``base`` (fp32 [n_rows, >= Dp],
    Dp = Q's width), sorted by (d, id) into best_d / best_i [nq, knn_list_capacity()] (+inf / 0x7fffffff behind the valid
    ones).  ``cand`` and ``best_i`` are different tensors."""
    qp, qld = _mat(Q)
    bp, bld = _mat(base)
    nq, Dp = Q.shape
    cap = knn_list_capacity()
    if base.shape[1] < Dp:
        raise ValueError("base rows must be at least as wide as the queries (%d < %d)" % (base.shape[1], Dp))
    if tuple(cand.shape) != (nq, cap) or tuple(best_d.shape) != (nq, cap) or tuple(best_i.shape) != (nq, cap):
        raise ValueError("cand, best_d and best_i must be [nq, %d]" % cap)
    if cand.data_ptr() == best_i.data_ptr():
        raise ValueError("cand and best_i must be different tensors")
    call("cdml_ivf_refine", qp, qld, nq, bp, bld, base.shape[0], Dp, _vec(cand, torch.int32, nq * cap, "cand"), int(r), int(k),
         _vec(best_d, torch.float32, nq * cap, "best_d"), _vec(best_i, torch.int32, nq * cap, "best_i"), _stream())


# ---------------------------------------- product-quantised lists of the IVF index (include/cdml_ivf_pq.h) ------
def _codebooks(codebooks):
    if codebooks.dtype != torch.float32 or codebooks.dim() != 3 or codebooks.shape[1] != 256 or not codebooks.is_contiguous():
        raise ValueError("codebooks must be a contiguous float32 [M, 256, dsub] tensor")
    return _p(codebooks), codebooks.shape[0], codebooks.shape[2]


def _pq_tile(symbol, M):
    s, r = C.c_int(0), C.c_int(0)
    call(symbol, int(M), C.byref(s), C.byref(r))
    return s.value, r.value


def _check_codes(codes, n, M):
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.stride(1) != 1 or codes.shape[0] < n or codes.shape[1] < M:
        raise ValueError("codes must be a uint8 [n, >= M] tensor with unit inner stride")


def _check_dist(dist, n, cols, cols_text):
    """(pointer, leading dimension) of the optional ``dist`` of an encoder: fp32 [n, >= cols], one column per subspace"""
    if dist is None:
        return C.c_void_p(0), 0
    dp, dld = _mat(dist)
    if dist.shape[0] < n or dist.shape[1] < cols:
        raise ValueError("dist must be a float32 [n, >= %s] tensor" % cols_text)
    return dp, dld


def _ivf_scan_pq_call(symbol, lut, codewords, slot_query, slot_start, slot_off, codes, list_start, tiles, scores, slot_base=None):
    """The three table-lookup scans: ``lut`` fp32 [n_queries, subspaces, codewords] with one subspace per code byte for 256
    codewords and two for 16; ``slot_base`` (fp32 [n_slots]) for the scan that starts its sums from it."""
    per_byte = 1 if codewords == 256 else 2
    if lut.dim() != 3 or lut.shape[2] != codewords or lut.shape[1] % per_byte or not lut.is_contiguous():
        raise ValueError("lut must be a contiguous float32 [n_queries, %s, %d] tensor" % ("M" if per_byte == 1 else "2 M", codewords))
    M = lut.shape[1] // per_byte
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.stride(1) != 1 or codes.shape[1] < M:
        raise ValueError("codes must be a uint8 [n_listed, >= M] tensor with unit inner stride")
    nlist = list_start.numel() - 1
    n_slots = slot_query.numel()
    if tiles.dim() != 2 or tiles.shape[1] != 4:
        raise ValueError("tiles must be int32 [n_tiles, 4]")
    base = () if slot_base is None else (_vec(slot_base, torch.float32, n_slots, "slot_base"),)
    call(symbol, _p(lut, torch.float32), lut.shape[0], _vec(slot_query, torch.int32, 0, "slot_query"),
         _vec(slot_start, torch.int32, nlist + 1, "slot_start"), _vec(slot_off, torch.int64, n_slots, "slot_off"), *base, _p(codes),
         codes.stride(0), _vec(list_start, torch.int32, nlist + 1, "list_start"), M, _vec(tiles, torch.int32, 4, "tiles"),
         tiles.shape[0], _p(scores, torch.float32), _stream())
    return scores


def ivf_pq_tile(M):
    """(S, R): the slots x rows of one work item of ``ivf_scan_pq`` for ``M`` bytes per row (host arithmetic)"""
    return _pq_tile("cdml_ivf_pq_tile", M)


def pq_encode(x, codebooks, codes, dist=None):
    """codes[r, m] (uint8 [n, >= M]; columns past M are not written) = the lowest codeword of subspace m nearest to
    x[r, m dsub:(m + 1) dsub] (x fp32 [n, >= M dsub]); ``dist`` (fp32 [n, >= M], optional) receives the attained minima."""
    xp, xld = _mat(x)
    cp, M, dsub = _codebooks(codebooks)
    n = x.shape[0]
    _check_codes(codes, n, M)
    if x.shape[1] < M * dsub:
        raise ValueError("x rows must hold M dsub = %d columns, got %d" % (M * dsub, x.shape[1]))
    dp, dld = _check_dist(dist, n, M, "M")
    call("cdml_pq_encode", xp, xld, n, cp, M, dsub, _p(codes), codes.stride(0), dp, dld, _stream())
    return codes


def pq_lut(Q, codebooks, lut):
    """lut[q, m, c] (fp32 [nq, M, 256], contiguous) = the inner product of Q[q, m dsub:(m + 1) dsub] with codeword c of
    subspace m."""
    qp, qld = _mat(Q)
    cp, M, dsub = _codebooks(codebooks)
    if Q.shape[1] < M * dsub:
        raise ValueError("query rows must hold M dsub = %d columns, got %d" % (M * dsub, Q.shape[1]))
    call("cdml_pq_lut", qp, qld, Q.shape[0], cp, M, dsub, _vec(lut, torch.float32, Q.shape[0] * M * 256, "lut"), _stream())
    return lut


def ivf_scan_pq(lut, slot_query, slot_start, slot_off, codes, list_start, tiles, scores):
    """``ivf_scan_f32`` by table lookup: for every tile (list c, slot tile, row tile; ``ivf_pq_tile(M)`` slots x rows) of
    ``tiles`` the sums over m of lut[query, m, codes[row, m]] into the ragged score buffer.  lut fp32 [n_queries, M, 256],
    codes uint8 [n_listed, M]."""
    return _ivf_scan_pq_call("cdml_ivf_scan_pq", lut, 256, slot_query, slot_start, slot_off, codes, list_start, tiles, scores)


# ---------------------------------------- residual product quantisation (include/cdml_ivf_pqr.h) ------
def pqr_encode(x, centroids, assign, codebooks, codes, dist=None):
    """``pq_encode`` of the residuals x[r] - centroids[assign[r]] (never materialised): centroids fp32 [nlist, >= M dsub],
    assign int64 [n]; a row whose assign is outside [0, nlist) gets codes 0 (and dist +inf)."""
    xp, xld = _mat(x)
    ep, eld = _mat(centroids)
    cp, M, dsub = _codebooks(codebooks)
    n = x.shape[0]
    _check_codes(codes, n, M)
    if x.shape[1] < M * dsub or centroids.shape[1] < M * dsub:
        raise ValueError("x rows and centroids must hold M dsub = %d columns, got %d and %d"
                         % (M * dsub, x.shape[1], centroids.shape[1]))
    dp, dld = _check_dist(dist, n, M, "M")
    call("cdml_pqr_encode", xp, xld, n, ep, eld, centroids.shape[0], _vec(assign, torch.int64, n, "assign"), cp, M, dsub,
         _p(codes), codes.stride(0), dp, dld, _stream())
    return codes


def ivf_slot_dots(Q, centroids, slot_query, slot_start, slot_base):
    """slot_base[s] (fp32 [n_slots]) = <Q[slot_query[s]], centroids[list of slot s]> over Q's (padded) width, in the fixed
    order of include/cdml_ivf_pqr.h; slot_start int32 [nlist + 1] names every slot's list."""
    qp, qld = _mat(Q)
    ep, eld = _mat(centroids)
    if Q.shape[1] != centroids.shape[1]:
        raise ValueError("queries and centroids of one padded width")
    nlist = centroids.shape[0]
    n_slots = slot_query.numel()
    call("cdml_ivf_slot_dots", qp, qld, Q.shape[0], ep, eld, Q.shape[1], _vec(slot_query, torch.int32, 0, "slot_query"),
         _vec(slot_start, torch.int32, nlist + 1, "slot_start"), nlist, _vec(slot_base, torch.float32, n_slots, "slot_base"),
         _stream())
    return slot_base


def ivf_scan_pqr(lut, slot_query, slot_start, slot_off, slot_base, codes, list_start, tiles, scores):
    """``ivf_scan_pq`` with every slot's sums starting from ``slot_base[slot]`` (``ivf_slot_dots``): the scan of an index with
    ``pq_residual=True``."""
    return _ivf_scan_pq_call("cdml_ivf_scan_pqr", lut, 256, slot_query, slot_start, slot_off, codes, list_start, tiles, scores,
                             slot_base=slot_base)


# ---------------------------------------- 4-bit product quantisation (include/cdml_ivf_pq4.h) ------
def _codebooks4(codebooks):
    if codebooks.dtype != torch.float32 or codebooks.dim() != 3 or codebooks.shape[1] != 16 or codebooks.shape[0] % 2 \
            or not codebooks.is_contiguous():
        raise ValueError("codebooks must be a contiguous float32 [2 M, 16, dsub] tensor")
    return _p(codebooks), codebooks.shape[0] // 2, codebooks.shape[2]


def ivf_pq4_tile(M):
    """(S, R): the slots x rows of one work item of ``ivf_scan_pq4`` for ``M`` bytes per row (host arithmetic)"""
    return _pq_tile("cdml_ivf_pq4_tile", M)


def pq4_encode(x, codebooks, codes, dist=None):
    """codes[r, b] (uint8 [n, >= M]; columns past M are not written) = code(2b) | code(2b + 1) << 4, code(m) the lowest of
    subspace m's 16 codewords nearest to x[r, m dsub:(m + 1) dsub] (x fp32 [n, >= 2 M dsub], codebooks fp32 [2 M, 16, dsub]);
    ``dist`` (fp32 [n, >= 2 M], optional) receives the attained minima per subspace."""
    xp, xld = _mat(x)
    cp, M, dsub = _codebooks4(codebooks)
    n = x.shape[0]
    _check_codes(codes, n, M)
    if x.shape[1] < 2 * M * dsub:
        raise ValueError("x rows must hold 2 M dsub = %d columns, got %d" % (2 * M * dsub, x.shape[1]))
    dp, dld = _check_dist(dist, n, 2 * M, "2 M")
    call("cdml_pq4_encode", xp, xld, n, cp, M, dsub, _p(codes), codes.stride(0), dp, dld, _stream())
    return codes


def pq4_lut(Q, codebooks, lut):
    """lut[q, m, c] (fp32 [nq, 2 M, 16], contiguous) = the inner product of Q[q, m dsub:(m + 1) dsub] with codeword c of
    subspace m."""
    qp, qld = _mat(Q)
    cp, M, dsub = _codebooks4(codebooks)
    if Q.shape[1] < 2 * M * dsub:
        raise ValueError("query rows must hold 2 M dsub = %d columns, got %d" % (2 * M * dsub, Q.shape[1]))
    call("cdml_pq4_lut", qp, qld, Q.shape[0], cp, M, dsub, _vec(lut, torch.float32, Q.shape[0] * 2 * M * 16, "lut"), _stream())
    return lut


def ivf_scan_pq4(lut, slot_query, slot_start, slot_off, codes, list_start, tiles, scores):
    """``ivf_scan_pq`` on 4-bit codes: for every tile (``ivf_pq4_tile(M)`` slots x rows) the sums over the row's bytes b of
    lut[query, 2b, low nibble] + lut[query, 2b + 1, high nibble] (the pair added first) into the ragged score buffer.  lut fp32
    [n_queries, 2 M, 16], codes uint8 [n_listed, M]."""
    return _ivf_scan_pq_call("cdml_ivf_scan_pq4", lut, 16, slot_query, slot_start, slot_off, codes, list_start, tiles, scores)


# ---------------------------------------- add / remove of the IVF index (include/cdml_ivf_update.h) ------
def _payload(t, what, allow_none=False):
    """(pointer, stride in bytes, rows, row bytes) of a list payload: any 2-D tensor with unit inner stride (opaque bytes)"""
    if t is None or (allow_none and t.shape[0] == 0):
        if not allow_none:
            raise ValueError("%s must be given" % what)
        return C.c_void_p(0), 0, 0, None
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("%s must be a 2-D tensor with unit inner stride" % what)
    es = t.element_size()
    return _p(t), t.stride(0) * es, t.shape[0], t.shape[1] * es


def ivf_lists_move(old_rows, old_ids, old_r_sq, old_pos, add_rows, add_r_sq, add_order, id0, kept_start, add_start, new_start,
                   new_rows, new_ids, new_r_sq):
    """The lists of an updated index in ONE launch (include/cdml_ivf_update.h): destination position o of list c takes kept old
    row ``kept_start[c] + off`` (through ``old_pos``, int32, when it is not None) while off = o - new_start[c] is below the
    list's kept count, else chunk row j = ``add_order[add_start[c] + off - kept]`` with the id ``id0 + j``.  The payloads
    (``old_rows``, ``add_rows``, ``new_rows``) are 2-D tensors of one row length in bytes (a multiple of 8) and any row stride;
    ids int32, r_sq fp32; the three start tables int32 [nlist + 1].  ``old_*`` may be None / empty (an index without rows),
    ``add_*`` too (a removal).  Writes rows [0, new_rows.shape[0]) of the three new arrays."""
    np_, nld, n_new, rb = _payload(new_rows, "new_rows")
    op, old_ld, n_old, rb_o = _payload(old_rows, "old_rows", True)
    ap, add_ld, n_chunk, rb_a = _payload(add_rows, "add_rows", True)
    if (rb_o is not None and rb_o != rb) or (rb_a is not None and rb_a != rb):
        raise ValueError("old, added and new payload rows must have one length in bytes (%s / %s / %s)" % (rb_o, rb_a, rb))
    nlist = new_start.numel() - 1
    n_kept = n_old if old_pos is None else old_pos.numel()
    n_add = 0 if add_order is None else add_order.numel()
    call("cdml_ivf_lists_move", op, old_ld, _vec(old_ids, torch.int32, n_old, "old_ids") if n_old else C.c_void_p(0),
         _vec(old_r_sq, torch.float32, n_old, "old_r_sq") if n_old else C.c_void_p(0), n_old,
         None if old_pos is None else _vec(old_pos, torch.int32, n_kept, "old_pos") if n_kept else C.c_void_p(0), n_kept,
         ap, add_ld, _vec(add_r_sq, torch.float32, n_chunk, "add_r_sq") if n_chunk else C.c_void_p(0), n_chunk,
         _vec(add_order, torch.int32, n_add, "add_order") if n_add else C.c_void_p(0), n_add, int(id0),
         _vec(kept_start, torch.int32, nlist + 1, "kept_start"), _vec(add_start, torch.int32, nlist + 1, "add_start"),
         _vec(new_start, torch.int32, nlist + 1, "new_start"), nlist, rb, np_, nld,
         _vec(new_ids, torch.int32, n_new, "new_ids"), _vec(new_r_sq, torch.float32, n_new, "new_r_sq"), n_new, _stream())
    return new_rows, new_ids, new_r_sq


def ivf_locate(q_ids, assign, ids, list_start, pos):
    """pos[q] (int32) = the position of catalogue id ``q_ids[q]`` (int64) in the cluster-major lists -- a binary search among
    the ascending ``ids`` (int32) of list ``assign[id]`` (int64 [n_rows]) -- or -1 where the id is in no list."""
    nq, nlist = q_ids.numel(), list_start.numel() - 1
    call("cdml_ivf_locate", _vec(q_ids, torch.int64, nq, "q_ids"), nq, _vec(assign, torch.int64, 0, "assign"), assign.numel(),
         _vec(ids, torch.int32, 0, "ids") if ids.numel() else C.c_void_p(0), ids.numel(),
         _vec(list_start, torch.int32, nlist + 1, "list_start"), nlist, _vec(pos, torch.int32, nq, "pos"), _stream())
    return pos


# ---------------------------------------- threshold-filter scan of the IVF index (include/cdml_ivf_filter.h) ------
def _ivf_filter(name, qp, qld, rp, rld, Q, slot_query, slot_start, q_sq, tau, cnt, rows, list_start, r_sq, ids, tiles, cand, cap):
    nlist = list_start.numel() - 1
    nq, n_listed, cap = Q.shape[0], rows.shape[0], int(cap)
    if tiles.dim() != 2 or tiles.shape[1] != 4:
        raise ValueError("tiles must be int32 [n_tiles, 4]")
    if cand.dtype != torch.int32 or not cand.is_contiguous() or cand.numel() < 2 * nq * cap:
        raise ValueError("cand must be a contiguous int32 tensor of at least [nq = %d, cap = %d, 2]" % (nq, cap))
    call(name, qp, qld, nq, _vec(slot_query, torch.int32, 0, "slot_query"), _vec(slot_start, torch.int32, nlist + 1, "slot_start"),
         _vec(q_sq, torch.float32, nq, "q_sq"), _vec(tau, torch.float32, nq, "tau"), _vec(cnt, torch.int32, nq, "cnt"), rp, rld,
         _vec(list_start, torch.int32, nlist + 1, "list_start"), _vec(r_sq, torch.float32, n_listed, "r_sq"),
         _vec(ids, torch.int32, n_listed, "ids"), Q.shape[1], _vec(tiles, torch.int32, 4, "tiles"), tiles.shape[0],
         _p(cand, torch.int32), cap, _stream())
    return cnt


def ivf_filter_f32(Q, slot_query, slot_start, q_sq, tau, cnt, rows, list_start, r_sq, ids, tiles, cand, cap):
    """``ivf_scan_f32``'s grouped product over the tiles of ``tiles`` with no score buffer: every (query q, listed row)
    element with d = max((q_sq[q] + r_sq[row]) - 2 s, 0) <= tau[q] takes slot pos = cnt[q]++ of the query's candidate list and,
    when pos < cap, writes cand[q, pos] = (the bits of d, ids[row]) (cand int32 [nq, cap, 2]; cap a power of two)."""
    qp, qld = _mat(Q)
    rp, rld = _mat(rows)
    if Q.shape[1] != rows.shape[1]:
        raise ValueError("queries and list rows of one padded width")
    return _ivf_filter("cdml_ivf_filter_f32", qp, qld, rp, rld, Q, slot_query, slot_start, q_sq, tau, cnt, rows, list_start, r_sq,
                       ids, tiles, cand, cap)


def ivf_filter_f16(Q, slot_query, slot_start, q_sq, tau, cnt, rows, list_start, r_sq, ids, tiles, cand, cap):
    """``ivf_filter_f32`` with fp16 queries and list rows (torch.float16): ``ivf_scan_f16``'s product on the fp16 MFMA."""
    if Q.dtype != torch.float16 or rows.dtype != torch.float16:
        raise ValueError("ivf_filter_f16 takes float16 queries and list rows")
    if Q.dim() != 2 or rows.dim() != 2 or Q.stride(1) != 1 or rows.stride(1) != 1 or Q.shape[1] != rows.shape[1]:
        raise ValueError("queries and list rows: 2-D, unit inner stride, one padded width")
    return _ivf_filter("cdml_ivf_filter_f16", _p(Q), Q.stride(0), _p(rows), rows.stride(0), Q, slot_query, slot_start, q_sq, tau,
                       cnt, rows, list_start, r_sq, ids, tiles, cand, cap)


# ---------------------------------------- filter scan over product-quantised lists (include/cdml_ivf_range.h) ------
def _ivf_filter_pq_call(symbol, lut, slot_query, slot_start, q_sq, tau, cnt, codes, list_start, r_sq, ids, tiles, cand, cap,
                        slot_base=None):
    """The two filter scans over 8-bit codes: ``_ivf_scan_pq_call``'s checks of lut / codes / tiles, ``_ivf_filter``'s of the
    candidate set."""
    if lut.dim() != 3 or lut.shape[2] != 256 or not lut.is_contiguous():
        raise ValueError("lut must be a contiguous float32 [n_queries, M, 256] tensor")
    nq, M, cap = lut.shape[0], lut.shape[1], int(cap)
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.stride(1) != 1 or codes.shape[1] < M:
        raise ValueError("codes must be a uint8 [n_listed, >= M] tensor with unit inner stride")
    nlist = list_start.numel() - 1
    n_slots, n_listed = slot_query.numel(), codes.shape[0]
    if tiles.dim() != 2 or tiles.shape[1] != 4:
        raise ValueError("tiles must be int32 [n_tiles, 4]")
    if cand.dtype != torch.int32 or not cand.is_contiguous() or cand.numel() < 2 * nq * cap:
        raise ValueError("cand must be a contiguous int32 tensor of at least [nq = %d, cap = %d, 2]" % (nq, cap))
    base = () if slot_base is None else (_vec(slot_base, torch.float32, n_slots, "slot_base"),)
    call(symbol, _p(lut, torch.float32), nq, _vec(slot_query, torch.int32, 0, "slot_query"),
         _vec(slot_start, torch.int32, nlist + 1, "slot_start"), *base, _vec(q_sq, torch.float32, nq, "q_sq"),
         _vec(tau, torch.float32, nq, "tau"), _vec(cnt, torch.int32, nq, "cnt"), _p(codes), codes.stride(0),
         _vec(list_start, torch.int32, nlist + 1, "list_start"), _vec(r_sq, torch.float32, n_listed, "r_sq"),
         _vec(ids, torch.int32, n_listed, "ids"), M, _vec(tiles, torch.int32, 4, "tiles"), tiles.shape[0], _p(cand, torch.int32),
         cap, _stream())
    return cnt


def ivf_filter_pq(lut, slot_query, slot_start, q_sq, tau, cnt, codes, list_start, r_sq, ids, tiles, cand, cap):
    """``ivf_scan_pq``'s sums over the tiles of ``tiles`` (``ivf_pq_tile(M)`` slots x rows) with no score buffer: every (query q,
    listed row) with d = max((q_sq[q] + r_sq[row]) - 2 s, 0) <= tau[q] takes slot pos = cnt[q]++ of the query's candidate list
    and, when pos < cap, writes cand[q, pos] = (the bits of d, ids[row]) (cand int32 [nq, cap, 2]; cap a power of two)."""
    return _ivf_filter_pq_call("cdml_ivf_filter_pq", lut, slot_query, slot_start, q_sq, tau, cnt, codes, list_start, r_sq, ids,
                               tiles, cand, cap)


def ivf_filter_pqr(lut, slot_query, slot_start, slot_base, q_sq, tau, cnt, codes, list_start, r_sq, ids, tiles, cand, cap):
    """``ivf_filter_pq`` with every slot's sums starting from ``slot_base[slot]`` (``ivf_slot_dots``): ``ivf_scan_pqr``'s sums."""
    return _ivf_filter_pq_call("cdml_ivf_filter_pqr", lut, slot_query, slot_start, q_sq, tau, cnt, codes, list_start, r_sq, ids,
                               tiles, cand, cap, slot_base=slot_base)


def knn_desim_prep(fI, fD, fI_end, threshold, out):
    """The raw-feature lists fI (int32 | int64 [n_f, kf]) with their distances fD (fp32) filtered into out (int32
    [n_f, kp], kp = 32 | 64): fI[r, t] for t < fI_end where fD <= threshold (float32), fI != r, fI >= 0; else -1."""
    if fI.dtype not in (torch.int32, torch.int64):
        raise ValueError("fI must be int32 or int64")
    fp, fld = _mat(fI, fI.dtype)
    dp, dld = _mat(fD)
    op, _ = _mat(out, torch.int32)
    if not out.is_contiguous() or out.shape[0] != fI.shape[0] or fD.shape[0] != fI.shape[0]:
        raise ValueError("fI, fD and out must have the same rows (out contiguous)")
    call("cdml_knn_desim_prep", fp, int(fI.dtype == torch.int64), fld, dp, dld, fI.shape[0], int(fI_end), float(threshold),
         op, out.shape[1], _stream())
    return out


def knn_desim(eI, f_filtered, out, query_id=None, row0=0):
    """The greedy near-duplicate rule of iter_desim_mp on every row of eI (int32 [nq, ke]) into out (int32 [nq, ke]):
    f_filtered = knn_desim_prep's matrix; query_id (int32 [nq], optional; default row0 + i) is removed at the end."""
    ep, eld = _mat(eI, torch.int32)
    op, old = _mat(out, torch.int32)
    fp, _ = _mat(f_filtered, torch.int32)
    if not f_filtered.is_contiguous() or out.shape[0] < eI.shape[0] or out.shape[1] < eI.shape[1]:
        raise ValueError("f_filtered must be contiguous and out at least eI's shape")
    if query_id is not None and (not query_id.is_contiguous() or query_id.numel() < eI.shape[0]):
        raise ValueError("query_id must be a contiguous int32 vector of nq ids")
    call("cdml_knn_desim", ep, eld, eI.shape[0], eI.shape[1], _p(query_id, torch.int32), int(row0), fp, f_filtered.shape[1],
         f_filtered.shape[0], op, old, _stream())
    return out


def _knn_lines_args(D, I, row0, guid_off):
    if D.dim() != 2 or tuple(D.shape) != tuple(I.shape):
        raise ValueError("D and I of one shape [n, k]")
    dp, dld = _mat(D)
    ip, ild = _mat(I, torch.int64)
    if not guid_off.is_contiguous() or guid_off.dim() != 1 or guid_off.numel() < 2:
        raise ValueError("guid_off must be a contiguous int64 vector of n_guid + 1 offsets")
    return dp, dld, ip, ild, int(row0), D.shape[0], D.shape[1], _p(guid_off, torch.int64), guid_off.numel() - 1


def knn_line_sizes(D, I, row0, guid_off, guid_total, sizes, flags):
    """sizes[r] (int64) = the bytes of the export's text line of row r of D (fp32) / I (int64) [n, k <= 128], whose own guid is
    ``row0 + r``; flags[r] (int32) = 1 where a kept distance is outside the shortest-repr routine's range
    (include/cdml_knn_writer.h).  guid_off int64 [n_guid + 1]: the byte offsets of the guid table (``guid_total`` bytes)."""
    a = _knn_lines_args(D, I, row0, guid_off)
    if sizes.numel() < D.shape[0] or flags.numel() < D.shape[0] or not sizes.is_contiguous() or not flags.is_contiguous():
        raise ValueError("sizes and flags: contiguous vectors of n entries")
    call("cdml_knn_line_sizes", *a, int(guid_total), _p(sizes, torch.int64), _p(flags, torch.int32), _stream())
    return sizes, flags


def knn_line_write(D, I, row0, guid_bytes, guid_off, off, out):
    """The lines ``knn_line_sizes`` measured, written into out (uint8): row r's bytes at [off[r], off[r + 1]) (off int64
    [n + 1], the exclusive scan of the sizes); no store leaves that extent or the buffer."""
    a = _knn_lines_args(D, I, row0, guid_off)
    if off.numel() < D.shape[0] + 1 or not off.is_contiguous() or not out.is_contiguous() or not guid_bytes.is_contiguous():
        raise ValueError("off: a contiguous vector of n + 1 entries; out and guid_bytes contiguous")
    call("cdml_knn_line_write", *a[:7], _p(guid_bytes, torch.uint8), a[7], a[8], guid_bytes.numel(), _p(off, torch.int64),
         _p(out, torch.uint8), out.numel(), _stream())
    return out


# ------------------------------------------------- fusion towers (N4) ---------
EW_MUL, EW_MUL_RES, EW_ADD = 0, 1, 2


def ew_combine(mode, a, b, out, M, N):
    ap, ald = _mat(a)
    bp, bld = _mat(b)
    op, old = _mat(out)
    call("cdml_ew_combine", mode, ap, ald, bp, bld, M, N, op, old, _stream())
    return out


def ew_fusion_bwd(residual, g, a, b, da, db, M, N, alpha=LRELU_ALPHA):
    gp, gld = _mat(g)
    ap, ald = _mat(a)
    bp, bld = _mat(b)
    dap, dald = _mat(da)
    dbp, dbld = _mat(db)
    call("cdml_ew_fusion_bwd", 1 if residual else 0, gp, gld, ap, ald, bp, bld, M, N, alpha, dap, dald,
         dbp, dbld, _stream())


def lrelu_bwd(g, y, out, M, N, alpha=LRELU_ALPHA):
    gp, gld = _mat(g)
    yp, yld = _mat(y)
    op, old = _mat(out)
    call("cdml_lrelu_bwd", gp, gld, yp, yld, M, N, alpha, op, old, _stream())
    return out


# ------------------------------------------- reduced precision (config 4) -----
BE_BIAS_LRELU_BF16, BE_BIAS_LRELU_F32, BE_MASK_BF16, BE_F32 = 0, 1, 2, 3
BE_BIAS_LRELU_BF16_BITS, BE_MASKBITS_BF16 = 4, 5      # 0 + sign bitmask out (aux) / 2 reading that bitmask


def gemm_bf16_epilogue_supported(epilogue, M, N, K, lda, ldb, ldc, ldaux):
    return bool(load_library().cdml_gemm_bf16_epilogue_supported(epilogue, M, N, K, lda, ldb, ldc, ldaux))


def _mat16(t):
    if t.dim() != 2 or t.stride(1) != 1 or t.element_size() != 2:
        raise ValueError("expected a 2-D 16-bit tensor with unit inner stride")
    return _p(t), t.stride(0)


def _mat8(t):
    """(pointer, leading dimension) of the codes of an fp8 catalogue (torch.float8_e4m3fn)."""
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float8_e4m3fn:
        raise ValueError("expected a 2-D float8_e4m3fn tensor with unit inner stride")
    return _p(t), t.stride(0)


def gemm_bf16_workspace(M, N, K):
    return int(load_library().cdml_gemm_bf16_workspace(M, N, K))


def gemm_bf16_nt(epilogue, A, B, C, M, N, K, bias=None, aux=None, alpha=LRELU_ALPHA, workspace=None):
    ap, ald = _mat16(A)
    bp, bld = _mat16(B)
    if C.dim() != 2 or C.stride(1) != 1:
        raise ValueError("C must be 2-D with unit inner stride")
    xld = aux.stride(0) if aux is not None else 0
    if aux is not None and (aux.dtype == torch.uint8) != (epilogue in (BE_BIAS_LRELU_BF16_BITS, BE_MASKBITS_BF16)):
        raise ValueError("epilogues 4 / 5 take a uint8 bitmask as aux, epilogue 2 bf16 values")
    call("cdml_gemm_bf16_nt", epilogue, ap, ald, bp, bld, M, N, K, _p(C), C.stride(0), _p(bias),
         _p(aux), xld, alpha, _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(),
         _stream())
    return C


def gemm_bf16_tn_supported(M, N, K, lda, ldb):
    return bool(load_library().cdml_gemm_bf16_tn_supported(M, N, K, lda, ldb))


def gemm_bf16_tn_workspace(M, N, K):
    return int(load_library().cdml_gemm_bf16_tn_workspace(M, N, K))


def gemm_bf16_tn(A, B, C, M, N, K, workspace=None, colsum=None):
    """C[M][N] f32 = sum_k A[k][M] * B[k][N]: the weight gradient from the activations as
    stored; colsum[n] = sum_k B[k][n] (the bias gradient) on request."""
    ap, ald = _mat16(A)
    bp, bld = _mat16(B)
    cp, cld = _mat(C)
    call("cdml_gemm_bf16_tn", ap, ald, bp, bld, M, N, K, cp, cld, _p(colsum, torch.float32), _p(workspace),
         0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())
    return C


# ---- fp32 products on the bf16 MFMA: operands as three bf16 planes (csrc/gemm_bf16x3.hip) ----
BE_BIAS_LRELU_X3, BE_MASK_X3, BE_ROWBIAS_LRELU_X3 = 6, 7, 8
BE_BIAS_LRELU_X3_BITS, BE_MASKBITS_X3 = 9, 10         # 6 + sign bitmask out (aux, uint8 [M][N / 8]) / 7 reading that bitmask
BE_MASKBITS_X3_KI = 12                                # 10 (7 without aux) with the result's planes k8-interleaved: [3][M / 8][ldc][8]


def split_f32_bf16x3(src, dst, plane, transpose=False):
    """dst[r][p*plane + c] = bf16 plane p (hi, mid, lo) of the fp32 src[r][c]; transpose: dst[c][p*plane + r]."""
    sp, sld = _mat(src)
    dp, dld = _mat16(dst)
    call("cdml_split_f32_bf16x3", sp, sld, src.shape[0], src.shape[1], dp, dld, plane, 1 if transpose else 0, _stream())
    return dst


def gemm_bf16x3_workspace(tn, M, N, K, products=6):
    return int(load_library().cdml_gemm_bf16x3_workspace(1 if tn else 0, M, N, K, products))


def gemm_bf16x3_nt(epilogue, A, plane_a, B, plane_b, C, M, N, K, products=6, plane_c=0, bias=None, aux=None,
                   alpha=LRELU_ALPHA, workspace=None, colsum=None, ldc=None, slab_steps=None):
    """C = epilogue(A . B^T) for fp32 operands given as bf16 planes [rows][hi K | mid K | lo K]; colsum[n] = sum_k
    B[n][k] on request.  Epilogue 12: C is the flat k8-interleaved buffer [3][M / 8][ldc][8] (``ldc`` = columns per row
    group, ``plane_c`` = elements per plane).  ``slab_steps`` (the narrow layer, N = 256): pin the K-slab length for this
    call (cdml_x3_slab_steps) instead of the rule by row-tile class."""
    if slab_steps:
        lib = load_library()
        prev = lib.cdml_x3_slab_steps(int(slab_steps))
        try:
            return gemm_bf16x3_nt(epilogue, A, plane_a, B, plane_b, C, M, N, K, products=products, plane_c=plane_c, bias=bias,
                                  aux=aux, alpha=alpha, workspace=workspace, colsum=colsum, ldc=ldc)
        finally:
            lib.cdml_x3_slab_steps(prev)
    ap, ald = _mat16(A)
    bp, bld = _mat16(B)
    if epilogue == BE_MASKBITS_X3_KI:
        if ldc is None or not C.is_contiguous() or C.dtype != torch.bfloat16:
            raise ValueError("epilogue 12 writes a contiguous bf16 buffer and needs ldc (columns per row group)")
    elif C.dim() != 2 or C.stride(1) != 1:
        raise ValueError("C must be 2-D with unit inner stride")
    if aux is not None and (aux.dtype == torch.uint8) != (epilogue in (BE_BIAS_LRELU_X3_BITS, BE_MASKBITS_X3, BE_MASKBITS_X3_KI)):
        raise ValueError("epilogues 9 / 10 / 12 take a uint8 bitmask as aux, epilogue 7 bf16 values")
    call("cdml_gemm_bf16x3_nt", epilogue, ap, ald, plane_a, bp, bld, plane_b, M, N, K, products, _p(C), C.stride(0) if ldc is None else ldc,
         plane_c, _p(bias), _p(aux), aux.stride(0) if aux is not None else 0, alpha, _p(colsum, torch.float32),
         _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())
    return C


def interleave8_bf16x3(src, plane_src, rows, cols, dst):
    """row-major planes [rows, >= 2 plane_src + cols] -> k8-interleaved [3, rows / 8, cols, 8] (csrc/gemm_bf16x3.hip)"""
    sp, sld = _mat16(src)
    if dst.dtype != torch.bfloat16 or not dst.is_contiguous() or dst.numel() < 3 * rows * cols:
        raise ValueError("interleave8_bf16x3: dst must be a contiguous bf16 buffer of 3 * rows * cols elements")
    call("cdml_interleave8_bf16x3", sp, sld, plane_src, rows, cols, C.c_void_p(dst.data_ptr()), _stream())
    return dst


def gemm_bf16x3_tnk(A, ma, a_col0, B, nb, b_col0, out, M, N, K, workspace=None, colsum=None):
    """out[M][N] f32 = sum_k A[k][a_col0 + m] B[k][b_col0 + n] on k8-interleaved operands [3, K / 8, ma | nb, 8] (six products)."""
    cp, cld = _mat(out)
    ws, wb = (C.c_void_p(0), 0) if workspace is None else (C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size())
    call("cdml_gemm_bf16x3_tnk", C.c_void_p(A.data_ptr()), ma, a_col0, C.c_void_p(B.data_ptr()), nb, b_col0, M, N, K, cp, cld,
         _p(colsum, torch.float32), ws, wb, _stream())
    return out


def gemm_bf16x3_tn_kb(A, plane_a, B, nb, b_col0, out, M, N, K, workspace=None, colsum=None):
    """out[M][N] f32 = sum_k A[k][m] B[k][b_col0 + n]: A row-major planes [K][hi | mid | lo], B k8-interleaved [3, K / 8, nb, 8]
    (six products; out and colsum bit-identical to gemm_bf16x3_tn)."""
    ap, ald = _mat16(A)
    cp, cld = _mat(out)
    ws, wb = (C.c_void_p(0), 0) if workspace is None else (C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size())
    call("cdml_gemm_bf16x3_tn_kb", ap, ald, plane_a, C.c_void_p(B.data_ptr()), nb, b_col0, M, N, K, cp, cld,
         _p(colsum, torch.float32), ws, wb, _stream())
    return out


def gemm_bf16x3_tn(A, plane_a, B, plane_b, C, M, N, K, products=6, workspace=None, colsum=None, bias=None,
                   alpha=LRELU_ALPHA, b_kint=None):
    """C[M][N] f32 = sum_k A[k][M] B[k][N] for fp32 operands given as bf16 planes [K][hi | mid | lo]
    (bias given: C = lrelu(. + bias)).  b_kint = (nb, b_col0): B is the k8-interleaved buffer of gemm_bf16x3_tn_kb instead
    (plane_b unused; six products, no bias)."""
    if b_kint is not None:
        if products != 6 or bias is not None:
            raise ValueError("gemm_bf16x3_tn: the interleaved B operand takes six products and no bias")
        return gemm_bf16x3_tn_kb(A, plane_a, B, b_kint[0], b_kint[1], C, M, N, K, workspace=workspace, colsum=colsum)
    ap, ald = _mat16(A)
    bp, bld = _mat16(B)
    cp, cld = _mat(C)
    call("cdml_gemm_bf16x3_tn", ap, ald, plane_a, bp, bld, plane_b, M, N, K, products, cp, cld, _p(bias), alpha,
         _p(colsum, torch.float32), _p(workspace),
         0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())
    return C


# ---- two fp16 planes per fp32 operand, three plane products (precision "f16x2"; csrc/gemm_f16x2_256.hip) ----
def split_f32_f16x2(src, dst, plane, scale, transpose=False):
    """dst[r][p*plane + c] = fp16 plane p (hi, lo) of src[r][c] * scale; transpose: dst[c][p*plane + r]."""
    sp, sld = _mat(src)
    dp, dld = _mat16(dst)
    call("cdml_split_f32_f16x2", sp, sld, src.shape[0], src.shape[1], dp, dld, plane, 1 if transpose else 0, float(scale), _stream())
    return dst


def gemm_f16x2_workspace(tn, M, N, K):
    return int(load_library().cdml_gemm_f16x2_workspace(1 if tn else 0, M, N, K))


def gemm_f16x2_nt(epilogue, A, plane_a, B, plane_b, C, M, N, K, out_scale, c_scale=1.0, plane_c=0, bias=None, aux=None,
                  alpha=LRELU_ALPHA, workspace=None, slab_steps=None):
    """C = epilogue(out_scale * A . B^T) for operands given as fp16 planes [rows][hi K | lo K] of (value * its scale);
    plane outputs (epilogues 6 / 7 / 9 / 10) are the fp16 planes of (result * c_scale)."""
    if slab_steps:
        lib = load_library()
        prev = lib.cdml_x3_slab_steps(int(slab_steps))
        try:
            return gemm_f16x2_nt(epilogue, A, plane_a, B, plane_b, C, M, N, K, out_scale, c_scale=c_scale, plane_c=plane_c,
                                 bias=bias, aux=aux, alpha=alpha, workspace=workspace)
        finally:
            lib.cdml_x3_slab_steps(prev)
    ap, ald = _mat16(A)
    bp, bld = _mat16(B)
    if C.dim() != 2 or C.stride(1) != 1:
        raise ValueError("C must be 2-D with unit inner stride")
    if aux is not None and (aux.dtype == torch.uint8) != (epilogue in (BE_BIAS_LRELU_X3_BITS, BE_MASKBITS_X3)):
        raise ValueError("epilogues 9 / 10 take a uint8 bitmask as aux, epilogue 7 16-bit values")
    call("cdml_gemm_f16x2_nt", epilogue, ap, ald, plane_a, bp, bld, plane_b, M, N, K, _p(C), C.stride(0), plane_c, _p(bias),
         _p(aux), aux.stride(0) if aux is not None else 0, alpha, float(out_scale), float(c_scale), _p(workspace),
         0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())
    return C


def gemm_f16x2_tn(A, plane_a, B, plane_b, C, M, N, K, out_scale, workspace=None, colsum=None, colsum_scale=1.0):
    """C[M][N] f32 = out_scale * sum_k A[k][M] B[k][N] on fp16 planes [K][hi | lo]; colsum[n] = colsum_scale * sum_k B[k][n]."""
    ap, ald = _mat16(A)
    bp, bld = _mat16(B)
    cp, cld = _mat(C)
    call("cdml_gemm_f16x2_tn", ap, ald, plane_a, bp, bld, plane_b, M, N, K, cp, cld, float(out_scale), _p(colsum, torch.float32),
         float(colsum_scale), _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(), _stream())
    return C


def gemm_bf16_tn2_workspace(M1, N1, M2, N2, K):
    """0 = shapes the joint launch does not take (use gemm_bf16_tn per product)."""
    return int(load_library().cdml_gemm_bf16_tn2_workspace(M1, N1, M2, N2, K))


def gemm_bf16_tn2(A1, B1, C1, M1, N1, A2, B2, C2, M2, N2, K, workspace, colsum1=None, colsum2=None):
    """C1 = A1^T.B1 and C2 = A2^T.B2 (k-strided operands, one K) in one stream-K launch + fix-up pass."""
    a1, lda1 = _mat16(A1)
    b1, ldb1 = _mat16(B1)
    c1, ldc1 = _mat(C1)
    a2, lda2 = _mat16(A2)
    b2, ldb2 = _mat16(B2)
    c2, ldc2 = _mat(C2)
    call("cdml_gemm_bf16_tn2", a1, lda1, b1, ldb1, M1, N1, c1, ldc1, _p(colsum1, torch.float32), a2, lda2, b2, ldb2,
         M2, N2, c2, ldc2, _p(colsum2, torch.float32), K, _p(workspace), workspace.numel() * workspace.element_size(),
         _stream())


def transpose_to_bf16(src, dst, rows, cols):
    call("cdml_transpose_to_bf16", 1 if src.dtype == torch.float32 else 0, _p(src), src.stride(0), rows, cols,
         _p(dst, torch.bfloat16), dst.stride(0), _stream())
    return dst


def cast_f32_bf16(src, dst, rows, cols):
    call("cdml_cast_f32_bf16", _p(src, torch.float32), src.stride(0), rows, cols, _p(dst, torch.bfloat16),
         dst.stride(0), _stream())
    return dst


def colsum_workspace_floats(rows, cols):
    return int(load_library().cdml_colsum_workspace_floats(rows, cols))


def colsum(src, rows, cols, out, workspace):
    call("cdml_colsum", 1 if src.dtype == torch.bfloat16 else 0, _p(src), src.stride(0), rows, cols,
         _p(out, torch.float32), _p(workspace, torch.float32), _stream())
    return out


def fill_uniform_table_f16(table, row0, feature_size, seed):
    call("cdml_fill_uniform_table_f16", _p(table, torch.float16), row0, table.shape[0], feature_size,
         table.stride(0), seed, _stream())
    return table


def gather_rows_f16(table, row0, idx, feature_size, x_out, oob_flag=None):
    call("cdml_gather_rows_f16", _p(table, torch.float16), row0, table.shape[0], table.stride(0),
         _p(idx, torch.int32), idx.numel(), feature_size, _p(x_out, torch.bfloat16), x_out.stride(0),
         _p(oob_flag, torch.int32), _stream())
    return x_out


# ---- the fp8 catalogue (include/cdml_f8.h): e4m3 codes -> l2-normalised bf16 rows, and the quantiser ----
def gather_rows_f8(table, row0, idx, feature_size, x_out, oob_flag=None):
    """gather_rows_f16 on the codes of an fp8 table: bit for bit its output on the fp16 table of the same values."""
    tp, tld = _mat8(table)
    call("cdml_gather_rows_f8", tp, row0, table.shape[0], tld, _p(idx, torch.int32), idx.numel(), feature_size,
         _p(x_out, torch.bfloat16), x_out.stride(0), _p(oob_flag, torch.int32), _stream())
    return x_out


def quantize_rows_f8(src, feature_size, codes, scale):
    """codes[r, :] (float8_e4m3fn, every column of the view written: the ones at or past feature_size as code 0) and scale[r]
    (fp32, a power of two) of the rows src[r, :feature_size] -- src fp32 or fp16 [n, stride]; codes may be a slice of a larger
    table, its stride is independent of src's."""
    if src.dim() != 2 or src.stride(1) != 1 or src.dtype not in (torch.float32, torch.float16):
        raise ValueError("quantize_rows_f8 needs a 2-D fp32 or fp16 source with unit inner stride")
    cp, cld = _mat8(codes)
    if codes.shape[0] != src.shape[0] or scale.numel() != src.shape[0] or not scale.is_contiguous():
        raise ValueError("quantize_rows_f8 needs one row of codes and one contiguous fp32 scale per source row")
    call("cdml_quantize_rows_f8_" + ("f32" if src.dtype == torch.float32 else "f16"), _p(src), src.shape[0], src.stride(0),
         feature_size, cp, cld, codes.shape[1], _p(scale, torch.float32), _stream())
    return codes, scale


# ------------------------------------------------------------- optimizers -----
def adam_step(w, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8, lr_dev=None, t_dev=None,
              advance_tickets=None):
    """advance_tickets (ops.new_tickets): also do global_step += 1 on *t_dev in the same launch."""
    call("cdml_adam_step", _p(w), _p(g), _p(m), _p(v), w.numel(), lr, _p(lr_dev), beta1, beta2, eps,
         0 if t is None else t, _p(t_dev, torch.int64), 0 if advance_tickets is None else 1,
         _p(advance_tickets, torch.int32), _stream())


def _seg_arrays(segments):
    """(n, offsets, sizes) of ``segments`` = [(offset, numel), ...] as the C arrays the LARS entries read."""
    n = len(segments)
    offs = (C.c_int64 * n)(*[int(o) for o, _ in segments])
    sizes = (C.c_int64 * n)(*[int(m) for _, m in segments])
    return n, C.cast(offs, C.c_void_p), C.cast(sizes, C.c_void_p)


def _copies(wt, wc, K, N, plane_t, plane_c, h2_scale=0.0):
    """The operand copies a matrix rule writes: wt = W^T [N, >= K], wc = W [K, >= N] (either may be None), as one bf16 copy,
    as three bf16 planes (plane_t / plane_c > 0, precision f32x3) or as two fp16 planes of W * h2_scale (precision f16x2)."""
    tp, tld = (C.c_void_p(0), 0) if wt is None else _mat16(wt)
    cp, cld = (C.c_void_p(0), 0) if wc is None else _mat16(wc)
    planes = 2 if h2_scale else 3 if (plane_t or plane_c) else 1
    if wt is not None and (wt.shape[0] < N or wt.shape[1] < ((planes - 1) * plane_t + K if planes > 1 else K)):
        raise ValueError("wt must be at least [N, K] (planes: [N, 2 plane_t + K]; fp16 planes: [N, plane_t + K])")
    if wc is not None and (wc.shape[0] < K or wc.shape[1] < ((planes - 1) * plane_c + N if planes > 1 else N)):
        raise ValueError("wc must be at least [K, N] (planes: [K, 2 plane_c + N]; fp16 planes: [K, plane_c + N])")
    return tp, tld, cp, cld, planes


def adam_matrix_bf16(W, g, m, v, lr, t, wt=None, wc=None, beta1=0.9, beta2=0.999, eps=1e-8, lr_dev=None, t_dev=None,
                     bias=None, advance_tickets=None, plane_t=0, plane_c=0, h2_scale=0.0):
    """Adam on the contiguous weight matrix W [K, N] (g, m, v alike) that also writes the operand copies (``_copies``).
    ``bias`` = (b, gb, mb, vb): the layer's bias vector updated in the same launch; ``advance_tickets``
    (ops.new_tickets): also global_step += 1 on *t_dev by the last block."""
    if W.dim() != 2 or not W.is_contiguous() or W.dtype != torch.float32:
        raise ValueError("W must be a contiguous fp32 matrix")
    K, N = W.shape
    for name, x in (("g", g), ("m", m), ("v", v)):
        if x.numel() != K * N or not x.is_contiguous() or x.dtype != torch.float32:
            raise ValueError("%s must be contiguous fp32 with W's size" % name)
    tp, tld, cp, cld, planes = _copies(wt, wc, K, N, plane_t, plane_c, h2_scale)
    b = bias if bias is not None else (None, None, None, None)
    if bias is not None and any(x.numel() != b[0].numel() or not x.is_contiguous() for x in b):
        raise ValueError("bias, its gradient and its moments must be contiguous vectors of one size")
    copies = {1: (tp, tld, cp, cld), 2: (tp, tld, plane_t, cp, cld, plane_c, float(h2_scale)),
              3: (tp, tld, plane_t, cp, cld, plane_c)}[planes]
    call("cdml_adam_matrix_" + {1: "bf16", 2: "h2", 3: "planes"}[planes], _p(W), _p(g), _p(m), _p(v), K, N, lr, _p(lr_dev),
         beta1, beta2, eps, 0 if t is None else t, _p(t_dev, torch.int64), *copies, _p(b[0]), _p(b[1]), _p(b[2]), _p(b[3]),
         0 if bias is None else b[0].numel(), 0 if advance_tickets is None else 1, _p(advance_tickets, torch.int32), _stream())


def table_adam_rows(table, row0, F, idx, grad_xhat, m_table, v_table, head, nxt, lr, t, beta1=0.9, beta2=0.999,
                    eps=1e-8, lr_dev=None, t_dev=None, grad_scale=1.0):
    """Lazy-Adam update of the catalogue rows a batch touched (see include/cdml.h)."""
    tp, tld = _mat(table)
    gp, gld = _mat(grad_xhat)
    if m_table.shape != table.shape or v_table.shape != table.shape or m_table.stride(0) != tld \
            or v_table.stride(0) != tld:
        raise ValueError("m/v tables must have the table's shape and stride")
    if head.numel() < table.shape[0] or nxt.numel() < idx.numel():
        raise ValueError("head needs one int32 per table row, next one per gathered row")
    call("cdml_table_adam_rows", tp, row0, table.shape[0], tld, F, _p(idx, torch.int32), idx.numel(), gp, gld,
         _p(m_table), _p(v_table), _p(head, torch.int32), _p(nxt, torch.int32), grad_scale, lr, _p(lr_dev), beta1, beta2,
         eps, 0 if t is None else t, _p(t_dev, torch.int64), _stream())


def grad_prepare(g, w, l2_scale, clip_norm, scratch, norms_out=None):
    """In place on one variable: g += l2_scale*w, then tf.clip_by_norm(g, clip_norm)."""
    call("cdml_grad_prepare", _p(g), _p(w), g.numel(), l2_scale, clip_norm, _p(scratch), _p(norms_out), _stream())


def momentum_step(w, g, acc, lr, momentum=0.9, use_nesterov=True, lr_dev=None):
    call("cdml_momentum_step", _p(w), _p(g), _p(acc), w.numel(), lr, _p(lr_dev), momentum,
         1 if use_nesterov else 0, _stream())


def lars_scratch_floats():
    return int(load_library().cdml_lars_scratch_floats())


def lars_step(w, g, acc, lr, scratch, momentum=0.9, weight_decay=1e-4, eeta=1e-3, eps=0.0,
              lr_dev=None):
    call("cdml_lars_step", _p(w), _p(g), _p(acc), w.numel(), lr, _p(lr_dev), momentum, weight_decay,
         eeta, eps, _p(scratch), _stream())


def lars_multi_scratch_floats():
    return int(load_library().cdml_lars_multi_scratch_floats())


def lars_multi(w, g, acc, segments, lr, scratch, momentum=0.9, weight_decay=1e-4, eeta=1e-3, eps=0.0,
               lr_dev=None, norms_out=None, step_dev=None, tickets=None):
    """LARS on every variable of the flat buffer in two launches: ``segments`` = [(offset, numel), ...]
    tiling w contiguously; step_dev (with tickets): also global_step += 1."""
    n, offs, sizes = _seg_arrays(segments)
    call("cdml_lars_multi", _p(w), _p(g), _p(acc), offs, sizes, n, lr, _p(lr_dev), momentum, weight_decay, eeta, eps,
         _p(scratch), _p(norms_out), _p(step_dev, torch.int64), _p(tickets, torch.int32), _stream())


def lars_multi_norms(w, g, segments, scratch):
    """Launch 1 of LARS alone: the per-block |w|^2, |g|^2 partials of every segment (then ``lars_matrix`` per matrix)."""
    n, offs, sizes = _seg_arrays(segments)
    call("cdml_lars_multi_norms", _p(w), _p(g), offs, sizes, n, _p(scratch), _stream())


def lars_matrix(w, g, acc, segments, seg_matrix, seg_bias, K, N, lr, scratch, wt=None, wc=None, plane_t=0, plane_c=0,
                momentum=0.9, weight_decay=1e-4, eeta=1e-3, eps=0.0, lr_dev=None, norms_out=None, step_dev=None,
                tickets=None, h2_scale=0.0):
    """LARS on the K x N weight matrix in segment ``seg_matrix`` of the flat buffers (+ the bias vector in segment
    ``seg_bias``, or None), after ``lars_multi_norms`` on the same segments; also writes the operand copies wt = W^T,
    wc = W (``_copies``).  step_dev (with tickets): also global_step += 1."""
    n, offs, sizes = _seg_arrays(segments)
    tp, tld, cp, cld, planes = _copies(wt, wc, K, N, plane_t, plane_c, h2_scale)
    call("cdml_lars_matrix_h2" if h2_scale else "cdml_lars_matrix", _p(w), _p(g), _p(acc), offs, sizes, n, seg_matrix,
         -1 if seg_bias is None else seg_bias, K, N, lr, _p(lr_dev), momentum, weight_decay, eeta, eps, _p(scratch),
         _p(norms_out), tp, tld, plane_t, cp, cld, plane_c, float(h2_scale) if h2_scale else planes,
         _p(step_dev, torch.int64), _p(tickets, torch.int32), _stream())


def momentum_matrix(W, g, acc, lr, wt=None, wc=None, plane_t=0, plane_c=0, momentum=0.9, use_nesterov=True, lr_dev=None,
                    bias=None, step_dev=None, tickets=None, h2_scale=0.0):
    """ApplyMomentum on the contiguous weight matrix W [K, N] (g, acc alike) + ``bias`` = (b, gb, accb), writing the
    operand copies like ``lars_matrix``."""
    if W.dim() != 2 or not W.is_contiguous() or W.dtype != torch.float32:
        raise ValueError("W must be a contiguous fp32 matrix")
    K, N = W.shape
    tp, tld, cp, cld, planes = _copies(wt, wc, K, N, plane_t, plane_c, h2_scale)
    b = bias if bias is not None else (None, None, None)
    call("cdml_momentum_matrix_h2" if h2_scale else "cdml_momentum_matrix", _p(W), _p(g), _p(acc), K, N, lr, _p(lr_dev),
         momentum, 1 if use_nesterov else 0, tp, tld, plane_t, cp, cld, plane_c, float(h2_scale) if h2_scale else planes,
         _p(b[0]), _p(b[1]), _p(b[2]), 0 if bias is None else b[0].numel(), _p(step_dev, torch.int64),
         _p(tickets, torch.int32), _stream())
