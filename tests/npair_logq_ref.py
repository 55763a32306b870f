"""fp64 reference of the N-pair loss with the sampling-bias (logQ) correction (ops.npair_loss(logq=...), include/cdml.h),
with and without a cross-batch memory, and a host model of the streaming estimator, for the tests."""
import numpy as np

import npair_memory_ref
import npair_ref


def _lse(x, mask, axis):
    return npair_ref._lse(x, mask, axis)


def npair_logq(A, P, ids, bias, temperature=0.1, symmetric=True, mem=None, mem_id=None, mem_bias=None):
    """A, P: [B, D] rows; bias [2B] each row's lq laid out like ids (bias[2i] = lq(a_i), bias[2i+1] = lq(p_i)); mem [M, D],
    mem_id [M] (-1 = empty) and mem_bias [M] the ring's (optional).  Returns loss, lse_row, lse_col (None unless
    symmetric), W [B, B], W_mem [B, M] (None without a memory), dA, dP, stats[4], masks."""
    A, P = np.asarray(A, np.float64), np.asarray(P, np.float64)
    B = A.shape[0]
    t = float(temperature)
    bias = np.asarray(bias, np.float64).reshape(B, 2)
    ba, bp = bias[:, 0], bias[:, 1]
    S = A @ P.T
    m, mc = npair_ref.masks(ids, B)
    eye = np.eye(B)
    X = S / t - bp[None, :]                         # row term: positive j's lq
    if mem is not None:
        mem = np.asarray(mem, np.float64)
        Sm = A @ mem.T
        cm = npair_memory_ref.mem_mask(ids, mem_id, B)
        Xm = Sm / t - np.asarray(mem_bias, np.float64)[None, :]
        lr = _lse(np.concatenate([X, Xm], 1), np.concatenate([m, cm], 1), 1)
    else:
        lr = _lse(X, m, 1)
    loss = L_row = np.mean(lr - (np.diag(S) / t - bp))
    W = np.where(m, np.exp(X - lr[:, None]), 0.0) - eye
    Wm = np.where(cm, np.exp(Xm - lr[:, None]), 0.0) if mem is not None else None
    lc = None
    if symmetric:
        Xc = S / t - ba[:, None]                    # column term: anchor i's lq
        lc = _lse(Xc, mc, 0)
        loss = 0.5 * (L_row + np.mean(lc - (np.diag(S) / t - ba)))
        W = 0.5 * (W + np.where(mc, np.exp(Xc - lc[None, :]), 0.0) - eye)
        if Wm is not None:
            Wm = 0.5 * Wm
    W = W / (B * t)
    dA = W @ P
    off = m & ~np.eye(B, dtype=bool)
    n, neg, den = off.sum(), (2 - 2 * S)[off].sum(), B * (B - 1)
    if Wm is not None:
        Wm = Wm / (B * t)
        dA = dA + Wm @ mem
        n, neg, den = n + cm.sum(), neg + (2 - 2 * Sm)[cm].sum(), den + B * mem.shape[0]
    stats = np.array([loss, np.mean(2 - 2 * np.diag(S)), neg / max(n, 1), n / den if den else 0.0])
    return {"loss": loss, "lse_row": lr, "lse_col": lc, "W": W, "W_mem": Wm, "dA": dA, "dP": W.T @ A, "S": S, "m": m,
            "mc": mc, "stats": stats}


def default_gap(n_videos, B):
    """g0 = max(1, n_videos / B): the expected gap between two draws of a video under uniform draws."""
    return max(1.0, n_videos / B)


def estimator_after(pos_ids_per_step, n_videos, B, alpha, g0=None, t0=0):
    """Host model of the streaming estimator after the steps t0, t0 + 1, ... whose positives' video ids are
    pos_ids_per_step[k]: (last int32 [n_videos], gap float32 [n_videos]).  Every positive video in [0, n_videos) is
    updated once per step from the state before that step: gap = (1 - a) gap + a (t - last) if last >= 0 (float32, each
    product and sum rounded on its own), last = t."""
    g0 = np.float32(default_gap(n_videos, B) if g0 is None else g0)
    last = np.full(n_videos, -1, np.int32)
    gap = np.full(n_videos, g0, np.float32)
    a = np.float32(alpha)
    oma = np.float32(np.float32(1.0) - a)
    for k, pos in enumerate(pos_ids_per_step):
        t = t0 + k
        pos = np.asarray(pos, np.int64)
        v = np.unique(pos[(pos >= 0) & (pos < n_videos)])
        L, G = last[v], gap[v]
        seen = L >= 0
        dt = (np.int64(t) - L.astype(np.int64)).astype(np.float32)
        upd = np.float32(oma * G) + np.float32(a * dt)
        gap[v] = np.where(seen, upd.astype(np.float32), G)
        last[v] = t
    return last, gap
