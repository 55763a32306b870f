"""fp64 reference of the N-pair loss with a cross-batch memory (ops.npair_loss(memory=...), include/cdml.h) for the tests."""
import numpy as np

import npair_ref


def mem_mask(ids, mem_id, B):
    """cm[i, k]: memory slot k counts for anchor i (filled, and neither id(a_i) nor id(p_i); ids None: filled)."""
    mem_id = np.asarray(mem_id).reshape(-1)
    filled = np.broadcast_to(mem_id[None, :] >= 0, (B, mem_id.size))
    if ids is None:
        return filled.copy()
    ids = np.asarray(ids).reshape(B, 2)
    return filled & (mem_id[None, :] != ids[:, 0:1]) & (mem_id[None, :] != ids[:, 1:2])


def _lse(x, mask):
    x = np.where(mask, x, -np.inf)
    mx = x.max(axis=1, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True)))[:, 0]


def npair_memory(A, P, ids, mem, mem_id, temperature=0.1, symmetric=True):
    """A, P: [B, D] rows; mem [M, D] ring rows, mem_id [M] (-1 = empty).  Returns loss, lse_row, lse_col, W [B, B],
    W_mem [B, M], dA, dP, stats[4], masks."""
    A, P, mem = (np.asarray(x, np.float64) for x in (A, P, mem))
    B, M = A.shape[0], mem.shape[0]
    t = float(temperature)
    S, Sm = A @ P.T, A @ mem.T
    m, mc = npair_ref.masks(ids, B)
    cm = mem_mask(ids, mem_id, B)
    eye = np.eye(B)
    lr = _lse(np.concatenate([S / t, Sm / t], 1), np.concatenate([m, cm], 1))
    d = np.diag(S) / t
    loss = L_row = np.mean(lr - d)
    W = np.where(m, np.exp(S / t - lr[:, None]), 0.0) - eye
    Wm = np.where(cm, np.exp(Sm / t - lr[:, None]), 0.0)
    lc = None
    if symmetric:                                   # the column term: in-batch only, unchanged
        lc = npair_ref._lse(S / t, mc, 0)
        loss = 0.5 * (L_row + np.mean(lc - d))
        W = 0.5 * (W + np.where(mc, np.exp(S / t - lc[None, :]), 0.0) - eye)
        Wm = 0.5 * Wm
    W, Wm = W / (B * t), Wm / (B * t)
    off = m & ~np.eye(B, dtype=bool)
    n = off.sum() + cm.sum()
    neg = (2 - 2 * S)[off].sum() + (2 - 2 * Sm)[cm].sum()
    den = B * (B - 1) + B * M
    stats = np.array([loss, np.mean(2 - 2 * np.diag(S)), neg / max(n, 1), n / den if den else 0.0])
    return {"loss": loss, "lse_row": lr, "lse_col": lc, "W": W, "W_mem": Wm, "dA": W @ P + Wm @ mem, "dP": W.T @ A,
            "m": m, "mc": mc, "cm": cm, "stats": stats}


def push_slot(t, start, M, B):
    """The first ring slot step t writes, or None (before ``start``)."""
    if t < start:
        return None
    return ((t - start) % (M // B)) * B


def ring_after(steps, start, M, positives, pos_ids):
    """Host model of the ring after steps 0 .. len(positives) - 1 (positives[t] [B, D], pos_ids[t] [B]): (rows, ids)."""
    B, D = positives[0].shape
    rows, ids = np.zeros((M, D)), np.full(M, -1, np.int64)
    for t in range(steps):
        s = push_slot(t, start, M, B)
        if s is not None:
            rows[s:s + B], ids[s:s + B] = positives[t], pos_ids[t]
    return rows, ids
