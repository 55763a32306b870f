"""fp64 reference of the multi-class N-pair loss (ops.npair_loss, include/cdml.h) for the tests."""
import numpy as np


def masks(ids, B):
    """(m, mc): m[i, j] = column j counts for anchor i's row term, mc[i, j] = row i counts for positive j's column term.
    ids: int [2B] (2i = id(a_i), 2i+1 = id(p_i)) or None."""
    eye = np.eye(B, dtype=bool)
    if ids is None:
        return np.ones((B, B), bool), np.ones((B, B), bool)
    ids = np.asarray(ids).reshape(B, 2)
    a, p = ids[:, 0], ids[:, 1]
    m = (p[None, :] != a[:, None]) & (p[None, :] != p[:, None]) | eye
    mc = (a[:, None] != a[None, :]) & (a[:, None] != p[None, :]) | eye
    return m, mc


def _lse(x, mask, axis):
    x = np.where(mask, x, -np.inf)
    mx = x.max(axis=axis, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(axis=axis, keepdims=True))).squeeze(axis)


def npair(A, P, ids=None, temperature=0.1, symmetric=True):
    """A, P: [B, D] rows (anchors, positives).  Returns loss, lse_row, lse_col (None unless symmetric), W, dA, dP, stats[4]."""
    A, P = np.asarray(A, np.float64), np.asarray(P, np.float64)
    B = A.shape[0]
    t = float(temperature)
    S = A @ P.T
    m, mc = masks(ids, B)
    eye = np.eye(B)
    lr = _lse(S / t, m, 1)
    d = np.diag(S) / t
    L_row = np.mean(lr - d)
    W = np.where(m, np.exp(S / t - lr[:, None]), 0.0) - eye
    lc = None
    loss = L_row
    if symmetric:
        lc = _lse(S / t, mc, 0)
        loss = 0.5 * (L_row + np.mean(lc - d))
        W = 0.5 * (W + np.where(mc, np.exp(S / t - lc[None, :]), 0.0) - eye)
    W = W / (B * t)
    off = m & ~np.eye(B, dtype=bool)
    n = off.sum()
    stats = np.array([loss, np.mean(2 - 2 * np.diag(S)), (2 - 2 * S)[off].sum() / max(n, 1),
                      n / (B * (B - 1)) if B > 1 else 0.0])
    return {"loss": loss, "lse_row": lr, "lse_col": lc, "W": W, "dA": W @ P, "dP": W.T @ A, "S": S, "m": m, "mc": mc,
            "stats": stats}


def interleave(dA, dP):
    """[B, D] x 2 -> the embedded rows' gradient [2B, D] (row 2i = anchor i, 2i+1 = positive i)."""
    B, D = dA.shape
    out = np.empty((2 * B, D), dtype=np.result_type(dA, dP))
    out[0::2], out[1::2] = dA, dP
    return out
