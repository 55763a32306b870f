"""fp64 reference of the N-pair loss with mixed negative sampling (ops.npair_mixed_loss, include/cdml_npair_mixed.h) for
the tests: the column set [P | N | Mem] -- in-batch positives, the batch's uniform catalogue negatives, the memory."""
import numpy as np

import npair_logq_ref  # noqa: F401  (the estimator's host model, re-exported for the tests)
import npair_memory_ref
import npair_ref


def split_ids(ids3, B):
    """ids3 int [3B] (a, p, n per triplet) -> (ids2 [2B] laid out like npair_ref's, n [B]); None -> (None, None)."""
    if ids3 is None:
        return None, None
    ids3 = np.asarray(ids3).reshape(B, 3)
    return ids3[:, :2].reshape(-1).copy(), ids3[:, 2].copy()


def neg_mask(ids3, B):
    """cn[i, j]: uniform negative j counts for anchor i (id(n_j) is neither id(a_i) nor id(p_i); ids None: all)."""
    if ids3 is None:
        return np.ones((B, B), bool)
    ids3 = np.asarray(ids3).reshape(B, 3)
    n = ids3[:, 2]
    return (n[None, :] != ids3[:, 0:1]) & (n[None, :] != ids3[:, 1:2])


def npair_mixed(A, P, N, ids3=None, temperature=0.1, symmetric=True, mem=None, mem_id=None, bias=None, lq_u=0.0,
                mem_bias=None):
    """A, P, N: [B, D] rows; ids3 [3B] or None; mem [M, D] / mem_id [M] (-1 = empty) optional; bias [2B] (lq(a_i),
    lq(p_i) per pair), lq_u (one scalar for the uniform block) and mem_bias [M]: the logQ correction (None: 0).
    Returns loss, lse_row, lse_col, W (in-batch), W_n, W_mem, dA, dP, dN, stats[4] and the masks m, mc, cn, cm."""
    A, P, N = (np.asarray(x, np.float64) for x in (A, P, N))
    B = A.shape[0]
    t = float(temperature)
    ids2, _ = split_ids(ids3, B)
    m, mc = npair_ref.masks(ids2, B)
    cn = neg_mask(ids3, B)
    b = np.zeros((B, 2)) if bias is None else np.asarray(bias, np.float64).reshape(B, 2)
    ba, bp = b[:, 0], b[:, 1]
    lq_u = float(lq_u) if bias is not None else 0.0
    S, U = A @ P.T, A @ N.T
    X, Xu = S / t - bp[None, :], U / t - lq_u
    blocks, masks = [X, Xu], [m, cn]
    M, cm, Sm, Xm = 0, None, None, None
    if mem is not None:
        mem = np.asarray(mem, np.float64)
        M = mem.shape[0]
        Sm = A @ mem.T
        cm = npair_memory_ref.mem_mask(ids2, mem_id, B)
        Xm = Sm / t - (0.0 if (mem_bias is None or bias is None) else np.asarray(mem_bias, np.float64)[None, :])
        blocks.append(Xm)
        masks.append(cm)
    lr = npair_ref._lse(np.concatenate(blocks, 1), np.concatenate(masks, 1), 1)
    eye = np.eye(B)
    d = np.diag(S) / t
    loss = L_row = np.mean(lr - (d - bp))
    W = np.where(m, np.exp(X - lr[:, None]), 0.0) - eye
    Wn = np.where(cn, np.exp(Xu - lr[:, None]), 0.0)
    Wm = np.where(cm, np.exp(Xm - lr[:, None]), 0.0) if mem is not None else None
    lc = None
    if symmetric:                                   # the column term: over the in-batch block only, unchanged
        Xc = S / t - ba[:, None]
        lc = npair_ref._lse(Xc, mc, 0)
        loss = 0.5 * (L_row + np.mean(lc - (d - ba)))
        W = 0.5 * (W + np.where(mc, np.exp(Xc - lc[None, :]), 0.0) - eye)
        Wn = 0.5 * Wn
        if Wm is not None:
            Wm = 0.5 * Wm
    W, Wn = W / (B * t), Wn / (B * t)
    dA = W @ P + Wn @ N
    off = m & ~np.eye(B, dtype=bool)
    n = off.sum() + cn.sum()
    neg = (2 - 2 * S)[off].sum() + (2 - 2 * U)[cn].sum()
    if Wm is not None:
        Wm = Wm / (B * t)
        dA = dA + Wm @ mem
        n, neg = n + cm.sum(), neg + (2 - 2 * Sm)[cm].sum()
    den = B * (B - 1) + B * B + B * M
    stats = np.array([loss, np.mean(2 - 2 * np.diag(S)), neg / max(n, 1), n / den])
    return {"loss": loss, "lse_row": lr, "lse_col": lc, "W": W, "W_n": Wn, "W_mem": Wm, "dA": dA, "dP": W.T @ A,
            "dN": Wn.T @ A, "m": m, "mc": mc, "cn": cn, "cm": cm, "stats": stats}


def interleave3(dA, dP, dN):
    """[B, D] x 3 -> the embedded rows' gradient [3B, D] (row 3i = anchor, 3i+1 = positive, 3i+2 = uniform negative)."""
    B, D = dA.shape
    out = np.empty((3 * B, D), dtype=np.float64)
    out[0::3], out[1::3], out[2::3] = dA, dP, dN
    return out


def default_uniform_logq(n_videos, B, stream=True, init_gap=None):
    """lq_u when none is given: -log(g0) with the streaming estimator (g0 = init_gap or max(1, n_videos / B): an unseen
    video's lq), -log(n_videos) with a fixed table of per-draw shares."""
    if stream:
        return -np.log(npair_logq_ref.default_gap(n_videos, B) if init_gap is None else init_gap)
    return -np.log(n_videos)
