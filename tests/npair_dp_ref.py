"""fp64 model of the data-parallel N-pair loss's three phases (ops.npair_dp_loss, include/cdml_npair_dp.h) for the tests:
per-rank row blocks and column partials, the rank-order fold, the partial positive gradients summed at their owners."""
import numpy as np

import npair_ref


def fold(colpart_all):
    """colpart_all [world, G, 2] (max, sum-exp) -> lse_col [G]: ranks folded in the order 0 .. world - 1; (-inf, 0) is the
    empty partial."""
    colpart_all = np.asarray(colpart_all, np.float64)
    world, G, _ = colpart_all.shape
    m = np.full(G, -np.inf)
    s = np.zeros(G)
    for r in range(world):
        m2, s2 = colpart_all[r, :, 0], colpart_all[r, :, 1]
        mx = np.maximum(m, m2)
        live = mx > -np.inf
        with np.errstate(invalid="ignore"):
            s = np.where(live, s * np.exp(np.where(live, m - mx, 0.0)) + s2 * np.exp(np.where(live, m2 - mx, 0.0)), s)
        m = mx
    with np.errstate(divide="ignore"):
        return m + np.log(s)


def npair_dp(A, P, ids, world, temperature=0.1, symmetric=True):
    """A, P [G, D], ids [2G] of the GLOBAL batch, split over ``world`` ranks of B = G / world pairs.  Returns per-rank lists:
    lse_row [B], colpart [G, 2], W [B, G] (scaled 1 / (B t): the local mean), dA [B, D], dP [B, D] (the owner's rank-order
    sum), loss (the rank's share), stats [4]; and lse_col [G] (None unless symmetric)."""
    A, P = np.asarray(A, np.float64), np.asarray(P, np.float64)
    G = A.shape[0]
    B = G // world
    t = float(temperature)
    m, mc = npair_ref.masks(ids, G)
    out = {k: [] for k in ("lse_row", "colpart", "W", "dA", "dP", "loss", "stats")}
    S, rows = [], []
    for r in range(world):
        sl = slice(r * B, (r + 1) * B)
        Sr = A[sl] @ P.T
        S.append(Sr)
        rows.append(sl)
        out["lse_row"].append(npair_ref._lse(Sr / t, m[sl], 1))
        x = np.where(mc[sl], Sr / t, -np.inf)
        mx = x.max(axis=0)
        with np.errstate(invalid="ignore"):
            sm = np.where(mx > -np.inf, np.exp(x - np.where(mx > -np.inf, mx, 0.0)[None, :]).sum(axis=0), 0.0)
        out["colpart"].append(np.stack([mx, sm], 1))
    lse_col = fold(np.stack(out["colpart"])) if symmetric else None
    part = []
    for r in range(world):
        sl, Sr = rows[r], S[r]
        eye = np.zeros((B, G))
        eye[np.arange(B), r * B + np.arange(B)] = 1.0
        d = Sr[np.arange(B), r * B + np.arange(B)]
        W = np.where(m[sl], np.exp(Sr / t - out["lse_row"][r][:, None]), 0.0) - eye
        loss = np.mean(out["lse_row"][r] - d / t)
        if symmetric:
            W = 0.5 * (W + np.where(mc[sl], np.exp(Sr / t - lse_col[None, :]), 0.0) - eye)
            loss = 0.5 * (loss + np.mean(lse_col[sl] - d / t))
        W = W / (B * t)
        off = m[sl] & (eye == 0)
        n = off.sum()
        out["W"].append(W)
        out["dA"].append(W @ P)
        part.append(W.T @ A[sl])
        out["loss"].append(loss)
        out["stats"].append(np.array([loss, np.mean(2 - 2 * d), (2 - 2 * Sr)[off].sum() / max(n, 1), n / (B * (G - 1))]))
    for r in range(world):
        acc = part[0][rows[r]].copy()
        for s in range(1, world):
            acc = acc + part[s][rows[r]]
        out["dP"].append(acc)
    out["lse_col"] = lse_col
    return out
