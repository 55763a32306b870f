"""Hard-negative candidate lists, mined with the exact kNN (ANCE, Xiong et al. 2020; build-defined).

``mine_lists`` turns the catalogue's current embeddings into one list of candidate negatives per video -- its nearest
neighbours, less itself, the ``skip_top`` nearest (the usual guard against false negatives) and its known co-watch
partners -- in the layout the listed sampler reads (include/cdml_hardneg.h: int32 [n, L], left-packed, -1 = empty).
``TrainStep(negative_lists=...)`` draws from them; ``TrainStep.refresh_negative_lists`` re-mines them as the model moves.
The search is ``knn.knn_search`` (HIP); the filtering below is a few torch calls over [n, k] ids, off the hot path.
"""
import numpy as np
import torch

from . import knn


def list_width(k):
    """L of the lists ``mine_lists(.., k)`` returns: k rounded up to a multiple of 4."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1, got %d" % k)
    return (k + 3) // 4 * 4


def empty_lists(n_rows, k, device="cpu"):
    """int32 [n_rows, list_width(k)] of -1: lists from which every draw falls through to the uniform sampler."""
    return torch.full((int(n_rows), list_width(k)), -1, dtype=torch.int32, device=device)


def pair_keys(pairs, n):
    """Sorted int64 keys a * n + b of every known partnership in BOTH directions (pairs: int [P, 2] tensor)."""
    p = pairs.to(torch.int64).reshape(-1, 2)
    keys = torch.cat([p[:, 0] * n + p[:, 1], p[:, 1] * n + p[:, 0]])
    return torch.sort(keys).values


def filter_lists(I, k, skip_top=0, pairs=None):
    """The list filter on neighbour ids ``I`` (int64 [n, k + skip_top + 1], nearest first, -1 = none; row i's own id
    usually first): drop the row itself (if it is not among them: the farthest instead), then the ``skip_top`` nearest,
    then every known partner of the row in either direction; left-pack and pad with -1 to [n, list_width(k)] int32."""
    n, w = I.shape
    k, skip_top = int(k), int(skip_top)
    if skip_top < 0 or w != k + skip_top + 1:
        raise ValueError("filter_lists needs k + skip_top + 1 = %d neighbour columns, got %d" % (k + skip_top + 1, w))
    dev = I.device
    I = I.to(torch.int64)
    rows = torch.arange(n, device=dev).unsqueeze(1)
    is_self = I == rows
    first = is_self & (torch.cumsum(is_self.to(torch.int32), 1) == 1)       # (ids are unique in a row; defensive)
    none = ~is_self.any(1, keepdim=True)
    cols = torch.arange(w, device=dev).unsqueeze(0)
    drop = first | (none & (cols == w - 1))                                 # exactly one column per row goes
    keep_cols = torch.argsort(drop.to(torch.int8), dim=1, stable=True)[:, :w - 1]
    J = torch.gather(I, 1, keep_cols)[:, skip_top:]                         # [n, k], still nearest first
    ok = J >= 0
    if pairs is not None and pairs.numel():
        keys = pair_keys(pairs.to(dev), n)
        q = rows * n + J.clamp(min=0)
        pos = torch.searchsorted(keys, q.reshape(-1)).clamp(max=keys.numel() - 1).reshape(q.shape)
        ok &= keys[pos] != q
    order = torch.argsort((~ok).to(torch.int8), dim=1, stable=True)         # kept entries first, in their order
    J = torch.where(ok, J, torch.full_like(J, -1))
    out = torch.full((n, list_width(k)), -1, dtype=torch.int32, device=dev)
    out[:, :k] = torch.gather(J, 1, order).to(torch.int32)
    return out


def mine_lists(embeddings, k, skip_top=0, pairs=None, device="cuda:0", precision="f32x3", nlist=0, nprobe=0, ivf_iters=10,
               ivf_seed=0, storage="f32", refine=0, scan="buffer"):
    """Candidate negatives of every row: int32 [n, L] device tensor, L = k rounded up to a multiple of 4.

    A self-kNN over ``embeddings`` ([n, D] ndarray or tensor; l2-normalised first, as ``knn.calc_knn`` does) with
    k + skip_top + 1 neighbours (``knn.knn_search``: exact, ties by id), then ``filter_lists``: the row itself, the
    ``skip_top`` nearest and -- with ``pairs`` (int [P, 2]) -- every known co-watch partner of the row are dropped; what
    remains is left-packed, nearest first, and padded with -1.
    ``nlist`` > 0: the neighbours come from an IVF index over the embeddings instead (``knn.IVFIndex.build(e, nlist,
    iters=ivf_iters, seed=ivf_seed)`` and its ``search(e, k + skip_top + 1, nprobe)``: approximate -- a neighbour outside a
    row's ``nprobe`` nearest lists is missed -- and sub-linear in the catalogue); the filter is the same.
    ``storage`` ("f32" | "f16") and ``refine`` go to that index (``knn.IVFIndex``: fp16 lists at half the bytes, scanned on
    the fp16 MFMA; ``refine=r`` re-ranks the r best candidates of a row against the fp32 embeddings given here); ``scan``
    ("buffer" | "filter") is that index's search mode (``IVFIndex.search``: the same lists either way, "filter" without a score
    buffer behind the seed probes)."""
    k, skip_top, nlist, nprobe = int(k), int(skip_top), int(nlist), int(nprobe)
    if nlist < 0 or (nlist == 0 and nprobe != 0):
        raise ValueError("mine_lists takes nlist >= 0, and nprobe only with nlist > 0 (got nlist = %d, nprobe = %d)" % (nlist, nprobe))
    if nlist == 0 and (storage != "f32" or int(refine) != 0):
        raise ValueError("mine_lists takes storage and refine only with nlist > 0 (got storage = %r, refine = %d)" % (storage, int(refine)))
    if scan not in knn.IVFIndex.SCANS or (nlist == 0 and scan != "buffer"):
        raise ValueError("mine_lists takes scan in %s, and \"filter\" only with nlist > 0 (got scan = %r)" % (knn.IVFIndex.SCANS, scan))
    if k < 1 or skip_top < 0:
        raise ValueError("mine_lists needs k >= 1 and skip_top >= 0, got %d and %d" % (k, skip_top))
    if list_width(k) > 1024:
        raise ValueError("the sampler reads lists of at most 1024 columns (k = %d)" % k)
    dev = torch.device(device)
    e = embeddings if torch.is_tensor(embeddings) else torch.as_tensor(np.asarray(embeddings, dtype=np.float32))
    e = e.to(device=dev, dtype=torch.float32)
    if nlist > 0:
        index = knn.IVFIndex.build(e, nlist, iters=ivf_iters, seed=ivf_seed, device=dev, precision=precision, storage=storage)
        _, I = index.search(e, k + skip_top + 1, nprobe, refine=int(refine), base=index.prepare(e) if int(refine) else None,
                            scan=scan)
    else:
        _, I = knn.knn_search(e, e, k + skip_top + 1, device=dev, precision=precision)
    if pairs is not None and not torch.is_tensor(pairs):
        pairs = torch.as_tensor(np.asarray(pairs))
    return filter_lists(I, k, skip_top, pairs)
