"""In-loop evaluation metric behind the reference's API (evaluate.py).

``Evaluation(features, cowatches)`` re-indexes the catalogue to the rows the
held-out co-watch pairs touch (evaluate.py:34-55); ``mean_dist(vectors,
cowatches)`` is the mean squared L2 distance between the embeddings of each
pair (evaluate.py:57-73) -- the model-selection signal of train.py:224-252.
The per-pair reduction runs as a HIP kernel; the re-indexing is host
bookkeeping on the (small) pair list.

Retrieval quality -- the reference's stubs ``Evaluation.knn`` / ``nDCG`` /
``MAP`` and ``KnnEvaluation(cowatches, I)`` (evaluate.py:92-107) -- comes from
EXACT ranks: ``Evaluation.ranks`` gives, for every directed co-watch pair
(anchor a, partner p), p's 0-based position in a's list of the whole catalogue
(a excluded, ties by id as ``knn.knn_search`` orders them; other partners of a
not removed).  The ranks are counted by the epilogue of the plane GEMM over the
query x catalogue product (csrc/knn.hip), with no score matrix and no cap on
k; ``metrics_from_ranks`` turns them into Recall@k, hit rate, nDCG@k, MAP@k,
MRR and the mean / median rank.  ``KnnEvaluation`` computes the same per-k
metrics from a kNN id matrix (``knn.calc_knn``'s ``I``).
"""
import numpy as np
import torch

from . import knn as _knn
from . import ops


def directed_queries(cowatches, symmetric=True):
    """(queries int64 [Q, 2] of distinct directed pairs (anchor, partner), sorted; the number of self-pairs a == p dropped).
    ``symmetric``: each pair gives (a, p) and (p, a) -- co-watch is undirected (parse_data.py:221-253)."""
    cw = np.asarray(cowatches, dtype=np.int64).reshape(-1, 2)
    if len(cw) and cw.min() < 0:
        raise IndexError("negative co-watch index")
    self_pair = cw[:, 0] == cw[:, 1]
    cw = cw[~self_pair]
    if symmetric:
        cw = np.concatenate([cw, cw[:, ::-1]])
    if len(cw) == 0:
        return np.zeros((0, 2), dtype=np.int64), int(self_pair.sum())
    base = max(int(cw.max()) + 1, 1)
    key = np.unique(cw[:, 0] * base + cw[:, 1])              # (one key per pair: far faster than unique over rows)
    return np.stack([key // base, key % base], axis=1), int(self_pair.sum())


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def metrics_from_ranks(queries, pos, ks=(1, 10, 50, 100)):
    """Retrieval metrics of directed queries (anchor, partner) [Q, 2] whose partners sit at 0-based positions ``pos`` [Q] of
    their anchors' lists.  Per anchor a with m = |R(a)| partners, averaged over anchors:
    recall@k = #{pos < k} / m; hit_rate@k = [any pos < k]; ndcg@k = sum_{pos < k} 1 / log2(pos + 2) over the ideal
    sum_{i < min(m, k)} 1 / log2(i + 2); map@k = sum_{pos_r < k} #{r': pos_r' <= pos_r} / (pos_r + 1) / min(m, k);
    mrr = 1 / (1 + min pos).  Over the directed pairs: mean_rank = mean(pos + 1), median_rank = median(pos + 1)."""
    q = _host(queries).astype(np.int64).reshape(-1, 2)
    ps = _host(pos).astype(np.int64).reshape(-1)
    if len(q) != len(ps):
        raise ValueError("queries and pos differ in length")
    if len(ps) == 0:
        raise ValueError("no queries")
    if ps.min() < 0:
        raise ValueError("negative rank")
    order = np.lexsort((ps, q[:, 0]))                        # by anchor, then position
    a, ps = q[order, 0], ps[order]
    starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    n_anchors = len(starts)
    m = np.diff(np.r_[starts, len(a)])
    grp = np.repeat(np.arange(n_anchors), m)
    key = grp * (int(ps.max()) + 1) + ps                     # ascending
    n_le = np.searchsorted(key, key, side="right") - starts[grp]    # #{r' of the same anchor: pos_r' <= pos_r}
    out = {}
    for k in ks:
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1")
        hit = ps < k
        nh = np.bincount(grp, weights=hit.astype(np.float64), minlength=n_anchors)
        ideal = np.cumsum(1.0 / np.log2(np.arange(min(k, int(m.max()))) + 2.0))[np.minimum(m, k) - 1]
        dcg = np.bincount(grp, weights=np.where(hit, 1.0 / np.log2(ps + 2.0), 0.0), minlength=n_anchors)
        ap = np.bincount(grp, weights=np.where(hit, n_le / (ps + 1.0), 0.0), minlength=n_anchors)
        out["recall@%d" % k] = float(np.mean(nh / m))
        out["hit_rate@%d" % k] = float(np.mean(nh > 0))
        out["ndcg@%d" % k] = float(np.mean(dcg / ideal))
        out["map@%d" % k] = float(np.mean(ap / np.minimum(m, k)))
    out["mrr"] = float(np.mean(1.0 / (1.0 + ps[starts])))
    out["mean_rank"] = float(np.mean(ps + 1.0))
    out["median_rank"] = float(np.median(ps + 1.0))
    out["n_queries"] = int(len(ps))
    out["n_anchors"] = int(n_anchors)
    return out


class Evaluation():
    def __init__(self, features, cowatches, device="cuda:0"):
        """features: ndarray [N,F] (or None); cowatches: list/array of [a,p] row ids."""
        self.device = torch.device(device)
        try:
            self.features, self.cowatches = self._rencode(features, cowatches)
        except Exception:                      # the reference logs and sets None (evaluate.py:30-32)
            self.features, self.cowatches = None, None

    def _rencode(self, features, cowatches):
        cw = np.asarray(cowatches, dtype=np.int64).reshape(-1, 2)
        sorted_indexes = np.unique(cw)          # == np.sort(get_unique_watched_guids(cowatches))
        eval_features = features[sorted_indexes]
        eval_cowatches = np.searchsorted(sorted_indexes, cw)   # old row id -> position in the subset
        return eval_features, eval_cowatches.tolist()

    def _pair_stats(self, vectors, cowatches):
        v = vectors if torch.is_tensor(vectors) else torch.as_tensor(np.asarray(vectors, np.float32))
        v = v.to(self.device, torch.float32).contiguous()
        D = v.shape[1]
        if D % 4:                                # kernels take 16-B rows: pad with zero columns
            v = torch.nn.functional.pad(v, (0, 4 - D % 4))
        pairs = torch.as_tensor(np.asarray(cowatches, np.int32).reshape(-1, 2)).to(self.device)
        if int(pairs.max()) >= v.shape[0] or int(pairs.min()) < 0:
            raise IndexError("co-watch index outside the embedding table")
        P = pairs.shape[0]
        sq, dot = torch.empty(P, device=self.device), torch.empty(P, device=self.device)
        means = torch.empty(4, device=self.device)
        ops.pair_dist(v, pairs, v.shape[1], sq, dot, means)
        return means

    def mean_dist(self, vectors, cowatches):
        """Mean over pairs of sum((a-b)^2) (evaluate.py:57-73)."""
        return float(self._pair_stats(vectors, cowatches)[1].item())

    def mean_cos_dist(self, vectors, cowatches):
        """Mean over pairs of sum(a*b) (evaluate.py:75-90)."""
        return float(self._pair_stats(vectors, cowatches)[2].item())

    # ---- retrieval: exact ranks on the plane kernels (the reference's knn / nDCG / MAP stubs, evaluate.py:92-100) ----
    def _ranks(self, vectors, cowatches, symmetric=True, precision="f32x3", l2_norm=False, q_chunk=65536,
               c_chunk=1048576):
        if precision not in ("f32x3", "f16x2"):
            raise ValueError("precision must be 'f32x3' or 'f16x2'")
        q_np, n_self = directed_queries(cowatches, symmetric)
        n = vectors.shape[0]
        if len(q_np) == 0:
            raise ValueError("no co-watch pair left after dropping self-pairs")
        if q_np.min() < 0 or q_np.max() >= n:
            raise IndexError("co-watch index outside the embedding table")
        dev = self.device
        h2 = precision == "f16x2"
        B = _knn._device_matrix(vectors, dev, 256, 128 if h2 else 64)    # rows to 256, columns to the K-tile walk
        Dp = B.shape[1]
        if l2_norm:                                          # as calc_knn (faiss_knn.py:99-104)
            ops.l2norm_fwd(B[:n], Dp, B)
        b_sq = torch.zeros(B.shape[0], dtype=torch.float32, device=dev)
        ops.row_sqnorm(B[:n], Dp, b_sq)
        if h2:
            B3, scale = _knn._planes_h2(B, Dp)
            osc = 1.0 / (scale * scale)
        else:
            B3 = _knn._planes(B, Dp)
        # a chunk's operands inside the 2 GiB window of a buffer descriptor
        lim = (2 ** 31) // (B3.shape[1] * 2) - 512
        q_chunk = max(256, min(_knn._round_up(q_chunk, 256), lim // 256 * 256))
        c_chunk = max(256, min(_knn._round_up(c_chunk, 256), lim // 256 * 256))
        queries = torch.as_tensor(q_np, device=dev)
        q32 = queries.to(torch.int32)
        nq = queries.shape[0]
        count = torch.zeros(nq, dtype=torch.int32, device=dev)
        tau = torch.empty(nq, dtype=torch.float32, device=dev)
        n_pad = B3.shape[0]
        for qs in range(0, nq, q_chunk):
            mq = min(q_chunk, nq - qs)
            a64, p64 = queries[qs:qs + mq, 0], queries[qs:qs + mq, 1]
            a32, p32 = q32[qs:qs + mq, 0].contiguous(), q32[qs:qs + mq, 1].contiguous()
            QA = B3.index_select(0, a64)                     # the anchors' planes
            q_sq = b_sq.index_select(0, a64)
            mp = _knn._round_up(mq, 256)
            PP = torch.zeros((mp, B3.shape[1]), dtype=B3.dtype, device=dev)
            PP[:mq] = B3.index_select(0, p64)                # the partners' planes, one per query
            p_sq = torch.zeros(mp, dtype=torch.float32, device=dev)
            p_sq[:mq] = b_sq.index_select(0, p64)
            t, cnt = tau[qs:qs + mq], count[qs:qs + mq]
            if h2:
                ops.rank_tau_h2(QA, Dp, PP, Dp, mq, Dp, osc, q_sq, p_sq, t)
            else:
                ops.rank_tau_x3(QA, Dp, PP, Dp, mq, Dp, q_sq, p_sq, t)
            for c0 in range(0, n_pad, c_chunk):
                nc = min(c_chunk, n_pad - c0)
                if h2:
                    ops.rank_count_h2(QA, Dp, B3[c0:c0 + nc], Dp, mq, nc, Dp, osc, q_sq, b_sq[c0:c0 + nc], t, p32, a32, c0, n, cnt)
                else:
                    ops.rank_count_x3(QA, Dp, B3[c0:c0 + nc], Dp, mq, nc, Dp, q_sq, b_sq[c0:c0 + nc], t, p32, a32, c0, n, cnt)
        return queries, count.to(torch.int64), n_self

    def ranks(self, vectors, cowatches, symmetric=True, precision="f32x3", l2_norm=False, q_chunk=65536, c_chunk=1048576):
        """Device tensors (queries int64 [Q, 2], pos int64 [Q]): every distinct directed co-watch pair (anchor a, partner p)
        (``symmetric``: both directions; self-pairs dropped) and p's 0-based position in a's list of the whole catalogue
        ``vectors`` [N, D] by squared L2 -- #{j != a, p: d(a,j) < d(a,p), or d(a,j) == d(a,p) and j < p}.  Distances on the
        vectors as given (``l2_norm``: normalised first, as calc_knn does).  ``precision``: "f32x3" (three bf16 planes per
        fp32 value, six products) or "f16x2" (two fp16 planes, three products).  ``q_chunk`` queries x ``c_chunk``
        catalogue rows per launch (the counts are integers: the same for any chunking).  A catalogue row with a non-finite
        coordinate is never counted ahead of a partner."""
        queries, pos, _ = self._ranks(vectors, cowatches, symmetric, precision, l2_norm, q_chunk, c_chunk)
        return queries, pos

    def retrieval_metrics(self, vectors, cowatches, ks=(1, 10, 50, 100), symmetric=True, precision="f32x3",
                          l2_norm=False):
        """metrics_from_ranks of ``ranks``: recall@k, hit_rate@k, ndcg@k, map@k per k, mrr, mean_rank, median_rank,
        n_queries, n_anchors and n_self_pairs_dropped."""
        queries, pos, n_self = self._ranks(vectors, cowatches, symmetric, precision, l2_norm)
        out = metrics_from_ranks(queries, pos, ks)
        out["n_self_pairs_dropped"] = n_self
        return out

    def knn(self, vectors, cowatches, k=10, **kw):
        """Recall@k of the co-watched items (the reference's stub, evaluate.py:92-93)."""
        return self.retrieval_metrics(vectors, cowatches, ks=(k,), **kw)["recall@%d" % k]

    def nDCG(self, vectors, cowatches, k=10, **kw):
        """nDCG@k (evaluate.py:95-96)."""
        return self.retrieval_metrics(vectors, cowatches, ks=(k,), **kw)["ndcg@%d" % k]

    def MAP(self, vectors, cowatches, k=10, **kw):
        """MAP@k (evaluate.py:98-99)."""
        return self.retrieval_metrics(vectors, cowatches, ks=(k,), **kw)["map@%d" % k]


class KnnEvaluation():
    """The same per-k metrics from a kNN id matrix (evaluate.py:101-107): ``I`` [N, L] = the neighbour ids of every
    catalogue row, nearest first (``knn.calc_knn``'s I; -1 = none).  The query's own id is dropped wherever it appears in
    its row, and the row keeps its first L - 1 remaining entries: metrics are defined for k <= L - 1."""

    def __init__(self, cowatches, I, symmetric=True):
        self.cowatches = cowatches
        self.I = _host(I).astype(np.int64)
        if self.I.ndim != 2 or self.I.shape[1] < 2:
            raise ValueError("I must be [N, L] with L >= 2")
        self.queries, self.n_self_pairs_dropped = directed_queries(cowatches, symmetric)
        if len(self.queries) and (self.queries.min() < 0 or self.queries.max() >= self.I.shape[0]):
            raise IndexError("co-watch index outside the kNN matrix")

    @property
    def max_k(self):
        return self.I.shape[1] - 1

    def ranks(self):
        """pos [Q] of each query's partner in its anchor's list (self dropped); max_k where the list does not hold it."""
        a, p = self.queries[:, 0], self.queries[:, 1]
        rows = self.I[a]
        keep = rows != a[:, None]
        kept = np.cumsum(keep, axis=1)
        match = keep & (kept <= self.max_k) & (rows == p[:, None])
        found = match.any(axis=1)
        col = match.argmax(axis=1)
        return np.where(found, kept[np.arange(len(a)), col] - 1, self.max_k).astype(np.int64)

    def metrics(self, ks=(1, 10, 50)):
        """recall@k, hit_rate@k, ndcg@k, map@k per k, n_queries, n_anchors, n_self_pairs_dropped."""
        ks = [int(k) for k in ks]
        if any(k > self.max_k for k in ks):
            raise ValueError("k must be <= %d (I has %d columns, one of them the query)" % (self.max_k, self.I.shape[1]))
        full = metrics_from_ranks(self.queries, self.ranks(), ks)
        out = {name: v for name, v in full.items() if "@" in name}
        out.update(n_queries=full["n_queries"], n_anchors=full["n_anchors"], n_self_pairs_dropped=self.n_self_pairs_dropped)
        return out

    def knn(self, k=10):
        return self.metrics((k,))["recall@%d" % k]

    def nDCG(self, k=10):
        return self.metrics((k,))["ndcg@%d" % k]

    def MAP(self, k=10):
        return self.metrics((k,))["map@%d" % k]
