"""Exact retrieval ranks on the MI355X (evaluate.py Evaluation.ranks / retrieval_metrics, csrc/knn.hip: the plane GEMM
with the rank count as its epilogue) against brute-force fp64 ranks, the tie / exclusion rule, chunking and determinism,
the kNN export as an independent second path, the reference catalogue size, and the Trainer's opt-in summaries."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5    # squared-L2 distance of unit vectors, plane kernels vs fp64 (as tests/test_gpu_knn.py)
PLANE_FORMS = ["f32x3", "f16x2"]


def _unit(n, D, seed):
    x = np.random.RandomState(seed).randn(n, D)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _rank_bounds(v, queries, tol=TOL):
    """fp64 brute force: for each query (a, p), lo = #{j != a, p: d < d_p - tol}, hi = #{j != a, p: d < d_p + tol}."""
    b = v.astype(np.float64)
    bsq = (b * b).sum(1)
    lo = np.empty(len(queries), np.int64)
    hi = np.empty(len(queries), np.int64)
    for s in range(0, len(queries), 1024):
        q = queries[s:s + 1024]
        a, p = q[:, 0], q[:, 1]
        d = np.maximum(bsq[a, None] + bsq[None, :] - 2.0 * (b[a] @ b.T), 0.0)
        r = np.arange(len(q))
        dp = d[r, p][:, None]
        d[r, a] = np.inf
        d[r, p] = np.inf
        lo[s:s + 1024] = (d < dp - tol).sum(1)
        hi[s:s + 1024] = (d < dp + tol).sum(1)
    return lo, hi


def _random_pairs(n, P, seed):
    rng = np.random.RandomState(seed)
    cw = rng.randint(0, n, size=(P, 2))
    cw[:5, 1] = cw[:5, 0]                                    # a few self-pairs: dropped and counted
    return cw


@pytest.mark.parametrize("precision", PLANE_FORMS)
@pytest.mark.parametrize("D", [64, 100])
def test_ranks_match_fp64(gpu, precision, D):
    from cdml_amd.evaluate import Evaluation, directed_queries
    n = 5000                                                 # not a multiple of 256: padding rows in the last tile
    v = _unit(n, D, D)
    cw = _random_pairs(n, 3000, 1)
    ev = Evaluation(None, [], device=gpu)
    queries, pos = ev.ranks(v, cw, precision=precision)
    torch.cuda.synchronize()
    want_q, n_self = directed_queries(cw)
    assert n_self == 5 and queries.dtype == torch.int64 and pos.dtype == torch.int64
    assert np.array_equal(queries.cpu().numpy(), want_q)
    pos = pos.cpu().numpy()
    lo, hi = _rank_bounds(v, want_q)
    assert ((pos >= lo) & (pos <= hi)).all(), np.flatnonzero((pos < lo) | (pos > hi))[:10]
    sharp = lo == hi                                         # no row within TOL of the partner's distance
    assert sharp.mean() > 0.5
    assert np.array_equal(pos[sharp], lo[sharp])


@pytest.mark.parametrize("precision", PLANE_FORMS)
def test_ties_go_by_id_and_exclusions(gpu, precision):
    """Exact duplicates of the partner count only below its id; a duplicate of the anchor counts (it is closer); the anchor,
    the partner and the catalogue's padding rows (zero rows: d = 1 < d_p here) never count."""
    from cdml_amd.evaluate import Evaluation
    n, D = 600, 64
    a = 300
    for p in range(400, 460):                                # the first partner with nothing else near either tie
        v = _unit(n, D, 7)
        v[100] = v[p]
        v[500] = v[p]                                        # duplicates of p below and above its id
        v[250] = v[a]
        v[350] = v[a]                                        # duplicates of a below and above its id
        b = v.astype(np.float64)
        d_a = ((b - b[a]) ** 2).sum(1)
        d_p = ((b - b[p]) ** 2).sum(1)
        others = np.ones(n, bool)
        others[[a, p, 100, 500, 250, 350]] = False
        if min(np.abs(d_a[others] - d_a[p]).min(), np.abs(d_p[others] - d_p[a]).min()) > 10 * TOL:
            break
    else:
        pytest.fail("no well-separated partner")
    assert d_a[p] > 1.5                                      # the zero padding rows (d = 1) would count if not excluded
    ev = Evaluation(None, [], device=gpu)
    queries, pos = ev.ranks(v, [[a, p]], precision=precision)
    assert queries.cpu().tolist() == [[a, p], [p, a]]
    # (a, p): strictly closer rows + the dup of p at 100 (not 500) + both dups of a (d = 0)
    want_ap = int((d_a[others] < d_a[p]).sum()) + 1 + 2
    # (p, a): strictly closer rows + both dups of p (d = 0) + the dup of a at 250 (not 350)
    want_pa = int((d_p[others] < d_p[a]).sum()) + 2 + 1
    assert pos.cpu().tolist() == [want_ap, want_pa]


@pytest.mark.parametrize("precision", PLANE_FORMS)
def test_chunking_and_determinism(gpu, precision):
    from cdml_amd.evaluate import Evaluation
    n, D = 3000, 128
    v = _unit(n, D, 11)
    cw = _random_pairs(n, 2000, 12)
    ev = Evaluation(None, [], device=gpu)
    q1, p1 = ev.ranks(v, cw, precision=precision)
    q2, p2 = ev.ranks(v, cw, precision=precision, q_chunk=256, c_chunk=512)
    q3, p3 = ev.ranks(v, cw, precision=precision)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and torch.equal(q1, q3)
    assert torch.equal(p1, p2) and torch.equal(p1, p3)


def _clustered_unit(n, D, seed):
    rng = np.random.RandomState(seed)
    cid = rng.randint(0, n // 8, size=n)
    x = rng.randn(n // 8, D)[cid] + 0.6 * rng.randn(n, D)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), cid


@pytest.mark.parametrize("precision", PLANE_FORMS)
def test_metrics_equal_the_knn_export_path(gpu, precision):
    """Two independent GPU paths -- the rank count and KnnEvaluation over calc_knn's id matrix -- give the same recall /
    nDCG / MAP on pairs whose every rank is determined within TOL."""
    from cdml_amd import knn
    from cdml_amd.evaluate import Evaluation, KnnEvaluation, directed_queries
    n, D = 4000, 64
    v, cid = _clustered_unit(n, D, 5)
    rng = np.random.RandomState(6)
    a = rng.randint(0, n, size=2000)
    p = np.array([rng.choice(np.flatnonzero(cid == cid[x])) for x in a])    # co-watched = same cluster
    cw = np.stack([a, p], 1)
    cw = cw[cw[:, 0] != cw[:, 1]]
    # keep the pairs whose both directions have a sharp rank (no other row within 2 TOL of the partner's distance)
    q, _ = directed_queries(cw)
    lo, hi = _rank_bounds(v, q, 2 * TOL)
    sharp = {tuple(x) for x in q[lo == hi].tolist()}
    cw = np.array([x for x in cw.tolist() if tuple(x) in sharp and (x[1], x[0]) in sharp])
    assert len(cw) > 800
    ev = Evaluation(None, [], device=gpu)
    got = ev.retrieval_metrics(v, cw, ks=(1, 10, 50), precision=precision, l2_norm=True)
    assert got["recall@50"] > 0.2                           # (the comparison is not between two empty lists)
    for k in (1, 10, 50):
        I = knn.calc_knn(v, nearest_num=k + 1, precision=precision)[1]
        ke = KnnEvaluation(cw, I).metrics((k,))
        for m in ("recall@%d", "ndcg@%d", "map@%d", "hit_rate@%d"):
            assert abs(got[m % k] - ke[m % k]) <= 1e-12, (m % k, got[m % k], ke[m % k])
    assert ev.knn(v, cw, k=10, precision=precision, l2_norm=True) == got["recall@10"]
    assert ev.nDCG(v, cw, k=10, precision=precision, l2_norm=True) == got["ndcg@10"]
    assert ev.MAP(v, cw, k=10, precision=precision, l2_norm=True) == got["map@10"]


@pytest.mark.parametrize("precision", PLANE_FORMS)
def test_ranks_at_the_reference_catalogue_size(gpu, precision):
    """doc_location = 343 455 embeddings of 256 (faiss_knn.py:389), 65 536 co-watch pairs: 256 sampled queries against
    fp64 on the host under the gate of test_ranks_match_fp64."""
    from cdml_amd.evaluate import Evaluation
    n, D = 343455, 256
    g = torch.Generator(device=gpu)
    g.manual_seed(3)
    e = torch.randn(n, D, device=gpu, generator=g)
    e = e / e.norm(dim=1, keepdim=True)
    cw = np.random.RandomState(4).randint(0, n, size=(65536, 2))
    ev = Evaluation(None, [], device=gpu)
    queries, pos = ev.ranks(e, cw, precision=precision)
    torch.cuda.synchronize()
    assert queries.shape[0] > 130000
    sel = np.random.RandomState(5).choice(queries.shape[0], 256, replace=False)
    q = queries.cpu().numpy()[sel]
    lo, hi = _rank_bounds(e.cpu().numpy(), q)
    got = pos.cpu().numpy()[sel]
    assert ((got >= lo) & (got <= hi)).all()
    sharp = lo == hi                                         # (few at this density: ~20 rows per 2 TOL of distance)
    assert np.array_equal(got[sharp], lo[sharp])


def _train_run(tmp_path, name, **kw):
    from cdml_amd import engine, train
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    n, F = 1500, 48
    centers = rng.random_sample((12, F))
    cid = rng.randint(0, 12, size=n)
    feats = (centers[cid] + 0.05 * rng.randn(n, F)).clip(0, None).astype(np.float32)
    a = rng.randint(0, n, size=5000)
    p = np.array([rng.choice(np.flatnonzero(cid == cid[x])) for x in a])
    pairs = np.stack([a, p], 1)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]].astype(np.int32)
    eval_pairs, train_pairs = pairs[:300], pairs[300:]
    table = engine.FeatureTable.from_numpy(feats, dev)
    ts = train.TrainStep(table, torch.as_tensor(train_pairs).to(dev), 128, hidden_size=128, output_size=32, margin=0.8,
                         mode="uniform", optimizer="adam", base_learning_rate=0.002, device=dev, precision="f32x3")
    path = tmp_path / (name + ".jsonl")
    tr = train.Trainer(ts, num_epochs=1, n_pairs=len(train_pairs), eval_features=feats, eval_cowatches=eval_pairs.tolist(),
                       check_stop_epoch=0.2, best_eval_dist=10.0, eval_per_epoch=4, require_improve_num=100,
                       summary_path=str(path), **kw)
    tr.run()
    return tr, [json.loads(ln) for ln in open(path)]


def test_trainer_records_retrieval_metrics_only_when_asked(gpu, tmp_path):
    new = {"eval/recall@10", "eval/ndcg@10", "eval/map@10", "eval/mrr"}
    tr, recs = _train_run(tmp_path, "with", eval_retrieval_ks=(10,))
    tr0, recs0 = _train_run(tmp_path, "without")
    assert len(recs) == len(recs0) >= 3
    for r, r0 in zip(recs, recs0):
        assert set(r) == set(r0) | new and not (set(r0) & new)
        assert all(np.isfinite(r[k]) and 0.0 <= r[k] <= 1.0 for k in new)
        assert r["eval/eval_dist"] == r0["eval/eval_dist"]       # selection still on eval_dist, the run unchanged
    assert tr0.eval_retrieval is None
    assert recs[-1]["eval/recall@10"] == tr.eval_retrieval["recall@10"]
