"""CPU checks of the retrieval metrics (evaluate.py: Recall@k, hit rate, nDCG@k, MAP@k, MRR from exact ranks; the
reference's Evaluation.knn / nDCG / MAP and KnnEvaluation stubs): the aggregation against a brute-force fp64
implementation of the definitions, known answers, the kNN-matrix path, the query expansion, and the argument checks of
the rank ABI (no GPU needed: validation comes before any HIP call)."""
import ctypes as C
import math

import numpy as np
import pytest


def _brute(queries, pos, ks):
    """The definitions, one anchor at a time, in Python floats."""
    by_anchor = {}
    for (a, p), r in zip(queries.tolist(), pos.tolist()):
        by_anchor.setdefault(a, []).append(r)
    out = {}
    for k in ks:
        rec, hit, ndcg, ap = [], [], [], []
        for rs in by_anchor.values():
            m = len(rs)
            inside = [r for r in rs if r < k]
            rec.append(len(inside) / m)
            hit.append(1.0 if inside else 0.0)
            ideal = sum(1.0 / math.log2(i + 2) for i in range(min(m, k)))
            ndcg.append(sum(1.0 / math.log2(r + 2) for r in inside) / ideal)
            ap.append(sum(sum(1 for r2 in rs if r2 <= r) / (r + 1) for r in inside) / min(m, k))
        out["recall@%d" % k] = np.mean(rec)
        out["hit_rate@%d" % k] = np.mean(hit)
        out["ndcg@%d" % k] = np.mean(ndcg)
        out["map@%d" % k] = np.mean(ap)
    out["mrr"] = np.mean([1.0 / (1 + min(rs)) for rs in by_anchor.values()])
    out["mean_rank"] = np.mean(pos + 1.0)
    out["median_rank"] = np.median(pos + 1.0)
    out["n_queries"] = len(pos)
    out["n_anchors"] = len(by_anchor)
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_metrics_from_ranks_matches_the_definitions(seed):
    from cdml_amd.evaluate import metrics_from_ranks
    rng = np.random.RandomState(seed)
    n_anchor, n = 300, 5000
    queries, pos = [], []
    for a in rng.choice(n, n_anchor, replace=False):
        m = rng.randint(1, 9)
        partners = rng.choice(n, m, replace=False)
        spread = [8, 30, 300, n][rng.randint(4)]
        ranks = rng.choice(spread, m, replace=False)          # distinct positions in one anchor's list
        queries += [[a, p] for p in partners]
        pos += ranks.tolist()
    queries, pos = np.array(queries, np.int64), np.array(pos, np.int64)
    perm = rng.permutation(len(pos))                            # any order of the queries
    ks = (1, 5, 10, 50, 100)
    got = metrics_from_ranks(queries[perm], pos[perm], ks)
    want = _brute(queries, pos, ks)
    assert set(got) == set(want)
    for name, v in want.items():
        assert abs(got[name] - v) <= 1e-12, (name, got[name], v)


def test_known_answers():
    from cdml_amd.evaluate import metrics_from_ranks
    # one relevant item at position 0, 3 and beyond k
    for p, rec, ndcg, ap, mrr in [(0, 1.0, 1.0, 1.0, 1.0), (3, 1.0, 1.0 / math.log2(5), 0.25, 0.25),
                                  (10, 0.0, 0.0, 0.0, 1.0 / 11)]:
        r = metrics_from_ranks(np.array([[7, 8]]), np.array([p]), (10,))
        assert r["recall@10"] == rec and r["hit_rate@10"] == (1.0 if rec else 0.0)
        assert abs(r["ndcg@10"] - ndcg) < 1e-15 and abs(r["map@10"] - ap) < 1e-15 and abs(r["mrr"] - mrr) < 1e-15
        assert r["mean_rank"] == r["median_rank"] == p + 1 and r["n_queries"] == r["n_anchors"] == 1
    # one anchor with 3 partners at positions 0, 2, 7, cut-off 5
    r = metrics_from_ranks(np.array([[1, 4], [1, 5], [1, 6]]), np.array([7, 0, 2]), (5,))
    assert abs(r["recall@5"] - 2 / 3) < 1e-15
    assert abs(r["ndcg@5"] - (1 + 0.5) / (1 + 1 / math.log2(3) + 0.5)) < 1e-15
    assert abs(r["map@5"] - (1 / 1 + 2 / 3) / 3) < 1e-15
    assert r["mrr"] == 1.0 and r["mean_rank"] == (8 + 1 + 3) / 3 and r["median_rank"] == 3
    with pytest.raises(ValueError):
        metrics_from_ranks(np.zeros((0, 2)), np.zeros(0), (1,))
    with pytest.raises(ValueError):
        metrics_from_ranks(np.array([[1, 2]]), np.array([0]), (0,))


def test_symmetric_expansion_dedup_and_self_pairs():
    from cdml_amd.evaluate import directed_queries
    cw = [[3, 1], [1, 3], [2, 2], [5, 4], [5, 4], [0, 0]]
    q, n_self = directed_queries(cw)
    assert n_self == 2
    assert q.tolist() == [[1, 3], [3, 1], [4, 5], [5, 4]] and q.dtype == np.int64
    q, n_self = directed_queries(cw, symmetric=False)
    assert q.tolist() == [[1, 3], [3, 1], [5, 4]] and n_self == 2
    q, n_self = directed_queries([[4, 4]])
    assert q.shape == (0, 2) and n_self == 1


def test_knn_evaluation_from_an_id_matrix():
    from cdml_amd.evaluate import KnnEvaluation, metrics_from_ranks
    # row r = r's neighbours, nearest first; the self id is NOT always in column 0 (a duplicate row may precede it) and
    # row 3 does not hold itself at all (its last column is then dropped)
    I = np.array([[0, 1, 2, 3],
                  [2, 1, 0, 3],
                  [0, 1, 2, 3],
                  [1, 2, 0, 4],
                  [4, 3, 2, 1]])
    ke = KnnEvaluation([[0, 2], [1, 3], [3, 4], [1, 1]], I)
    assert ke.n_self_pairs_dropped == 1 and ke.max_k == 3
    assert ke.queries.tolist() == [[0, 2], [1, 3], [2, 0], [3, 1], [3, 4], [4, 3]]
    # 0: [1, 2, 3] -> 2 at 1; 1: [2, 0, 3] -> 3 at 2; 2: [0, 1, 3] -> 0 at 0; 3: [1, 2, 0] -> 1 at 0, 4 not in the list;
    # 4: [3, 2, 1] -> 3 at 0
    assert ke.ranks().tolist() == [1, 2, 0, 0, 3, 0]
    got = ke.metrics((1, 2, 3))
    want = metrics_from_ranks(ke.queries, np.array([1, 2, 0, 0, 3, 0]), (1, 2, 3))
    for name in ("recall@1", "ndcg@2", "map@3", "hit_rate@3"):
        assert got[name] == want[name]
    assert "mrr" not in got and got["n_queries"] == 6 and got["n_anchors"] == 5
    assert got["recall@1"] == (0 + 0 + 1 + 0.5 + 1) / 5
    assert ke.knn(3) == got["recall@3"] and ke.nDCG(2) == got["ndcg@2"] and ke.MAP(1) == got["map@1"]
    with pytest.raises(ValueError):
        ke.metrics((4,))                                        # k > I.shape[1] - 1
    with pytest.raises(IndexError):
        KnnEvaluation([[0, 9]], I)


def test_rank_abi_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    v = C.c_void_p(1 << 20)                  # a 16-B aligned non-null address: never dereferenced by a refused call

    def count(fn, Q=v, n_cols=512, D=64, ldq=192, plane=64, extra=()):
        return getattr(lib, fn)(Q, ldq, plane, v, ldq, plane, 300, n_cols, D, *extra, v, v, v, v, v, 0, 1000, v, None)

    for fn, extra in (("cdml_rank_count_x3", ()), ("cdml_rank_count_h2", (2.0 ** -26,))):
        ld = 192 if fn.endswith("x3") else 128
        assert count(fn, Q=None, ldq=ld, extra=extra) == -1 and b"null pointer" in lib.cdml_last_error()
        assert count(fn, n_cols=300, ldq=ld, extra=extra) == -4 and b"multiple of 256" in lib.cdml_last_error()
        assert count(fn, D=100, ldq=ld, extra=extra) == -4 and b"D of 64" in lib.cdml_last_error()
        assert count(fn, ldq=ld - 8, extra=extra) == -3 and b"plane + D" in lib.cdml_last_error()
    assert count("cdml_rank_count_h2", ldq=128, extra=(0.0,)) == -1 and b"out_scale" in lib.cdml_last_error()
    assert lib.cdml_rank_tau_x3(v, 192, 64, None, 192, 64, 300, 64, v, v, v, None) == -1
    assert b"null pointer" in lib.cdml_last_error()
    assert lib.cdml_rank_tau_h2(v, 128, 64, v, 128, 64, 300, 96, 1.0, v, v, v, None) == -4
    assert b"multiple of 64" in lib.cdml_last_error()


def test_precision_is_checked_before_any_device_work():
    from cdml_amd.evaluate import Evaluation
    ev = Evaluation(None, [])
    with pytest.raises(ValueError):
        ev.ranks(np.zeros((8, 4), np.float32), [[0, 1]], precision="f32")
