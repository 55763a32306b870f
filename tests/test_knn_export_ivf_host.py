"""CPU-side checks of the export at catalogue scale (cdml_amd.knn.export / cross_knn / ivf_knn with an IVF index; DESIGN.md
section 9a.1): every refusal by name (raised before any device work, so a machine without a GPU reaches them), ``cross_nlist``
by hand values, the audit's sampling rule, the numpy model of the audit counts (tests/export_audit_ref.py) on hand-made 6-row
cases, and -- with the device searches replaced by the fp64 oracle -- the whole of ``export`` on the host: the audit's JSON
against the model, the ``stats`` keys, ``feature_knn`` from arrays and from a directory."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_audit_ref as aref  # noqa: E402
from test_knn_desim_host import greedy_desim  # noqa: E402

from oracle import knn as oknn  # noqa: E402


@pytest.fixture(scope="module")
def knn():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import knn
    return knn


def _arrays(n=12, seed=0):
    rng = np.random.RandomState(seed)
    return rng.randn(n, 8).astype(np.float32), rng.randn(n, 16).astype(np.float32), ["g%d" % i for i in range(n)]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,msg", [
    (dict(nprobe=4), "nprobe = 4 without nlist"),
    (dict(feature_nprobe=2), "feature_nprobe = 2 without feature_nlist"),
    (dict(storage="f16"), "storage, refine and scan belong to an IVF search"),
    (dict(scan="filter"), "storage, refine and scan belong to an IVF search"),
    (dict(storage="f16", refine=8), "refine and scan belong to an IVF search"),
    (dict(refine=8, nlist=2, nprobe=1), "refine belongs to storage=\"f16\""),
    (dict(storage="f8", nlist=2, nprobe=1), "storage must be one of"),
    (dict(scan="tree", nlist=2, nprobe=1), "scan must be one of"),
    (dict(storage="f16", refine=2, nlist=2, nprobe=1), "refine must be 0 or in [k = 5"),
    (dict(nlist=13, nprobe=1), "nlist = 13 exceeds the 12 rows"),
    (dict(feature_nlist=13, feature_nprobe=1), "feature_nlist = 13 exceeds the 12 rows"),
    (dict(nlist=4, nprobe=5), "nprobe must be in [1, nlist = 4]"),
    (dict(nlist=4), "nprobe must be in [1, nlist = 4]"),
    (dict(nlist=-1), "must be >= 0"),
    (dict(feature_knn=(np.zeros((12, 3), np.float32), np.zeros((12, 4), np.int64))), "two [n = 12, >= 1] arrays of one shape"),
    (dict(feature_knn=(np.zeros((11, 3), np.float32), np.zeros((11, 3), np.int64))), "two [n = 12, >= 1] arrays of one shape"),
    (dict(feature_knn=(np.zeros((12, 0), np.float32), np.zeros((12, 0), np.int64))), "two [n = 12, >= 1] arrays of one shape"),
    (dict(feature_knn=(np.zeros(12, np.float32), np.zeros(12, np.int64))), "two [n = 12, >= 1] arrays of one shape"),
    (dict(feature_knn=3), "feature_knn must be a pair"),
    (dict(feature_knn=(np.zeros((12, 3), np.float32), np.zeros((12, 3), np.int64)), feature_nlist=2, feature_nprobe=1),
     "feature_knn and feature_nlist > 0 exclude each other"),
    (dict(audit_rows=-1), "audit_rows must be in [0, n = 12]"),
    (dict(audit_rows=13), "audit_rows must be in [0, n = 12]"),
    (dict(writer="gpu"), "writer must be one of"),
])
def test_export_refuses_by_name_before_any_device_work(knn, tmp_path, kw, msg):
    emb, feats, names = _arrays()
    out = tmp_path / "never"
    with pytest.raises(ValueError) as e:
        knn.export(emb, feats, names, str(out), doc_location=0, nearest_num=5, desim_nearest_num=3, **kw)
    assert msg in str(e.value), str(e.value)
    assert not out.exists()                                       # nothing was started


def test_cross_export_refuses_an_nlist_above_a_side(knn, tmp_path):
    emb, feats, names = _arrays()
    # 12 rows, a side of one row: cross_nlist(12, 1, 12) = 1 is fine, but nlist = 12 is above neither; nlist 13 is above n
    with pytest.raises(ValueError, match="exceeds the 12 rows"):
        knn.export(emb, feats, names, str(tmp_path / "x"), doc_location=1, nearest_num=5, nlist=13, nprobe=1)
    with pytest.raises(ValueError, match="nprobe = 1 without nlist"):
        knn.cross_knn(emb, 6, nearest_num=5, nprobe=1)
    with pytest.raises(ValueError, match="belong to nlist > 0"):
        knn.cross_knn(emb, 6, nearest_num=5, scan="filter")
    with pytest.raises(ValueError, match="nlist = 13 exceeds"):
        knn.cross_knn(emb, 6, nearest_num=5, nlist=13, nprobe=1)
    with pytest.raises(ValueError, match="writer must be one of"):
        knn.write_knn(str(tmp_path / "w"), emb[:, :2], np.zeros((12, 2), np.int64), names, writer="gpu")
    assert not (tmp_path / "w").exists() and not (tmp_path / "x").exists()


def test_cross_nlist_by_hand(knn):
    assert knn.cross_nlist(1024, 343455, 343455 + 100000) == 794          # ceil(1024 * 343455 / 443455) = ceil(793.08)
    assert knn.cross_nlist(1024, 100000, 443455) == 231                   # ceil(230.91)
    assert knn.cross_nlist(16, 1, 2000) == 1                              # a 1-row side: one list, never none
    assert knn.cross_nlist(16, 1999, 2000) == 16
    assert knn.cross_nlist(16, 1000, 2000) == 8 and knn.cross_nlist(16, 1001, 2000) == 9
    assert knn.cross_nlist(1, 7, 9) == 1 and knn.cross_nlist(9, 9, 9) == 9
    for nlist, n_side, n in ((16, 1200, 2000), (32, 800, 2000), (5, 3, 7)):
        got = knn.cross_nlist(nlist, n_side, n)
        assert got == max(1, -(-nlist * n_side // n)) and (got - 1) * n < nlist * n_side <= got * n
    with pytest.raises(ValueError):
        knn.cross_nlist(0, 3, 7)
    with pytest.raises(ValueError):
        knn.cross_nlist(4, 8, 7)


def test_audit_sample_is_the_sorted_head_of_a_seeded_randperm(knn):
    for n, m, seed in ((600, 32, 0), (10, 10, 3), (7, 0, 1), (2000, 1, 9)):
        g = torch.Generator()
        g.manual_seed(seed)
        want = np.sort(torch.randperm(n, generator=g)[:m].numpy())
        got = knn.audit_sample(n, m, seed)
        assert got.dtype == torch.int64 and got.device.type == "cpu" and np.array_equal(got.numpy(), want)
        assert len(set(got.tolist())) == m
    assert not np.array_equal(knn.audit_sample(600, 32, 0).numpy(), knn.audit_sample(600, 32, 1).numpy())


# ---- the numpy model on hand-made 6-row cases -----------------------------------------------------------------------------------
def _six():
    """six points on a circle at angles 0, 10, 25, 90, 100, 180 degrees (embeddings); raw features: rows 0 and 1 duplicates of
    each other, rows 3 and 4 close, the others far apart"""
    a = np.deg2rad([0.0, 10.0, 25.0, 90.0, 100.0, 180.0])
    emb = np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)
    feats = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0.05], [0, 0, 0, 1]], dtype=np.float32)
    return emb, feats


def test_model_counts_on_a_strict_case_by_hand():
    emb, feats = _six()
    k, k_f = 3, 2
    _, I, _ = oknn.calc_knn_exact(emb, nearest_num=k)
    assert I.tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 4, 2], [4, 3, 2], [5, 4, 3]]
    fD, fI, _ = oknn.calc_knn_exact(feats, nearest_num=k_f)
    assert fI[:2].tolist() == [[0, 1], [0, 1]] and fI[3:5].tolist() == [[3, 4], [4, 3]]
    des = greedy_desim(I, fI, fD.astype(np.float32), 1.4, k_f)
    # row 0: 0 removes 1 (its duplicate), the query 0 goes at the end: {2}; row 3: 3 removes 4, then 3 is the query: {2}
    assert des.tolist() == [[-1, -1, 2], [-1, -1, 2], [-1, 1, -1], [-1, -1, 2], [-1, -1, 2], [-1, 4, -1]]
    sample = np.array([0, 3, 5])
    c = aref.audit_counts(emb, feats, 0, sample, I, fI, des, k, k_f, fI_end=k_f)
    assert c == {"audit_rows": 3, "union_rows": 6, "e_hits": 9, "e_possible": 9, "f_hits": 6, "f_possible": 6,
                 "desim_rows_equal": 3, "desim_kept_intersection": 3, "desim_kept_union": 3}
    # an export that lost row 0's neighbour 2 and row 5's neighbour 4, and whose feature list of row 3 misses row 4
    I2, fI2, des2 = I.copy(), fI.copy(), des.copy()
    I2[0, 2], I2[5, 1], fI2[3, 1] = 5, 0, 0
    des2[0] = [-1, -1, 5]
    des2[5] = [-1, 0, 3]
    c = aref.audit_counts(emb, feats, 0, sample, I2, fI2, des2, k, k_f, fI_end=k_f)
    assert (c["e_hits"], c["e_possible"], c["f_hits"], c["f_possible"]) == (7, 9, 5, 6)
    # row 0: {5} against {2}; row 3: equal; row 5: {0, 3} against {4}
    assert (c["desim_rows_equal"], c["desim_kept_intersection"], c["desim_kept_union"]) == (1, 1, 1 + 2 + 3)
    assert c["union_rows"] == 6 and tuple(sorted(c)) == tuple(sorted(aref.COUNT_KEYS))


def test_model_counts_on_a_cross_case_by_hand():
    emb, feats = _six()
    k, k_f, loc = 2, 2, 4                                         # videos 0..3, documents 4, 5
    D, I, _ = aref.exact_lists(emb, loc, np.arange(6), k)
    # a video's neighbours are documents (global ids 4, 5), a document's are videos
    assert I.tolist() == [[4, 5], [4, 5], [4, 5], [4, 5], [3, 2], [3, 2]]
    fD, fI, _ = oknn.calc_knn_exact(feats, nearest_num=k_f)
    des = greedy_desim(I, fI, fD.astype(np.float32), 1.4, k_f)
    sample = np.array([1, 4])
    c = aref.audit_counts(emb, feats, loc, sample, I, fI, des, k, k_f, fI_end=k_f)
    assert c["union_rows"] == 5 and c["e_hits"] == c["e_possible"] == 4 and c["f_hits"] == c["f_possible"] == 4   # U = {1, 4} + {4, 5, 3, 2}
    assert c["desim_rows_equal"] == 2 and c["desim_kept_intersection"] == c["desim_kept_union"]
    one = aref.exact_lists(emb, loc, np.array([5]), 3)[1]
    assert one.tolist() == [[3, 2, 1]]
    short = aref.exact_lists(emb, 5, np.array([0]), 3)            # one document: the list runs out
    assert short[1].tolist() == [[5, -1, -1]] and np.isinf(short[0][0, 1:]).all()


# ---- export() on the host: the device searches replaced by the oracle -----------------------------------------------------------
@pytest.fixture()
def host_export(knn, monkeypatch):
    """``knn`` with knn_search / desim replaced by the fp64 oracle and the greedy rule, and ivf_knn by an "approximate" search
    that loses every list's last neighbour (it returns the exact list with its tail replaced by the next one): export(device=
    "cpu") then runs end to end without a GPU."""
    def search(base, queries, k, l2_norm=True, device="cpu", precision="f32x3", **_):
        b = base.numpy() if torch.is_tensor(base) else np.asarray(base)
        q = queries.numpy() if torch.is_tensor(queries) else np.asarray(queries)
        D, I, _ = oknn.calc_knn_exact(b, q, k, l2_norm=l2_norm)
        return torch.from_numpy(D.astype(np.float32)), torch.from_numpy(I)

    def lossy(base, queries=None, k=51, stats=None, **kw):
        D, I = search(base, base if queries is None else queries, k + 1)
        if stats is not None:
            stats.update(chunks=[(0, 1)], n_tiles=3, n_floats=7, probe=torch.zeros(1), scan=kw.get("scan", "buffer"))
        return torch.cat([D[:, :k - 1], D[:, k:]], 1).contiguous(), torch.cat([I[:, :k - 1], I[:, k:]], 1).contiguous()

    def desim(eI, fI, fD, fD_threshold=1.4, fI_end=31, query_ids=None, device="cpu"):
        e = eI.numpy() if torch.is_tensor(eI) else np.asarray(eI)
        f, d = (x.numpy() if torch.is_tensor(x) else np.asarray(x) for x in (fI, fD))
        q = None if query_ids is None else (query_ids.numpy() if torch.is_tensor(query_ids) else np.asarray(query_ids))
        return torch.from_numpy(greedy_desim(e, f, d, fD_threshold, min(fI_end, f.shape[1]), query_ids=q))

    monkeypatch.setattr(knn, "knn_search", search)
    monkeypatch.setattr(knn, "ivf_knn", lossy)
    monkeypatch.setattr(knn, "desim", desim)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda *a, **k: 0)
    return knn


def _clustered(n, D, seed):
    rng = np.random.RandomState(seed)
    return (np.repeat(rng.randn(n // 4, D), 4, axis=0) + 0.3 * rng.randn(n, D)).astype(np.float32)


@pytest.mark.parametrize("loc", [0, 14])
def test_host_export_audit_equals_the_model_and_stats_keys(host_export, tmp_path, loc):
    knn = host_export
    n, k, k_f, m = 24, 5, 3, 7
    emb, feats, names = _clustered(n, 6, 1), _clustered(n, 10, 2), ["v%d" % i for i in range(n)]
    mode = "cross" if loc else "strict"
    for nlist, f_nlist, tag in ((0, 0, "exact"), (4, 0, "emb"), (0, 4, "feat"), (4, 4, "both")):
        out, st = str(tmp_path / tag), {}
        kw = dict(nlist=nlist, nprobe=1 if nlist else 0, feature_nlist=f_nlist, feature_nprobe=2 if f_nlist else 0)
        knn.export(emb, feats, names, out, doc_location=loc, nearest_num=k, desim_nearest_num=k_f, split_num=3, device="cpu",
                   audit_rows=m, audit_seed=5, stats=st, **kw)
        rep = json.load(open(os.path.join(out, "export_audit.json")))
        I, fI, des = (np.load(os.path.join(out, f)) for f in (mode + "I.npy", "fI.npy", mode + "I_desim.npy"))
        want = aref.audit_counts(emb, feats, loc, knn.audit_sample(n, m, 5).numpy(), I, fI, des, k, k_f)
        assert {key: rep[key] for key in aref.COUNT_KEYS} == want
        assert all(isinstance(rep[key], int) for key in aref.COUNT_KEYS)
        assert (rep["e_hits"] == rep["e_possible"]) == (nlist == 0) and (rep["f_hits"] == rep["f_possible"]) == (f_nlist == 0)
        if not nlist and not f_nlist:
            assert rep["desim_rows_equal"] == m and rep["desim_kept_intersection"] == rep["desim_kept_union"]
        for key, v in dict(kw, mode=mode, n=n, doc_location=loc, nearest_num=k, desim_nearest_num=k_f, storage="f32", refine=0,
                           scan="buffer", ivf_iters=10, ivf_seed=0, audit_seed=5, feature_knn_given=False).items():
            assert rep[key] == v, key
        # stats: one entry per stage, each with seconds and the peak memory; the IVF numbers where an index was used
        assert sorted(st) == ["audit", "desim", "embedding_knn", "feature_knn", "write"]
        for stage in st.values():
            assert stage["seconds"] >= 0 and "max_memory_allocated" in stage
        assert ("ivf" in st["embedding_knn"]) == bool(nlist) and ("ivf" in st["feature_knn"]) == bool(f_nlist)
        assert st["write"]["writer"] == "host" and {key: st["audit"][key] for key in aref.COUNT_KEYS} == want
        if f_nlist:
            assert st["feature_knn"]["ivf"] == {"n_chunks": 1, "n_tiles": 3, "n_floats": 7, "scan": "buffer"}   # no tensors
        if nlist and loc:
            assert sorted(st["embedding_knn"]["ivf"]) == ["doc_to_video", "video_to_doc"]
        json.dumps(st)                                              # a report: plain numbers and strings only


def test_host_export_defaults_and_feature_knn_round_trip(host_export, tmp_path):
    knn = host_export
    n, k, k_f = 24, 5, 3
    emb, feats, names = _clustered(n, 6, 3), _clustered(n, 10, 4), ["v%d" % i for i in range(n)]
    a, b, c, d = (str(tmp_path / x) for x in "abcd")
    knn.export(emb, feats, names, a, doc_location=10, nearest_num=k, desim_nearest_num=k_f, split_num=3, device="cpu")
    assert "export_audit.json" not in os.listdir(a)
    st = {}
    knn.export(emb, None, names, b, doc_location=10, nearest_num=k, desim_nearest_num=k_f, split_num=3, device="cpu",
               feature_knn=(np.load(os.path.join(a, "fD.npy")), np.load(os.path.join(a, "fI.npy"))), stats=st)
    assert "feature_knn" not in st and sorted(st) == ["desim", "embedding_knn", "write"]
    knn.export(emb, None, names, c, doc_location=10, nearest_num=k, desim_nearest_num=k_f, split_num=3, device="cpu", feature_knn=a)
    knn.export(emb, feats, names, d, doc_location=10, nearest_num=k, desim_nearest_num=k_f, split_num=3, device="cpu",
               nlist=0, feature_nlist=0)
    files = sorted(os.listdir(a))
    assert files == sorted(["fD.npy", "fI.npy", "crossD.npy", "crossI.npy", "crossI_desim.npy", "decode_map.json",
                            "cross_knn0", "cross_knn1", "cross_knn2"])
    for other in (b, c, d):
        assert sorted(os.listdir(other)) == files
        for f in files:
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(other, f), "rb").read(), f
    with pytest.raises(ValueError, match="needs features"):
        knn.export(emb, None, names, str(tmp_path / "e"), doc_location=10, nearest_num=k, device="cpu", feature_knn=a, audit_rows=2)
    with pytest.raises(ValueError, match="features is None"):
        knn.export(emb, None, names, str(tmp_path / "e"), doc_location=10, nearest_num=k, device="cpu")
