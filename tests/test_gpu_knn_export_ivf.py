"""The kNN export through IVF indexes on the MI355X (cdml_amd.knn.export(nlist=, feature_nlist=, feature_knn=, audit_rows=);
DESIGN.md section 9a.1).  n = 2 000 rows: 1 628-d clustered raw features (40 clusters of 50 consecutive rows, three rows exact
duplicates of each other) and 256-d clustered embeddings (20 clusters, row i in cluster i % 20), nearest_num = 26,
desim_nearest_num = 10, strict and cross (doc_location 1 200: every embedding cluster has 60 videos and 40 documents).

(i)   the defaults and nlist = 0 write identical files;
(ii)  every list probed (nprobe = nlist), f32 lists: the exact answer -- test_gpu_knn.check against the fp64 oracle;
(iii) the same on f16 lists with the fp32 re-rank and the filter scan, on the rows that meet section 9f.1's recovery condition;
(iv)  nlist 32, nprobe 4: bit-equal to the composition of IVFIndex.build / search, desim and the writer called by hand;
(v)   feature_knn= from arrays and from a directory;
(vi)  the audit's counts against the numpy model of tests/export_audit_ref.py.
The fp64 references are computed once per module."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_audit_ref as aref  # noqa: E402
import ivf_f16_ref as f16  # noqa: E402
from test_gpu_knn import TOL, check  # noqa: E402
from test_knn_desim_host import greedy_desim  # noqa: E402

from oracle import knn as oknn  # noqa: E402

pytestmark = pytest.mark.gpu

N, F, E, K, KF, LOC = 2000, 1628, 256, 26, 10, 1200
MODES = {"strict": 0, "cross": LOC}


def clustered(n, dim, cluster_of, sigma, seed):
    rng = np.random.RandomState(seed)
    c = rng.randn(int(cluster_of.max()) + 1, dim)
    return (c[cluster_of] + sigma * rng.randn(n, dim)).astype(np.float32)


def make_data(n, f_dim, e_dim, seed, f_clusters, e_clusters):
    feats = clustered(n, f_dim, np.arange(n) // (n // f_clusters), 0.5, seed)
    emb = clustered(n, e_dim, np.arange(n) % e_clusters, 0.6, seed + 1)
    feats[500] = feats[100]
    feats[1500] = feats[100]                                      # three rows, exact duplicates of each other: ties go by id
    return emb, feats, ["guid-%05d" % i for i in range(n)]


@pytest.fixture(scope="module")
def knn(gpu):
    import cdml_amd
    from cdml_amd import knn
    cdml_amd.load_library()
    return knn


@pytest.fixture(scope="module")
def data():
    emb, feats, names = make_data(N, F, E, 11, 40, 20)
    d = {"emb": emb, "feats": feats, "names": names}
    d["fD"], d["fI"], d["fd"] = oknn.calc_knn_exact(feats, nearest_num=KF)
    for mode, loc in MODES.items():
        D, I, rows = aref.exact_lists(emb, loc, np.arange(N), K)
        d[mode] = (D, I, rows if loc == 0 else None)
    # cross mode: the full distance rows against the searched side, ids local to it
    v, t = emb[:LOC], emb[LOC:]
    d["cross_parts"] = (oknn.calc_knn_exact(t, v, K), oknn.calc_knn_exact(v, t, K))
    return d


def run(knn, data, out, mode, **kw):
    st = {}
    D, I = knn.export(data["emb"], data["feats"], data["names"], str(out), doc_location=MODES[mode], nearest_num=K,
                      desim_nearest_num=KF, split_num=7, stats=st, **kw)
    torch.cuda.synchronize()
    return D, I, st


def files(out):
    return {f: open(os.path.join(str(out), f), "rb").read() for f in sorted(os.listdir(str(out)))}


def arrays(out, mode):
    return {k: np.load(os.path.join(str(out), f)) for k, f in (("fD", "fD.npy"), ("fI", "fI.npy"), ("D", mode + "D.npy"),
                                                               ("I", mode + "I.npy"), ("des", mode + "I_desim.npy"))}


def text_of(knn, tmp, D, I, names, prefix):
    knn.write_knn(str(tmp), D, I, names, split_num=7, prefix=prefix)
    return {f: open(os.path.join(str(tmp), f), "rb").read() for f in sorted(os.listdir(str(tmp)))}


def check_embedding(data, mode, a, rows=None):
    """``check`` of the export's D / I against the fp64 oracle (cross: every side against its own distance rows)"""
    rows = np.ones(N, dtype=bool) if rows is None else rows
    if mode == "strict":
        Dr, Ir, d = data["strict"]
        check(a["D"][rows], a["I"][rows], Dr[rows], Ir[rows], d[rows])
        return
    for (Dr, Ir, d), sl, shift in ((data["cross_parts"][0], slice(0, LOC), LOC), (data["cross_parts"][1], slice(LOC, N), 0)):
        I = a["I"][sl]
        m = rows[sl]
        check(a["D"][sl][m], np.where(I >= 0, I - shift, I)[m], Dr[m], Ir[m], d[m])


def check_own_lists(knn, tmp_path, out, mode, a, names):
    """desim and the text of an export are functions of its own arrays: the greedy rule, and the host writer"""
    assert np.array_equal(a["des"], greedy_desim(a["I"], a["fI"], a["fD"], 1.4, min(31, KF)))
    got = {f: b for f, b in files(out).items() if f.startswith(mode + "_knn")}
    assert got == text_of(knn, tmp_path / "by_hand", a["D"], a["des"], names, mode + "_knn") and len(got) == 7
    assert sum(b.count(b"#") for b in got.values()) > N             # lists with entries below 1.4: the writer had work


# ---- (i) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_defaults_and_zero_lists_write_identical_files(knn, data, tmp_path, mode):
    D0, I0, st0 = run(knn, data, tmp_path / "a", mode)
    D1, I1, st1 = run(knn, data, tmp_path / "b", mode, nlist=0, nprobe=0, feature_nlist=0, feature_nprobe=0)
    assert files(tmp_path / "a") == files(tmp_path / "b") and len(files(tmp_path / "a")) == 6 + 7
    assert torch.equal(D0, D1) and torch.equal(I0, I1)
    assert sorted(st0) == ["desim", "embedding_knn", "feature_knn", "write"] and "ivf" not in st0["embedding_knn"]
    a = arrays(tmp_path / "a", mode)
    check(a["fD"], a["fI"], data["fD"], data["fI"], data["fd"])
    check_embedding(data, mode, a)
    assert a["fI"][[100, 500, 1500], :3].tolist() == [[100, 500, 1500]] * 3        # the duplicates, by id


# ---- (ii) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_every_list_probed_is_the_exact_export(knn, data, tmp_path, mode):
    out = tmp_path / "o"
    _, _, st = run(knn, data, out, mode, nlist=8, nprobe=8, feature_nlist=8, feature_nprobe=8)
    a = arrays(out, mode)
    check(a["fD"], a["fI"], data["fD"], data["fI"], data["fd"])
    check_embedding(data, mode, a)
    assert a["fI"][[100, 500, 1500], :3].tolist() == [[100, 500, 1500]] * 3
    check_own_lists(knn, tmp_path, out, mode, a, data["names"])
    assert "ivf" in st["feature_knn"] and "ivf" in st["embedding_knn"] and st["feature_knn"]["ivf"]["n_tiles"] > 0


# ---- (iii) ----------------------------------------------------------------------------------------------------------------------
def recoverable_rows(d_rows, k, r):
    """section 9f.1's condition with every list probed, in fp64: the (r + 1)-th distance exceeds the k-th by more than
    2 E + 4 TOL (fewer than r + 1 rows: every row is a candidate)"""
    ds = np.sort(np.asarray(d_rows), axis=1)
    if ds.shape[1] <= r:
        return np.ones(ds.shape[0], dtype=bool)
    return ds[:, r] - ds[:, k - 1] > 2 * f16.rounding_bound() + 4 * TOL


@pytest.mark.parametrize("mode", list(MODES))
def test_f16_lists_with_rerank_and_filter_scan(knn, data, tmp_path, mode):
    out, r = tmp_path / "o", 128
    run(knn, data, out, mode, nlist=8, nprobe=8, feature_nlist=8, feature_nprobe=8, storage="f16", refine=r, scan="filter")
    a = arrays(out, mode)
    okf = recoverable_rows(data["fd"], KF, r)
    if mode == "strict":
        oke = recoverable_rows(data["strict"][2], K, r)
    else:
        oke = np.concatenate([recoverable_rows(data["cross_parts"][0][2], K, r), recoverable_rows(data["cross_parts"][1][2], K, r)])
    print("rows that meet the recovery condition: features %.4f, embeddings %.4f" % (okf.mean(), oke.mean()))
    assert okf.mean() >= 0.95 and oke.mean() >= 0.95                 # a condition on the inputs
    check(a["fD"][okf], a["fI"][okf], data["fD"][okf], data["fI"][okf], data["fd"][okf])
    check_embedding(data, mode, a, oke)
    check_own_lists(knn, tmp_path, out, mode, a, data["names"])


# ---- (iv) -----------------------------------------------------------------------------------------------------------------------
def by_hand(knn, base, queries, k, nlist, nprobe, dev):
    idx = knn.IVFIndex.build(torch.from_numpy(base), nlist, iters=10, seed=0, device=dev)
    return idx.search(torch.from_numpy(queries), k, nprobe)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", ["both", "embedding", "feature"])
def test_probed_export_is_the_composition_of_its_parts(knn, data, tmp_path, gpu, mode, which):
    out = tmp_path / "o"
    kw = {}
    if which != "feature":
        kw.update(nlist=32, nprobe=4)
    if which != "embedding":
        kw.update(feature_nlist=32, feature_nprobe=4)
    D, Ides, st = run(knn, data, out, mode, **kw)
    a = arrays(out, mode)
    emb, feats = data["emb"], data["feats"]
    if which != "embedding":
        fD, fI = by_hand(knn, feats, feats, KF, 32, 4, gpu)
    else:
        fD, fI = knn.knn_search(torch.from_numpy(feats), torch.from_numpy(feats), KF, device=gpu)
    if which == "feature":
        De, Ie = knn.cross_knn(torch.from_numpy(emb).to(gpu), LOC, nearest_num=K, device=gpu) if mode == "cross" else \
            knn.knn_search(torch.from_numpy(emb), torch.from_numpy(emb), K, device=gpu)
    elif mode == "strict":
        De, Ie = by_hand(knn, emb, emb, K, 32, 4, gpu)
    else:
        v, t = emb[:LOC], emb[LOC:]
        nl_t, nl_v = knn.cross_nlist(32, N - LOC, N), knn.cross_nlist(32, LOC, N)
        assert (nl_t, nl_v) == (13, 20)
        D1, I1 = by_hand(knn, t, v, K, nl_t, min(4, nl_t), gpu)
        D2, I2 = by_hand(knn, v, t, K, nl_v, min(4, nl_v), gpu)
        De, Ie = torch.cat([D1, D2]), torch.cat([torch.where(I1 >= 0, I1 + LOC, I1), I2])
    des = knn.desim(Ie, fI, fD, device=gpu)
    for got, want in ((a["fD"], fD), (a["fI"], fI), (a["D"], De), (a["I"], Ie), (a["des"], des)):
        assert torch.equal(torch.from_numpy(got), want.cpu())
    assert torch.equal(D, De) and torch.equal(Ides, des)
    got = {f: b for f, b in files(out).items() if f.startswith(mode + "_knn")}
    assert got == text_of(knn, tmp_path / "by_hand", De, des, data["names"], mode + "_knn")
    assert ("ivf" in st["embedding_knn"]) == (which != "feature") and ("ivf" in st["feature_knn"]) == (which != "embedding")
    if which == "both":                                               # four of 32 lists: not the exact answer any more
        assert not np.array_equal(a["I"], data[mode][1])


# ---- (v) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_feature_knn_from_arrays_and_from_a_directory(knn, data, tmp_path, mode):
    first = tmp_path / "first"
    run(knn, data, first, mode, nlist=32, nprobe=4, feature_nlist=32, feature_nprobe=4)
    want = files(first)
    a = arrays(first, mode)
    for tag, given in (("arrays", (a["fD"], a["fI"])), ("tensors", (torch.from_numpy(a["fD"]), torch.from_numpy(a["fI"]))),
                       ("dir", str(first))):
        st = {}
        knn.export(data["emb"], None, data["names"], str(tmp_path / tag), doc_location=MODES[mode], nearest_num=K,
                   desim_nearest_num=KF, split_num=7, nlist=32, nprobe=4, feature_knn=given, stats=st)
        assert files(tmp_path / tag) == want, tag
        assert "feature_knn" not in st and sorted(st) == ["desim", "embedding_knn", "write"]


# ---- (vi) -----------------------------------------------------------------------------------------------------------------------
A_N, A_K, A_KF, A_M, A_LOC = 600, 9, 5, 32, 360


def cube(n, w2):
    """Rows 0 .. n - 1 as corners of a weighted hypercube: bit b of the row index picks one of two coordinates of weight
    sqrt(w2[b]), so every row has the same norm and d(i, j) = 2 sum(w2[b] over the bits of i xor j) / sum(w2).  With
    w2[b] = c_b + 2^b the sums over different bit sets differ by at least one unit: from any row, no two distances are
    closer than 2 / sum(w2)."""
    bits = (np.arange(n)[:, None] >> np.arange(len(w2))[None, :]) & 1
    x = np.zeros((n, 2 * len(w2)))
    for b, w in enumerate(w2):
        x[np.arange(n), 2 * b + bits[:, b]] = np.sqrt(w)
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def audit_data():
    """Random rows cannot meet the audit test's precondition (a few thousand gaps, each below 8 TOL with probability near
    1 %), so the distances are built: embeddings with w2 = 1024 + 2^b (a row's neighbours flip one bit of its index, low bits
    first; gaps >= 2 / 11263 = 1.8e-4), raw features with two light bits, w2 = 64 + 2^b for b < 2 (rows i ^ 1, i ^ 2, i ^ 3 are
    near-duplicates of row i, so desim removes something; gaps >= 2 / 9343 = 2.1e-4)."""
    emb = cube(A_N, [1024 + 2 ** b for b in range(10)])
    feats = cube(A_N, [64 + 1, 64 + 2] + [1024 + 2 ** b for b in range(2, 10)])
    return {"emb": emb, "feats": feats, "names": ["guid-%05d" % i for i in range(A_N)]}


def min_gap(d_rows, k):
    """the smallest difference between two of the first k + 1 sorted distances of any row"""
    ds = np.sort(np.asarray(d_rows), axis=1)[:, :k + 1]
    return float(np.diff(ds, axis=1).min())


@pytest.mark.parametrize("mode,loc", [("strict", 0), ("cross", A_LOC)])
def test_audit_counts_equal_the_numpy_model(knn, audit_data, tmp_path, mode, loc):
    emb, feats, names = audit_data["emb"], audit_data["feats"], audit_data["names"]
    sample = knn.audit_sample(A_N, A_M, 3).numpy()
    # the precondition, from fp64: the device's exact searches order the sampled rows' lists as the oracle does
    _, ex, d_rows = aref.exact_lists(emb, loc, sample, A_K)
    gap_e = min(min_gap(np.asarray(d)[None, :], A_K) for d in d_rows)
    U = np.unique(np.concatenate([sample, ex[ex >= 0]]))
    gap_f = min_gap(oknn.calc_knn_exact(feats, feats[U], A_KF)[2], A_KF)
    print("smallest gap among the first k + 1 exact distances: embeddings %.3g, features %.3g (8 TOL = %.3g)" % (gap_e, gap_f, 8 * TOL))
    assert gap_e >= 8 * TOL and gap_f >= 8 * TOL
    reports = {}
    for tag, nprobe in (("one", 1), ("all", 16)):
        out, st = tmp_path / tag, {}
        knn.export(emb, feats, names, str(out), doc_location=loc, nearest_num=A_K, desim_nearest_num=A_KF, split_num=3,
                   nlist=16, nprobe=nprobe, feature_nlist=16, feature_nprobe=nprobe, audit_rows=A_M, audit_seed=3, stats=st)
        rep = json.load(open(os.path.join(str(out), "export_audit.json")))
        a = arrays(out, mode)
        want = aref.audit_counts(emb, feats, loc, sample, a["I"], a["fI"], a["des"], A_K, A_KF)
        print(tag, {key: rep[key] for key in aref.COUNT_KEYS})
        assert {key: rep[key] for key in aref.COUNT_KEYS} == want
        assert {key: st["audit"][key] for key in aref.COUNT_KEYS} == want and st["audit"]["seconds"] > 0
        assert (rep["nlist"], rep["nprobe"], rep["feature_nlist"], rep["feature_nprobe"], rep["mode"]) == (16, nprobe, 16, nprobe, mode)
        reports[tag] = rep
    one, full = reports["one"], reports["all"]
    assert one["e_possible"] == full["e_possible"] == A_M * A_K and one["f_possible"] == full["f_possible"] == A_M * A_KF
    assert one["e_hits"] < one["e_possible"]
    assert full["e_hits"] == full["e_possible"] and full["f_hits"] == full["f_possible"]
    assert full["desim_rows_equal"] == A_M and full["desim_kept_intersection"] == full["desim_kept_union"]
