"""Near-duplicate suppression of the kNN export on the GPU (csrc/knn_desim.hip; faiss_knn.py:146-244), the raw-feature
search at the reference's 1 628-wide features, and the export end to end (faiss_knn.main, :359-400)."""
import os
import time

import numpy as np
import pytest
import torch

from oracle import knn as oknn
from test_gpu_knn import check
from test_knn_desim_host import greedy_desim

pytestmark = pytest.mark.gpu

F_RAW = 1628          # online_data.py:38: the raw feature width (padded to 1 664 by the search)


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(os.path.join(golden_dir, "knn_desim_ref.npz"))


@pytest.mark.parametrize("fi_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("case", ["strict", "cross"])
def test_kernel_is_the_reference_iter_desim_mp_bit_for_bit(gpu, ref, case, fi_dtype):
    from cdml_amd import knn
    eI, fI, fD = ref[case + "_eI"], ref[case + "_fI"].astype(fi_dtype), ref[case + "_fD"]
    thr, fI_end = float(ref["threshold"]), int(ref["fI_end"])
    want = ref[case + "_out"]
    got = knn.desim(eI, fI, fD, fD_threshold=thr, fI_end=fI_end)
    assert isinstance(got, np.ndarray) and got.dtype == eI.dtype and np.array_equal(got, want)
    got2 = knn.iter_desim_mp(eI.copy(), fI.copy(), fD.copy(), thr, fI_end, process_num=22)
    assert np.array_equal(got2, want)
    # device tensors in, device tensors out (the kind and dtype of eI)
    gt = knn.desim(torch.from_numpy(eI).to(gpu), torch.from_numpy(fI).to(gpu), torch.from_numpy(fD).to(gpu), thr, fI_end)
    assert gt.is_cuda and gt.dtype == torch.int64 and np.array_equal(gt.cpu().numpy(), want)


def _random_case(rng, n_f, kf, nq, ke, dup_range):
    """fI rows of near ids (so lists overlap), distances around the threshold, -1 tails; eI rows drawn from the
    neighbourhood of their query with a few ids >= n_f and -1 entries."""
    fI = (np.arange(n_f)[:, None] + rng.randint(-dup_range, dup_range + 1, size=(n_f, kf))) % n_f
    fI[:, 0] = np.arange(n_f)
    fD = rng.uniform(0.0, 2.0, size=(n_f, kf)).astype(np.float32)
    fD[rng.rand(n_f, kf) < 0.05] = np.float32(1.4)
    fI[rng.rand(n_f, kf) < 0.03] = -1
    q = rng.randint(0, n_f, size=nq)
    eI = (q[:, None] + rng.randint(-dup_range, dup_range + 1, size=(nq, ke))) % n_f
    eI[:, 0] = q
    eI[rng.rand(nq, ke) < 0.02] = -1
    eI[rng.rand(nq, ke) < 0.01] = n_f + 3                    # past the catalogue: never kept
    return eI.astype(np.int64), fI.astype(np.int64), fD, q.astype(np.int32)


@pytest.mark.parametrize("ke", [1, 26, 51, 81, 128])
@pytest.mark.parametrize("fI_end", [1, 26, 31, 64])
def test_kernel_matches_the_greedy_rule_on_random_lists(gpu, ke, fI_end):
    from cdml_amd import knn
    rng = np.random.RandomState(1000 * ke + fI_end)
    n_f, kf, nq = 3000, 64 if fI_end == 64 else 40, 400
    eI, fI, fD, q = _random_case(rng, n_f, kf, nq, ke, 60)
    want = greedy_desim(eI, fI, fD, 1.4, fI_end, query_ids=q)
    a = knn.desim(eI, fI, fD, 1.4, fI_end, query_ids=q)
    b = knn.desim(eI, fI.astype(np.int32), fD, 1.4, fI_end, query_ids=torch.from_numpy(q).to(gpu))
    assert np.array_equal(a, want) and np.array_equal(b, a)               # two runs, two id types: the same bits
    assert (a[eI >= n_f] == -1).all()
    # default query ids: the row index (global row order)
    assert np.array_equal(knn.desim(eI, fI, fD, 1.4, fI_end), greedy_desim(eI, fI, fD, 1.4, fI_end))


def _clustered(n, width, seed, dev, cluster=8, noise=0.5):
    """rows in clusters of ~``cluster`` around shared centres: near-duplicates in raw-feature space (normalised squared
    distance ~0.4 inside a cluster, ~2 across), so desim has something to remove"""
    gw = torch.Generator(device=dev)
    gw.manual_seed(1234)                                     # the same clusters in every space: embedding neighbours
    which = torch.randint(0, n // cluster + 1, (n,), generator=gw, device=dev)   # are raw-feature near-duplicates
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn((n // cluster + 1, width), generator=g, device=dev, dtype=torch.float32)
    return centres[which] + noise * torch.randn((n, width), generator=g, device=dev, dtype=torch.float32)


def test_knn_search_1628_wide_score_blocks(gpu):
    """20 000 rows, separate queries, D = 1 628 (padded to 1 664): the score-block path against the fp64 search."""
    from cdml_amd import knn
    rng = np.random.RandomState(11)
    base = rng.randn(20000, F_RAW).astype(np.float32)
    base[7000:7004] = base[42]
    q = np.concatenate([rng.randn(150, F_RAW).astype(np.float32), base[42:43]])
    D, I = knn.knn_search(torch.from_numpy(base), torch.from_numpy(q), 26)
    Dr, Ir, dfull = oknn.calc_knn_exact(base, q, 26)
    check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, dfull)
    assert sorted(I[-1, :5].cpu().tolist()) == [42, 7000, 7001, 7002, 7003]


def test_knn_search_1628_wide_filter_path_and_chunks(gpu):
    """70 000 rows + 200 queries at D = 1 628 through the filter epilogue (n > 2 x FIRST_BLOCK), equal to the score-block
    form, and again in several query and catalogue chunks (q_chunk / c_chunk far below the 2 GiB descriptor limit)."""
    from cdml_amd import knn
    rng = np.random.RandomState(12)
    base = rng.randn(70000, F_RAW).astype(np.float32)
    base[50000:50003] = base[9]
    q = np.concatenate([rng.randn(199, F_RAW).astype(np.float32), base[9:10]])
    bt, qt = torch.from_numpy(base), torch.from_numpy(q)
    D, I = knn.knn_search(bt, qt, 26)
    Dr, Ir, dfull = oknn.calc_knn_exact(base, q, 26)
    check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, dfull)
    D2, I2 = knn.knn_search(bt, qt, 26, fused=False)
    assert torch.equal(I, I2) and torch.equal(D, D2)
    D3, I3 = knn.knn_search(bt, qt, 26, q_block=64, q_chunk=128, c_chunk=8192)
    assert torch.equal(I, I3) and torch.equal(D, D3)
    assert sorted(I[-1, :4].cpu().tolist()) == [9, 50000, 50001, 50002]


@pytest.mark.parametrize("doc_location", [5000, 3200])
def test_export_end_to_end(gpu, tmp_path, doc_location):
    """export on 5 000 rows (1 628-d features, 256-d embeddings): strict (doc_location >= n) and cross.  The .npy lists
    against the fp64 search (ids may swap only between candidates fp32 cannot tell apart, as in test_gpu_knn.check), the
    desimmed ids against the greedy rule on the export's own lists, the text files against the writer on those arrays."""
    from cdml_amd import knn
    n, k, kf, fI_end = 5000, 81, 26, 31
    feats = _clustered(n, F_RAW, 13, gpu).cpu().numpy()
    feats[100:103] = feats[17]                               # exact duplicates in raw-feature space
    emb = _clustered(n, 256, 14, gpu, noise=0.8).cpu().numpy()
    decode = ["g%05d" % i for i in range(n)]
    out = str(tmp_path)
    knn.export(emb, feats, decode, out, doc_location=doc_location, nearest_num=k, desim_nearest_num=kf)
    fD, fI = np.load(os.path.join(out, "fD.npy")), np.load(os.path.join(out, "fI.npy"))
    Dr, Ir, dfull = oknn.calc_knn_exact(feats, nearest_num=kf)
    check(fD, fI, Dr, Ir, dfull)
    cross = doc_location < n
    mode = "cross" if cross else "strict"
    D, I = np.load(os.path.join(out, mode + "D.npy")), np.load(os.path.join(out, mode + "I.npy"))
    if cross:
        v, d = emb[:doc_location], emb[doc_location:]
        a = oknn.calc_knn_exact(d, v, k)
        b = oknn.calc_knn_exact(v, d, k)
        check(D[:doc_location], I[:doc_location] - doc_location, *a)
        check(D[doc_location:], I[doc_location:], *b)
    else:
        check(D, I, *oknn.calc_knn_exact(emb, nearest_num=k))
    Id = np.load(os.path.join(out, mode + "I_desim.npy"))
    assert np.array_equal(Id, greedy_desim(I, fI, fD, 1.4, fI_end))
    if not cross:
        assert (Id[:, 0] == -1).all()
    assert (Id >= 0).sum() > 0.5 * I.size
    ref_dir = os.path.join(out, "rewrite")
    knn.write_knn(ref_dir, D, Id, decode, split_num=10, prefix=mode + "_knn")
    for s in range(10):
        assert open(os.path.join(out, "%s_knn%d" % (mode, s)), "rb").read() == open(os.path.join(ref_dir, "%s_knn%d" % (mode, s)), "rb").read()
    dm, _ = knn.load_decode_map(os.path.join(out, "decode_map.json"))
    assert dm == dict(enumerate(decode))


def test_desim_at_the_reference_scale(gpu):
    """343 455 rows: the raw-feature kNN (1 628-d, k = 26), the embedding kNN (256-d, k = 81), strict desim; a seeded
    sample of 2 000 rows against the greedy rule (rows are independent), the self column -1, inside the time limit."""
    from cdml_amd import knn
    n = 343455
    t0 = time.time()
    feats = _clustered(n, F_RAW, 5, gpu)
    fD, fI = knn.knn_search(feats, feats, 26)
    del feats
    emb = _clustered(n, 256, 6, gpu, noise=0.8)
    eD, eI = knn.knn_search(emb, emb, 81)
    out = knn.desim(eI, fI, fD)
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    assert elapsed < 600, elapsed
    assert (eI[:, 0].cpu().numpy() == np.arange(n)).all() and (out[:, 0] == -1).all().item()
    rows = np.sort(np.random.RandomState(3).choice(n, 2000, replace=False))
    sample = eI[torch.from_numpy(rows).to(gpu)].cpu().numpy()
    want = greedy_desim(sample, fI.cpu().numpy(), fD.cpu().numpy(), 1.4, 31, query_ids=rows)
    assert np.array_equal(out[torch.from_numpy(rows).to(gpu)].cpu().numpy(), want)
    assert 0 < (want[:, 1:] < 0).sum() < want[:, 1:].size      # something removed, something kept
    assert fI.dtype == torch.int64 and (fI[:, 0].cpu().numpy() == np.arange(n)).all()
