"""Near-duplicate suppression ("desim") of the kNN export and its text writer (faiss_knn.py:134-305) -- the parts that
need no GPU: the rule restated here against the reference's own iter_desim_mp output, the writer against the reference's
bytes (tests/golden/knn_desim_ref.npz, made by tests/golden/make_golden_knn_desim.py), and the C ABI's argument checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def greedy_desim(eI, fI, fD, thr=1.4, fI_end=31, query_ids=None):
    """The reference's iter_desim_mp as a per-row greedy rule (ids < 0 or >= n_f never kept)."""
    eI = np.asarray(eI, dtype=np.int64)
    fI = np.asarray(fI, dtype=np.int64)
    fD = np.asarray(fD, dtype=np.float32)
    n_f = fI.shape[0]
    thr = np.float32(thr)
    out = np.full(eI.shape, -1, dtype=np.int64)
    for i in range(eI.shape[0]):
        e = eI[i]
        keep = (e >= 0) & (e < n_f)
        for c in range(e.shape[0]):
            if not keep[c]:
                continue
            j = e[c]
            f = fI[j, :fI_end]
            d = fD[j, :fI_end]
            F = set(f[~(d > thr) & (f != j) & (f >= 0)].tolist())
            for c2 in range(c, e.shape[0]):
                if keep[c2] and e[c2] in F:
                    keep[c2] = False
        q = i if query_ids is None else query_ids[i]
        keep &= e != q
        out[i, keep] = e[keep]
    return out


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(os.path.join(golden_dir, "knn_desim_ref.npz"))


@pytest.mark.parametrize("case", ["strict", "cross"])
def test_greedy_rule_is_the_reference_iter_desim_mp(ref, case):
    eI, fI, fD = ref[case + "_eI"], ref[case + "_fI"], ref[case + "_fD"]
    got = greedy_desim(eI, fI, fD, float(ref["threshold"]), int(ref["fI_end"]))
    assert np.array_equal(got, ref[case + "_out"])
    kept = got >= 0
    assert 0 < kept.sum() < (eI >= 0).sum()                   # the case removes something and keeps something


def test_golden_covers_the_threshold_edges(ref):
    thr = np.float32(1.4)
    for case in ("strict", "cross"):
        fD, fI, eI = ref[case + "_fD"], ref[case + "_fI"], ref[case + "_eI"]
        assert (fD == thr).any() and (fD == np.nextafter(thr, np.float32(0))).any() and (fD == np.nextafter(thr, np.float32(3))).any()
        assert (fI < 0).any() and (eI < 0).any() and int(ref["fI_end"]) < fI.shape[1]
    assert (ref["strict_eI"][:, 0] == np.arange(ref["strict_eI"].shape[0])).all()   # strict: column 0 the query
    assert (ref["strict_out"][:, 0] == -1).all()


def test_write_knn_reproduces_the_reference_bytes(ref, tmp_path):
    from cdml_amd import knn
    decode = {int(k): v for k, v in json.loads(str(ref["w_decode"])).items()}
    knn.write_knn(str(tmp_path), ref["w_D"], ref["w_I"], decode, split_num=int(ref["w_split"]), prefix="knn_test")
    names = [str(x) for x in ref["w_names"]]
    assert sorted(os.listdir(tmp_path)) == names
    for i, name in enumerate(names):
        assert open(os.path.join(tmp_path, name), "rb").read() == ref["w_file%d" % i].tobytes(), name
    assert b"#1e-05<" in ref["w_file1"].tobytes()


def test_write_knn_fewer_rows_than_parts(tmp_path):
    """n // split_num == 0: the first parts are empty files, the last holds every row (faiss_knn.py:289-301)."""
    from cdml_amd import knn
    D = np.array([[0.0, 0.25], [0.0, 0.5]], dtype=np.float32)
    I = np.array([[0, 1], [1, 0]])
    knn.write_knn(str(tmp_path), D, I, ["a", "b"], split_num=3, prefix="p")
    assert [open(os.path.join(tmp_path, "p%d" % s)).read() for s in range(3)] == ["", "", "a,b#0.25<\nb,\n"]


def test_load_decode_map(tmp_path):
    from cdml_amd import knn
    p = tmp_path / "decode_map.json"
    p.write_text(json.dumps({"0": "g0", "5": "g5"}))
    dm, em = knn.load_decode_map(str(p))
    assert dm == {0: "g0", 5: "g5"} and em == {"g0": 0, "g5": 5}


def test_desim_abi_exported_and_checks_arguments_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    assert "cdml_knn_desim" in _lib.SIGNATURES and "cdml_knn_desim_prep" in _lib.SIGNATURES
    p = C.c_void_p(4096)
    # prep: null pointer, kp not 32 / 64, fI_end > kp, bad id type
    assert lib.cdml_knn_desim_prep(None, 0, 26, p, 26, 10, 26, 1.4, p, 32, None) == -1
    assert b"null" in lib.cdml_last_error()
    assert lib.cdml_knn_desim_prep(p, 0, 26, p, 26, 10, 26, 1.4, p, 48, None) == -4
    assert b"kp" in lib.cdml_last_error()
    assert lib.cdml_knn_desim_prep(p, 0, 40, p, 40, 10, 33, 1.4, p, 32, None) == -4
    assert b"fI_end" in lib.cdml_last_error()
    assert lib.cdml_knn_desim_prep(p, 2, 26, p, 26, 10, 26, 1.4, p, 32, None) == -1
    # desim: null pointer, ke > 128, kp, strides, misaligned filtered matrix
    assert lib.cdml_knn_desim(None, 81, 10, 81, None, 0, p, 32, 10, p, 81, None) == -1
    assert lib.cdml_knn_desim(p, 129, 10, 129, None, 0, p, 32, 10, p, 129, None) == -4
    assert b"128" in lib.cdml_last_error()
    assert lib.cdml_knn_desim(p, 81, 10, 81, None, 0, p, 16, 10, p, 81, None) == -4
    assert lib.cdml_knn_desim(p, 80, 10, 81, None, 0, p, 32, 10, p, 81, None) == -1
    assert lib.cdml_knn_desim(p, 81, 10, 81, None, 0, C.c_void_p(4100), 32, 10, p, 81, None) == -3
    assert lib.cdml_last_error()


def test_desim_argument_errors_in_python():
    from cdml_amd import knn
    with pytest.raises(ValueError):
        knn.desim(np.zeros((2, 129), np.int64), np.zeros((4, 8), np.int64), np.zeros((4, 8), np.float32))
    with pytest.raises(ValueError):
        knn.desim(np.zeros((2, 8), np.int64), np.zeros((4, 80), np.int64), np.zeros((4, 80), np.float32), fI_end=65)
