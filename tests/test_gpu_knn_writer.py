"""The device writer of the kNN export on the MI355X (csrc/knn_writer.hip, include/cdml_knn_writer.h; cdml_amd.knn.write_knn(
writer="device")): the files it writes equal the host writer's byte for byte -- on the lists of a probed export, on a hand-made
case with every edge the line rule has, and on 50 000 random distances in one call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_knn_export_ivf import E, F, K, KF, MODES, N, make_data  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def knn(gpu):
    import cdml_amd
    from cdml_amd import knn
    cdml_amd.load_library()
    return knn


def files(out):
    return {f: open(os.path.join(str(out), f), "rb").read() for f in sorted(os.listdir(str(out)))}


def both(knn, tmp_path, D, I, names, split_num, **kw):
    """the files of the two writers; asserts them equal and returns (files, the device writer's stats)"""
    st = {}
    knn.write_knn(str(tmp_path / "host"), D, I, names, split_num=split_num, prefix="p")
    knn.write_knn(str(tmp_path / "device"), D, I, names, split_num=split_num, prefix="p", writer="device", stats=st, **kw)
    h, d = files(tmp_path / "host"), files(tmp_path / "device")
    assert sorted(h) == sorted(d) == sorted("p%d" % s for s in range(split_num))
    for f in h:
        assert h[f] == d[f], (f, h[f][:200], d[f][:200])
    return h, st


@pytest.mark.parametrize("mode", list(MODES))
def test_export_with_the_device_writer_writes_the_host_writers_files(knn, tmp_path, mode):
    emb, feats, names = make_data(N, F, E, 11, 40, 20)
    out = {}
    for writer in ("host", "device"):
        st = {}
        knn.export(emb, feats, names, str(tmp_path / writer), doc_location=MODES[mode], nearest_num=K, desim_nearest_num=KF,
                   split_num=7, nlist=32, nprobe=4, feature_nlist=32, feature_nprobe=4, writer=writer, stats=st)
        out[writer] = files(tmp_path / writer)
        assert st["write"]["writer"] == writer
    assert out["host"] == out["device"] and len(out["host"]) == 6 + 7
    assert st["write"]["host_parts"] == 0 and st["write"]["write_launches"] == 7
    assert sum(b.count(b"#") for f, b in out["device"].items() if f.startswith(mode + "_knn")) > N


def hand_case(n, k, tiny):
    """n rows x k columns with every edge of the line rule; ``tiny``: values below the digit routine's range (rows 3 and 9)"""
    rng = np.random.RandomState(k)
    D = rng.uniform(0.0, 1.39, size=(n, k)).astype(np.float32)
    I = rng.randint(1, n, size=(n, k)).astype(np.int64)
    cols = [c for c in range(1, k)]
    c0, c1 = cols[0], cols[-1]
    I[0, c0], I[1, c0], I[2, c1] = -1, 0, 0                        # no neighbour; catalogue row 0 is never written
    D[4, c0], D[4, c1] = 0.0, -0.25                                # d <= 0
    D[5, c0], D[5, c1] = np.float32(1.4), np.nextafter(np.float32(1.4), np.float32(0))    # >= 1.4 dropped, the float below kept
    D[6, c0], D[6, c1] = np.nan, np.inf
    D[7, c0], D[7, c1] = 1.5, -np.inf
    D[8, c0], D[8, c1] = 1e-5, 9.999e-5                            # scientific layout
    D[10, c0], D[10, c1] = np.float32(1e-4), np.nextafter(np.float32(1e-4), np.float32(1))     # the layout switch
    D[11, c0], D[11, c1] = 2.0 ** -64, 1.0                         # the range's lowest value; "1.0"
    D[12, :] = 2.0                                                 # a row with no kept entry
    I[13, :] = -1                                                  # another one
    D[14, c0], D[14, c1] = 0.5, 0.1
    if tiny:
        D[3, c1] = 1e-30                                           # below the range: the part falls back to the host
        D[9, c0] = 1e-45                                           # a denormal
    D[:, 0] = 0.0                                                  # column 0 is skipped whatever it holds
    return D, I


NAMES = ["plain", "", "é", "漢字-guid", "\U0001f600", "a,b;c d", "x" * 70, "ÿ" * 33]


@pytest.mark.parametrize("k", [2, 128])
@pytest.mark.parametrize("tiny", [False, True])
def test_hand_made_edges(knn, tmp_path, k, tiny):
    n = 23
    D, I = hand_case(n, k, tiny)
    names = [NAMES[i % len(NAMES)] + (str(i) if i % 5 else "") for i in range(n)]
    names[9] = names[14] = ""                                      # empty guids: a row's own, and a neighbour's
    assert "" in names and any(len(s.encode()) > len(s) for s in names)
    h, st = both(knn, tmp_path, D, I, names, 5)                    # parts of 4 rows, the last with the remainder: 7 rows
    assert st["host_parts"] == (2 if tiny else 0)                  # rows 3 and 9: parts 0 and 2
    assert [b.count(b"\n") for b in h.values()] == [4, 4, 4, 4, 7]
    text = b"".join(h["p%d" % s] for s in range(5)).decode("utf-8").split("\n")
    assert text[12] == names[12] + "," and text[13] == names[13] + ","
    if k == 128:                                                   # (k = 2 has one column: the second value of a pair wins)
        assert "#1e-05<" in text[8] and "#9.999e-05<" in text[8] and "#1e-04<" in text[10] and "#0.000100000005<" in text[10]
        assert "#5.421011e-20<" in text[11] and "#1.0<" in text[11] and text[5].count("#1.3999999<") == 1 and "#1.4<" not in text[5]
        assert text[4].count("#") == k - 3 and text[6].count("#") == k - 3 and text[7].count("#") == k - 3
    if tiny:
        assert "#1e-30<" in text[3] and "#1e-45<" in text[9]
    # device tensors go in as they are
    h2, _ = both(knn, tmp_path / "t", torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda(), names, 5)
    assert h2 == h


def test_fewer_rows_than_parts_and_a_dict_decode_map(knn, tmp_path):
    D = np.array([[0.0, 0.25, 0.5], [0.0, 0.5, 1.25], [0.0, 1.0, 0.75]], dtype=np.float32)
    I = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0]])
    h, st = both(knn, tmp_path, D, I, {0: "a", 1: "b", 2: "c"}, 5)
    assert [h["p%d" % s] for s in range(5)] == [b"", b"", b"", b"", b"a,b#0.25<c#0.5<\nb,c#1.25<\nc,b#1.0<\n"]
    assert st["write_launches"] == 1
    with pytest.raises(ValueError, match="names 2 rows"):
        knn.write_knn(str(tmp_path / "x"), D, I, ["a", "b"], writer="device")
    with pytest.raises(ValueError, match="not in decode_map"):
        knn.write_knn(str(tmp_path / "x"), D[:2], np.array([[0, 1, 7], [1, 0, 1]]), ["a", "b"], writer="device")


def test_fifty_thousand_random_distances_in_one_call(knn, tmp_path):
    rng = np.random.RandomState(5)
    n, k = 1000, 51
    D = np.where(rng.rand(n, k) < 0.5, rng.uniform(0.0, 1.5, size=(n, k)), np.exp(rng.uniform(np.log(1e-7), np.log(1.4), size=(n, k))))
    D = D.astype(np.float32)
    I = rng.randint(-1, n, size=(n, k)).astype(np.int64)
    names = ["guid-%d" % (i * 7919) for i in range(n)]
    h, st = both(knn, tmp_path, D, I, names, 1)
    assert st == {"writer": "device", "host_parts": 0, "write_launches": 1}
    assert h["p0"].count(b"#") == int(((I[:, 1:] > 0) & (D[:, 1:] > 0) & (D[:, 1:] < np.float32(1.4))).sum()) > 40000
    # a buffer smaller than the part: the same bytes in row ranges, one launch each
    h2, st2 = both(knn, tmp_path / "small", D, I, names, 3, buffer_bytes=20000)
    assert st2["write_launches"] > 10 and b"".join(h2["p%d" % s] for s in range(3)) == h["p0"]
