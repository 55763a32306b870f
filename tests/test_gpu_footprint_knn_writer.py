"""Write footprint of the two launches of the export's device writer (include/cdml_knn_writer.h, csrc/knn_writer.hip), in the
style of tests/footprint.py: inputs in poisoned, guarded buffers that must come back bit-identical; outputs fully poisoned, every
payload element stored, nothing outside it.  For cdml_knn_line_write the payload is the bytes [off[0], off[n]) of a LARGER
buffer: the bytes in front of off[0] and behind off[n], and the guards, keep their poison -- also when ``off`` gives every row a
shorter extent than its line needs (every store is clipped to the row's own extent)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as fp  # noqa: E402

pytestmark = pytest.mark.gpu

N, K, ROW0, N_GUID = 37, 70, 5, 64           # 37 rows (ten blocks of four waves, the last with one row), columns in both halves of a lane's pair


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import knn, ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.dev = knn, ops, gpu
    return ns


def case():
    rng = np.random.RandomState(2)
    D = np.where(rng.rand(N, K) < 0.8, rng.uniform(0.0, 1.5, size=(N, K)), np.exp(rng.uniform(np.log(1e-9), 0.0, size=(N, K))))
    D = D.astype(np.float32)
    D[3, 5], D[3, 6], D[8, 9] = np.nan, np.inf, -1.0
    I = rng.randint(-1, N_GUID + 3, size=(N, K)).astype(np.int64)              # ids past the table too: never kept
    names = [("g%d" % i) * (1 + i % 4) if i % 9 else "" for i in range(N_GUID)]
    names[7] = "漢字" * 30                                                       # a guid longer than a wave
    return D, I, names


def host_lines(cd, D, I, names):
    """the lines of rows ROW0 .. ROW0 + N - 1, formatted by the host writer (ids past the table dropped first, as the
    kernels drop them)"""
    Ih = np.where(I >= N_GUID, -1, I)
    text = cd.knn._part_text_host(D, Ih, 0, N, names, row0=ROW0)
    return [ln.encode("utf-8") + b"\n" for ln in text.split("\n")[:-1]]


def operands(cd, D, I, names):
    gb, go = cd.knn.guid_table(names, device=cd.dev)
    gD = fp.Guarded((N, K), torch.float32, cd.dev, ld=K + 3).fill_from(torch.from_numpy(D))
    gI = fp.Guarded((N, K), torch.int64, cd.dev, ld=K + 1).fill_from(torch.from_numpy(I))
    gB = fp.Guarded(gb.numel(), torch.uint8, cd.dev).fill_from(gb.view(1, -1))
    gO = fp.Guarded(go.numel(), torch.int64, cd.dev).fill_from(go.view(1, -1))
    return gD, gI, gB, gO


def test_line_sizes_footprint(cd):
    D, I, names = case()
    gD, gI, gB, gO = operands(cd, D, I, names)
    want = np.array([len(b) for b in host_lines(cd, D, I, names)], dtype=np.int64)
    sizes = fp.Guarded(N, torch.int64, cd.dev)
    flags = fp.Guarded(N, torch.int32, cd.dev)

    def launch(pattern):
        sizes.rearm(pattern)
        flags.rearm(pattern)
        cd.ops.knn_line_sizes(gD.view, gI.view, ROW0, gO.view, gB.view.numel(), sizes.view, flags.view)
        torch.cuda.synchronize()
        sizes.assert_guards_intact("sizes")
        flags.assert_guards_intact("flags")
        return {"sizes": sizes.payload(), "flags": flags.payload()}

    with fp.frozen(gD.raw, gI.raw, gB.raw, gO.raw, names=["D", "I", "guid_bytes", "guid_off"]):
        got = fp.assert_fully_written(launch)
    assert np.array_equal(got["sizes"].cpu().numpy(), want)
    assert not got["flags"].any()
    # a kept distance below the routine's range raises the row's flag and only that
    D2 = D.copy()
    D2[11, 1], I[11, 1] = 1e-30, 9
    gD.fill_from(torch.from_numpy(D2))
    gI.fill_from(torch.from_numpy(I))
    got = launch(0)
    assert got["flags"].cpu().tolist() == [int(r == 11) for r in range(N)]


@pytest.mark.parametrize("extents", ["scanned", "short"])
def test_line_write_footprint(cd, extents):
    D, I, names = case()
    gD, gI, gB, gO = operands(cd, D, I, names)
    lines = host_lines(cd, D, I, names)
    sizes = np.array([len(b) for b in lines], dtype=np.int64)
    if extents == "short":
        sizes = sizes // 2                                            # every row's extent holds half its line
        sizes[4] = 0                                                  # ... and one holds nothing
    front, back = 100, 300
    off_h = front + np.concatenate([[0], np.cumsum(sizes)])
    total = int(off_h[-1]) + back
    inside = np.zeros(total, dtype=bool)
    inside[off_h[0]:off_h[-1]] = True
    out = fp.Guarded(total, torch.uint8, cd.dev, mask=torch.from_numpy(inside).view(1, -1))
    gOff = fp.Guarded(N + 1, torch.int64, cd.dev).fill_from(torch.from_numpy(off_h).view(1, -1))

    def launch(pattern):
        out.rearm(pattern)
        cd.ops.knn_line_write(gD.view, gI.view, ROW0, gB.view, gO.view, gOff.view, out.view)
        torch.cuda.synchronize()
        out.assert_guards_intact("out")                               # the guards, and the bytes outside [off[0], off[n])
        return out.payload()

    with fp.frozen(gD.raw, gI.raw, gB.raw, gO.raw, gOff.raw, names=["D", "I", "guid_bytes", "guid_off", "off"]):
        got = fp.assert_fully_written(launch)
    want = b"".join(b[:s] for b, s in zip(lines, sizes.tolist()))     # every line, clipped to its extent
    assert bytes(got["out"].cpu().tolist()) == want and len(want) == int(off_h[-1] - off_h[0])
    if extents == "scanned":
        assert want.count(b"\n") == N and want.count(b"#") > N
