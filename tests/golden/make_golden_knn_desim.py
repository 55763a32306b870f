#!/usr/bin/env python3
"""Generate tests/golden/knn_desim_ref.npz by RUNNING the reference's own faiss_knn.py (near-duplicate suppression
``iter_desim_mp`` and the text writer ``write_knn`` / ``write_process``).

Run in the build container only (``python tests/golden/make_golden_knn_desim.py``); the reference does not exist on
the GPU box and nothing at test time reads it.  Only data (inputs + expected outputs) is written.

faiss_knn.py imports faiss (the HNSW index: not used by the functions run here) and ``tensorflow.flags`` at module
level, so both are stubbed; ``np.int`` (removed from numpy) is restored as ``int`` for ``add_invalid_row``.  The
writer's workers read a module global ``DECODE_MAP`` that the reference's ``main`` only binds locally: it is set on the
module before the call.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_faiss_knn():
    sys.modules["faiss"] = types.ModuleType("faiss")
    tf = types.ModuleType("tensorflow")
    flags = types.ModuleType("tensorflow.flags")

    class _Flags:
        pass
    flags.FLAGS = _Flags()

    def _define(name, default, _doc=None):
        setattr(flags.FLAGS, name, default)
    flags.DEFINE_string = flags.DEFINE_integer = flags.DEFINE_float = flags.DEFINE_bool = _define
    tf.flags = flags
    sys.modules["tensorflow"] = tf
    sys.modules["tensorflow.flags"] = flags
    np.int = int
    sys.path.insert(0, REF)
    import faiss_knn
    return faiss_knn


def _raw_lists(rng, n_f, kf):
    """fI / fD as calc_knn returns them: the row itself first at distance 0, then ascending distances; -1 tails on some
    rows; distances exactly float32(1.4) and one ulp either side of it."""
    thr = np.float32(1.4)
    fI = np.empty((n_f, kf), dtype=np.int64)
    fD = np.empty((n_f, kf), dtype=np.float32)
    for r in range(n_f):
        others = rng.choice(np.delete(np.arange(n_f), r), kf - 1, replace=False)
        fI[r] = np.concatenate([[r], others])
        fD[r] = np.sort(np.concatenate([[0.0], rng.uniform(0.2, 2.0, kf - 1)]).astype(np.float32))
    specials = [thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(3))]
    for r in range(n_f):
        for t in rng.choice(np.arange(1, kf), 3, replace=False):
            fD[r, t] = specials[rng.randint(3)]
        fD[r] = np.sort(fD[r])
    for r in rng.choice(n_f, 4, replace=False):          # -1 tails (catalogue shorter than k)
        cut = rng.randint(kf // 2, kf)
        fI[r, cut:] = -1
        fD[r, cut:] = np.float32(np.finfo(np.float32).max)
    return fI, fD


def _duplicate_pair(fI, fD, a, b):
    """rows a and b exact duplicates: each the other's first neighbour at distance 0"""
    for x, y in ((a, b), (b, a)):
        fI[x] = [x, y] + [i for i in fI[x, 1:] if i != y][:fI.shape[1] - 2]
        fD[x, :2] = 0.0


def _strict_case(rng, n, kf, ke):
    fI, fD = _raw_lists(rng, n, kf)
    _duplicate_pair(fI, fD, 3, 7)
    eI = np.empty((n, ke), dtype=np.int64)
    for r in range(n):                                    # column 0 the query itself (strict mode)
        pool = np.concatenate([fI[r, 1:][fI[r, 1:] >= 0], rng.choice(n, ke, replace=False)])
        cand = [r] + [i for i in dict.fromkeys(pool.tolist()) if i != r]
        eI[r] = cand[:ke]
    eI[3, 1], eI[3, 2] = 7, 11                            # the duplicate pair in one list
    for r in rng.choice(n, 4, replace=False):
        eI[r, rng.randint(ke // 2, ke):] = -1             # -1 tails
    return eI, fI, fD


def _cross_case(rng, n, doc, kf, ke):
    fI, fD = _raw_lists(rng, n, kf)
    _duplicate_pair(fI, fD, 2, doc + 1)
    eI = np.empty((n, ke), dtype=np.int64)
    for r in range(n):                                    # videos list documents, documents list videos: ids global
        side = np.arange(doc, n) if r < doc else np.arange(doc)
        near = [i for i in fI[r, 1:] if i >= 0 and (i >= doc) == (r < doc)]
        rest = [i for i in rng.permutation(side).tolist() if i not in near]
        eI[r] = (near + rest)[:ke]
    for r in rng.choice(n, 3, replace=False):
        eI[r, rng.randint(ke // 2, ke):] = -1
    return eI, fI, fD


def main():
    fk = _import_faiss_knn()
    rng = np.random.RandomState(20190710)
    out = {}
    fI_end = 9                                            # < kf = 12
    eI, fI, fD = _strict_case(rng, 48, 12, 16)
    res = fk.iter_desim_mp(eI.copy(), fI.copy(), fD.copy(), fD_threshold=1.4, fI_end=fI_end, process_num=2)
    out.update(strict_eI=eI, strict_fI=fI, strict_fD=fD, strict_out=np.asarray(res, dtype=np.int64))
    doc = 30
    eI, fI, fD = _cross_case(rng, 50, doc, 12, 16)
    res = fk.iter_desim_mp(eI.copy(), fI.copy(), fD.copy(), fD_threshold=1.4, fI_end=fI_end, process_num=2)
    out.update(cross_eI=eI, cross_fI=fI, cross_fD=fD, cross_out=np.asarray(res, dtype=np.int64), cross_doc=np.int64(doc))
    out["fI_end"] = np.int64(fI_end)
    out["threshold"] = np.float64(1.4)

    # the writer: 11 rows in 3 parts (3, 3, 5 rows), ids 0 and -1, distances 0, float32(1.4), one ulp below it, 1e-05
    n, k = 11, 6
    wI = rng.randint(-1, n, size=(n, k)).astype(np.int64)
    wI[:, 0] = np.arange(n)
    wD = np.sort(rng.uniform(0.0, 1.6, size=(n, k)).astype(np.float32), axis=1)
    wD[:, 0] = 0.0
    wI[1, 2], wD[1, 2] = 0, np.float32(0.5)               # id 0: never written
    wD[2, 1] = 0.0                                        # d == 0: not written
    wD[4, 3] = np.float32(1.4)                            # d == 1.4: not written
    wD[4, 2] = np.nextafter(np.float32(1.4), np.float32(0))
    wD[5, 1] = np.float32(1e-5)
    decode = {i: "guid%03d_%s" % (i, "abcdefghijk"[i]) for i in range(n)}
    fk.DECODE_MAP = decode
    with tempfile.TemporaryDirectory() as tmp:
        fk.write_knn(tmp, split_num=3, D=wD, I=wI, prefix="knn_test")
        names = sorted(os.listdir(tmp))
        assert names == ["knn_test0", "knn_test1", "knn_test2"], names
        files = [open(os.path.join(tmp, f), "rb").read() for f in names]
    out.update(w_D=wD, w_I=wI, w_decode=np.array(json.dumps({str(k): v for k, v in decode.items()})),
               w_names=np.array(names), w_split=np.int64(3))
    for i, b in enumerate(files):
        out["w_file%d" % i] = np.frombuffer(b, dtype=np.uint8)
    path = os.path.join(OUT, "knn_desim_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "strict dropped", int((out["strict_out"] < 0).sum()),
          "cross dropped", int((out["cross_out"] < 0).sum()))


if __name__ == "__main__":
    main()
