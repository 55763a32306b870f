"""CPU-side checks of the IVF index's update path (include/cdml_ivf_update.h, cdml_amd.knn.IVFIndex.add / remove / locate /
reconstruct / train / reset): header == binding table == library for the two new symbols, every argument error of both entry
points (before any HIP call, with never-dereferenced pointers), the numpy model of tests/ivf_update_ref.py against the stable
argsort of the final catalogue on random ragged cases and against its own single mutations, every refusal by name, the default
``state_dict()`` key lists, and the VGPR ceilings as they were."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_update_ref as ur  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cdml_ivf_lists_move", "cdml_ivf_locate"]


def _lib():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    return _lib, _lib.load_library()


# ---- header == table == library ---------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree():
    _l, lib = _lib()
    text = open(os.path.join(ROOT, "include", "cdml_ivf_update.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_l.SIGNATURES_IVF_UPDATE) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _l.SIGNATURES_IVF_UPDATE[s][1]
        # the table's argument count is the header's
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_l.SIGNATURES_IVF_UPDATE[s][1]), s
    for name in dir(_l):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_IVF_UPDATE":
            assert not set(syms) & set(getattr(_l, name)), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "cdml_ivf_update.h":
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            assert not any(s in other for s in syms), h
    import __graft_entry__ as g
    assert g.IVF_UPDATE_KERNELS == ("k_ivf_lists_move", "k_ivf_locate")
    assert "IVF_UPDATE_KERNELS" in inspect.getsource(g._check_no_scratch) and "SIGNATURES_IVF_UPDATE" in inspect.getsource(g.build)
    assert g.VGPR_CEILINGS == {"k_ivf_scan_pq4": 128}                     # not extended
    rem = os.path.join(ROOT, "build", "obj", "ivf_update.remarks")
    if os.path.exists(rem):                                               # (written when the object was compiled here)
        text = open(rem).read()
        frames = re.findall(r"Function Name: \S*(k_ivf_lists_move|k_ivf_locate)\S*.*?ScratchSize \[bytes/lane\]: (\d+)", text, flags=re.S)
        assert len(frames) == 3 and all(int(b) == 0 for _, b in frames), frames     # the 16-B and 8-B moves, the locate


def test_argument_errors_need_no_gpu():
    _l, lib = _lib()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(264)                                 # 8-B aligned, not 16
    big = 2 ** 31

    def move(old_rows=p, old_ld=16, old_ids=p, old_r_sq=p, n_old=10, old_pos=None, n_kept=10, add_rows=p, add_ld=16, add_r_sq=p,
             n_chunk=6, add_order=p, n_add=5, id0=10, kept_start=p, add_start=p, new_start=p, nlist=3, row_bytes=16, new_rows=p,
             new_ld=16, new_ids=p, new_r_sq=p, n_new=15):
        return lib.cdml_ivf_lists_move(old_rows, old_ld, old_ids, old_r_sq, n_old, old_pos, n_kept, add_rows, add_ld, add_r_sq,
                                       n_chunk, add_order, n_add, id0, kept_start, add_start, new_start, nlist, row_bytes,
                                       new_rows, new_ld, new_ids, new_r_sq, n_new, None)

    def loc(q=p, nq=4, assign=p, n_rows=10, ids=p, n_listed=8, start=p, nlist=3, pos=p):
        return lib.cdml_ivf_locate(q, nq, assign, n_rows, ids, n_listed, start, nlist, pos, None)

    cases = [(move, dict(kept_start=None), b"null"), (move, dict(add_start=None), b"null"), (move, dict(new_start=None), b"null"),
             (move, dict(new_rows=None), b"null"), (move, dict(new_ids=None), b"null"), (move, dict(new_r_sq=None), b"null"),
             (move, dict(old_rows=None), b"null"), (move, dict(old_ids=None), b"null"), (move, dict(old_r_sq=None), b"null"),
             (move, dict(add_rows=None), b"null"), (move, dict(add_r_sq=None), b"null"), (move, dict(add_order=None), b"null"),
             (move, dict(n_new=0), b"positive"), (move, dict(n_new=-1), b"positive"), (move, dict(nlist=0), b"positive"),
             (move, dict(n_old=-1), b"negative"), (move, dict(n_kept=-1), b"negative"), (move, dict(n_chunk=-1), b"negative"),
             (move, dict(n_add=-1), b"negative"), (move, dict(id0=-1), b"negative"),
             (move, dict(n_new=big, n_kept=big - 5, n_old=big - 5), b"too large"), (move, dict(n_old=big), b"too large"),
             (move, dict(n_chunk=big), b"too large"), (move, dict(id0=2 ** 31 - 3), b"too large"),
             (move, dict(n_new=16), b"sizes disagree"), (move, dict(n_add=7, n_kept=8), b"sizes disagree"),
             (move, dict(n_old=9), b"sizes disagree"), (move, dict(n_old=0, old_rows=None, old_ids=None, old_r_sq=None), b"sizes disagree"),
             (move, dict(row_bytes=0), b"multiple of 8"), (move, dict(row_bytes=-8), b"multiple of 8"),
             (move, dict(row_bytes=12), b"multiple of 8"), (move, dict(row_bytes=20), b"multiple of 8"),
             (move, dict(row_bytes=(1 << 20) + 8), b"multiple of 8"),
             (move, dict(new_ld=8), b"stride"), (move, dict(old_ld=8), b"stride"), (move, dict(add_ld=8), b"stride"),
             (move, dict(new_ld=20), b"stride"), (move, dict(old_ld=28), b"stride"), (move, dict(add_ld=36), b"stride"),
             (move, dict(new_rows=odd), b"aligned"), (move, dict(old_rows=odd), b"aligned"), (move, dict(add_rows=odd), b"aligned"),
             (loc, dict(q=None), b"null"), (loc, dict(assign=None), b"null"), (loc, dict(start=None), b"null"),
             (loc, dict(pos=None), b"null"), (loc, dict(ids=None), b"null"),
             (loc, dict(nq=0), b"positive"), (loc, dict(nq=-2), b"positive"), (loc, dict(n_rows=0), b"positive"),
             (loc, dict(nlist=0), b"positive"), (loc, dict(n_listed=-1), b"n_listed"), (loc, dict(n_listed=11), b"n_listed"),
             (loc, dict(nq=big), b"too large"), (loc, dict(n_rows=big, n_listed=8), b"too large")]
    for fn, kw, word in cases:
        rc = fn(**kw)
        msg = lib.cdml_last_error()
        assert rc < 0 and word in msg and (b"ivf_lists_move" if fn is move else b"ivf_locate") in msg, (kw, rc, word, msg)
    # what may be null IS accepted as null by the checks: the call below gets past them all and fails only on its stride
    assert move(n_old=0, n_kept=0, old_rows=None, old_ids=None, old_r_sq=None, n_new=5, new_ld=8) < 0 \
        and b"stride" in lib.cdml_last_error()
    assert move(n_chunk=0, n_add=0, add_rows=None, add_r_sq=None, add_order=None, n_new=10, new_ld=8) < 0 \
        and b"stride" in lib.cdml_last_error()


# ---- the model against the truth and against its mutations -------------------------------------------------------------------
def test_model_is_the_stable_argsort_of_the_final_catalogue():
    rng = np.random.RandomState(0)
    for seed in range(40):
        nlist = int(rng.randint(1, 12))
        old_lens = rng.randint(0, 9, size=nlist) * (rng.rand(nlist) < 0.7)
        add_lens = rng.randint(0, 9, size=nlist) * (rng.rand(nlist) < 0.7)
        if old_lens.sum() + add_lens.sum() == 0:
            add_lens[0] = 1
        for drop in (False, True):
            if drop and old_lens.sum() == 0:
                continue
            c = ur.move_case(seed, tuple(int(v) for v in old_lens), tuple(int(v) for v in add_lens), row_bytes=8, drop=drop,
                             old_unlisted=int(rng.randint(0, 4)), add_unlisted=int(rng.randint(0, 4)))
            assert ur.matches(ur.model_of(c), c), (seed, drop)
            # ids ascend inside every list, and locate inverts them
            for l in range(c["nlist"]):
                seg = c["want_ids"][c["new_start"][l]:c["new_start"][l + 1]]
                assert (np.diff(seg) > 0).all()
            pos = ur.locate(np.arange(len(c["final_assign"])), c["final_assign"], c["want_ids"], c["new_start"])
            listed = c["final_assign"] >= 0
            assert (pos[~listed] == -1).all() and np.array_equal(c["want_ids"][pos[listed]], np.nonzero(listed)[0])


def test_every_single_mutation_of_the_model_is_seen():
    for rb in (8, 24):
        c = ur.move_case(5, row_bytes=rb, drop=True)
        assert c["old_pos"] is not None and len(c["dropped"]) == 4 and ur.matches(ur.model_of(c), c)
        for mutation in ("added_first", "ignore_old_pos", "id_from_sorted"):
            assert not ur.matches(ur.model_of(c, **{mutation: True}), c), mutation
        plain = ur.move_case(5, row_bytes=rb)
        assert plain["old_pos"] is None and ur.matches(ur.model_of(plain), plain)
        assert not ur.matches(ur.model_of(plain, added_first=True), plain)
        assert not ur.matches(ur.model_of(plain, id_from_sorted=True), plain)
        # n_add = 0: a pure removal
        gone = ur.move_case(5, add_lens=(0,) * 9, add_unlisted=0, row_bytes=rb, drop=True)
        assert len(gone["add_order"]) == 0 and ur.matches(ur.model_of(gone), gone)
        assert not ur.matches(ur.model_of(gone, ignore_old_pos=True), gone)
    assert sum(ur.OLD_LENS) == 437 and sum(ur.ADD_LENS) == 326 and len(ur.OLD_LENS) == len(ur.ADD_LENS) == 9
    assert ur.ROW_BYTES == (8, 16, 24, 40, 64, 128, 6016)


# ---- refusals by name, state ---------------------------------------------------------------------------------------------------
def _blank(storage="f32", n_rows=300, bits=8):
    from cdml_amd import knn
    idx = knn.IVFIndex._blank(3, 40, True, "cpu", "f32x3", storage, 8 if storage == "pq" else None, False, bits)
    idx.n_rows, idx.n_listed = n_rows, n_rows
    idx.assign = torch.zeros(n_rows, dtype=torch.int64)
    return idx


def test_refusals_by_name_need_no_gpu():
    _lib()
    from cdml_amd import hardneg, knn
    for storage in ("f32", "f16", "pq"):
        idx = _blank(storage)
        with pytest.raises(ValueError, match="add: row / index dimension mismatch"):
            idx.add(torch.zeros(5, 41))
        with pytest.raises(ValueError, match="add: row / index dimension mismatch"):
            idx.add(np.zeros(40, dtype=np.float32))
        with pytest.raises(ValueError, match="add needs m >= 1"):
            idx.add(torch.zeros(0, 40))
        for b in (0, -4):
            with pytest.raises(ValueError, match="block_rows must be >= 1"):
                idx.add(torch.zeros(5, 40), block_rows=b)
        idx.n_rows = 2 ** 31 - 5
        with pytest.raises(ValueError, match="exceeds 2\\^31 - 1"):
            idx.add(torch.zeros(5, 40))
        idx.n_rows = 300
        for fn in (idx.remove, idx.locate, idx.reconstruct):
            for bad in ([300], [-1], [0, 5, 1000], np.array([2 ** 40])):
                with pytest.raises(ValueError, match="outside \\[0, n_rows = 300\\)"):
                    fn(bad)
            with pytest.raises(ValueError, match="integer vector"):
                fn(torch.zeros(3))
            with pytest.raises(ValueError, match="integer vector"):
                fn(torch.zeros((2, 2), dtype=torch.int64))
        idx.assign[7] = -1
        with pytest.raises(ValueError, match="reconstruct: id 7 is unlisted"):
            idx.reconstruct([3, 7, 9])
        # an index that lists no row: the named error instead of a division by zero
        idx.n_listed = 0
        q = torch.zeros(4, 40)
        for call in (lambda: idx.search(q, 5, 2), lambda: idx.scanned_share(torch.zeros((4, 2), dtype=torch.int64)),
                     lambda: idx.default_seed_probes(10, 2)):
            with pytest.raises(ValueError, match="lists no row.*IVFIndex.add"):
                call()
        with pytest.raises(ValueError, match="k must be in"):              # (the argument checks still come first)
            idx.search(q, 0, 2)
    # load_state_dict(base=None) on a state without lists
    idx = _blank("f32")
    idx.centroids = torch.zeros(3, 40)
    st = idx.state_dict()
    with pytest.raises(ValueError, match="base=None.*carries its lists.*lacks n_rows, ids, list_start, r_sq, rows"):
        knn.IVFIndex.load_state_dict(st)
    with pytest.raises(ValueError, match="base=None.*carries its lists"):
        knn.IVFIndex.load_state_dict(st, None, device="cpu")
    full = dict(st, n_rows=300, ids=torch.zeros(0, dtype=torch.int32), list_start=torch.zeros(4, dtype=torch.int32),
                r_sq=torch.zeros(0), rows=torch.zeros(0, 64))
    with pytest.raises(ValueError, match="storage='f16' needs base="):
        knn.IVFIndex.load_state_dict(full, storage="f16")
    # signatures: all of it is new, nothing old moved
    sig = inspect.signature(knn.IVFIndex.add).parameters
    assert list(sig)[:3] == ["self", "rows", "block_rows"] and sig["block_rows"].default == 1 << 20
    assert list(inspect.signature(knn.IVFIndex.load_state_dict).parameters) == ["state", "base", "device", "storage"]
    assert inspect.signature(knn.IVFIndex.load_state_dict).parameters["base"].default is None
    assert list(inspect.signature(knn.IVFIndex.state_dict).parameters) == ["self", "lists"]
    assert inspect.signature(knn.IVFIndex.state_dict).parameters["lists"].default is False
    build, train = inspect.signature(knn.IVFIndex.build).parameters, inspect.signature(knn.IVFIndex.train).parameters
    assert list(train)[0] == "sample" and list(train)[1:] == list(build)[1:]
    assert [train[k].default for k in list(train)[2:]] == [build[k].default for k in list(build)[2:]]
    assert not {"add", "remove", "block_rows"} & set(inspect.signature(hardneg.mine_lists).parameters)    # (the miner is not taught it)


def test_default_state_dict_keys_are_what_they_were():
    _lib()
    from cdml_amd import knn
    keys = ["centroids", "assign", "l2_norm", "precision", "init_rows", "objective"]
    for storage, bits, residual, want in (("f32", 8, False, keys), ("f16", 8, False, keys + ["storage"]),
                                          ("pq", 8, False, keys + ["storage", "pq_m", "codebooks"]),
                                          ("pq", 8, True, keys + ["storage", "pq_m", "codebooks", "pq_residual"]),
                                          ("pq", 4, False, keys + ["storage", "pq_m", "codebooks", "pq_bits"])):
        # a blank index that has only centroids and assign (and codebooks): the default path touches nothing else
        idx = knn.IVFIndex._blank(3, 8, True, "cpu", "f32x3", storage, 8 if storage == "pq" else None, residual, bits)
        idx.centroids, idx.assign = torch.zeros(3, 8), torch.zeros(10, dtype=torch.int64)
        if storage == "pq":
            idx.codebooks = torch.ones(16, 16, 2) if bits == 4 else torch.ones(8, 256, 4)
        assert list(idx.state_dict()) == want == list(idx.state_dict(lists=False)), (storage, bits)
        # with lists: exactly five more keys, the payload under its own name
        idx.n_rows, idx.ids, idx.list_start, idx.r_sq = 10, torch.zeros(10, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(10)
        payload = "codes" if storage == "pq" else "rows"
        setattr(idx, payload, torch.zeros((10, 8), dtype=torch.uint8) if storage == "pq" else torch.zeros(10, 32))
        st = idx.state_dict(lists=True)
        assert list(st) == want + ["n_rows", "ids", "list_start", "r_sq", payload]
        assert st["n_rows"] == 10 and all(not st[k].is_cuda for k in ("ids", "list_start", "r_sq", payload))


def test_reset_empties_the_lists_and_keeps_the_training():
    _lib()
    from cdml_amd import knn
    for storage, cols, dt in (("f32", 64, torch.float32), ("f16", 64, torch.float16), ("pq", 8, torch.uint8)):
        idx = _blank(storage)
        idx.centroids = torch.ones(3, 40)
        idx.init_rows, idx.train_ids, idx.objective = torch.arange(3), torch.arange(9), torch.ones(4, dtype=torch.float64)
        assert idx.reset() is idx
        assert (idx.n_rows, idx.n_listed, idx.n_unlisted) == (0, 0, 0)
        payload = idx.codes if storage == "pq" else idx.rows
        assert tuple(payload.shape) == (0, cols) and payload.dtype == dt
        assert idx.ids.numel() == idx.r_sq.numel() == idx.assign.numel() == 0 and idx.assign.dtype == torch.int64
        assert torch.equal(idx.list_start, torch.zeros(4, dtype=torch.int32)) and torch.equal(idx.list_len, torch.zeros(3, dtype=torch.int64))
        assert torch.equal(idx.init_rows, torch.arange(3)) and torch.equal(idx.train_ids, torch.arange(9)) and idx.objective.numel() == 4
        assert torch.equal(idx.centroids, torch.ones(3, 40))
        with pytest.raises(ValueError, match="lists no row"):
            idx.search(torch.zeros(2, 40), 1, 1)
        assert idx.locate(torch.zeros(0, dtype=torch.int64)).numel() == 0 and idx.remove(torch.zeros(0, dtype=torch.int64)) == 0
