"""The IVF index's update path on the device (include/cdml_ivf_update.h; cdml_amd.knn.IVFIndex.add / remove / locate /
reconstruct / train): the move launch against the numpy model of tests/ivf_update_ref.py on random payload bytes, and the two
contracts of DESIGN.md section 9f.6 -- after any sequence of add and remove the index equals, bit for bit, ``from_assignment`` of
the final catalogue with the index's own assign; ``train(sample).add(sample)`` equals ``build(sample)`` in every attribute -- for
every storage.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_update_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("f32", "f16", "pq", "pqr", "pq4")
LISTS = ("ids", "list_start", "list_len", "r_sq", "assign")
COUNTS = ("n_rows", "n_listed", "n_unlisted")


@pytest.fixture(scope="module")
def cd(gpu):
    import cdml_amd
    from cdml_amd import knn, ops
    cdml_amd.load_library()

    class NS:
        pass
    ns = NS()
    ns.knn, ns.ops, ns.dev = knn, ops, gpu
    x, chunk, cent, assign = ur.index_fixture()
    ns.x, ns.chunk, ns.cent, ns.assign = (torch.from_numpy(a) for a in (x, chunk, cent, assign))
    rng = np.random.RandomState(2)
    Dp = 64
    ns.cb = {"pq": torch.from_numpy((0.5 * rng.randn(ur.IDX_PQ_M, 256, Dp // ur.IDX_PQ_M)).astype(np.float32)),
             "pqr": torch.from_numpy((0.2 * rng.randn(ur.IDX_PQ_M, 256, Dp // ur.IDX_PQ_M)).astype(np.float32)),
             "pq4": torch.from_numpy((0.5 * rng.randn(2 * ur.IDX_PQ_M, 16, Dp // (2 * ur.IDX_PQ_M))).astype(np.float32))}
    ns.queries = torch.from_numpy((cent[rng.randint(0, ur.IDX_NLIST, 40)] + 0.3 * rng.randn(40, ur.IDX_D)).astype(np.float32))
    return ns


def _kw(cd, kind):
    if kind == "f32":
        return dict(storage="f32")
    if kind == "f16":
        return dict(storage="f16", l2_norm=False)                         # (so that the 1e6 row overflows fp16)
    return dict(storage="pq", codebooks=cd.cb[kind], pq_residual=kind == "pqr")


def _make(cd, kind):
    return cd.knn.IVFIndex.from_assignment(cd.x, cd.cent, cd.assign, **_kw(cd, kind))


def _rebuilt(cd, idx, catalogue):
    """``from_assignment`` of the final catalogue with the index's own centroids, assign and options: the contract's right side"""
    kw = dict(l2_norm=idx.l2_norm, precision=idx.precision, storage=idx.storage)
    if idx.storage == "pq":
        kw.update(codebooks=idx.codebooks, pq_residual=idx.pq_residual, pq_bits=idx.pq_bits)
    return cd.knn.IVFIndex.from_assignment(catalogue, idx.centroids, idx.assign, **kw)


def _assert_same(a, b, extra=()):
    payload = "codes" if a.storage == "pq" else "rows"
    for name in LISTS + (payload,) + tuple(extra):
        ta, tb = getattr(a, name), getattr(b, name)
        assert ta.dtype == tb.dtype and ta.shape == tb.shape and torch.equal(ta, tb), name
    for name in COUNTS:
        assert getattr(a, name) == getattr(b, name), name


def _assert_same_search(cd, a, b, catalogue):
    Da, Ia = a.search(cd.queries, 10, 3)
    Db, Ib = b.search(cd.queries, 10, 3)
    assert torch.equal(Da, Db) and torch.equal(Ia, Ib) and bool((Ia >= 0).any())
    if a.storage != "f32":
        base = a.prepare(catalogue)
        Da, Ia = a.search(cd.queries, 10, 3, refine=16, base=base)
        Db, Ib = b.search(cd.queries, 10, 3, refine=16, base=base)
        assert torch.equal(Da, Db) and torch.equal(Ia, Ib)


# ---- the launch against the model ----------------------------------------------------------------------------------------------
def _launch(cd, c, add_pad=0):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cd.dev)
    rb, n_new = c["row_bytes"], c["n_new"]
    add_rows = t(c["add_rows"])
    if add_pad:                                                           # the chunk's stride exceeds row_bytes
        wide = torch.full((add_rows.shape[0], rb + add_pad), 0xEE, dtype=torch.uint8, device=cd.dev)
        wide[:, :rb] = add_rows
        add_rows = wide[:, :rb]
        assert add_rows.stride(0) == rb + add_pad
    new_rows = torch.full((n_new, rb), 0xCC, dtype=torch.uint8, device=cd.dev)
    new_ids = torch.full((n_new,), -7, dtype=torch.int32, device=cd.dev)
    new_r_sq = torch.full((n_new,), -1.0, dtype=torch.float32, device=cd.dev)
    cd.ops.ivf_lists_move(t(c["old_rows"]), t(c["old_ids"]), t(c["old_r_sq"]), t(c["old_pos"]), add_rows, t(c["add_r_sq"]),
                          t(c["add_order"]), c["id0"], t(c["kept_start"]), t(c["add_start"]), t(c["new_start"]), new_rows, new_ids,
                          new_r_sq)
    return new_rows.cpu().numpy(), new_ids.cpu().numpy(), new_r_sq.cpu().numpy()


@pytest.mark.parametrize("row_bytes", ur.ROW_BYTES)
def test_move_launch_is_the_model(cd, row_bytes):
    cases = {"append": ur.move_case(1, row_bytes=row_bytes),                                   # old_pos null
             "drop": ur.move_case(2, row_bytes=row_bytes, drop=True),                          # first row, last row, a whole list
             "no_add": ur.move_case(3, add_lens=(0,) * 9, add_unlisted=0, row_bytes=row_bytes, drop=True),
             "chunk_in_no_list": ur.move_case(4, add_lens=(0,) * 9, add_unlisted=3, row_bytes=row_bytes, drop=True),
             "no_old": ur.move_case(5, old_lens=(0,) * 9, old_unlisted=2, row_bytes=row_bytes)}
    assert cases["append"]["old_pos"] is None and len(cases["drop"]["dropped"]) == 4 and len(cases["no_add"]["add_order"]) == 0
    assert len(cases["append"]["add_rows"]) == sum(ur.ADD_LENS) + 3        # chunk rows that are in no list
    for name, c in cases.items():
        want = ur.model_of(c)
        assert ur.matches(want, c), name                                  # (the model is the truth: the host test, restated)
        got = _launch(cd, c, add_pad=24 if (name == "append" and row_bytes in (8, 64)) else 0)
        assert np.array_equal(got[0], want[0]), name
        assert np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), name


def test_move_launch_addresses_past_two_to_the_31_bytes(cd):
    """357 000 old rows of 6 016 B are 2.148 GB: the byte offsets of the last rows pass 2^31 on both sides.  Three lists, a pure
    append; the expected arrays are slices of the inputs put together with torch on the device."""
    dev, rb = cd.dev, 6016
    old_lens, add_lens = (100000, 0, 257000), (5, 7, 20)
    n_old, m = sum(old_lens), sum(add_lens) + 2
    assert n_old * rb > 2 ** 31
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    old_rows = torch.randint(0, 256, (n_old, rb), dtype=torch.uint8, device=dev, generator=g)
    old_r_sq = torch.rand(n_old, device=dev, generator=g)
    old_ids = torch.arange(n_old, dtype=torch.int32, device=dev) * 2
    add_rows = torch.randint(0, 256, (m, rb), dtype=torch.uint8, device=dev, generator=g)
    add_r_sq = torch.rand(m, device=dev, generator=g)
    a_add = torch.tensor([2] * 10 + [-1] + [1] * 7 + [0] * 5 + [-1] + [2] * 10, device=dev)
    order = torch.argsort(torch.where(a_add >= 0, a_add, torch.full_like(a_add, 3)), stable=True)[:m - 2]
    t32 = lambda lens: torch.from_numpy(ur.starts(lens)).to(dev)
    kept_start, add_start = t32(old_lens), t32(add_lens)
    new_start = kept_start + add_start
    n_new = n_old + m - 2
    id0 = 2 * n_old
    new_rows = torch.empty((n_new, rb), dtype=torch.uint8, device=dev)
    new_ids = torch.empty(n_new, dtype=torch.int32, device=dev)
    new_r_sq = torch.empty(n_new, dtype=torch.float32, device=dev)
    cd.ops.ivf_lists_move(old_rows, old_ids, old_r_sq, None, add_rows, add_r_sq, order.to(torch.int32), id0, kept_start, add_start,
                          new_start, new_rows, new_ids, new_r_sq)
    k, s = kept_start.tolist(), add_start.tolist()
    src = torch.cat([torch.cat([torch.arange(k[c], k[c + 1], device=dev), n_old + order[s[c]:s[c + 1]]]) for c in range(3)])
    assert src.numel() == n_new
    assert torch.equal(new_ids, torch.cat([old_ids, id0 + torch.arange(m, dtype=torch.int32, device=dev)])[src])
    assert torch.equal(new_r_sq, torch.cat([old_r_sq, add_r_sq])[src])
    for lo in range(0, n_new, 65536):                                     # (in pieces: no second 2 GB copy)
        part = src[lo:lo + 65536]
        want = torch.where((part < n_old)[:, None], old_rows[part.clamp(max=n_old - 1)], add_rows[(part - n_old).clamp(min=0)])
        assert torch.equal(new_rows[lo:lo + 65536], want), lo


def test_locate_launch_is_the_model(cd):
    c = ur.move_case(6, drop=True)
    n_rows = len(c["final_assign"])
    q = np.concatenate([np.arange(n_rows)[::-1], [3, 3]]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cd.dev)
    pos = torch.full((len(q),), -9, dtype=torch.int32, device=cd.dev)
    cd.ops.ivf_locate(t(q), t(c["final_assign"]), t(c["want_ids"]), t(c["new_start"]), pos)
    assert np.array_equal(pos.cpu().numpy(), ur.locate(q, c["final_assign"], c["want_ids"], c["new_start"]))


# ---- contract 1: add ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_add_equals_from_assignment_of_the_final_catalogue(cd, kind):
    idx = _make(cd, kind)
    before = (idx.centroids.clone(), idx.init_rows.clone(), idx.objective.clone())
    assert idx.n_rows == 300 and idx.n_listed == 298 and int(idx.list_len[ur.IDX_EMPTY_LIST]) == 0
    assert idx.add(cd.chunk) == 300
    cat = torch.cat([cd.x, cd.chunk])
    assert idx.n_rows == 430 and idx.assign.shape[0] == 430 and int(idx.assign[300 + 7]) == -1     # the NaN row: its id is consumed
    assert idx.n_unlisted == (4 if kind == "f16" else 3) and (int(idx.assign[300 + 9]) == -1) == (kind == "f16")
    assert torch.equal(idx.assign[:300].cpu(), cd.assign)                 # old rows keep their hand-made lists
    want = _rebuilt(cd, idx, cat)
    _assert_same(idx, want)
    _assert_same_search(cd, idx, want, cat)
    assert torch.equal(idx.centroids, before[0]) and torch.equal(idx.init_rows, before[1]) and torch.equal(idx.objective, before[2])
    # three adds (130 rows, 1 row, an all-NaN chunk) equal one add of their concatenation; block_rows = 64 equals the default
    one = cd.x[:1] * 0.5
    nans = torch.full((3, ur.IDX_D), float("nan"))
    assert idx.add(one) == 430 and idx.add(nans) == 431 and idx.n_rows == 434
    whole = _make(cd, kind)
    assert whole.add(torch.cat([cd.chunk, one, nans])) == 300
    _assert_same(idx, whole)
    blocks = _make(cd, kind)
    blocks.add(torch.cat([cd.chunk, one, nans]), block_rows=64)
    _assert_same(idx, blocks)
    _assert_same(idx, _rebuilt(cd, idx, torch.cat([cat, one, nans])))
    # numpy and device rows are taken alike
    dev_rows = _make(cd, kind)
    dev_rows.add(cd.chunk.to(cd.dev))
    np_rows = _make(cd, kind)
    np_rows.add(cd.chunk.numpy())
    _assert_same(dev_rows, want)
    _assert_same(np_rows, want)


# ---- contract 2: train + add == build -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "pq4"])
def test_train_then_add_is_build(cd, kind):
    sample = torch.cat([cd.x, cd.chunk])
    assert sample.shape[0] == 430
    kw = dict(iters=3, seed=5)
    if kind == "pq4":
        kw.update(storage="pq", pq_m=ur.IDX_PQ_M, pq_bits=4, pq_iters=2)
    built = cd.knn.IVFIndex.build(sample, ur.IDX_NLIST, **kw)
    extra = ("centroids", "_C", "init_rows", "train_ids", "objective") + (("codebooks", "pq_objective") if kind == "pq4" else ())
    for block_rows in (64, None):
        idx = cd.knn.IVFIndex.train(sample, ur.IDX_NLIST, **kw)
        assert idx.n_rows == idx.n_listed == 0 and idx.ids.numel() == 0 and not bool(idx.list_start.any())
        with pytest.raises(ValueError, match="lists no row.*IVFIndex.add"):
            idx.search(cd.queries, 10, 3)
        assert idx.add(sample, **({} if block_rows is None else {"block_rows": block_rows})) == 0
        _assert_same(idx, built, extra)
        Da, Ia = idx.search(cd.queries, 10, 3)
        Db, Ib = built.search(cd.queries, 10, 3)
        assert torch.equal(Da, Db) and torch.equal(Ia, Ib)


# ---- remove, locate, reconstruct ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_remove_locate_reconstruct(cd, kind):
    idx = _make(cd, kind)
    idx.add(cd.chunk)
    cat = torch.cat([cd.x, cd.chunk])
    ids, start = idx.ids.cpu(), idx.list_start.cpu()
    # locate over all ids is the inverse of ids; -1 for the unlisted ones; reconstruct is what the lists hold
    pos = idx.locate(torch.arange(430))
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (430,)
    listed = (idx.assign >= 0).cpu()
    assert bool((pos.cpu()[~listed] == -1).all()) and torch.equal(ids[pos.cpu()[listed].long()].long(), torch.nonzero(listed).flatten())
    some = torch.nonzero(listed).flatten()[::7]
    rec = idx.reconstruct(some)
    where = idx.locate(some).long()
    held = idx.decode(where) if idx.storage == "pq" else idx.rows[where].float()
    assert rec.dtype == torch.float32 and tuple(rec.shape) == (some.numel(), 64) and torch.equal(rec, held)
    with pytest.raises(ValueError, match="reconstruct: id 17 is unlisted"):
        idx.reconstruct([1, 17])
    # remove: an unlisted id, a duplicate, a list's first and last row, a whole list
    first, last = int(ids[start[0]]), int(ids[start[1] - 1])
    whole = ids[start[2]:start[3]].tolist()
    gone = [17, first, first, last] + whole + [300 + 7]
    n_before = idx.n_listed
    assert idx.remove(gone) == 2 + len(whole)
    assert idx.n_rows == 430 and idx.n_listed == n_before - 2 - len(whole) and int(idx.list_len[2]) == 0
    assert bool((idx.assign[torch.tensor(gone, device=cd.dev)] == -1).all())
    want = _rebuilt(cd, idx, cat)
    _assert_same(idx, want)
    _assert_same_search(cd, idx, want, cat)
    assert idx.remove(gone) == 0                                          # already unlisted: nothing moves
    _assert_same(idx, want)
    _, I = idx.search(cat[listed], 10, ur.IDX_NLIST)                      # every listed row against every list
    assert not bool(torch.isin(I, torch.tensor(gone, device=cd.dev)).any()) and bool((I >= 0).all())
    assert bool((idx.locate(gone) == -1).all())
    # add after remove
    more = cd.x[:33] * 1.25
    assert idx.add(more, block_rows=16) == 430
    cat2 = torch.cat([cat, more])
    want2 = _rebuilt(cd, idx, cat2)
    _assert_same(idx, want2)
    _assert_same_search(cd, idx, want2, cat2)
    # removing everything is allowed; a search then raises the named error; add fills the index again
    assert idx.remove(torch.arange(idx.n_rows, device=cd.dev)) == want2.n_listed
    assert idx.n_listed == 0 and idx.n_rows == 463 and idx.ids.numel() == 0 and not bool(idx.list_start.any())
    assert bool((idx.assign == -1).all())
    with pytest.raises(ValueError, match="lists no row.*IVFIndex.add"):
        idx.search(cd.queries, 10, 3)
    assert idx.add(cd.x[:50]) == 463
    _assert_same(idx, _rebuilt(cd, idx, torch.cat([cat2, cd.x[:50]])))


# ---- the lists travel in the state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "pq"])
def test_state_with_lists_loads_without_a_catalogue(cd, kind):
    idx = _make(cd, kind)
    idx.add(cd.chunk)
    idx.remove([0, 1, 2, 299, 301])
    state = idx.state_dict(lists=True)
    assert all(not v.is_cuda for v in state.values() if torch.is_tensor(v))
    back = cd.knn.IVFIndex.load_state_dict(state)                         # base=None
    _assert_same(idx, back, ("centroids", "_C") + (("codebooks",) if kind == "pq" else ()))
    assert (back.storage, back.l2_norm, back.precision, back.nlist, back.dim) == (idx.storage, idx.l2_norm, idx.precision, idx.nlist, idx.dim)
    Da, Ia = idx.search(cd.queries, 10, 3)
    Db, Ib = back.search(cd.queries, 10, 3)
    assert torch.equal(Da, Db) and torch.equal(Ia, Ib)
    # the default state covers all n_rows ids and loads as before, against the concatenated catalogue
    cat = torch.cat([cd.x, cd.chunk])
    plain = idx.state_dict()
    assert "ids" not in plain and plain["assign"].shape[0] == 430
    _assert_same(idx, cd.knn.IVFIndex.load_state_dict(plain, cat))
    with pytest.raises(ValueError, match="base=None.*carries its lists"):
        cd.knn.IVFIndex.load_state_dict(plain)
