"""Hard negatives, host side: the invariants of the draw's host model (tests/hardneg_ref.py), the argument checks of
include/cdml_hardneg.h through the C ABI without a GPU, the refusals of TrainStep, and the torch list filter of
cdml_amd.hardneg against the brute force."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hardneg_ref as ref  # noqa: E402
from oracle import sampler as osampler  # noqa: E402


def _pairs(rng, n_rows, n=64, unique_anchors=False):
    a = rng.permutation(n_rows)[:n] if unique_anchors else rng.integers(0, n_rows, size=n)
    p = (a + 1 + rng.integers(0, n_rows - 1, size=n)) % n_rows
    return np.stack([a, p], 1).astype(np.int32)


def test_draw_with_no_hard_fraction_is_the_uniform_sampler():
    rng = np.random.default_rng(0)
    n_rows, L = 500, 8
    pairs = _pairs(rng, n_rows)
    lists = rng.integers(0, n_rows, size=(n_rows, L)).astype(np.int32)
    for step in (0, 3, 2 ** 32 + 5):
        got, kind = ref.listed_triplets(pairs, n_rows, 99, step, 48, lists, L, 0.0, slot0=48, batch_global=96)
        want = osampler.device_triplets(pairs, n_rows, 99, step, 48, slot0=48, batch_global=96)
        assert np.array_equal(got, want) and not kind.any()


def test_draw_from_empty_lists_is_the_uniform_sampler():
    rng = np.random.default_rng(1)
    n_rows, L = 500, 4
    pairs = _pairs(rng, n_rows)
    lists = np.full((n_rows, L), -1, dtype=np.int32)
    for h in (0.5, 1.0):
        got, kind = ref.listed_triplets(pairs, n_rows, 7, 2, 64, lists, L, h)
        assert np.array_equal(got, osampler.device_triplets(pairs, n_rows, 7, 2, 64)) and not kind.any()


def test_list_of_anchor_and_positive_falls_through_and_a_real_entry_is_taken():
    rng = np.random.default_rng(2)
    n_rows, L = 300, 4
    pairs = _pairs(rng, n_rows, 32, unique_anchors=True)      # (one list per anchor: a repeated anchor would share it)
    lists = np.full((n_rows, L), -1, dtype=np.int32)
    for a, p in pairs:
        lists[a] = (a, p, a, p)
    got, kind = ref.listed_triplets(pairs, n_rows, 5, 1, 32, lists, L, 1.0)
    assert np.array_equal(got, osampler.device_triplets(pairs, n_rows, 5, 1, 32)) and not kind.any()
    # one candidate that is neither: every hard draw returns it (L = 1: all four positions are column 0)
    cand = ((pairs[:, 0].astype(np.int64) + pairs[:, 1] + 7) % n_rows).astype(np.int32)
    one = np.full((n_rows, 1), -1, dtype=np.int32)
    ok = (cand != pairs[:, 0]) & (cand != pairs[:, 1])
    one[pairs[:, 0], 0] = cand
    got, kind = ref.listed_triplets(pairs, n_rows, 5, 1, 32, one, 1, 1.0)
    for i, (a, p, n) in enumerate(got):
        if ok[i]:
            assert n == cand[i] and kind[i] == 1
    assert ok.sum() >= 30 and kind.sum() == ok.sum()
    # ids outside the catalogue and out-of-catalogue anchors are passed over
    big = np.full((n_rows, 2), n_rows + 3, dtype=np.int32)
    got, kind = ref.listed_triplets(pairs, n_rows, 5, 1, 32, big, 2, 1.0)
    assert np.array_equal(got, osampler.device_triplets(pairs, n_rows, 5, 1, 32)) and not kind.any()
    assert ref.listed_negative(5, 1, 0, n_rows + 9, 3, n_rows, one, 1, 2 ** 32) == \
        (osampler.uniform_negative(5, 1, 0, n_rows + 9, 3, n_rows), 0)


def test_hard_share_follows_the_threshold():
    rng = np.random.default_rng(3)
    n_rows, L = 1000, 16
    pairs = _pairs(rng, n_rows, 512)
    lists = rng.integers(0, n_rows, size=(n_rows, L)).astype(np.int32)
    _, kind = ref.listed_triplets(pairs, n_rows, 11, 0, 512, lists, L, 0.5)
    assert abs(kind.mean() - 0.5) < 5 * np.sqrt(0.25 / 512)             # five standard deviations of a fair coin
    assert ref.hard_threshold(0.0) == 0 and ref.hard_threshold(1.0) == 2 ** 32 and ref.hard_threshold(0.5) == 2 ** 31


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cdml_hardneg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_table_and_library_agree():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib, ops
    lib = _lib.load_library()
    syms = _header_symbols()
    assert syms == sorted(_lib.SIGNATURES_HARDNEG) and len(syms) == 4
    for s in syms:
        assert hasattr(lib, s), s
    assert not set(syms) & set(_lib.SIGNATURES)
    assert ops.hard_threshold(0.5) == 2 ** 31 and ops.hard_threshold(1.0) == 2 ** 32 and ops.hard_threshold(0) == 0
    with pytest.raises(ValueError, match="hard_fraction"):
        ops.hard_threshold(1.5)


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    p = C.c_void_p(256)                                   # never dereferenced: every call below fails its checks first
    T32 = 2 ** 32

    def ids(pairs=p, lists=p, ldl=8, L=8, th=T32, idx=p, n_rows=1000, batch=32):
        return lib.cdml_sample_listed, (pairs, 64, n_rows, 1, 0, None, batch, 0, batch, lists, ldl, L, th, idx, None, None)

    def fused(name, lists=p, ldl=8, L=8, th=T32, n_steps=1, kss=0, kind=None, table=p, x=p, ld=64, xki=False, F=64):
        fn = getattr(lib, name)
        a = (p, 64, 1, 0, None, 32, 0, 32, table, 1000, 64, F, lists, ldl, L, th, p, kind, x, ld, n_steps,
             32 * 3 * ld, 96, kss, None)
        if name.endswith("_x3"):
            a += (p if xki else None, 0)
        return fn, a + (None,)

    cases = [(ids(lists=None), b"lists"), (ids(L=0), b"L = 0"), (ids(L=1025), b"L = 1025"), (ids(ldl=7), b"ldl"),
             (ids(th=T32 + 1), b"hard_thresh"), (ids(pairs=None), b"bad argument"), (ids(idx=None), b"bad argument"),
             (ids(n_rows=2), b"n_rows"), (ids(batch=0), b"bad argument")]
    for name, ld in (("cdml_sample_gather_listed", 64), ("cdml_sample_gather_listed_x3", 192),
                     ("cdml_sample_gather_listed_f16", 64)):
        cases += [(fused(name, ld=ld, lists=None), b"lists"), (fused(name, ld=ld, L=0), b"outside [1, 1024]"),
                  (fused(name, ld=ld, L=2000), b"outside [1, 1024]"), (fused(name, ld=ld, ldl=4), b"ldl"),
                  (fused(name, ld=ld, th=T32 + 1), b"hard_thresh"),
                  (fused(name, ld=ld, n_steps=2, kss=31, kind=p), b"kind_step_stride"),
                  (fused(name, ld=ld, table=None), b"bad argument"), (fused(name, ld=ld, x=None), b"bad argument"),
                  (fused(name, ld=ld, n_steps=65), b"n_steps")]
    for (fn, args), msg in cases:
        rc = fn(*args)
        assert rc == -1, (rc, args)                       # CDML_E_BADARG
        assert msg in lib.cdml_last_error(), (args, lib.cdml_last_error())
    fn, args = fused("cdml_sample_gather_listed", ld=64, F=4000)
    assert fn(*args) < 0 and b"feature size" in lib.cdml_last_error()
    fn, args = fused("cdml_sample_gather_listed_x3", ld=190)
    assert fn(*args) < 0 and b"out_stride" in lib.cdml_last_error()
    fn, args = fused("cdml_sample_gather_listed_x3", ld=192, xki=True)       # plane 64 is no multiple of 256
    assert fn(*args) < 0 and b"x_ki" in lib.cdml_last_error()


def test_train_step_refusals_name_the_argument():
    from cdml_amd import train
    table = types.SimpleNamespace(n_rows_global=1000, data=torch.zeros(1), feature_size=8)
    pairs = torch.zeros((4, 2), dtype=torch.int32)
    lists = torch.full((1000, 8), -1, dtype=torch.int32)
    mk = lambda **kw: train.TrainStep(table, pairs, 256, device="cpu", negative_lists=lists, **kw)
    with pytest.raises(ValueError, match="negative_lists.*f16x2"):
        mk(mode="uniform", precision="f16x2")
    for name in ("exchange", "grad_sync", "npair_sync"):
        with pytest.raises(ValueError, match="negative_lists.*" + name):
            mk(mode="uniform", **{name: object()})
        with pytest.raises(ValueError, match="negative_lists.*" + name):
            mk(mode="npair", uniform_negatives=True, **{name: object()})
    with pytest.raises(ValueError, match="negative_lists.*train_table"):
        mk(mode="uniform", train_table=True)
    for kw in (dict(mode="inbatch"), dict(mode="semihard"), dict(mode="npair")):
        with pytest.raises(ValueError, match="negative_lists.*draws a negative.*%s" % kw["mode"]):
            mk(**kw)
    with pytest.raises(ValueError, match="hard_fraction"):
        mk(mode="uniform", hard_fraction=1.5)
    with pytest.raises(ValueError, match="hard_fraction"):
        mk(mode="uniform", hard_fraction=-0.1)
    for bad in (torch.full((999, 8), -1, dtype=torch.int32), torch.full((1000, 8), -1, dtype=torch.int64),
                torch.full((1000,), -1, dtype=torch.int32), torch.full((1000, 1028), -1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="negative_lists must be"):
            train.TrainStep(table, pairs, 256, device="cpu", negative_lists=bad)
    # the mixed chain's own refusals still come first where they apply
    with pytest.raises(ValueError, match="precision"):
        mk(mode="npair", uniform_negatives=True, precision="bf16")


def _clustered(rng, n, D, n_clusters):
    c = rng.standard_normal((n_clusters, D))
    return c[rng.integers(0, n_clusters, size=n)] + 0.3 * rng.standard_normal((n, D))


@pytest.mark.parametrize("skip_top", [0, 2])
@pytest.mark.parametrize("with_pairs", [False, True])
def test_list_filter_matches_the_brute_force(skip_top, with_pairs):
    """hardneg.filter_lists on the brute force's own neighbour ids == the brute-force lists: self, skip_top, partners in
    both directions, left-packing, padding."""
    from cdml_amd import hardneg
    rng = np.random.default_rng(4)
    n, k = 64, 6
    emb = _clustered(rng, n, 8, 5)
    ids, _ = ref.neighbours(emb, k + skip_top + 1)
    pairs = None
    if with_pairs:
        # partners taken from the neighbour lists themselves, in both orientations, so that the filter has work to do
        fwd = [(i, int(ids[i, 1 + skip_top + (i % 3)])) for i in range(0, n, 2)]
        bwd = [(int(ids[i, 2 + skip_top]), i) for i in range(1, n, 4)]
        pairs = np.asarray(fwd + bwd + [(3, 3), (5, 60)], dtype=np.int32)
    want = ref.mine_lists(emb, k, skip_top, pairs)
    got = hardneg.filter_lists(torch.from_numpy(ids), k, skip_top, None if pairs is None else torch.from_numpy(pairs))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, hardneg.list_width(k)) == (n, 8)
    assert np.array_equal(got.numpy(), want)
    assert (want[:, k:] == -1).all()
    if with_pairs:
        assert (want == -1)[:, :k].sum() >= len(fwd)                     # the filter dropped entries ...
        for a, b in pairs:
            assert b not in want[a] and a not in want[b]                 # ... in both directions
        packed = (want >= 0)
        assert (packed[:, :-1] >= packed[:, 1:]).all()                   # left-packed
    for i in range(n):
        assert i not in want[i]


def test_list_filter_edge_cases():
    from cdml_amd import hardneg
    # a row whose own id is not among its neighbours (exact duplicates ahead of it) loses its farthest neighbour instead
    I = torch.tensor([[1, 2, 3, 0], [1, 0, 2, 3], [0, 1, 3, -1]], dtype=torch.int64)
    got = hardneg.filter_lists(I, 3, 0)
    assert got.tolist() == [[1, 2, 3, -1], [0, 2, 3, -1], [0, 1, 3, -1]]
    assert hardneg.list_width(1) == 4 and hardneg.list_width(16) == 16 and hardneg.list_width(17) == 20
    assert hardneg.empty_lists(5, 3).tolist() == [[-1] * 4] * 5
    with pytest.raises(ValueError):
        hardneg.filter_lists(I, 2, 0)
    with pytest.raises(ValueError):
        hardneg.list_width(0)
