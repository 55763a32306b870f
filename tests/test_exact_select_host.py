"""The exact-arithmetic selection tests' own footing (tests/exact_select.py), checked without a GPU on the very cases
tests/test_gpu_exact_select.py launches:

* exactness -- every case has passed ``assert_select_exact_safe``, and its distances recomputed in float32, the products
  summed in shuffled orders, the distance formed with and without an fma, give the integer oracle's bits;
* the integer oracles ARE the existing specification: on the same values they agree with oracle.knn.calc_knn_exact and
  oracle.tower.semihard_select (fp64, exact for these inputs), and the streaming model agrees with the one-block oracle;
* sensitivity -- every single mutation of a rule (tie to the larger id, < for <=, > for >=, no clamp, n_valid off by one,
  self / partner not excluded, rows or columns swapped inside a tile, a K tile dropped, a strip of the miner ignored)
  changes the expected output of at least one committed case of every kernel it concerns: the GPU comparison can fail;
* the conditions on the inputs, from the oracle alone: candidate counts within ``cap`` (the small cap below exactly one
  query's), ties across and inside the k-th place, the miner's anchor classes, the rank sweep over all 256 columns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_gemm as xg  # noqa: E402
import exact_select as xs  # noqa: E402

from oracle import knn as oknn, tower as otower  # noqa: E402

# the cases are built inside the tests (and cached in exact_select): collection builds nothing
MERGE_P = [pytest.param(*a, id="%s-%d-%s-%d%s" % (a[0], a[1], "+".join(map(str, a[2])), a[3], "-" + a[5] if a[5] else "")) for a in xs.merge_params()]
FILTER_P = xs.filter_params()
RANK_P = list(xs.RANK_PARAMS)
MINER_P = list(xs.MINER_PARAMS)


class _Lazy:
    """a list of cases built at first use"""
    def __init__(self, make):
        self.make, self.v = make, None

    def __iter__(self):
        if self.v is None:
            self.v = self.make()
        return iter(self.v)


MERGE, FILTER, RANK, MINER = _Lazy(xs.all_merge_cases), _Lazy(xs.all_filter_cases), _Lazy(xs.all_rank_cases), _Lazy(xs.all_miner_cases)


def _same_bits(forms, d_units, unit, what):
    want = xs.from_units(d_units, unit).numpy()
    for i, f in enumerate(forms):
        assert f.dtype == np.float32 and np.array_equal(f.view(np.int32), want.view(np.int32)), "%s: form %d differs" % (what, i)


# ---- exactness -------------------------------------------------------------------------------------------------------------
def test_every_case_is_exact_safe():
    """no case without the check; the bound is 2^24 units, derived in assert_select_exact_safe"""
    cases = list(MERGE) + list(FILTER) + list(RANK) + list(MINER) + [xs.knn_pipeline_case(), xs.rank_pipeline_case(), xs.unit_rows_case(),
                                            xs.nonfinite_knn_case(), xs.nonfinite_rank_case()]
    for c in cases:
        assert 0 < c["safe"] < 2.0 ** 24, c["name"]
    with pytest.raises(AssertionError):                         # a norm below the unit is refused
        xs.assert_select_exact_safe([0.5], [1.0], 1.0, score=np.zeros((1, 1)))
    with pytest.raises(AssertionError):                         # a score that is no multiple of half the unit
        xs.assert_select_exact_safe([1.0], [1.0], 1.0, score=np.full((1, 1), 0.25))
    with pytest.raises(AssertionError):                         # 2^24 units are refused
        xs.assert_select_exact_safe([2.0 ** 23], [2.0 ** 23], 1.0, score=np.ones((1, 1)))
    with pytest.raises(AssertionError):                         # a product term below the accumulator's unit
        xs.assert_select_exact_safe([1.0], [1.0], 1.0, [np.array([[0.25]])], [np.array([[1.0]])], xg.PAIRS1)
    with pytest.raises(AssertionError):                         # 2^17: outside fp16's range
        xs.assert_h2_exact(np.array([64.0]), 2.0 ** 11)
    with pytest.raises(AssertionError):
        xs.assert_h2_exact(np.array([1.0 + 2.0 ** -11]), 1.0)


@pytest.mark.parametrize("order,nq,calls_nb,col0,n_valid,tag", MERGE_P)
def test_merge_cases_fp32_and_model(order, nq, calls_nb, col0, n_valid, tag):
    """d = (qs + bs) - 2 s in float32, every form, is the integer; the streaming model is the one-block oracle"""
    c = xs.merge_case(order, nq, calls_nb, col0, n_valid, tag)
    for x in c["calls"]:
        _same_bits(xs.dist_f32_forms(c["q_sq"], x["b_sq"], x["score"]), x["d"], c["unit"], c["name"])
    d, ids = xs.merge_stream(c)
    for k in xs.MERGE_KS:
        D, I = xs.merge_model(xs.merge_calls(c), k)
        D1, I1 = xs.knn_from_dist(d, ids, k, c["n_valid"])
        assert np.array_equal(D, D1) and np.array_equal(np.where(I == xs.NO_ID, -1, I), I1)


@pytest.mark.parametrize("kind,args", [("filter", a) for a in FILTER_P] + [("rank", a) for a in RANK_P])
def test_plane_cases_fp32_orders(kind, args):
    """the plane product summed in a shuffled k order in float32 (exact_gemm.resum_f32), the distance formed three ways"""
    c = xs.filter_case(*args) if kind == "filter" else xs.rank_case(*args)
    Bp = c["Bp"] if "n" not in c else [x[:c["n"]] for x in c["Bp"]]
    bs = c["b_sq"][:Bp[0].shape[0]]
    K = c["Ap"][0].shape[1]
    for seed in (1, 2):
        s = xg.resum_f32(c["Ap"], Bp, c["pairs"], np.random.RandomState(seed).permutation(K), chunk=16 if seed == 1 else 64)
        _same_bits(xs.dist_f32_forms(c["q_sq"], bs, s, c["scale"]), c["d"], c["unit"], c["name"])
    # the layout: plane gaps and row tails poisoned, the planes where the kernels read them
    for buf, plane, planes in ((c.get("Q"), c.get("plane_q"), c["Ap"]), (c["B"], c["plane_b"], c["Bp"])):
        if buf is None:
            continue
        cols, n_planes = planes[0].shape[1], len(planes)
        assert plane > cols and buf.shape[1] > n_planes * plane and plane % 8 == 0 and buf.shape[1] % 8 == 0
        assert torch.isnan(buf[:, cols:plane].float()).all() and torch.isnan(buf[:, n_planes * plane:].float()).all()
        rows = c.get("n", buf.shape[0])
        for p in range(n_planes):
            assert np.array_equal(buf[:rows, p * plane:p * plane + cols].double().numpy(), planes[p][:rows])
    assert all((p != 0).any() for p in c["Ap"]) and all((p != 0).any() for p in c["Bp"])      # every plane non-zero


def _grid_forms(q, b, d_units, unit, what, scales=(1.0, 1.0)):
    """norms and products of float32 rows (times the fp16 form's scales) in two k orders; the distance three ways"""
    K = q.shape[1]
    sq, sb = scales
    for seed in (3, 4):
        order = np.random.RandomState(seed).permutation(K)
        qs, bs = xs.sqnorm_f32(q, order), xs.sqnorm_f32(b, order)
        acc = xs.grid_score_f32(q * np.float32(sq), b * np.float32(sb), order)
        _same_bits(xs.dist_f32_forms(qs, bs, acc, 1.0 / (sq * sb)), d_units, unit, what)


def test_grid_cases_fp32_orders():
    c = xs.knn_pipeline_case()
    _grid_forms(c["q"], c["b"], c["d"], c["unit"], c["name"])
    _grid_forms(c["q"], c["b"], c["d"], c["unit"], c["name"] + " f16x2", (xs.h2_scale_of(c["q"]), xs.h2_scale_of(c["b"])))
    c = xs.rank_pipeline_case()
    _grid_forms(c["v"], c["v"], c["d"], c["unit"], c["name"])
    _grid_forms(c["v"], c["v"], c["d"], c["unit"], c["name"] + " f16x2", (xs.h2_scale_of(c["v"]),) * 2)
    c = xs.unit_rows_case()
    _grid_forms(c["q"], c["b"], c["d"], c["unit"], c["name"])
    _grid_forms(c["q"], c["b"], c["d"], c["unit"], c["name"] + " f16x2", (xs.h2_scale_of(c["q"]), xs.h2_scale_of(c["b"])))
    for c in MINER:
        E = c["E"].astype(np.float32)
        _grid_forms(E[0::2], E, c["dist"], c["unit"], c["name"])
        _grid_forms(E[0::2], E, c["dist"], c["unit"], c["name"] + " f16x2", (xs.MINER_H2_SCALE,) * 2)


# ---- the integer oracles are the existing specification -----------------------------------------------------------------------
def test_knn_int_is_calc_knn_exact():
    c = xs.knn_pipeline_case()
    for k in xs.KNN_KS:
        D, I = xs.knn_int(c["qi"], c["bi"], k)
        Dr, Ir, _ = oknn.calc_knn_exact(c["b"], c["q"], k, l2_norm=False)
        assert np.array_equal(I, Ir) and np.array_equal(D * c["unit"], Dr)
    D, I = xs.knn_int(c["qi"][:20], c["bi"][:30], 51)           # fewer rows than k: -1 / +inf
    Dr, Ir, _ = oknn.calc_knn_exact(c["b"][:30], c["q"][:20], 51, l2_norm=False)
    assert np.array_equal(I, Ir) and np.array_equal(xs.from_units(D, c["unit"]).double().numpy(), Dr)
    u = xs.unit_rows_case()
    D, I = xs.knn_from_dist(u["d"], np.arange(xs.UNIT_N), xs.UNIT_K)
    Dr, Ir, _ = oknn.calc_knn_exact(u["b"], u["q"], xs.UNIT_K, l2_norm=True)       # (unit rows: the normalisation divides by 1)
    assert np.array_equal(I, Ir) and np.array_equal(D * u["unit"], Dr)


@pytest.mark.parametrize("B,D,videos", MINER_P)
def test_semihard_int_is_the_oracle(B, D, videos):
    c = xs.miner_case(B, D, videos)
    want, dist = otower.semihard_select(c["E"].astype(np.float64), c["rows"])
    assert np.array_equal(dist, c["dist"].astype(np.float64))
    assert np.array_equal(xs.semihard_int(c["E"], c["rows"]), want) and np.array_equal(c["neg"], want)


def test_rank_int_is_the_documented_rule():
    """Evaluation.ranks' docstring: #{j != a, p: d(a, j) < d(a, p), or equal and j < p}, by brute force; the pipeline
    expectation is rank_int on the rows the queries name"""
    c = xs.rank_pipeline_case()
    d = np.maximum(c["d"], 0)
    q = c["cw"][:40]
    want = xs.pipeline_ranks_want(c["d"], q)
    for (a, p), w in zip(q.tolist(), want.tolist()):
        assert w == sum(1 for j in range(xs.RANKP_N) if j not in (a, p) and (d[a, j] < d[a, p] or (d[a, j] == d[a, p] and j < p)))


# ---- the conditions on the inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,n_cols,D,col0,small_cap", FILTER_P)
def test_filter_case_conditions(form, n_cols, D, col0, small_cap):
    c = xs.filter_case(form, n_cols, D, col0, small_cap)
    counts, cap = c["counts"], c["cap"]
    if c["small_cap"]:
        assert int((counts > cap).sum()) == 1, "the small cap is below exactly one query's count"
    else:
        assert counts.max() <= cap
        assert {"inf", "zero", "dup", "stat"} <= set(c["kind"])
        zero = [i for i, t in enumerate(c["kind"]) if t == "zero"]
        assert all(c["tau"][i] == 0 and counts[i] >= 1 for i in zero)
        several = [i for i, t in enumerate(c["kind"]) if t == "dup" and int((c["cands"][i][:, 0] == c["tau"][i]).sum()) >= 2]
        assert len(several) >= 10, "tau equal to several candidates' distance"
    assert (c["n_valid"] - c["col0"]) % 4 and c["n_valid"] < c["col0"] + c["n_cols"]      # n_valid cuts a 4-vector of the last tile
    assert c["nq"] == 300
    ties = sum(1 for i in range(c["nq"]) if c["tau"][i] != xs.INF_I and c["list_d"][i, c["k"] - 1] == c["tau"][i]
               and (c["cands"][i][:, 0] == c["tau"][i]).any())
    assert ties >= 100, "candidates tie with the list's k-th entry"


@pytest.mark.parametrize("form,D", RANK_P)
def test_rank_case_conditions(form, D):
    c = xs.rank_case(form, D)
    a, p = c["a"], c["p"]
    assert c["nq"] >= 512 and c["n"] % 256
    assert set((a % 256).tolist()) == set(range(256)) and set((p % 256).tolist()) == set(range(256))    # every (cb, r, q16) of in_lane
    d = np.maximum(c["d"], 0)
    below = above = dup_anchor = 0
    for i in range(c["nq"]):
        same = np.nonzero((d[i] == c["tau"][i]) & (np.arange(c["n"]) != p[i]) & (np.arange(c["n"]) != a[i]))[0]
        below += int((same < p[i]).any())
        above += int((same > p[i]).any())
        dup_anchor += int(c["tau"][i] == 0)
    assert below >= 4 and above >= 4 and dup_anchor >= 4
    assert (c["d"] < 0).any()
    # the rows behind n_valid are launched as they are in d_pad: finite planes, every one of them (a NaN row would never be
    # counted by a clamp that keeps NaN, whatever n_valid says), and the upper n_valid edge changes counts
    plane, cols = c["plane_b"], c["D"]
    assert c["B"].shape[0] == c["n_pad"] == 768 and c["d_pad"].shape[1] == 768
    for pl in range(len(c["Bp"])):
        assert np.array_equal(c["B"][:, pl * plane:pl * plane + cols].double().numpy(), c["Bp"][pl])
    assert np.isfinite(c["b_sq"]).all()
    assert (xs.rank_int(c["d_pad"], c["a"], c["p"], c["n_pad"])[1] > c["count"]).sum() >= c["nq"] // 4


@pytest.mark.parametrize("B,D,videos", MINER_P)
def test_miner_case_conditions(B, D, videos):
    """anchors of each class.  "Nothing eligible" means every row's video is the anchor's or its positive's: possible only
    with two videos in the batch, so that class is required of the two-video cases (and of every shape through them)."""
    c = xs.miner_case(B, D, videos)
    cl = xs.miner_classes(c)
    for name in ("tied_closest", "eq_dp", "tied_farthest"):
        assert cl[name].any(), name
    assert cl["none"].any() == (c["videos"] == "two")
    assert (c["neg"][cl["none"]] == -1).all() and (c["neg"][~cl["none"]] >= 0).all()


def test_knn_pipeline_conditions():
    c = xs.knn_pipeline_case()
    for k in xs.KNN_KS:
        D, _ = xs.knn_int(c["qi"], c["bi"], k + 1)
        assert int((D[:, k - 1] == D[:, k]).sum()) >= 32, "ties straddling the k-th place"
        assert int((D[:, 1:k] == D[:, :k - 1]).any(1).sum()) > xs.KNN_NQ // 2, "ties inside the top k in most rows"
    k = 51                                                      # the filter path: candidates behind the first block
    D1, _ = xs.knn_int(c["qi"], c["bi"][:xs.KNN_FIRST], k)
    behind = (np.maximum(c["d"][:, xs.KNN_FIRST:], 0) <= D1[:, k - 1:k]).sum(1)
    assert behind.min() >= 1
    assert xs.KNN_FIRST >= 4 * k and xs.KNN_N > 2 * xs.KNN_FIRST   # knn_search's own conditions for the filter path
    # no list overflows in any configuration the GPU tests run (an overflow sends knn_search back through score blocks
    # without a sign: the filter would go untested): the lists' size as knn_search picks it, the counts from the oracle
    u, nf = xs.unit_rows_case(), xs.nonfinite_knn_case()
    for what, d, c_chunk, bad in (("default", c["d"], 1048576, ()), ("c_chunk 512", c["d"], 512, ()),
                                  ("unit rows", u["d"], 1048576, ()), ("non-finite", nf["d"], 1048576, nf["bad"])):
        cap, worst = xs.filter_plan(d, k, xs.KNN_FIRST, c_chunk, bad)
        print("%s: list_cap %d, at most %d candidates per query and launch" % (what, cap, worst))
        assert 1 <= worst <= cap, what
    assert xs.filter_plan(c["d"], k, xs.KNN_FIRST, 1048576)[0] == 1024 and xs.filter_plan(c["d"], k, xs.KNN_FIRST, 512)[0] == 512
    assert xs.UNIT_K == k and xs.UNIT_N > 2 * xs.KNN_FIRST
    D, _ = xs.knn_from_dist(u["d"], np.arange(xs.UNIT_N), xs.UNIT_K + 1)
    assert int((D[:, xs.UNIT_K - 1] == D[:, xs.UNIT_K]).sum()) >= 32, "ties straddling the k-th place"
    assert int((D[:, 1:xs.UNIT_K] == D[:, :xs.UNIT_K - 1]).any(1).sum()) > xs.UNIT_NQ // 2, "ties inside the top k in most rows"


def test_merge_case_conditions():
    assert {c["order"] for c in MERGE} == set(xs.MERGE_ORDERS)
    for order in xs.MERGE_ORDERS:
        got = {(c["nq"], c["calls"][0]["nb"]) for c in MERGE if c["order"] == order and len(c["calls"]) == 1 and c["calls"][0]["col0"] == 0}
        assert {(q, b) for q in xs.MERGE_NQ for b in xs.MERGE_NB} <= got
    assert any(c["n_valid"] % 4 and c["n_valid"] < c["calls"][-1]["col0"] + c["calls"][-1]["nb"] for c in MERGE)
    assert any(c["calls"][0]["col0"] + c["calls"][0]["nb"] - c["n_valid"] >= 256 for c in MERGE), "a whole pass behind n_valid"
    assert any(len(c["calls"]) == 2 for c in MERGE) and any(len(c["calls"]) == 3 for c in MERGE)
    assert any(c["n_valid"] - c["calls"][0]["col0"] < 51 for c in MERGE), "fewer valid rows than k"
    for c in MERGE:
        if c["order"] == "descending":                         # every valid element enters: more than one compaction
            assert all((np.diff(x["d"], axis=1) < 0).all() for x in c["calls"])
        if c["order"] == "negative":
            assert (c["calls"][0]["d"] < 0).any()


# ---- sensitivity: each single mutation changes some committed case of every kernel it concerns ---------------------------------
def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, (tuple, list)) else not np.array_equal(a, b)


def _knn_merge_out(c, k, d=None, **rule):
    dd, ids = xs.merge_stream(c)
    nv = rule.pop("n_valid", c["n_valid"])
    return xs.knn_from_dist(dd if d is None else d, ids, k, nv, **rule)


def _merge_mutations():
    muts = {"tie -> larger id": lambda c, k: _knn_merge_out(c, k, tie_larger=True),
            "no clamp at 0": lambda c, k: _knn_merge_out(c, k, clamp=False),
            "n_valid - 1": lambda c, k: _knn_merge_out(c, k, n_valid=c["n_valid"] - 1),
            "n_valid + 1": lambda c, k: _knn_merge_out(c, k, n_valid=c["n_valid"] + 1)}
    muts["rows r^1"] = lambda c, k: _knn_merge_out(c, k, d=xs.permute_tile(xs.merge_stream(c)[0], "r^1"))
    for kind in ("c^1", "c^4", "c^16"):
        muts["columns " + kind] = lambda c, k, kind=kind: _knn_merge_out(c, k, d=xs.permute_tile(xs.merge_stream(c)[0], kind))
    return muts


def test_mutations_knn_merge():
    for name, mut in _merge_mutations().items():
        assert any(_differs(mut(c, k), _knn_merge_out(c, k)) for c in MERGE for k in xs.MERGE_KS), "no merge case notices: " + name


def _filter_out(c, d=None, **rule):
    nv = rule.pop("n_valid", c["n_valid"])
    return xs.filter_int(c["d"] if d is None else d, c["ids"], c["tau"], nv, **rule)


def _dropped(c, Bp=None):
    Bp = c["Bp"] if Bp is None else Bp
    return xs.plane_dist(c["Ap"], Bp, c["pairs"], c["q_sq"], c["b_sq"][:Bp[0].shape[0]], c["unit"], c["scale"], drop_k=(0, 64))


@pytest.mark.parametrize("form", ["x3", "h2"])
def test_mutations_knn_filter_and_merge_list(form):
    cases = [c for c in FILTER if c["form"] == form]
    muts = {"<= -> < at tau": lambda c: _filter_out(c, strict=True),
            "no clamp at 0": lambda c: _filter_out(c, clamp=False),
            "n_valid - 1": lambda c: _filter_out(c, n_valid=c["n_valid"] - 1),
            "n_valid + 1": lambda c: _filter_out(c, n_valid=c["n_valid"] + 1),
            "a K tile dropped": lambda c: _filter_out(c, d=_dropped(c))}
    for kind in xs.TILE_PERMUTATIONS:
        muts["tile " + kind] = lambda c, kind=kind: _filter_out(c, d=xs.permute_tile(c["d"], kind))
    for name, mut in muts.items():
        assert any(_differs(mut(c), c["cands"]) for c in cases), "no filter case (%s) notices: %s" % (form, name)
    # cdml_knn_merge_list: the order of its keys
    assert any(_differs(xs.merge_lists_int(c["list_d"], c["list_i"], c["cands"], c["k"], tie_larger=True), (c["want_d"], c["want_i"]))
               for c in cases), "no merge-list case notices a tie going to the larger id"
    # ... and it is the exact kNN over the list's rows and the block's (tau is the list's k-th distance)
    for c in cases:
        for i in range(0, c["nq"], 7):
            alld = np.concatenate([c["list_d"][i], np.maximum(c["d"][i], 0)])
            alli = np.concatenate([c["list_i"][i], c["ids"]])
            ok = alli < np.where(np.arange(len(alli)) < xs.LIST, xs.INF_I, c["n_valid"])
            o = np.lexsort((alli[ok], alld[ok]))[:c["k"]]
            assert np.array_equal(alld[ok][o], c["want_d"][i]) and np.array_equal(alli[ok][o], c["want_i"][i])


def _rank_out(c, d=None, **rule):
    nv = rule.pop("n_valid", c["n"])
    return xs.rank_int((c["d_pad"] if nv > c["n"] else c["d"]) if d is None else d, c["a"], c["p"], nv, **rule)


@pytest.mark.parametrize("form", ["x3", "h2"])
def test_mutations_rank_count(form):
    cases = [c for c in RANK if c["form"] == form]
    muts = {"tie -> larger id": lambda c: _rank_out(c, tie="larger"),
            "< -> <= at tau": lambda c: _rank_out(c, tie="all"),
            "d < tau only": lambda c: _rank_out(c, tie="none"),
            "no clamp at 0": lambda c: _rank_out(c, clamp=False),
            "n_valid - 1": lambda c: _rank_out(c, n_valid=c["n"] - 1),
            "n_valid + 1": lambda c: _rank_out(c, n_valid=c["n"] + 1),
            "self not excluded": lambda c: _rank_out(c, exclude_self=False),
            "a K tile dropped": lambda c: _rank_out(c, d=_dropped(c, [x[:c["n"]] for x in c["Bp"]]))}
    for kind in xs.TILE_PERMUTATIONS:
        muts["tile " + kind] = lambda c, kind=kind: _rank_out(c, d=xs.permute_tile(c["d"], kind))
    for name, mut in muts.items():
        assert any(_differs(mut(c), (c["tau"], c["count"])) for c in cases), "no rank case (%s) notices: %s" % (form, name)
    # "partner not excluded" alone is the identity on EVERY input: the partner's own distance is tau and its id is not
    # below itself, so the rule's tie term never counts it.  The exclusion is what holds once the tie term is wrong: under
    # "<= at tau" it changes every query's count -- which is how a case can see it.
    for c in cases:
        assert not _differs(_rank_out(c, exclude_partner=False), (c["tau"], c["count"]))
        assert (_rank_out(c, tie="all", exclude_partner=False)[1] == _rank_out(c, tie="all")[1] + 1).all()


def test_mutations_pipelines():
    c = xs.knn_pipeline_case()
    ids = np.arange(xs.KNN_N)
    for k in xs.KNN_KS:
        want = xs.knn_from_dist(c["d"], ids, k)
        assert _differs(xs.knn_from_dist(c["d"], ids, k, tie_larger=True), want)
        assert _differs(xs.knn_from_dist(c["d"], ids, k, n_valid=xs.KNN_N - 1), want)
        assert _differs(xs.knn_from_dist(xs.grid_dist(c["qi"], c["bi"], drop_k=(0, 64)), ids, k), want)
        for kind in xs.TILE_PERMUTATIONS:
            assert _differs(xs.knn_from_dist(xs.permute_tile(c["d"], kind), ids, k), want), kind
    r = xs.rank_pipeline_case()
    q = np.concatenate([r["cw"], r["cw"][:, ::-1]])
    a, p = q[:, 0], q[:, 1]
    want = xs.rank_int(r["d"][a], a, p, xs.RANKP_N)[1]
    for rule in (dict(tie="larger"), dict(tie="all"), dict(tie="none"), dict(exclude_self=False)):
        assert _differs(xs.rank_int(r["d"][a], a, p, xs.RANKP_N, **rule)[1], want), rule
    assert _differs(xs.rank_int(r["d"][a], a, p, xs.RANKP_N - 1)[1], want)
    assert _differs(xs.rank_int(xs.with_zero_row(r["d"], r["vi"])[a], a, p, xs.RANKP_N + 1)[1], want)   # (the zero padding row counted)
    for kind in ("c^1", "c^4", "c^16"):
        assert _differs(xs.rank_int(xs.permute_tile(r["d"], kind)[a], a, p, xs.RANKP_N)[1], want), kind


@pytest.mark.parametrize("B,D", xs.MINER_SHAPES)
def test_mutations_miner(B, D):
    cases = [xs.miner_case(B, D, v) for v in xs.MINER_VIDEOS]
    muts = {"tie -> larger column": lambda c: xs.semihard_from_dist(c["dist"], c["rows"], tie_larger=True),
            "> -> >= at d_p": lambda c: xs.semihard_from_dist(c["dist"], c["rows"], ge=True),
            "a K tile dropped": lambda c: xs.semihard_int(c["E"], c["rows"], drop_k=(0, 64))}
    for kind in xs.TILE_PERMUTATIONS:
        muts["tile " + kind] = lambda c, kind=kind: xs.semihard_from_dist(xs.permute_tile(c["dist"], kind), c["rows"])
    for s in range(2 * B // 64):
        muts["strip %d ignored" % s] = lambda c, s=s: xs.semihard_from_dist(c["dist"], c["rows"], skip_cols=(64 * s, 64 * s + 64))
    for name, mut in muts.items():
        assert any(_differs(mut(c), c["neg"]) for c in cases), "no miner case (B = %d) notices: %s" % (B, name)
    # the planted anchors are the classes they were planted for
    for c in cases:
        cl = xs.miner_classes(c)
        assert cl["eq_dp"][3] and cl["tied_farthest"][5] and c["neg"][5] == 70


# ---- the non-finite cases' expectation ---------------------------------------------------------------------------------------------
def test_nonfinite_expectations():
    c = xs.nonfinite_knn_case()
    assert sorted(c["bad"].tolist()) == [3, 512, 700] and min(c["bad"]) < xs.KNN_FIRST < max(c["bad"])
    for k in xs.KNN_KS:
        D, I = xs.nonfinite_want(c, k)
        assert not np.isin(I.numpy(), c["bad"]).any()
        assert (I[xs.NONFINITE_QUERY] == -1).all() and torch.isinf(D[xs.NONFINITE_QUERY]).all()
        keep = np.arange(xs.KNN_NQ) != xs.NONFINITE_QUERY
        assert (I.numpy()[keep] >= 0).all()
        Df, If = xs.knn_from_dist(xs.knn_pipeline_case()["d"], np.arange(xs.KNN_N), k)
        assert _differs(If[keep], I.numpy()[keep]), "a non-finite row was somebody's neighbour in the finite case"
    r = xs.nonfinite_rank_case()
    assert not np.isin(r["cw"], r["bad"]).any() and len(r["cw"]) >= 290
    q = np.concatenate([r["cw"], r["cw"][:, ::-1]])
    assert _differs(xs.pipeline_ranks_want(r["d"], q, r["bad"]), xs.pipeline_ranks_want(r["d"], q))
