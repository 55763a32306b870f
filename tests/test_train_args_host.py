"""train.validate_args on the host: every refusal TrainStep's constructor documents for its arguments, matched on the
message, and what precision "auto" resolves to -- reachable without a device since the validation is one function over
the arguments and a table's row count and dtype."""
import types

import pytest
import torch

from cdml_amd import train

N = 1000


def table(dtype=torch.float32):
    return types.SimpleNamespace(n_rows_global=N, n_rows=N, feature_size=8, data=torch.zeros((1, 8), dtype=dtype))


def validate_args(tab, batch, use_graph=False, **kw):
    """The two device-free halves of the constructor's checks in its order: the arguments, then -- after the device and
    pair-id checks -- the precision for the step's rows."""
    a = train.validate_args(tab, batch, **kw)
    rows = batch * (3 if a.uniform_negatives or kw.get("mode", "uniform") == "uniform" else 2)
    a.precision = train.resolve_precision(tab, rows, a.precision, use_graph, kw.get("exchange"), kw.get("grad_sync"))
    return a


def refused(match, batch=256, dtype=torch.float32, exc=ValueError, **kw):
    with pytest.raises(exc, match=match):
        validate_args(table(dtype), batch, **kw)


HOOK = types.SimpleNamespace(world=2, rank=1)          # stands for an exchange / grad_sync / dist.NPairSync
LISTS = torch.zeros((N, 8), dtype=torch.int32)


@pytest.mark.parametrize("name", ["exchange", "grad_sync", "npair_sync", "train_table"])
def test_negative_lists_refuse_what_is_not_one_gpu_over_a_frozen_catalogue(name):
    refused("negative_lists does not go with %s yet: listed negatives run on one GPU over a frozen catalogue" % name,
            negative_lists=LISTS, **{name: True if name == "train_table" else HOOK})


def test_negative_lists_refusals():
    refused(r"negative_lists does not go with precision 'f16x2' \(its gather has no listed form\)", negative_lists=LISTS,
            precision="f16x2")
    refused("negative_lists goes with a mode that draws a negative .*, not mode 'inbatch'", negative_lists=LISTS, mode="inbatch")
    refused("negative_lists goes with a mode that draws a negative .*, not mode 'npair'", negative_lists=LISTS, mode="npair")
    refused(r"hard_fraction must be in \[0, 1\], got 1.5", negative_lists=LISTS, hard_fraction=1.5)
    for bad in (LISTS.long(), LISTS[:-1], LISTS[0], torch.zeros((N, 1025), dtype=torch.int32)):
        refused(r"negative_lists must be an int32 \[n_rows = 1000, L in \[1, 1024\]\] tensor, got", negative_lists=bad)
    a = validate_args(table(), 128, negative_lists=LISTS.numpy(), hard_fraction="0.25")
    assert a.hard_fraction == 0.25 and a.negative_lists.dtype == torch.int32 and a.precision == "f32x3"
    assert validate_args(table(), 256, mode="npair", uniform_negatives=True, negative_lists=LISTS).uniform_negatives is True


def test_mode_and_optimizer():
    refused("mode must be 'uniform', 'inbatch', 'semihard' or 'npair'", mode="hinge")
    refused("optimizer must be 'adam', 'lars' or 'momentum'", optimizer="sgd")


def test_npair_sync_refusals():
    sync = dict(npair_sync=HOOK, batch_global=512, slot0=256)
    refused("npair_sync goes with mode 'npair' .*, not 'uniform'", **sync)
    for name, kw in (("memory_size", dict(memory_size=256)), ("logq", dict(logq="stream")),
                     ("uniform_negatives", dict(uniform_negatives=True)), ("train_table", dict(train_table=True))):
        refused("npair_sync does not go with %s yet: the data-parallel N-pair loss is the plain in-batch" % name, mode="npair",
                **sync, **kw)
    refused(r"npair_sync over 2 ranks needs batch_global = world x batch = 512 and slot0 = rank x batch = 256 \(got 256 and 256\)",
            mode="npair", npair_sync=HOOK, slot0=256)
    refused(r"needs batch_global = world x batch = 512 and slot0 = rank x batch = 256 \(got 512 and 0\)", mode="npair",
            npair_sync=HOOK, batch_global=512)
    assert validate_args(table(), 256, mode="npair", exchange=HOOK, grad_sync=HOOK, **sync).precision == "f32x3"
    refused("mode 'npair' runs on one GPU unless npair_sync", mode="npair", exchange=HOOK)
    refused("mode 'npair' runs on one GPU unless npair_sync", mode="npair", grad_sync=HOOK)


def test_memory_refusals():
    refused("memory_size > 0 goes with mode 'npair' .*, not 'uniform'", memory_size=256)
    refused("memory_size and memory_start must be >= 0, got -256 and 0", mode="npair", memory_size=-256)
    refused("memory_size and memory_start must be >= 0, got 0 and -1", mode="npair", memory_start=-1)
    # a multiple of the batch and of the precision's tile: 256 pairs on f32x3 and bf16, 64 on f32
    refused(r"memory_size must be a multiple of the batch \(256 pairs\) and of 256 on precision 'f32x3' \(got 384\)", mode="npair",
            memory_size=384)
    refused(r"memory_size must be a multiple of the batch \(64 pairs\) and of 64 on precision 'f32' \(got 96\)", batch=64,
            mode="npair", memory_size=96)
    refused(r"memory_size must be a multiple of the batch \(512 pairs\) and of 256 on precision 'bf16' \(got 768\)", batch=512,
            dtype=torch.float16, mode="npair", memory_size=768)
    a = validate_args(table(), 64, mode="npair", memory_size="128", memory_start="3")
    assert (a.memory_size, a.memory_start, a.precision) == (128, 3, "f32")


def test_logq_refusals():
    refused("logq goes with mode 'npair' .*, not 'inbatch'", mode="inbatch", logq="stream")
    refused("logq must be None, 'stream' or a tensor of one log-probability per video, not 'table'", mode="npair", logq="table")
    for alpha in (0.0, 1.5, -1):
        refused(r"logq_alpha must be in \(0, 1\], got", mode="npair", logq="stream", logq_alpha=alpha)
    for gap in (0.5, float("inf")):
        refused("logq_init_gap must be finite and >= 1, got", mode="npair", logq="stream", logq_init_gap=gap)
    refused(r"a logq table needs one entry per catalogue row \(1000\), got shape \(999,\)", mode="npair", logq=torch.zeros(N - 1))
    refused(r"a logq table needs one entry per catalogue row \(1000\), got shape \(1000, 1\)", mode="npair",
            logq=torch.zeros((N, 1)))
    refused("every entry of the logq table must be a finite float", mode="npair", logq=torch.zeros(N, dtype=torch.int32))
    refused("every entry of the logq table must be a finite float", mode="npair", logq=torch.full((N,), float("-inf")))
    a = validate_args(table(), 256, mode="npair", logq=[-1.0] * N, logq_alpha="0.5")
    assert not a.logq_stream and a.logq.shape == (N,) and a.logq_alpha == 0.5
    assert validate_args(table(), 256, mode="npair", logq="stream", logq_init_gap=1).logq_stream


def test_uniform_negatives_refusals():
    refused("uniform_negatives goes with mode 'npair' .*, not 'uniform'", uniform_negatives=True)
    refused(r"uniform_logq goes with uniform_negatives=True", mode="npair", logq="stream", uniform_logq=-3.0)
    refused(r"uniform_logq goes with a logQ correction \(logq=...\): without one no logit is corrected", mode="npair",
            uniform_negatives=True, uniform_logq=-3.0)
    for bad in (float("inf"), float("nan")):
        refused("uniform_logq must be a finite float, got", mode="npair", uniform_negatives=True, logq="stream", uniform_logq=bad)
    a = validate_args(table(), 256, mode="npair", uniform_negatives=1, logq="stream", uniform_logq="-3")
    assert a.uniform_negatives is True and a.uniform_logq == -3.0


def test_npair_precision_and_tile_rules():
    refused("mode 'npair' does not train the catalogue", mode="npair", train_table=True)
    for p in ("f16x2", "f32x3-3", "fp8"):
        refused("mode 'npair' runs on precision 'f32x3' or 'f32' .* or 'bf16' .*, not %r" % p, mode="npair", precision=p)
    refused("mode 'npair' on precision 'bf16' does not take uniform_negatives", dtype=torch.float16, mode="npair",
            uniform_negatives=True)
    refused("mode 'npair' on precision 'bf16' does not take npair_sync", dtype=torch.float16, mode="npair", npair_sync=HOOK,
            batch_global=512, slot0=256)
    refused(r"mode 'npair' on precision 'f32x3' needs a batch that is a multiple of 256 pairs \(got 128\)", batch=128,
            mode="npair", precision="f32x3")
    refused(r"mode 'npair' on precision 'f32' needs a batch that is a multiple of 64 pairs \(got 96\)", batch=96, mode="npair")
    refused(r"mode 'npair' on precision 'bf16' needs a batch that is a multiple of 256 pairs \(got 128\)", batch=128,
            dtype=torch.float16, mode="npair")
    for t in (0.0, -0.1, float("inf")):
        refused("temperature must be finite and > 0, got", mode="npair", temperature=t)
    assert validate_args(table(), 256, mode="npair", temperature="0.2").temperature == 0.2


def test_precision_and_table_dtype():
    refused("precision must be 'auto', 'f32', 'f32x3', 'f16x2' or 'bf16'", precision="fp8")
    mismatch = "precision 'bf16' goes with an fp16 FeatureTableF16, 'f32' / 'f32x3' with an fp32 table"
    refused(mismatch, precision="bf16")
    for p in ("f32", "f32x3", "f32x3-3", "f16x2"):
        refused(mismatch, dtype=torch.float16, precision=p)
    refused(mismatch, dtype=torch.float16, mode="npair", precision="f32")
    for kw in (dict(use_graph="split"), dict(use_graph=True, exchange=HOOK), dict(use_graph=True, grad_sync=HOOK)):
        refused("precision 'f16x2' replays from a hipGraph on one GPU only", precision="f16x2", **kw)
    assert validate_args(table(), 128, precision="f16x2", use_graph=True, ).precision == "f16x2"
    assert validate_args(table(), 128, precision="f16x2", exchange=HOOK, grad_sync=HOOK).precision == "f16x2"


def test_refusals_keep_the_constructors_order():
    """The argument checks come first and in order; the precision rule is a function of its own, called after the
    constructor's device and pair-id checks."""
    refused("optimizer must be", optimizer="sgd", precision="fp8")
    refused("mode must be", mode="hinge", memory_size=-1)
    refused("negative_lists does not go with", mode="hinge", negative_lists=LISTS, train_table=True)
    assert train.validate_args(table(), 128, precision="fp8").precision == "fp8"         # (refused by resolve_precision)
    assert train.validate_args(table(), 128).precision == "auto" and train.validate_args(table(), 256, mode="npair").precision == "f32x3"
    with pytest.raises(ValueError, match="precision must be 'auto'"):
        train.resolve_precision(table(), 384, "fp8")


@pytest.mark.parametrize("mode,batch,dtype,want", [
    ("uniform", 128, torch.float16, "bf16"), ("npair", 256, torch.float16, "bf16"),
    ("uniform", 128, torch.float32, "f32x3"),       # 384 rows
    ("uniform", 64, torch.float32, "f32"),          # 192 rows
    ("uniform", 100, torch.float32, "f32"),
    ("inbatch", 64, torch.float32, "f32x3"),        # 128 rows
    ("semihard", 96, torch.float32, "f32"),         # 192 rows
    ("npair", 256, torch.float32, "f32x3"), ("npair", 512, torch.float32, "f32x3"),
    ("npair", 128, torch.float32, "f32"),           # 256 rows, but the loss chain's tile is 256 PAIRS
    ("npair", 64, torch.float32, "f32"),
])
def test_auto_precision(mode, batch, dtype, want):
    for auto in ("auto", None):
        assert validate_args(table(dtype), batch, mode=mode, precision=auto).precision == want


def test_auto_precision_counts_three_rows_with_uniform_negatives():
    assert validate_args(table(), 256, mode="npair", uniform_negatives=True).precision == "f32x3"
