"""Host-side logic of bench.py that needs no GPU: the PMC-summary lookup behind `roofline.traffic` withholds a byte count
that was profiled on other kernel sources than the ones this tree holds."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _summary(tmp_path, sha):
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "latest_pmc_x3.csv").write_text(
        'kernel,counter,dispatches,mean_per_launch\n'
        '"k_gemm_bf16_256<true, 3, true, true, false, false, true>",FETCH_SIZE,8,1000.0\n'
        '"k_gemm_bf16_256<true, 3, true, true, false, false, true>",WRITE_SIZE,8,500.0\n'
        '"k_gemm_bf16_256<false, 6, true, true, false, false, true>",FETCH_SIZE,4,300.0\n'
        '"k_gemm_bf16_256<false, 6, true, true, false, false, true>",WRITE_SIZE,4,100.0\n'
        '"k_gemm_f32_sk",FETCH_SIZE,4,700.0\n"k_gemm_f32_sk",WRITE_SIZE,4,70.0\n'
        '"k_gemm_f32_sk_fixup",FETCH_SIZE,4,7.0\n"k_gemm_f32_sk_fixup",WRITE_SIZE,4,3.0\n')
    (prof / "latest_pmc.json").write_text(json.dumps({"latest_pmc_x3": {"date": "d", "commit": "c", "command": "x",
                                                                        "csrc_sha16": sha}}))


def test_pmc_traffic_is_withheld_when_the_kernel_sources_changed(tmp_path, monkeypatch):
    real_root = bench.ROOT
    sha = bench.csrc_hash()
    assert len(sha) == 16 and sha == bench.csrc_hash()
    _summary(tmp_path, sha)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "csrc_hash", lambda: sha)
    # prefix lookup (trailing template arguments left open); FETCH_SIZE doubled (gfx950), KiB -> bytes
    tr, src = bench.pmc_traffic("k_gemm_bf16_256<true, 3, true, true", name="latest_pmc_x3")
    assert tr == (2 * 1000.0 + 500.0) * 1024 and "latest_pmc_x3.csv" in src and "STALE" not in src
    tr, _ = bench.pmc_traffic("k_gemm_bf16_256<false, 6, true, true, false", name="latest_pmc_x3")
    assert tr == (2 * 300.0 + 100.0) * 1024
    # an exact name wins over a longer name that starts with it (round 5: the stream-K launch was reported with its fix-up's bytes)
    assert bench.pmc_traffic("k_gemm_f32_sk", name="latest_pmc_x3")[0] == (2 * 700.0 + 70.0) * 1024
    # a summary of ANOTHER workload is withheld like one of other kernel sources (stamps without a workload: config 1's)
    tr, src = bench.pmc_traffic("k_gemm_bf16_256<true, 3, true, true", name="latest_pmc_x3", workload="rows=10000000 batch=8192 mode=inbatch")
    assert tr is None and "OTHER WORKLOAD" in src
    tr, _ = bench.pmc_traffic("k_gemm_bf16_256<true, 3, true, true", name="latest_pmc_x3", workload="rows=1000000 batch=4096 mode=inbatch")
    assert tr == (2 * 1000.0 + 500.0) * 1024
    # another tree: the same summary is not evidence for its kernels
    monkeypatch.setattr(bench, "csrc_hash", lambda: "0" * 16)
    tr, src = bench.pmc_traffic("k_gemm_bf16_256<true, 3, true, true", name="latest_pmc_x3")
    assert tr is None and "STALE" in src
    # a summary without a stamp (rounds 1-3) is treated the same way
    (tmp_path / "profiles" / "latest_pmc.json").write_text(json.dumps({"latest_pmc_x3": {"date": "d", "commit": "c"}}))
    assert bench.pmc_traffic("k_gemm_bf16_256<true, 3, true, true", name="latest_pmc_x3")[0] is None
    assert bench.pmc_traffic("k_gemm_bf16_256<true, 3", name="no_such_summary") == (None, None)
    assert real_root == ROOT


def test_dump_outputs_writes_float_arrays_and_a_seeded_sample(tmp_path):
    """--dump-outputs: float64 stays float64, everything else is written as float32; an array of more than DUMP_CAP
    elements is written as <name>_sample, the same elements in every run; more than 64 MB in all is refused."""
    import numpy as np
    import pytest
    arrays = {"loss": np.array([0.25]), "ids": np.arange(7, dtype=np.int32),
              "W": np.arange(bench.DUMP_CAP + 1000, dtype=np.float32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == ["W_sample.npy", "ids.npy", "loss.npy"]
    assert np.load(tmp_path / "a" / "loss.npy").dtype == np.float64
    ids = np.load(tmp_path / "a" / "ids.npy")
    assert ids.dtype == np.float32 and np.array_equal(ids, np.arange(7))
    w = np.load(tmp_path / "a" / "W_sample.npy")
    assert w.dtype == np.float32 and w.shape == (bench.DUMP_CAP,) and np.all(np.diff(w) > 0)
    assert np.array_equal(w, np.load(tmp_path / "b" / "W_sample.npy"))
    with pytest.raises(RuntimeError, match="more than"):
        bench.dump_outputs(str(tmp_path / "c"), {"x%d" % i: np.zeros(bench.DUMP_CAP, np.float32) for i in range(4)})
    assert not (tmp_path / "c").exists()                 # refused before anything was written


def test_step_triplets_names_the_negative_of_every_mode():
    """The dumped triplets are (anchor, positive, negative) catalogue rows: uniform negatives as sampled; in-batch the
    positive of triplet (i + shift) mod B (oracle.sampler.device_inbatch); semi-hard the mined row, -1 where none."""
    import types
    import numpy as np
    import torch
    from oracle import sampler as osampler
    B = 6
    pairs = np.stack([np.arange(0, 40, 2), np.arange(1, 40, 2)], 1).astype(np.int32)
    rows, tri, _, s = osampler.device_inbatch(pairs, 1234, 5, B)
    ts = types.SimpleNamespace(mode="inbatch", B=B, R=2 * B, idx=torch.from_numpy(rows), shift=torch.tensor([s], dtype=torch.int32))
    assert np.array_equal(bench.step_triplets(ts).numpy(), rows[tri])
    neg_row = torch.tensor([3, -1, 0, 11, 5, 2], dtype=torch.int32)
    ts = types.SimpleNamespace(mode="semihard", B=B, R=2 * B, idx=torch.from_numpy(rows), neg_row=neg_row)
    got = bench.step_triplets(ts).numpy()
    assert np.array_equal(got[:, :2], rows.reshape(B, 2))
    assert list(got[:, 2]) == [rows[3], -1, rows[0], rows[11], rows[5], rows[2]]
    u = torch.arange(3 * B, dtype=torch.int32)
    ts = types.SimpleNamespace(mode="uniform", B=B, R=3 * B, idx=u)
    assert np.array_equal(bench.step_triplets(ts).numpy(), u.view(B, 3).numpy())


def test_bench_refuses_arguments_it_cannot_honour():
    """--steps sets the number of timed steps (0 is refused, not divided by); --only records have no job outputs to dump.
    Both are refused before anything touches a GPU."""
    import subprocess
    for extra, word in ((["--steps", "0"], "--steps must be >= 1"), (["--only", "f16x2", "--dump-outputs", "out"], "--only records have none")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, r.stderr[-2000:]
