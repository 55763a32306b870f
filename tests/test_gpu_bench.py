"""bench.py at N = 1 as a caller runs it: the plain line times exactly --steps steps and measures nothing else, and
--dump-outputs writes what the last timed step computed, from inputs that are the same in every run with the same
arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_its_outputs(gpu, tmp_path):
    B, steps = 256, 3
    outs, lines = [], []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        lines.append(_bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rows", "40000", "--batch", str(B),
                             "--dump-outputs", d]))
        outs.append({f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    for out in lines:
        assert out["metric"] == "triplets/sec" and out["steps"] == steps and out["ms_per_step"] > 0
        assert abs(out["value"] - B * 1e3 / out["ms_per_step"]) < 1e-3 * out["value"]
        assert not {"gather", "cpu_baseline", "config1", "f16x2", "predict"} & set(out), sorted(out)
    a, b = outs
    # (W1 has 7.5 M elements: more than bench.DUMP_CAP = 2^22, so it is written as a fixed sample of them)
    assert sorted(a) == ["W1_sample", "W2", "b1", "b2", "embeddings", "loss", "triplet_row_ids"]
    assert a["W1_sample"].shape == (1 << 22,) and a["W2"].shape == (5000, 256) and a["embeddings"].shape == (2 * B, 256)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    assert np.abs(np.linalg.norm(a["embeddings"], axis=1) - 1).max() < 1e-5
    # the inputs: the same triplets in both runs; what was computed from them agrees
    t = a["triplet_row_ids"]
    assert t.shape == (B, 3) and np.array_equal(t, b["triplet_row_ids"])
    # in-batch negatives: triplet i's negative is the positive of triplet (i + s) mod B for the step's one shift s
    assert any(np.array_equal(t[:, 2], np.roll(t[:, 1], -s)) for s in range(B))
    assert abs(float(a["loss"][0]) - lines[0]["loss"]) < 1e-6 and abs(float(a["loss"][0] - b["loss"][0])) < 1e-4


@pytest.mark.gpu
def test_predict_line_honours_steps_and_dumps_a_sample(gpu, tmp_path):
    d = str(tmp_path / "p")
    out = _bench(["--gpus", "1", "--mode", "predict", "--rows", "20000", "--steps", "2", "--warmup", "1", "--dump-outputs", d])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    e, rows = np.load(os.path.join(d, "embeddings_sample.npy")), np.load(os.path.join(d, "embeddings_sample_row_ids.npy"))
    assert e.shape == (16384, 256) and e.dtype == np.float32 and rows.dtype == np.float64
    assert np.all(np.diff(rows) > 0) and rows[-1] < 20000
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-5


@pytest.mark.gpu
def test_semihard_dump_names_the_mined_negatives(gpu, tmp_path):
    d = str(tmp_path / "s")
    B = 256
    out = _bench(["--gpus", "1", "--mode", "semihard", "--rows", "40000", "--batch", str(B), "--steps", "2", "--warmup", "1",
                  "--dump-outputs", d])
    assert out["steps"] == 2 and out["config"]["rows_per_triplet"] == 2
    t = np.load(os.path.join(d, "triplet_row_ids.npy"))
    assert t.shape == (B, 3)
    # a mined negative is one of the batch's own rows, never the triplet's anchor or positive video (-1: none found)
    found = t[:, 2] >= 0
    assert found.mean() > 0.9 and np.isin(t[found, 2], t[:, :2]).all()
    assert ((t[found, 2] != t[found, 0]) & (t[found, 2] != t[found, 1])).all()
