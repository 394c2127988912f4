"""bench.py's command line: a plain run prints the headline fields alone, `--full` is where every other measurement
lives, and `--dump-outputs DIR` writes the timed call's result as float32 .npy files, the same elements every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("cg_checked", "raster_mpix_s", "roofline", "lm_step", "cpu_baseline", "peak_mem")


def _bench():
    import bench
    return bench


def test_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = _bench().parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = _bench().parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_small_array_whole(tmp_path):
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4) / 7
    _bench().dump_outputs(str(tmp_path / "out"), {"x": x})
    got = np.load(tmp_path / "out" / "x.npy")
    assert got.dtype == np.float32 and got.shape == (12,)
    np.testing.assert_array_equal(got, x.reshape(-1).to(torch.float32).numpy())


def test_dump_large_array_fixed_sample(tmp_path, monkeypatch):
    """Over the budget: one element of every stride-long run, the same ones in every call."""
    b = _bench()
    monkeypatch.setattr(b, "MAX_DUMP_ELEMS", 1000)
    n = 2501  # stride 3: 833 whole runs, a 2-element remainder left out
    x = torch.arange(n, dtype=torch.float32)
    b.dump_outputs(str(tmp_path / "a"), {"x": x})
    b.dump_outputs(str(tmp_path / "b"), {"x": x})
    ga, gb = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    np.testing.assert_array_equal(ga, gb)
    assert ga.dtype == np.float32 and ga.shape == (833,) and ga.size <= 1000
    idx = ga.astype(np.int64)  # x holds its own indices
    np.testing.assert_array_equal(idx // 3, np.arange(833))
    assert len(set((idx % 3).tolist())) == 3  # the offsets vary: not a plain stride


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps(tmp_path):
    """A small scene through the real command: the plain line has the headline fields and none of the `--full` ones,
    `steps` is the number asked for, and the dump is the whole float32 iterate."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--P", "2000", "--sh", "1", "--width", "64", "--height", "48", "--s0", "0.03",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-6 * 1e3  # one view
    assert sorted(os.listdir(out)) == ["x.npy"]
    x = np.load(out / "x.npy")
    assert x.dtype == np.float32 and x.ndim == 1 and x.size > 0
    assert np.isfinite(x).all() and np.abs(x).max() > 0
