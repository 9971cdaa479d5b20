"""bench.py without a GPU: what --dump-outputs writes (the whole frame, or a fixed seeded sample of it above the budget) and
the argument checks that run before anything touches HIP."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_writes_the_whole_frame_within_budget(tmp_path):
    frame = np.random.RandomState(1).rand(27, 41, 4).astype(np.float32)
    assert bench.write_outputs(str(tmp_path / "d"), frame) == ["frame.npy"]
    got = np.load(tmp_path / "d" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)
    # a 1080p frame fits whole
    assert 1920 * 1080 * 4 * 4 <= bench.DUMP_BUDGET_BYTES <= 64_000_000


def test_dump_samples_a_frame_above_budget_the_same_way_every_time(tmp_path):
    frame = np.random.RandomState(2).rand(120, 100, 4).astype(np.float32)
    budget = 4096 + 24 * 1000
    names = bench.write_outputs(str(tmp_path / "a"), frame, budget=budget)
    assert names == ["frame_sample.npy", "frame_sample_pixel.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= budget
    vals, pix = np.load(tmp_path / "a" / "frame_sample.npy"), np.load(tmp_path / "a" / "frame_sample_pixel.npy")
    assert vals.dtype == np.float32 and pix.dtype == np.float64 and vals.shape == (1000, 4) and pix.shape == (1000,)
    assert np.all(np.diff(pix) > 0) and pix[-1] < 120 * 100
    assert np.array_equal(vals, frame.reshape(-1, 4)[pix.astype(np.int64)])
    bench.write_outputs(str(tmp_path / "b"), frame * 2, budget=budget)
    assert np.array_equal(np.load(tmp_path / "b" / "frame_sample_pixel.npy"), pix)


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--steps" in out.stderr
