"""bench.py --dump-outputs without a GPU: a frame up to the size cap is written whole, a larger one as a fixed, seeded
sample of its pixels; and a --steps / --warmup that cannot define the timed region is refused before anything runs."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_the_whole_frame_under_the_cap(tmp_path):
    frame = torch.rand((6, 10, 3), generator=torch.Generator().manual_seed(0))
    paths = bench.dump_outputs(str(tmp_path), frame)
    assert paths == [str(tmp_path / "frame.npy")]
    got = np.load(paths[0])
    assert got.dtype == np.float32 and np.array_equal(got, frame.numpy())


def test_dump_samples_a_frame_over_the_cap(tmp_path):
    frame = torch.arange(200 * 300 * 3, dtype=torch.float64).reshape(200, 300, 3)
    cap = 64 << 10
    paths = bench.dump_outputs(str(tmp_path / "a"), frame, max_bytes=cap)
    assert [os.path.basename(p) for p in paths] == ["frame_sample.npy", "frame_sample_pixels.npy"]
    assert sum(os.path.getsize(p) for p in paths) <= cap
    sample, pixels = np.load(paths[0]), np.load(paths[1])
    assert sample.dtype == np.float64 and pixels.dtype == np.float64 and sample.shape == (len(pixels), 3)
    idx = pixels.astype(np.int64)
    assert len(idx) > 1000 and np.array_equal(idx, pixels) and np.all(np.diff(idx) > 0) and idx[-1] < 200 * 300
    assert np.array_equal(sample, frame.numpy().reshape(-1, 3)[idx])
    # the sample is fixed: another frame of the same size is sampled at the same pixels
    again = bench.dump_outputs(str(tmp_path / "b"), frame * 2, max_bytes=cap)
    assert np.array_equal(np.load(again[1]), pixels) and np.array_equal(np.load(again[0]), 2 * sample)


def test_steps_and_warmup_must_define_a_timed_region():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *bad], capture_output=True,
                           text=True, env=env, timeout=120)
        assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and not r.stdout.strip(), bad
