"""bench.py's plain run and its two options: --dump-outputs DIR writes the last timed frame (so that two builds can be
compared output for output), --full adds the figures that take runs of their own (variants, CPU baseline)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ptlib

sys.path.insert(0, ptlib.ROOT)
import bench  # noqa: E402

pkg = importlib.import_module("path-tracer-rust_amd")
BENCH = os.path.join(ptlib.ROOT, "bench.py")
TINY = ["--steps", "2", "--warmup", "1", "--spp", "8", "--width", "128", "--height", "96"]


def run_bench(args):
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_writes_whole_frames_and_a_fixed_sample_of_large_ones(tmp_path):
    small = torch.arange(64 * 48 * 3, dtype=torch.float32).reshape(-1, 3)
    bench.dump_outputs(str(tmp_path / "small"), small, 12345)
    img = np.load(tmp_path / "small" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (64 * 48, 3) and (img == small.numpy()).all()
    rb = np.load(tmp_path / "small" / "ray_bounces.npy")
    assert rb.dtype == np.float64 and rb.tolist() == [12345.0]

    npix = bench.DUMP_MAX_PIXELS + 1000
    big = torch.rand((npix, 3), generator=torch.Generator().manual_seed(1))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, 1 << 40)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["image_sample.npy", "image_sample_pixels.npy", "ray_bounces.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    idx = np.load(tmp_path / "a" / "image_sample_pixels.npy")
    sample = np.load(tmp_path / "a" / "image_sample.npy")
    assert idx.dtype == np.float64 and sample.dtype == np.float32 and sample.shape == (bench.DUMP_MAX_PIXELS, 3)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < npix
    assert (sample == big.numpy()[idx.astype(np.int64)]).all()
    for f in files:  # the same pixels every run
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()


def test_steps_below_one_is_a_usage_error():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_it_timed(tmp_path):
    """A plain run: the headline only (no variants, no CPU baseline), --steps timed steps, and the last one's frame in DIR -
    the frame whose hash the line reports - equal from run to run."""
    lines = [run_bench(TINY + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for line in lines:
        assert "variants" not in line and "cpu_baseline" not in line
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["metric"] == "ray_bounces_per_sec"
    img = np.load(tmp_path / "a" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (128 * 96, 3)
    assert "%016x" % pkg.image_hash(torch.from_numpy(img)) == lines[0]["config"]["image_hash"]
    assert np.load(tmp_path / "a" / "ray_bounces.npy").tolist() == [float(lines[0]["config"]["ray_bounces_per_frame"])]
    for f in ("image.npy", "ray_bounces.npy"):
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()


@pytest.mark.gpu
def test_full_run_adds_variants_and_cpu_baseline():
    line = run_bench(TINY + ["--full", "--cpu-spp", "1"])
    v = line["variants"]
    assert v["megakernel"]["value"] > 0 and v["wavefront_2_concurrent_pipelines"]["value"] > 0 and v["mesh_json"]["value"] > 0
    assert line["cpu_baseline"]["value"] > 0
