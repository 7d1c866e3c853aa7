"""ptrace --adaptive: the PPM is the library call's frame through pt_write_ppm, the --spp-map PFM holds the counts, and the
flag combinations the CLI does not support are refused with a message."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpudev
import ptlib
from gpudev import L, pfm_to_framebuffer, read_pfm  # noqa: F401  (L: fixture)
from test_gpu_adaptive import ADev, scenes  # noqa: F401  (scenes: fixture)

pytestmark = pytest.mark.gpu

CLI = os.path.join(ptlib.PKG, "ptrace")
W, H, CAP, TE = 36, 24, 64, 0.12


def ppm_body(path):
    return np.array(open(path).read().split("255\n", 1)[1].split(), dtype=np.int64)


def test_cli_adaptive_writes_the_librarys_frame_and_the_counts(L, scenes, tmp_path):
    pfm = str(tmp_path / "spp.pfm")
    r = subprocess.run([CLI, str(CAP), str(H), "cornell", "--adaptive", str(TE), "--spp-map", pfm, "--root", ptlib.ROOT, "--seed", "3",
                        "--out", str(tmp_path / "a")], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Adaptive, tile error 0.12:" in r.stdout and "wrote " + pfm in r.stdout
    files = [f for f in os.listdir(tmp_path / "a") if f.endswith(".ppm")]
    assert len(files) == 1
    with ADev(L, scenes["cornell"], W * H) as d:
        want = d.adaptive(gpudev.config(W, H, CAP, backend=ptlib.BACKEND_MEGAKERNEL, seed=3), TE, tile=0)
    ref = str(tmp_path / "ref.ppm")
    img = np.ascontiguousarray(want["img"])
    assert L.pt_write_ppm(ref.encode(), img.ctypes.data_as(C.POINTER(C.c_float)), W, H, CAP, b"cornell", 0) == 0
    assert np.array_equal(ppm_body(tmp_path / "a" / files[0]), ppm_body(ref))
    counts = pfm_to_framebuffer(read_pfm(pfm))
    assert counts.shape == (W * H, 1) and np.array_equal(counts[:, 0], want["spp"].astype(np.float32))
    assert len(np.unique(want["spp"])) >= 2  # (the frame the CLI drew was an adaptive one)


def test_cli_refuses_what_adaptive_does_not_combine_with(tmp_path):
    def run(*args):
        return subprocess.run([CLI, "64", "24", "cornell", "--root", ptlib.ROOT, *args], cwd=str(tmp_path), capture_output=True,
                              text=True, timeout=60)

    for extra in (("--checkpoint", str(tmp_path / "x.ptacc")), ("--noise-target", "0.1")):
        r = run("--adaptive", "0.1", *extra)
        assert r.returncode != 0 and "--adaptive cannot be combined with --checkpoint or --noise-target" in r.stderr, r.stderr
    r = run("--spp-map", str(tmp_path / "m.pfm"))
    assert r.returncode != 0 and "need --adaptive" in r.stderr
    r = run("--adaptive", "0.1", "--tile", "7")
    assert r.returncode != 0 and "tile must be" in r.stderr
    assert not os.path.exists(tmp_path / "x.ptacc")
