"""ptrace --preview: the P6 file pt_ctx_present's bytes go to.  At the frame's own size its payload is the P3 image's numbers,
pixel for pixel; at another size it is tests/present_ref.py's restatement over the frame the same run wrote as floats (--aov's
beauty.pfm is the frame, bit for bit)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import present_ref as ref
import ptlib
from gpudev import pfm_to_framebuffer, read_pfm

pytestmark = pytest.mark.gpu

CLI = os.path.join(ptlib.PKG, "ptrace")


def run(tmp_path, *extra):
    out = tmp_path / "out"
    r = subprocess.run([CLI, "8", "48", "cornell", "--root", ptlib.ROOT, "--seed", "3", "--out", str(out)] + list(extra),
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_preview_is_the_p3_image(tmp_path):
    out = run(tmp_path, "--preview", str(tmp_path / "p.ppm"))
    (p3,) = glob.glob(str(out / "*-.ppm"))
    want = ref.read_p3(p3)
    assert want.shape == (48, 72, 3)
    assert np.array_equal(ref.read_p6(str(tmp_path / "p.ppm")), want)


def test_preview_at_a_size_is_the_restatement(tmp_path):
    out = run(tmp_path, "--preview", str(tmp_path / "p.ppm"), "--preview-size", "32x24", "--aov", "1")
    (beauty,) = glob.glob(str(out / "*-beauty.pfm"))
    frame = pfm_to_framebuffer(read_pfm(beauty))
    table = ref.thresholds(ptlib.product())
    got = ref.read_p6(str(tmp_path / "p.ppm"))
    assert got.shape == (24, 32, 3)
    assert np.array_equal(got, ref.present(table, frame, 72, 48, 32, 24, fmt=ref.RGB8))
    # --exposure reaches the call: doubled, the same frame gives the restatement's doubled bytes
    run(tmp_path, "--preview", str(tmp_path / "q.ppm"), "--preview-size", "32x24", "--exposure", "2", "--no-ppm")
    assert np.array_equal(ref.read_p6(str(tmp_path / "q.ppm")), ref.present(table, frame, 72, 48, 32, 24, exposure=2.0, fmt=ref.RGB8))


def test_preview_options_are_checked(tmp_path):
    for extra in (["--preview-size", "32x24"], ["--preview", "p.ppm", "--preview-size", "32"], ["--preview", "p.ppm", "--exposure", "-1"],
                  ["--preview", "p.ppm", "--gpus", "2"]):
        r = subprocess.run([CLI, "1", "8", "cornell", "--root", ptlib.ROOT] + extra, cwd=str(tmp_path), capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1, (extra, r.stdout + r.stderr)
