"""ptrace --trace-scale K --retrace: after the frame is filled in through the guides, the pixels the upsampler could not serve are
selected (pt_ctx_select_pixels, weight_max 0) and traced at full size into it (pt_ctx_render_masked).  The image differs from the
one written without the flag in those pixels at most."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import present_ref
import ptlib

pytestmark = pytest.mark.gpu

CLI = os.path.join(ptlib.PKG, "ptrace")
SPP, RES_Y, SEED = 8, 48, 3


def run(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([CLI, str(SPP), str(RES_Y), "mesh", "--root", ptlib.ROOT, "--seed", str(SEED), "--out", str(out)] + list(extra),
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    return r, out


def test_retrace_replaces_the_fallback_pixels_and_nothing_else(tmp_path):
    r0, out0 = run(tmp_path, "plain", "--trace-scale", "2")
    r1, out1 = run(tmp_path, "retraced", "--trace-scale", "2", "--retrace")
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout + r0.stderr + r1.stdout + r1.stderr
    assert "Retraced" not in r0.stdout
    m = re.search(r"Retraced (\d+) of (\d+) pixels", r1.stdout)
    assert m, r1.stdout
    n, total = int(m.group(1)), int(m.group(2))
    (a,), (b,) = glob.glob(str(out0 / "*-.ppm")), glob.glob(str(out1 / "*-.ppm"))
    img0, img1 = present_ref.read_p3(a), present_ref.read_p3(b)
    assert img0.shape == img1.shape == (RES_Y, total // RES_Y, 3)
    assert 0 < n < total
    changed = int((img0 != img1).any(axis=2).sum())
    print("retraced %d of %d pixels, %d of them changed in the 8-bit image" % (n, total, changed))
    assert changed <= n


def test_retrace_needs_trace_scale(tmp_path):
    r, _ = run(tmp_path, "refused", "--retrace")
    assert r.returncode == 1 and "--trace-scale" in r.stderr, r.stdout + r.stderr
