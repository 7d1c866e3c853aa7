"""ptrace --trace-scale K: the paths traced at ceil(W/K) x ceil(H/K) and the frame filled in through the guides.  The P3 file it
writes is the one pt_write_ppm makes of tests/upsample_ref.py's restatement over planes rendered in this process with the same
configuration; without the flag the file is the plain frame's, byte for byte."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import gpudev
import present_ref
import ptlib
import upsample_ref as ref
from upsample_ref import F32, I32

pytestmark = pytest.mark.gpu

CLI = os.path.join(ptlib.PKG, "ptrace")
SPP, RES_Y, WIDTH, SEED = 4, 30, 45, 3  # 45 x 30: K = 2 traces 23 x 15, no integer ratio on the width


def run(tmp_path, *extra, want=0):
    out = tmp_path / "out"
    r = subprocess.run([CLI, str(SPP), str(RES_Y), "cornell", "--root", ptlib.ROOT, "--seed", str(SEED), "--out", str(out)] + list(extra),
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == want, r.stdout + r.stderr
    return out


def without_time(path):
    return b"\n".join(ln for ln in open(path, "rb").read().split(b"\n") if not ln.startswith(b"# rendering time"))


@pytest.fixture(scope="module")
def planes():
    """what the CLI's calls write, made here through the C ABI: the plain frame, and the low-resolution colour with the guides of
    both sizes"""
    L = ptlib.product()
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    W, H = WIDTH, RES_Y
    w, h = (W + 1) // 2, (H + 1) // 2

    def frame(dev, wd, ht, color):
        n = wd * ht
        cfg = gpudev.config(wd, ht, SPP, seed=SEED)
        d = dict(color=dev.alloc(n * 12), albedo=dev.alloc(n * 12), normal=dev.alloc(n * 12), depth=dev.alloc(n * 4), oid=dev.alloc(n * 4))
        if color:
            dev.render(cfg, d["color"])
        assert L.pt_ctx_render_aov(dev.ctx, C.byref(cfg), d["albedo"], d["normal"], d["depth"], d["oid"], None) == 0, L.pt_last_error()
        return dict(color=dev.pixels(d["color"], n), albedo=dev.pixels(d["albedo"], n), normal=dev.pixels(d["normal"], n),
                    depth=dev.download(d["depth"], n), oid=dev.download(d["oid"], n, I32))

    with gpudev.Device(L, sc) as dev:
        full = frame(dev, W, H, True)
        lo = frame(dev, w, h, True)
        params = ref.defaults(L)
    return L, (W, H, w, h), full, lo, params


def written_by_the_library(L, tmp_path, name, rgb, W, H):
    path = str(tmp_path / name)
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    assert L.pt_write_ppm(path.encode(), rgb.ctypes.data_as(C.c_void_p), W, H, SPP, b"cornell", 0) == 0
    return path


def test_trace_scale_writes_what_the_restatement_predicts(tmp_path, planes):
    L, (W, H, w, h), full, lo, params = planes
    out = run(tmp_path, "--width", str(W), "--trace-scale", "2")
    (p3,) = glob.glob(str(out / "*-.ppm"))
    exp, wgt = ref.want(W, H, w, h, full, lo, params=params)
    want = written_by_the_library(L, tmp_path, "want.ppm", exp, W, H)
    assert without_time(p3) == without_time(want)
    got = present_ref.read_p3(p3)
    assert got.shape == (H, W, 3)
    # it is a picture of the scene, not the plain frame's bytes: close to the frame traced at full size, and not equal to it
    plain = present_ref.read_p3(written_by_the_library(L, tmp_path, "plain.ppm", full["color"], W, H))
    diff = np.abs(got.astype(np.int64) - plain.astype(np.int64))
    print("mean |upsampled - plain| %.2f of 255, taps found on %.3f of the pixels" % (diff.mean(), (wgt > 0).mean()))
    assert 0 < diff.mean() < 64 and (wgt > 0).mean() > 0.75


def test_without_the_flag_nothing_changes(tmp_path, planes):
    L, (W, H, w, h), full, lo, params = planes
    out = run(tmp_path, "--width", str(W))
    (p3,) = glob.glob(str(out / "*-.ppm"))
    want = written_by_the_library(L, tmp_path, "want.ppm", full["color"], W, H)
    assert without_time(p3) == without_time(want)


def test_trace_scale_combines_with_denoise_and_preview(tmp_path, planes):
    L, (W, H, w, h), full, lo, params = planes
    out = run(tmp_path, "--width", str(W), "--trace-scale", "2", "--denoise", "4", "--preview", str(tmp_path / "p.ppm"))
    assert present_ref.read_p6(str(tmp_path / "p.ppm")).shape == (H, W, 3)
    (dn,) = glob.glob(str(out / "*-denoised.ppm"))
    assert present_ref.read_p3(dn).shape == (H, W, 3)
    # the image itself is the upsampled frame, as without the two
    exp, _ = ref.want(W, H, w, h, full, lo, params=params)
    (p3,) = glob.glob(str(out / "*-.ppm"))
    assert without_time(p3) == without_time(written_by_the_library(L, tmp_path, "want.ppm", exp, W, H))


def test_trace_scale_options_are_checked(tmp_path):
    for extra in (["--trace-scale", "1"], ["--trace-scale", "9"], ["--trace-scale", "x"], ["--trace-scale", "2", "--gpus", "2"],
                  ["--trace-scale", "2", "--checkpoint", "c.bin"], ["--trace-scale", "2", "--noise-target", "0.1"],
                  ["--trace-scale", "2", "--adaptive", "0.1"], ["--trace-scale"]):
        r = subprocess.run([CLI, "1", "8", "cornell", "--root", ptlib.ROOT] + extra, cwd=str(tmp_path), capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1, (extra, r.stdout + r.stderr)
