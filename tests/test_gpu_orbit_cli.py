"""ptrace --orbit: the viewport loop of INTEGRATION.md from the command line, the camera moved with pt_ctx_set_camera.  Its frames
are, byte for byte, the ones of the same loop driven through ctypes with pt_ctx_set_scene per frame - the behaviour before
pt_ctx_set_camera existed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpudev
import ptlib
import reproject_ref
from ptlib import PtConfig, PtDenoiseVarParams, PtPresentParams, PtReprojectVarParams, PtStats

pytestmark = pytest.mark.gpu

W, H, SPP, SEED, FRAMES = 48, 32, 2, 5, 3
CLI = os.path.join(ptlib.PKG, "ptrace")
PT_PRESENT_RGB8 = ptlib.abi.PT_PRESENT_RGB8


def cam_dict(cam):
    return {"position": tuple(cam.position), "direction": tuple(cam.direction), "focal_length": cam.focal_length,
            "sensor_width": cam.sensor_width, "aspect_ratio": cam.aspect_ratio}


def loop_with_set_scene(L, sc, step, out_size=None, exposure=0.0):
    """frames 0..FRAMES-1 as RGB8 bytes: pt_ctx_set_scene -> render -> render_aov -> reproject_var -> denoise_var -> present"""
    n = W * H
    ow, oh = out_size or (W, H)
    own = gpudev.Device(L)
    ctx, dev = own.ctx, own.alloc
    # a side: colour, len, moments, depth, object id, normal
    sides = [[dev(n * k * 4) for k in (3, 1, 2, 1, 1, 3)] for _ in range(2)]
    albedo, error, shown, px = dev(n * 12), dev(n * 4), dev(n * 12), dev(ow * oh * 3)
    cfg = PtConfig(W, H, SPP, 0, SEED, 0, 0, 0, 0)
    rp = PtReprojectVarParams(SPP, 0, 0, 0, 0, 0, 0)
    dp = PtDenoiseVarParams(0, 2.0, 0, 0)
    pp = PtPresentParams(out_size[0] if out_size else 0, out_size[1] if out_size else 0, exposure, PT_PRESENT_RGB8, 0)
    frames, hist_cam = [], None
    cur, hist = sides
    try:
        for k in range(FRAMES):
            d = reproject_ref.orbit(cam_dict(sc.cam), k * step)
            cam = ptlib.make_camera(d["position"], d["direction"], d["focal_length"], d["sensor_width"], d["aspect_ratio"])
            st = PtStats()
            own.set_scene(sc, cam)
            assert L.pt_ctx_render(ctx, C.byref(cfg), cur[0], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
            assert L.pt_ctx_render_aov(ctx, C.byref(cfg), albedo, cur[5], cur[3], cur[4], None) == 0, L.pt_last_error()
            h = [hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]] if hist_cam is not None else [None] * 6
            assert L.pt_ctx_reproject_var(ctx, W, H, C.byref(rp), C.byref(cam), cur[0], cur[3], cur[4], cur[5],
                                          C.byref(hist_cam) if hist_cam is not None else None, *h,
                                          cur[0], cur[1], cur[2], error, None) == 0, L.pt_last_error()
            assert L.pt_ctx_denoise_var(ctx, W, H, C.byref(dp), cur[0], error, albedo, cur[5], cur[3], shown, None) == 0, L.pt_last_error()
            assert L.pt_ctx_present(ctx, W, H, C.byref(pp), shown, px, None) == 0, L.pt_last_error()
            frames.append(own.download(px, ow * oh * 3, np.uint8).tobytes())
            cur, hist = hist, cur
            hist_cam = cam
    finally:
        own.close()
    return frames


def ppm_pixels(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head), data[:24]
    return data[len(head):]


@pytest.mark.parametrize("step,extra,out_size,exposure", [(None, [], None, 0.0), (40.0, ["--preview-size", "30x20", "--exposure", "1.5"], (30, 20), 1.5)],
                         ids=["default-step", "step-40-resized"])
def test_orbit_frames_equal_the_set_scene_loop(tmp_path, step, extra, out_size, exposure):
    L = ptlib.product()
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    args = [CLI, str(SPP), str(H), "cornell", "--root", ptlib.ROOT, "--seed", str(SEED), "--orbit", str(FRAMES), "--preview",
            str(tmp_path / "orbit.ppm")] + ([] if step is None else ["--orbit-step", repr(step)]) + extra
    r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".ppm"))
    assert files == ["orbit-%03d.ppm" % k for k in range(FRAMES)], files
    lines = [l for l in r.stderr.splitlines() if l.startswith("frame ")]
    assert len(lines) == FRAMES and all("pt_ctx_set_camera" in l and " ms" in l for l in lines), r.stderr
    # 2 degrees per frame stays inside the scene's reach; 40 and 80 degrees each leave the box in force (the growth rule
    # evaluated on the host: test_gpu_set_camera's restatement gives [0, 1, 1] for 0, 40, 80 degrees)
    rebuilt = ["(rebuilt)" in l for l in lines]
    assert rebuilt == ([False, False, False] if step is None else [False, True, True]), lines
    want = loop_with_set_scene(L, sc, 2.0 if step is None else step, out_size, exposure)
    ow, oh = out_size or (W, H)
    for k in range(FRAMES):
        assert ppm_pixels(tmp_path / files[k], ow, oh) == want[k], "frame %d" % k
    assert want[0] != want[1] != want[2]


def test_orbit_refuses_what_it_does_not_combine_with(tmp_path):
    base = [CLI, "2", str(H), "cornell", "--root", ptlib.ROOT, "--orbit", "3"]
    pv = ["--preview", str(tmp_path / "o.ppm")]
    for extra in (pv + ["--trace-scale", "2"], pv + ["--adaptive", "0.05"], pv + ["--noise-target", "0.05"],
                  pv + ["--checkpoint", str(tmp_path / "c.ptacc")], pv + ["--denoise"], pv + ["--noise-target", "0.05", "--denoise-var"],
                  pv + ["--gpus", "2"], []):
        r = subprocess.run(base + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--orbit" in r.stderr, (extra, r.returncode, r.stderr)
    for bad in (["--orbit", "0"], ["--orbit", "x"], ["--orbit", "3", "--orbit-step", "nan"]):
        r = subprocess.run(base[:-2] + pv + bad, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--orbit" in r.stderr, (bad, r.stderr)
    r = subprocess.run(base[:-2] + pv + ["--orbit-step", "3"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--orbit-step goes with --orbit" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".ppm")]
