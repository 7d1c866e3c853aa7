"""ptrace --preview with --select / --outline-radius / --sky / --grid: the P6 files hold, byte for byte, what the same calls give
through the ABI - pt_overlay_defaults for the frame's camera with the command line's values on top, pt_ctx_overlay in place after
the denoiser, pt_ctx_present - for the single frame (over a 1-sample pt_ctx_render_aov) and for every frame of --orbit.  Without
--preview the flags are refused."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import gpudev
import overlay_ref as ref
import present_ref
import ptlib
import reproject_ref
from gpudev import pfm_to_framebuffer, read_pfm
from ptlib import PtConfig, PtDenoiseVarParams, PtPresentParams, PtReprojectVarParams, PtStats

pytestmark = pytest.mark.gpu

CLI = os.path.join(ptlib.PKG, "ptrace")
W, H, SEED = 48, 32, 5
RGB8 = ptlib.abi.PT_PRESENT_RGB8
I32 = np.int32


def overlay_params(L, cam, selected, radius, flags):
    """what the command line builds: the defaults for the camera, then the values it names"""
    p = ref.PtOverlayParams()
    assert L.pt_overlay_defaults(C.byref(cam), C.byref(p)) == 0, L.pt_last_error()
    p.flags, p.n_selected = flags, len(selected)
    for i, v in enumerate(selected):
        p.selected[i] = v
    if radius:
        p.radius = radius
    return p


def centre_object(L, sc):
    """the object under the centre pixel of the frame's first-hit ids"""
    with gpudev.Device(L, sc) as d:
        d_id = d.alloc(W * H * 4)
        cfg = PtConfig(W, H, 1, 0, SEED, 0, 0, 0, 0)
        assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), None, None, None, d_id, None) == 0, L.pt_last_error()
        k = int(d.download(d_id, W * H, I32)[(H // 2) * W + W // 2])
    assert k >= 0
    return k


def test_single_frame_preview_is_the_abi_calls(tmp_path):
    L = ptlib.product()
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    k = centre_object(L, sc)
    out = tmp_path / "out"
    r = subprocess.run([CLI, "4", str(H), "cornell", "--root", ptlib.ROOT, "--seed", str(SEED), "--out", str(out), "--aov", "1", "--preview",
                        str(tmp_path / "p.ppm"), "--select", "%d,70000" % k, "--outline-radius", "3", "--sky", "--grid"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    (beauty,) = glob.glob(str(out / "*-beauty.pfm"))
    frame = pfm_to_framebuffer(read_pfm(beauty))  # the frame before the cues, bit for bit
    n = W * H
    with gpudev.Device(L, sc) as d:
        d_rgb, d_z, d_id, d_px = d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 4), d.alloc(n * 3)
        d.upload(d_rgb, frame)
        one = PtConfig(W, H, 1, 0, SEED, 0, 0, 0, 0)
        assert L.pt_ctx_render_aov(d.ctx, C.byref(one), None, None, d_z, d_id, None) == 0, L.pt_last_error()
        p = overlay_params(L, sc.cam, (k, 70000), 3, ref.SKY | ref.GRID)
        assert L.pt_ctx_overlay(d.ctx, W, H, C.byref(p), C.byref(sc.cam), d_rgb, d_id, d_z, d_rgb) == 0, L.pt_last_error()
        drawn = d.pixels(d_rgb, n)
        pp = PtPresentParams(0, 0, 0.0, RGB8, 0)
        assert L.pt_ctx_present(d.ctx, W, H, C.byref(pp), d_rgb, d_px, None) == 0, L.pt_last_error()
        want = d.download(d_px, n * 3, np.uint8).reshape(H, W, 3)
        oid = d.download(d_id, n, I32)
    got = present_ref.read_p6(str(tmp_path / "p.ppm"))
    assert np.array_equal(got, want)
    # the cues are there: the selected object's outline is pure green, and the frame changed
    M = ref.mask(oid, (k,))
    ring = ref.window(M, W, H, 3) & ~M
    assert ring.any() and (drawn[ring] == np.array([0.0, 1.0, 0.0], dtype=np.float32)).all()
    assert drawn.tobytes() != frame.tobytes()


def test_orbit_previews_are_the_abi_loop(tmp_path):
    L = ptlib.product()
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    k = centre_object(L, sc)
    spp, frames = 2, 2
    r = subprocess.run([CLI, str(spp), str(H), "cornell", "--root", ptlib.ROOT, "--seed", str(SEED), "--orbit", str(frames), "--preview",
                        str(tmp_path / "o.ppm"), "--select", str(k), "--sky", "--grid"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    n = W * H
    with gpudev.Device(L, sc) as d:
        sides = [[d.alloc(n * c * 4) for c in (3, 1, 2, 1, 1, 3)] for _ in range(2)]  # colour, len, moments, depth, id, normal
        albedo, error, shown, px = d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 12), d.alloc(n * 3)
        cfg = PtConfig(W, H, spp, 0, SEED, 0, 0, 0, 0)
        rp = PtReprojectVarParams(spp, 0, 0, 0, 0, 0, 0)
        dp = PtDenoiseVarParams(0, 2.0, 0, 0)
        pp = PtPresentParams(0, 0, 0.0, RGB8, 0)
        cur, hist = sides
        hist_cam = None
        plain = []
        for f in range(frames):
            c = reproject_ref.orbit(reproject_ref.cam_dict(sc.cam), f * 2.0)
            cam = reproject_ref.pt_camera(c)
            rebuilt, st = C.c_int(), PtStats()
            assert L.pt_ctx_set_camera(d.ctx, C.byref(cam), C.byref(rebuilt)) == 0, L.pt_last_error()
            assert L.pt_ctx_render(d.ctx, C.byref(cfg), cur[0], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
            assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), albedo, cur[5], cur[3], cur[4], None) == 0, L.pt_last_error()
            h = list(hist) if hist_cam is not None else [None] * 6
            assert L.pt_ctx_reproject_var(d.ctx, W, H, C.byref(rp), C.byref(cam), cur[0], cur[3], cur[4], cur[5],
                                          C.byref(hist_cam) if hist_cam is not None else None, *h, cur[0], cur[1], cur[2], error,
                                          None) == 0, L.pt_last_error()
            assert L.pt_ctx_denoise_var(d.ctx, W, H, C.byref(dp), cur[0], error, albedo, cur[5], cur[3], shown, None) == 0, L.pt_last_error()
            plain.append(d.pixels(shown, n).tobytes())
            p = overlay_params(L, cam, (k,), 0, ref.SKY | ref.GRID)
            assert L.pt_ctx_overlay(d.ctx, W, H, C.byref(p), C.byref(cam), shown, cur[4], cur[3], shown) == 0, L.pt_last_error()
            assert d.pixels(shown, n).tobytes() != plain[-1]
            assert L.pt_ctx_present(d.ctx, W, H, C.byref(pp), shown, px, None) == 0, L.pt_last_error()
            want = d.download(px, n * 3, np.uint8).reshape(H, W, 3)
            got = present_ref.read_p6(str(tmp_path / ("o-%03d.ppm" % f)))
            assert np.array_equal(got, want), "frame %d" % f
            cur, hist = hist, cur
            hist_cam = cam


def test_the_flags_are_refused_without_a_preview(tmp_path):
    base = [CLI, "1", "8", "cornell", "--root", ptlib.ROOT, "--no-ppm"]
    for extra in (["--select", "1"], ["--outline-radius", "3"], ["--sky"], ["--grid"], ["--orbit", "2", "--sky"]):
        r = subprocess.run(base + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and ("go with --preview" in r.stderr or "--orbit needs --preview" in r.stderr), (extra, r.returncode, r.stderr)
    pv = ["--preview", str(tmp_path / "p.ppm")]
    for extra, word in ((["--select", "-1"], "--select"), (["--select", "1,"], "--select"), (["--select", ",".join(["1"] * 17)], "--select"),
                        (["--select", "x"], "--select"), (["--outline-radius", "0"], "--outline-radius"), (["--outline-radius", "9"], "--outline-radius")):
        r = subprocess.run(base + pv + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word + " needs" in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "p.ppm")
