"""The inputs of the CPU study behind pt_ctx_denoise_var's defaults (tools/denoise_var_cpu_study.py) and of the quality tests
that hold the contract to it: for a scene at 96x64 and n samples per pixel, two oracle frames of n/2 samples (seeds 5 and 6)
stand for the two halves, as in tools/noise_cpu_study.py; m = their mean is the frame of all n samples and e its noise
estimate (tests/noise_ref.py, w = 1/2).  Guides: the oracle's first hits at 16 samples.  Truth: the committed 4096-sample
frame.  No GPU is involved; results are cached per (scene, n) and must not be modified."""
import functools
import os

import numpy as np

import noise_ref
import ptlib

W, H, SEEDS, GUIDE_SPP = 96, 64, (5, 6), 16
SCENES = ("cornell", "mesh")
SPP = (16, 256)
F32 = np.float32


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@functools.lru_cache(maxsize=None)
def guides(sid):
    """(scene, albedo, normal, depth, converged)"""
    from test_gpu_aov import call_pixels, rebuild

    sc = ptlib.load_scene_py(ptlib.scene_path(sid))
    albedo, normal, depth, _ = rebuild(sc, W, H, SEEDS[0], call_pixels(W, H), GUIDE_SPP)
    gold = np.load(os.path.join(ptlib.ROOT, "tests", "golden", "denoise_%s_%dx%d_4096.npz" % (sid, W, H)))
    assert (int(gold["width"]), int(gold["height"]), int(gold["spp"]), int(gold["seed"])) == (W, H, 4096, SEEDS[0])
    return sc, albedo, normal, depth, gold["frame"].reshape(W * H, 3)


@functools.lru_cache(maxsize=None)
def inputs(sid, n):
    """(noisy (W*H, 3), error (W*H,), albedo, normal, depth, converged (W*H, 3)) of one (scene, n) cell"""
    sc, albedo, normal, depth, conv = guides(sid)
    a, b = (ptlib.oracle_render(sc, W, H, n // 2, seed)[0].reshape(W * H, 3).astype(F32) for seed in SEEDS)
    m = noise_ref.clamp01((a + b) * F32(0.5))
    e = noise_ref.error_from_means(a.T, b.T, m.T, F32(0.5))
    return m, e, albedo, normal, depth, conv
