#!/usr/bin/env python3
"""The CPU study behind pt_ctx_denoise's default sigmas and behind the bound R of the quality tests.

For cornell and mesh at 96x64: the oracle's frame at 16 samples per pixel (seed 5), the guides rebuilt from the oracle at 16
samples (tests/test_gpu_aov.py::rebuild), denoised by the numpy restatement of the contract (tests/denoise_ref.py) at 5
levels over a grid of (sigma_color, sigma_depth), measured against the oracle's frame at 4096 samples
(tests/golden/denoise_*_96x64_4096.npz): ratio = rmse(denoised, converged) / rmse(noisy, converged).  The chosen point is
the grid's minimum of the mean ratio over the two scenes.  No GPU is involved.

    python tools/denoise_cpu_study.py            # writes profiles/denoise_cpu_study.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref  # noqa: E402
import ptlib  # noqa: E402
from test_gpu_aov import call_pixels, rebuild  # noqa: E402

W, H, SPP, SEED, LEVELS = 96, 64, 16, 5, 5
SIGMA_COLOR = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
SIGMA_DEPTH = (0.0078125, 0.015625, 0.03125, 0.0625, 0.125, 0.25, 0.5, 1.0, 2.0)
SCENES = ("cornell", "mesh")


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def inputs(sid):
    """(noisy, albedo, normal, depth, converged) of one scene"""
    sc = ptlib.load_scene_py(ptlib.scene_path(sid))
    noisy, _, _ = ptlib.oracle_render(sc, W, H, SPP, SEED)
    albedo, normal, depth, _ = rebuild(sc, W, H, SEED, call_pixels(W, H), SPP)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "denoise_%s_%dx%d_4096.npz" % (sid, W, H)))
    assert int(gold["seed"]) == SEED and int(gold["spp"]) == 4096
    return noisy, albedo, normal, depth, gold["frame"]


def ratio(inp, sigma_color, sigma_depth, levels=LEVELS):
    noisy, albedo, normal, depth, conv = inp
    out = denoise_ref.denoise(noisy, W, H, albedo, normal, depth, levels, sigma_color, sigma_depth)
    return rmse(out, conv) / rmse(noisy, conv)


def main():
    inp = {sid: inputs(sid) for sid in SCENES}
    grid = []
    for sc_ in SIGMA_COLOR:
        for sd in SIGMA_DEPTH:
            r = {sid: ratio(inp[sid], sc_, sd) for sid in SCENES}
            grid.append({"sigma_color": sc_, "sigma_depth": sd, "ratio": r, "mean": sum(r.values()) / len(r)})
            print("sigma_color %-6g sigma_depth %-7g  %s" % (sc_, sd, "  ".join("%s %.4f" % kv for kv in r.items())), flush=True)
    best = min(grid, key=lambda g: g["mean"])
    doc = {
        "command": "python tools/denoise_cpu_study.py",
        "what": "rmse(denoised, converged) / rmse(noisy, converged); 96x64, noisy = oracle at 16 spp seed 5, guides = oracle "
                "first hits at 16 samples, converged = oracle at 4096 spp, denoiser = tests/denoise_ref.py at 5 levels",
        "noisy_rmse": {sid: rmse(inp[sid][0], inp[sid][4]) for sid in SCENES},
        "grid": grid,
        "chosen": best,
        "R": {sid: best["ratio"][sid] * 1.15 for sid in SCENES},
    }
    path = os.path.join(ROOT, "profiles", "denoise_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("chosen:", best, "->", path)


if __name__ == "__main__":
    main()
