#!/usr/bin/env python3
"""The CPU study behind pt_ctx_denoise_var's default sigmas and behind the bounds of its quality tests.

For cornell and mesh at 96x64 and n = 16 and 256 samples per pixel (tests/denoise_var_inputs.py): two oracle frames of n/2
samples (seeds 5 and 6) are the halves, their mean the noisy frame, e(p) its noise estimate by tests/noise_ref.py; the guides
are the oracle's first hits at 16 samples.  The frame is denoised by the numpy restatement of the contract
(tests/denoise_var_ref.py) at 5 levels over a grid of (sigma_var, sigma_depth) and measured against the oracle's frame at 4096
samples (tests/golden/denoise_*_96x64_4096.npz): ratio = rmse(denoised, converged) / rmse(noisy, converged).  The chosen point
is the grid's minimum of the mean ratio over the four (scene, n) cells.  pt_ctx_denoise's restatement at pt_ctx_denoise's
defaults is measured on the same four inputs.  No GPU is involved.

    python tools/denoise_var_cpu_study.py            # writes profiles/denoise_var_cpu_study.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref  # noqa: E402
import denoise_var_inputs as inp  # noqa: E402
import denoise_var_ref  # noqa: E402

LEVELS = 5
SIGMA_VAR = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
SIGMA_DEPTH = (0.0078125, 0.015625, 0.03125, 0.0625, 0.125, 0.25, 0.5, 1.0, 2.0)
CELLS = [(sid, n) for sid in inp.SCENES for n in inp.SPP]


def key(cell):
    return "%s_%d" % cell


def ratio(cell, sigma_var, sigma_depth, levels=LEVELS):
    noisy, e, albedo, normal, depth, conv = inp.inputs(*cell)
    out = denoise_var_ref.denoise_var(noisy, e, inp.W, inp.H, albedo, normal, depth, levels, sigma_var, sigma_depth)
    return inp.rmse(out, conv) / inp.rmse(noisy, conv)


def fixed_ratio(cell):
    """pt_ctx_denoise at its own defaults (profiles/denoise_cpu_study.json) on the same input"""
    noisy, _, albedo, normal, depth, conv = inp.inputs(*cell)
    d = json.load(open(os.path.join(ROOT, "profiles", "denoise_cpu_study.json")))["chosen"]
    out = denoise_ref.denoise(noisy, inp.W, inp.H, albedo, normal, depth, LEVELS, d["sigma_color"], d["sigma_depth"])
    return inp.rmse(out, conv) / inp.rmse(noisy, conv)


def main():
    grid = []
    for sv in SIGMA_VAR:
        for sd in SIGMA_DEPTH:
            r = {key(c): ratio(c, sv, sd) for c in CELLS}
            grid.append({"sigma_var": sv, "sigma_depth": sd, "ratio": r, "mean": sum(r.values()) / len(r)})
            print("sigma_var %-6g sigma_depth %-7g  %s" % (sv, sd, "  ".join("%s %.4f" % kv for kv in r.items())), flush=True)
    best = min(grid, key=lambda g: g["mean"])
    doc = {
        "command": "python tools/denoise_var_cpu_study.py",
        "what": "rmse(denoised, converged) / rmse(noisy, converged); 96x64, halves = oracle at n/2 spp seeds 5 and 6, noisy = "
                "their mean, e = tests/noise_ref.py error_from_means (w = 1/2), guides = oracle first hits at 16 samples, "
                "converged = oracle at 4096 spp, denoiser = tests/denoise_var_ref.py at 5 levels",
        "noisy_rmse": {key(c): inp.rmse(inp.inputs(*c)[0], inp.inputs(*c)[5]) for c in CELLS},
        "grid": grid,
        "chosen": best,
        "R": {k: v * 1.15 for k, v in best["ratio"].items()},
        "pt_ctx_denoise_defaults": {key(c): fixed_ratio(c) for c in CELLS},
    }
    path = os.path.join(ROOT, "profiles", "denoise_var_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("chosen:", best, "fixed:", doc["pt_ctx_denoise_defaults"], "->", path)


if __name__ == "__main__":
    main()
