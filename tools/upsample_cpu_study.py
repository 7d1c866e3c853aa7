#!/usr/bin/env python3
"""The CPU study behind pt_ctx_upsample's defaults, and what tracing at half the resolution costs in error.

Per scene, at WxH (the half size is still a picture): oracle renders with the oracle's first-hit guides, built the way
tests/test_gpu_aov.py builds its expectation.  Truth is the oracle at TRUTH_SPP samples at full size.  For n in N_SPP three
frames are compared, each before and after pt_ctx_denoise at its defaults (tests/denoise_ref.py, guided by the full-size guides):
  (a) full size at n spp;
  (b) half size at 4n spp, upsampled (tests/upsample_ref.py): the same number of rays as (a);
  (c) half size at n spp, upsampled: a quarter of the rays.
Reported: the mean absolute error against truth over the full-size hit pixels, and for (b), (c) the share of hit pixels that
took the fallback (weight 0), over the grid depth_tol x normal_min.  A grid point's score is the mean, over scenes and n, of
(c)'s error after the filter; the chosen point - pt_upsample_defaults - is the grid's minimum.  No GPU is involved.

    python tools/upsample_cpu_study.py [scene ...]     # default: cornell mesh; writes profiles/upsample_cpu_study.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref  # noqa: E402
import ptlib  # noqa: E402
import test_gpu_aov as aov  # noqa: E402
import upsample_ref as ref  # noqa: E402

W, H = 192, 128
LW, LH = W // 2, H // 2
N_SPP = (2, 8)
TRUTH_SPP = 2048
DEPTH_TOL = (0.03125, 0.0625, 0.125, 0.25, 0.5)
NORMAL_MIN = (0.5, 0.8, 0.9, 0.95)
DENOISE = dict(levels=5, sigma_color=2.0, sigma_depth=0.03125)  # pt_denoise_defaults


def frame(sc, w, h, spp, seed):
    color = ptlib.oracle_render(sc, w, h, spp, seed)[0]
    albedo, normal, depth, oid = aov.rebuild(sc, w, h, seed, aov.call_pixels(w, h), spp)
    return dict(color=color, albedo=albedo, normal=normal, depth=depth, oid=oid)


def mae(a, b, mask):
    return float(np.abs(a[mask].astype(np.float64) - b[mask]).mean())


def filtered(color, full):
    return denoise_ref.denoise(color, W, H, albedo=full["albedo"], normal=full["normal"], depth=full["depth"], **DENOISE)


def study(sid):
    sc = ptlib.load_scene_py(ptlib.scene_path(sid))
    truth = ptlib.oracle_render(sc, W, H, TRUTH_SPP, 1000)[0]
    print("%s: truth rendered" % sid, flush=True)
    rows = []
    for n in N_SPP:
        full = frame(sc, W, H, n, 20 + n)
        hit = full["oid"] >= 0
        a = {"before": mae(np.clip(full["color"], 0, 1), truth, hit), "after": mae(filtered(full["color"], full), truth, hit)}
        halves = {"b": frame(sc, LW, LH, 4 * n, 40 + n), "c": frame(sc, LW, LH, n, 60 + n)}
        print("%s n=%d: frames rendered; (a) %.5f -> %.5f" % (sid, n, a["before"], a["after"]), flush=True)
        grid = []
        for dt in DEPTH_TOL:
            for nm in NORMAL_MIN:
                g = dict(depth_tol=dt, normal_min=nm)
                for name, lo in halves.items():
                    out, wgt = ref.upsample(W, H, LW, LH, lo["color"], lo["depth"], lo["oid"], full["depth"], full["oid"],
                                            lo_normal=lo["normal"], lo_albedo=lo["albedo"], normal=full["normal"],
                                            albedo=full["albedo"], depth_tol=dt, normal_min=nm)
                    g[name] = {"before": mae(out, truth, hit), "after": mae(filtered(out, full), truth, hit),
                               "fallback_share": float((wgt[hit] == 0).mean())}
                grid.append(g)
                print("%s n=%d depth_tol %-8g normal_min %-5g (b) %.5f -> %.5f  (c) %.5f -> %.5f  fallback %.4f" % (
                    sid, n, dt, nm, g["b"]["before"], g["b"]["after"], g["c"]["before"], g["c"]["after"], g["c"]["fallback_share"]),
                    flush=True)
        rows.append({"scene": sid, "n": n, "hit_pixels": int(hit.sum()), "a": a, "grid": grid})
    return rows


def main():
    scenes = sys.argv[1:] or ["cornell", "mesh"]
    rows = [r for sid in scenes for r in study(sid)]
    grid = []
    for dt in DEPTH_TOL:
        for nm in NORMAL_MIN:
            pts = [g for r in rows for g in r["grid"] if g["depth_tol"] == dt and g["normal_min"] == nm]
            grid.append({"depth_tol": dt, "normal_min": nm, "score": float(np.mean([g["c"]["after"] for g in pts]))})
    best = min(grid, key=lambda g: g["score"])
    chosen = {"depth_tol": best["depth_tol"], "normal_min": best["normal_min"]}
    at_chosen = []
    for r in rows:
        g = next(g for g in r["grid"] if g["depth_tol"] == chosen["depth_tol"] and g["normal_min"] == chosen["normal_min"])
        at_chosen.append({"scene": r["scene"], "n": r["n"], "a": r["a"], "b": g["b"], "c": g["c"]})
    doc = {
        "command": "python tools/upsample_cpu_study.py " + " ".join(scenes),
        "what": "mean |frame - truth| over the full-size hit pixels, before and after pt_ctx_denoise at its defaults "
                "(tests/denoise_ref.py): (a) %dx%d at n spp; (b) %dx%d at 4n spp upsampled by tests/upsample_ref.py (the rays of (a)); "
                "(c) %dx%d at n spp upsampled (a quarter of the rays); fallback_share = hit pixels with weight 0; frames and "
                "guides = oracle, truth = oracle at %d spp; score = mean over scenes and n of (c) after the filter" % (
                    W, H, LW, LH, LW, LH, TRUTH_SPP),
        "size": [W, H], "lo_size": [LW, LH], "scenes": scenes, "n": list(N_SPP), "truth_spp": TRUTH_SPP, "denoise": DENOISE,
        "grid": grid,
        "chosen": chosen,
        "chosen_result": at_chosen,
        "frames": rows,
    }
    path = os.path.join(ROOT, "profiles", "upsample_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("chosen:", chosen, "->", path)
    for r in at_chosen:
        print(r)


if __name__ == "__main__":
    main()
