#!/usr/bin/env python3
"""The CPU study behind pt_ctx_reproject_var's defaults (min_frames, radius), behind the sigma_var INTEGRATION.md names for the
viewport loop, and behind the figures of its end-to-end test.

cornell at 96x64, the orbit of tools/reproject_cpu_study.py: STEPS steps of reproject_ref.ORBIT_DEGREES, every frame an oracle
render (its own seed) with the oracle's first-hit guides, truth the oracle at 4096 samples per camera.  The orbit runs twice: at
reproject_ref.ORBIT_SPP samples per frame and at 2.  The numpy restatement (tests/reproject_var_ref.py) carries colour, length
and moments from frame to frame at pt_reproject_defaults' values; frame 0 starts the history.  Per frame - frame 0 included - the
study records the mean absolute error against truth over the hit pixels after
  - reprojection alone,
  - pt_ctx_denoise at its defaults (tests/denoise_ref.py),
  - pt_ctx_denoise_var (tests/denoise_var_ref.py, its default levels and sigma_depth) fed by this estimate, over the grid
    min_frames x radius x sigma_var,
  - the same fed by the temporal-only estimate (min_frames = 0 in the restatement: no pixel takes the spatial estimate),
the share of hit pixels that are short, and the number of hit pixels left without an estimate (e = +inf: a short pixel alone
with its object id and depth in its window).  The colour, the length and the moments do not depend on (min_frames, radius):
only the error map does.  The chosen point is the minimum of the mean, over both orbits and all frames, of the ratio "error
after pt_ctx_denoise_var / error after pt_ctx_denoise", among the grid points that leave no hit pixel of any frame without an
estimate: the first frame and the disocclusions are what the spatial estimate is there for.  No GPU is involved.

    python tools/reproject_var_cpu_study.py        # writes profiles/reproject_var_cpu_study.json (several minutes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref  # noqa: E402
import denoise_var_ref  # noqa: E402
import ptlib  # noqa: E402
import reproject_ref as ref  # noqa: E402
import reproject_var_ref as rv  # noqa: E402
import test_gpu_aov as aov  # noqa: E402

W, H = ref.ORBIT_SIZE
SPPS = (ref.ORBIT_SPP, 2)
STEPS = 5
TRUTH_SPP = 4096
MIN_FRAMES = (1, 2, 4, 8)
RADIUS = (1, 2, 3)
SIGMA_VAR = (0.5, 1.0, 2.0, 4.0)
LEVELS = 5
DN_VAR_SIGMA_DEPTH = 0.125  # pt_denoise_var_defaults


def scene_at(cam):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    sc.cam = ref.pt_camera(cam)
    return sc


def truth_of(cam, seed):
    return ptlib.oracle_render(scene_at(cam), W, H, TRUTH_SPP, 1000 + seed)[0]


def frame(cam, seed, spp, truth):
    sc = scene_at(cam)
    color = ptlib.oracle_render(sc, W, H, spp, seed)[0]
    albedo, normal, depth, oid = aov.rebuild(sc, W, H, seed, aov.call_pixels(W, H), spp)
    return dict(cam=cam, color=color, albedo=albedo, normal=normal, depth=depth, oid=oid, truth=truth, hit=oid >= 0)


def mae(a, b, mask):
    return float(np.abs(np.asarray(a).reshape(-1, 3)[mask].astype(np.float64) - b[mask]).mean())


def reproject(cur, hist, spp, min_frames, radius):
    kw = {}
    if hist is not None:
        kw = dict(hist_cam=hist["cam"], hist_color=hist["out"], hist_len=hist["len"], hist_moments=hist["mom"],
                  hist_depth=hist["depth"], hist_object_id=hist["oid"], hist_normal=hist["normal"])
    return rv.reproject_var(W, H, cur["cam"], cur["color"], cur["depth"], cur["oid"], cur["normal"], weight=spp,
                            min_frames=min_frames, radius=radius, parts=True, **kw)


def dn_var(cur, out, e, sigma_var):
    return denoise_var_ref.denoise_var(out, e, W, H, cur["albedo"], cur["normal"], cur["depth"], LEVELS, sigma_var, DN_VAR_SIGMA_DEPTH)


def orbit(frames, spp, fixed):
    """per frame: the errors and the short share; the history is carried at the reprojection's defaults"""
    rows = []
    hist = None
    for k, cur in enumerate(frames):
        hit = cur["hit"]
        row = {"frame": k, "var": [], "temporal_only": {}, "short_share": {}, "no_estimate": {}}
        out = ln = mom = None
        for mf in MIN_FRAMES:
            for r in RADIUS:
                out, ln, mom, e, parts = reproject(cur, hist, spp, mf, r)
                row["short_share"][str(mf)] = float((~parts["long"])[hit].mean())
                row["no_estimate"]["%d,%d" % (mf, r)] = int((np.isinf(e) & hit).sum())
                for sv in SIGMA_VAR:
                    row["var"].append({"min_frames": mf, "radius": r, "sigma_var": sv, "error": mae(dn_var(cur, out, e, sv), cur["truth"], hit)})
        e0 = reproject(cur, hist, spp, 0, 1)[3]
        for sv in SIGMA_VAR:
            row["temporal_only"][str(sv)] = mae(dn_var(cur, out, e0, sv), cur["truth"], hit)
        row["reprojected"] = mae(out, cur["truth"], hit)
        row["unfiltered_input"] = mae(cur["color"], cur["truth"], hit)
        row["fixed"] = mae(denoise_ref.denoise(out, W, H, cur["albedo"], cur["normal"], cur["depth"], LEVELS, fixed["sigma_color"],
                                               fixed["sigma_depth"]), cur["truth"], hit)
        rows.append(row)
        hist = dict(cur, out=out, len=ln, mom=mom)
        print("spp %d frame %d: reprojected %.4f fixed %.4f best var %.4f temporal-only %.4f short(4) %.3f" % (
            spp, k, row["reprojected"], row["fixed"], min(v["error"] for v in row["var"]), min(row["temporal_only"].values()),
            row["short_share"]["4"]), flush=True)
    return rows


def main():
    base = ref.cam_dict(ptlib.load_scene_py(ptlib.scene_path("cornell")).cam)
    cams = [ref.orbit(base, k * ref.ORBIT_DEGREES) for k in range(STEPS + 1)]
    truths = []
    for k, cam in enumerate(cams):
        truths.append(truth_of(cam, 11 + k))
        print("truth %d rendered" % k, flush=True)
    fixed = json.load(open(os.path.join(ROOT, "profiles", "denoise_cpu_study.json")))["chosen"]
    orbits = {}
    for spp in SPPS:
        frames = [frame(cam, 11 + k, spp, truths[k]) for k, cam in enumerate(cams)]
        orbits[str(spp)] = orbit(frames, spp, fixed)
    # the grid's mean ratio against the fixed filter, over both orbits and all frames
    grid = []
    for i, (mf, r, sv) in enumerate((mf, r, sv) for mf in MIN_FRAMES for r in RADIUS for sv in SIGMA_VAR):
        ratios = [row["var"][i]["error"] / row["fixed"] for rows in orbits.values() for row in rows]
        later = [row["var"][i]["error"] / row["fixed"] for rows in orbits.values() for row in rows[1:]]
        assert all((row["var"][i]["min_frames"], row["var"][i]["radius"], row["var"][i]["sigma_var"]) == (mf, r, sv)
                   for rows in orbits.values() for row in rows)
        grid.append({"min_frames": mf, "radius": r, "sigma_var": sv, "mean_ratio": float(np.mean(ratios)),
                     "mean_ratio_after_first": float(np.mean(later)),
                     "no_estimate": sum(row["no_estimate"]["%d,%d" % (mf, r)] for rows in orbits.values() for row in rows)})
    best = min((g for g in grid if g["no_estimate"] == 0), key=lambda g: g["mean_ratio"])
    bi = grid.index(best)
    chosen = {k: best[k] for k in ("min_frames", "radius", "sigma_var")}
    at_chosen = {spp: [{"frame": row["frame"], "reprojected": row["reprojected"], "fixed": row["fixed"], "var": row["var"][bi]["error"],
                        "temporal_only": row["temporal_only"][str(best["sigma_var"])],
                        "short_share": row["short_share"][str(best["min_frames"])]} for row in rows]
                 for spp, rows in orbits.items()}
    doc = {
        "command": "python tools/reproject_var_cpu_study.py",
        "what": "mean |x - truth| over the hit pixels per frame of an orbit of %d steps of %g degrees, cornell %dx%d, at %s samples "
                "per frame: x = the reprojected colour (tests/reproject_var_ref.py at pt_reproject_defaults), pt_ctx_denoise of it at "
                "its defaults, pt_ctx_denoise_var of it fed by the error map over the grid min_frames x radius x sigma_var, and fed "
                "by the temporal-only map; short_share = the share of hit pixels with len_out < min_frames * wt; frames = oracle "
                "(seeds 11..), guides = oracle first hits, truth = oracle at %d spp per camera; mean_ratio = mean over both "
                "orbits and all frames of var / fixed; no_estimate = hit pixels with e = +inf, summed over both orbits and all frames; "
                "chosen = the least mean_ratio among the grid points with no_estimate 0" % (STEPS, ref.ORBIT_DEGREES, W, H, " and ".join(map(str, SPPS)), TRUTH_SPP),
        "orbits": orbits,
        "grid": grid,
        "unconstrained_minimum": min(grid, key=lambda g: g["mean_ratio"]),
        "chosen": chosen,
        "chosen_result": dict(best, frames=at_chosen),
    }
    path = os.path.join(ROOT, "profiles", "reproject_var_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("chosen:", best, "->", path)
    for spp, rows in at_chosen.items():
        for row in rows:
            print(spp, row)


if __name__ == "__main__":
    main()
