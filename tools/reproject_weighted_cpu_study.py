#!/usr/bin/env python3
"""The CPU study of what per-pixel sample counts in the blend (pt_ctx_reproject_var_weighted) buy the viewport loop.  No outcome
is fixed in advance: the numbers below are what the documents report, whichever way they fall.  No GPU is involved.

tools/retrace_cpu_study.py's orbit (b): cornell 96x64, 2 degrees per step, six frames, at 8 and at 2 samples per frame, oracle
frames and first-hit guides, truth at 4096 samples per camera; error after pt_ctx_denoise_var at sigma_var 2
(tests/denoise_var_ref.py), mean over frames 1 to 5.

(a) The 4x boost.  Per frame, as the CLI's --boost does it: pt_ctx_reproject (tests/reproject_ref.py) for the lengths, the hit
    pixels with len <= weight are replaced IN THE INPUT FRAME by their pixel of another render at 4x the frame's samples, then
      uniform   pt_ctx_reproject_var with weight = the frame's samples (tests/reproject_var_ref.py): the boosted pixels enter
                the history as one frame's worth, and the error map scales them as such;
      weighted  pt_ctx_reproject_var_weighted (tests/reproject_weighted_ref.py) with the true plane, samples or 4x samples.
    Each variant carries its own history; "as it is" is the loop without a boost.  Reported: the error over the pixels boosted
    in this frame, over the pixels boosted in the frame BEFORE (where the carried length acts), and over the hit pixels.
(b) An adaptive frame per step.  The oracle's pixels at per-tile counts: tiles of 8x8, the count 2, 8 or 32 by the thirds of the
    tile's mean absolute difference between two independent 8-sample renders (the noisiest third gets 32), the pixel taken from
    the oracle's render at that count.
      uniform   pt_ctx_reproject_var with weight = the frame's mean count, rounded;
      weighted  the true plane.
    Reported: the error over the hit pixels and over the pixels of each count.

    python tools/reproject_weighted_cpu_study.py        # writes profiles/reproject_weighted_cpu_study.json (several minutes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ptlib  # noqa: E402
import reproject_ref  # noqa: E402
import reproject_var_cpu_study as orbit_study  # noqa: E402
import reproject_var_ref as rv  # noqa: E402
import reproject_weighted_ref as wref  # noqa: E402

SIGMA_VAR = 2.0  # what INTEGRATION.md names for the loop
BOOST = 4
TILE = 8
COUNTS = (2, 8, 32)
W, H = orbit_study.W, orbit_study.H
DEFAULTS = dict(min_frames=2, radius=3)  # pt_reproject_var_defaults


def mae(a, b, mask):
    if not mask.any():
        return None
    return float(np.abs(np.asarray(a).reshape(-1, 3)[mask].astype(np.float64) - b[mask]).mean())


def render(cam, spp, seed):
    return np.clip(ptlib.oracle_render(orbit_study.scene_at(cam), W, H, spp, seed)[0], 0, 1).astype(np.float32)


def hist_kw(hist):
    if hist is None:
        return {}
    return dict(hist_cam=hist["cam"], hist_color=hist["out"], hist_len=hist["len"], hist_moments=hist["mom"], hist_depth=hist["depth"],
                hist_object_id=hist["oid"], hist_normal=hist["normal"])


def blend(cur, color, hist, weight, plane=None):
    args = (W, H, cur["cam"], color, cur["depth"], cur["oid"], cur["normal"])
    if plane is None:
        return rv.reproject_var(*args, weight=weight, **DEFAULTS, **hist_kw(hist))
    return wref.reproject_var_weighted(*args, spp=plane, weight=weight, **DEFAULTS, **hist_kw(hist))


def mean_of(rows, *keys):
    vals = []
    for r in rows:
        for k in keys:
            r = r[k]
        if r is not None:
            vals.append(r)
    return float(np.mean(vals)) if vals else None


# --------------------------------------------------------------------------------------------------------- (a) the boost
def boost_orbit(cams, truths, spp):
    frames = [orbit_study.frame(cam, 11 + k, spp, truths[k]) for k, cam in enumerate(cams)]
    again = [render(cam, BOOST * spp, 540 + k) for k, cam in enumerate(cams)]
    hist = {"as_it_is": None, "uniform": None, "weighted": None}
    before = {v: np.zeros(W * H, bool) for v in hist}
    rows = []
    for k, cur in enumerate(frames):
        hit = cur["hit"]
        row = {"frame": k}
        for v in hist:
            color = np.asarray(cur["color"], dtype=np.float32).reshape(-1, 3)
            sel = np.zeros(W * H, bool)
            if v != "as_it_is" and k:
                h = hist[v]
                ln = reproject_ref.reproject(W, H, cur["cam"], color, cur["depth"], cur["oid"], cur["normal"], hist_cam=h["cam"],
                                             hist_color=h["out"], hist_len=h["len"], hist_depth=h["depth"], hist_object_id=h["oid"],
                                             hist_normal=h["normal"], weight=spp)[1]
                sel = (ln <= np.float32(spp)) & hit
                color = color.copy()
                color[sel] = again[k][sel]
            plane = np.where(sel, BOOST * spp, spp).astype(np.uint32) if v == "weighted" else None
            out, ln, mom, e = blend(cur, color, hist[v], spp, plane)
            shown = orbit_study.dn_var(cur, out, e, SIGMA_VAR)
            row[v] = {"boosted_pixels": int(sel.sum()), "extra_samples_over_frame_samples": (BOOST - 1) * float(sel.sum()) / (W * H),
                      "boosted": mae(shown, cur["truth"], sel), "boosted_before": mae(shown, cur["truth"], before[v] & hit),
                      "frame": mae(shown, cur["truth"], hit), "frame_blended": mae(out, cur["truth"], hit)}
            before[v] = sel
            hist[v] = dict(cur, out=out, len=ln, mom=mom)
        rows.append(row)
        print("boost, spp %d frame %d:" % (spp, k), {v: (row[v]["boosted_pixels"], row[v]["boosted"], row[v]["boosted_before"],
                                                        row[v]["frame"]) for v in hist}, flush=True)
    return rows


# ------------------------------------------------------------------------------------------------- (b) the adaptive frame
def adaptive_orbit(cams, truths):
    tiles_x = (W + TILE - 1) // TILE
    x, r = np.arange(W * H) % W, np.arange(W * H) // W
    tile_of = (r // TILE) * tiles_x + x // TILE
    hist = {"uniform": None, "weighted": None}
    rows = []
    for k, cam in enumerate(cams):
        cur = orbit_study.frame(cam, 11 + k, 8, truths[k])
        hit = cur["hit"]
        renders = {c: render(cam, c, 700 + 10 * k + i) for i, c in enumerate(COUNTS)}
        diff = np.abs(renders[8].astype(np.float64) - np.clip(cur["color"], 0, 1).reshape(-1, 3)).mean(axis=1)
        per_tile = np.bincount(tile_of, weights=diff) / np.bincount(tile_of)
        rank = np.argsort(np.argsort(per_tile))
        third = (rank * 3) // len(per_tile)
        plane = np.array(COUNTS, dtype=np.uint32)[third][tile_of]
        color = np.zeros((W * H, 3), np.float32)
        for c in COUNTS:
            color[plane == c] = renders[c][plane == c]
        mean_count = int(round(float(plane.mean())))
        row = {"frame": k, "mean_count": float(plane.mean()), "uniform_weight": mean_count,
               "pixels_by_count": {str(c): int((plane == c).sum()) for c in COUNTS}}
        for v in hist:
            out, ln, mom, e = blend(cur, color, hist[v], mean_count, plane if v == "weighted" else None)
            shown = orbit_study.dn_var(cur, out, e, SIGMA_VAR)
            row[v] = {"frame": mae(shown, cur["truth"], hit), "frame_blended": mae(out, cur["truth"], hit),
                      "by_count": {str(c): mae(shown, cur["truth"], hit & (plane == c)) for c in COUNTS}}
            hist[v] = dict(cur, out=out, len=ln, mom=mom)
        rows.append(row)
        print("adaptive, frame %d (mean count %.1f):" % (k, plane.mean()), {v: (row[v]["frame"], row[v]["by_count"]) for v in hist}, flush=True)
    return rows


def main():
    doc = {"command": "python tools/reproject_weighted_cpu_study.py",
           "what": "tools/retrace_cpu_study.py's orbit (cornell %dx%d, %g degrees per step, %d frames, oracle frames and guides, truth at "
                   "%d samples); mean |x - truth| after pt_ctx_denoise_var at sigma_var %g.  boost: the hit pixels with pt_ctx_reproject's "
                   "len <= weight replaced in the input frame by another render's at %dx the frame's samples, then blended under the "
                   "uniform weight (uniform) and under the true plane (weighted), each with its own history; 'boosted' = the pixels "
                   "boosted in this frame, 'boosted_before' = those boosted in the frame before, 'frame' = the hit pixels.  adaptive: "
                   "per-tile counts %s by the thirds of a tile's noise, uniform weight = the mean count against the true plane"
                   % (W, H, reproject_ref.ORBIT_DEGREES, orbit_study.STEPS + 1, orbit_study.TRUTH_SPP, SIGMA_VAR, BOOST, list(COUNTS))}
    base = reproject_ref.cam_dict(ptlib.load_scene_py(ptlib.scene_path("cornell")).cam)
    cams = [reproject_ref.orbit(base, k * reproject_ref.ORBIT_DEGREES) for k in range(orbit_study.STEPS + 1)]
    truths = []
    for k, cam in enumerate(cams):
        truths.append(orbit_study.truth_of(cam, 11 + k))
        print("truth %d rendered" % k, flush=True)
    doc["boost"] = {str(spp): boost_orbit(cams, truths, spp) for spp in orbit_study.SPPS}
    doc["adaptive"] = adaptive_orbit(cams, truths)
    doc["boost_mean_after_first"] = {
        spp: {v: {m: mean_of(rows[1:], v, m) for m in ("boosted", "boosted_before", "frame", "extra_samples_over_frame_samples")}
              for v in ("as_it_is", "uniform", "weighted")} for spp, rows in doc["boost"].items()}
    later = doc["adaptive"][1:]
    doc["adaptive_mean_after_first"] = {
        v: dict({"frame": mean_of(later, v, "frame")}, **{"count_%d" % c: mean_of(later, v, "by_count", str(c)) for c in COUNTS})
        for v in ("uniform", "weighted")}
    doc["adaptive_first_frame"] = {v: doc["adaptive"][0][v]["frame"] for v in ("uniform", "weighted")}
    path = os.path.join(ROOT, "profiles", "reproject_weighted_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("boost_mean_after_first", "adaptive_mean_after_first", "adaptive_first_frame")}, indent=1), "->", path)


if __name__ == "__main__":
    main()
