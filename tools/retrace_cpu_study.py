#!/usr/bin/env python3
"""The CPU study of what pt_ctx_select_pixels + pt_ctx_render_masked buy the viewport loop.  No outcome is fixed in advance:
the numbers below are what INTEGRATION.md reports, whichever way they fall.  No GPU is involved.

(a) Fallback retrace.  tools/upsample_cpu_study.py's frames (cornell and mesh.json, 192x128 <- 96x64, oracle frames and guides,
    the same seeds, truth at 2048 samples), its case (c): half size at n spp, upsampled by tests/upsample_ref.py at
    pt_upsample_defaults.  The pixels with weight 0 are replaced by the full-size frame's pixels at n spp - what
    pt_ctx_render_masked writes.  Reported for n = 2 and 8: the mean absolute error against truth over the fallback pixels and
    over the hit pixels of the frame, before -> after the retrace, and again after pt_ctx_denoise at its defaults
    (tests/denoise_ref.py); the share of pixels retraced; the retraced samples as a fraction of the low-resolution frame's.

(b) Disocclusion boost.  tools/reproject_var_cpu_study.py's orbit (cornell 96x64, 2 degrees per step, six frames, at 8 and at
    2 samples per frame, truth at 4096).  After pt_ctx_reproject_var (tests/reproject_var_ref.py at its defaults) the pixels
    with len_out <= weight - no history: a disocclusion - are replaced in the blended frame by their pixel of another render
    at 1x and at 4x the frame's samples (another seed: at 1x the replacement is as noisy as what it replaces, which is the
    frame's own pixel).  Length, moments and error map stay what the reprojection wrote: stale for those pixels.  Each variant
    carries its own history.  Reported per frame after the first (on frame 0 every pixel is short: the boost would be the
    whole frame): the error over those pixels and over the hit pixels after pt_ctx_denoise_var at sigma_var 2
    (tests/denoise_var_ref.py), and the extra samples as a fraction of the frame's.

    python tools/retrace_cpu_study.py        # writes profiles/retrace_cpu_study.json (several minutes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import denoise_ref  # noqa: E402
import denoise_var_ref  # noqa: E402
import masked_ref  # noqa: E402
import ptlib  # noqa: E402
import reproject_ref  # noqa: E402
import reproject_var_cpu_study as orbit_study  # noqa: E402
import reproject_var_ref as rv  # noqa: E402
import upsample_cpu_study as up_study  # noqa: E402
import upsample_ref  # noqa: E402

SIGMA_VAR = 2.0  # what INTEGRATION.md names for the loop
BOOST = (1, 4)


def mae(a, b, mask):
    if not mask.any():
        return None
    return float(np.abs(np.asarray(a).reshape(-1, 3)[mask].astype(np.float64) - b[mask]).mean())


# ------------------------------------------------------------------------------------------------- (a) fallback retrace
def fallback_retrace(sid):
    W, H, LW, LH = up_study.W, up_study.H, up_study.LW, up_study.LH
    sc = ptlib.load_scene_py(ptlib.scene_path(sid))
    truth = ptlib.oracle_render(sc, W, H, up_study.TRUTH_SPP, 1000)[0]
    print("%s: truth rendered" % sid, flush=True)
    chosen = json.load(open(os.path.join(ROOT, "profiles", "upsample_cpu_study.json")))["chosen"]
    rows = []
    for n in up_study.N_SPP:
        full = up_study.frame(sc, W, H, n, 20 + n)  # its colour is what pt_ctx_render writes at full size, n spp
        lo = up_study.frame(sc, LW, LH, n, 60 + n)
        hit = full["oid"] >= 0
        out, wgt = upsample_ref.upsample(W, H, LW, LH, lo["color"], lo["depth"], lo["oid"], full["depth"], full["oid"],
                                         lo_normal=lo["normal"], lo_albedo=lo["albedo"], normal=full["normal"], albedo=full["albedo"],
                                         **chosen)
        mask, count = masked_ref.select(weight=wgt, weight_max=0.0)
        sel = mask != 0
        retraced = out.copy()
        retraced[sel] = np.clip(full["color"][sel], 0, 1)
        f_out, f_re = up_study.filtered(out, full), up_study.filtered(retraced, full)
        row = {"scene": sid, "n": n, "pixels": W * H, "retraced_pixels": count, "retraced_share": count / (W * H),
               "retraced_samples_over_lo_samples": count * n / (LW * LH * n),
               "fallback": {"before": mae(out, truth, sel), "after": mae(retraced, truth, sel),
                            "filtered_before": mae(f_out, truth, sel), "filtered_after": mae(f_re, truth, sel)},
               "frame": {"before": mae(out, truth, hit), "after": mae(retraced, truth, hit),
                         "filtered_before": mae(f_out, truth, hit), "filtered_after": mae(f_re, truth, hit)}}
        rows.append(row)
        print(row, flush=True)
    return rows


# ------------------------------------------------------------------------------------------------ (b) disocclusion boost
def boost_orbit(cams, truths, spp):
    W, H = orbit_study.W, orbit_study.H
    frames = [orbit_study.frame(cam, 11 + k, spp, truths[k]) for k, cam in enumerate(cams)]
    # the replacements: the same cameras rendered again, other seeds, at 1x and 4x the frame's samples
    again = {b: [np.clip(ptlib.oracle_render(orbit_study.scene_at(cam), W, H, b * spp, 500 + 10 * b + k)[0], 0, 1)
                 for k, cam in enumerate(cams)] for b in BOOST}
    rows = []
    hist = {v: None for v in (0,) + BOOST}  # 0: the loop as it is
    for k, cur in enumerate(frames):
        hit = cur["hit"]
        row = {"frame": k}
        for v in hist:
            out, ln, mom, e, _ = orbit_study.reproject(cur, hist[v], spp, 2, 3)  # min_frames, radius: pt_reproject_var_defaults
            sel = (ln <= np.float32(spp)) & hit
            if v and k:
                out = out.copy()
                out[sel] = again[v][k][sel]
            shown = orbit_study.dn_var(cur, out, e, SIGMA_VAR)
            row[str(v)] = {"short_pixels": int(sel.sum()), "short_share_of_hit": float(sel[hit].mean()),
                           "extra_samples_over_frame_samples": (v * float(sel.sum()) / (W * H)) if (v and k) else 0.0,
                           "short": {"blended": mae(out, cur["truth"], sel), "filtered": mae(shown, cur["truth"], sel)},
                           "frame": {"blended": mae(out, cur["truth"], hit), "filtered": mae(shown, cur["truth"], hit)}}
            hist[v] = dict(cur, out=out, len=ln, mom=mom)
        rows.append(row)
        print("spp %d frame %d:" % (spp, k), {v: (row[v]["short_pixels"], row[v]["short"]["filtered"], row[v]["frame"]["filtered"])
                                             for v in ("0", "1", "4")}, flush=True)
    return rows


def main():
    doc = {"command": "python tools/retrace_cpu_study.py",
           "what": "(a) fallback retrace: tools/upsample_cpu_study.py's case (c) at pt_upsample_defaults with the weight-0 pixels "
                   "replaced by the full-size frame's at n spp; mean |x - truth| over the retraced pixels ('fallback') and over the "
                   "hit pixels ('frame'), before / after the retrace, unfiltered and after pt_ctx_denoise at its defaults.  (b) "
                   "disocclusion boost: tools/reproject_var_cpu_study.py's orbit; variant 0 = the loop as it is, 1 and 4 = the "
                   "pixels with len_out <= weight replaced in the blended frame by another render's at 1x / 4x the frame's samples "
                   "from frame 1 on, each variant with its own history; errors over those pixels ('short') and over the hit pixels "
                   "('frame'), blended and after pt_ctx_denoise_var at sigma_var %g; the moments and the error map are not "
                   "updated for the replaced pixels" % SIGMA_VAR}
    doc["fallback_retrace"] = [r for sid in ("cornell", "mesh") for r in fallback_retrace(sid)]
    base = reproject_ref.cam_dict(ptlib.load_scene_py(ptlib.scene_path("cornell")).cam)
    cams = [reproject_ref.orbit(base, k * reproject_ref.ORBIT_DEGREES) for k in range(orbit_study.STEPS + 1)]
    truths = []
    for k, cam in enumerate(cams):
        truths.append(orbit_study.truth_of(cam, 11 + k))
        print("truth %d rendered" % k, flush=True)
    doc["disocclusion_boost"] = {str(spp): boost_orbit(cams, truths, spp) for spp in orbit_study.SPPS}
    # the means over frames 1.. that the documents quote
    summary = {}
    for spp, rows in doc["disocclusion_boost"].items():
        later = rows[1:]
        summary[spp] = {v: {"short_filtered": float(np.mean([r[v]["short"]["filtered"] for r in later if r[v]["short"]["filtered"] is not None])),
                            "frame_filtered": float(np.mean([r[v]["frame"]["filtered"] for r in later])),
                            "extra_samples_over_frame_samples": float(np.mean([r[v]["extra_samples_over_frame_samples"] for r in later]))}
                        for v in ("0", "1", "4")}
    doc["disocclusion_boost_mean_after_first"] = summary
    path = os.path.join(ROOT, "profiles", "retrace_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1), "->", path)


if __name__ == "__main__":
    main()
