#!/usr/bin/env python3
"""The CPU study behind ptrace --move-history's default and behind what README, INTEGRATION.md and DESIGN.md say pt_ctx_reproject_moved
is worth: history carried on a dragged object against history dropped.

tools/reproject_var_cpu_study.py's method: cornell at 96x64, every frame an oracle render (its own seed) with the oracle's first-hit
guides, truth the oracle at 4096 samples of the EDITED scene per frame.  FRAMES frames; from frame 1 on the first sphere stands at
its position + k * DRAG (binary32, as ptrace --move forms it).  The loop runs under a still camera and on the study's orbit
(reproject_ref.ORBIT_DEGREES per frame), each at reproject_ref.ORBIT_SPP and at 2 samples per frame.  The numpy restatements carry
colour, length and moments from frame to frame at pt_reproject_var_defaults' values, each policy with its own history:
  (a) dropped   every move frame starts a new history (ptrace --move without --move-history);
  (b) plain     pt_ctx_reproject_var with the history kept: the reprojection follows the camera only;
  (c) table     pt_ctx_reproject_var_moved with pt_object_motion_between's record, max_history on move frames one of
                64 samples (the default), 16, 8, 4, 2 frames' samples (x wt).
Per frame and policy the mean absolute error of the reprojected colour against truth over three pixel sets:
  all     the hit pixels;
  object  the moved object's pixels;
  stale   the hit pixels NOT on the object (in this frame) whose truth changed between frame k-1's scene and frame k's, both seen
          by frame k's camera: mean over the channels of |truth_k - truth_k^prev| above THRESHOLD_FACTOR x the median of that
          difference over the pixels off the object.  The two truths have independent seeds, so the median is the truth's own
          noise floor (most pixels did not change), and the set is the moved object's shadow, its bounce light and its mirror
          images.  Under the still camera truth_k^prev is truth_{k-1}; on the orbit it is rendered for the purpose.
The pick: the max_history of (c) with the least mean, over both cameras, both sample counts and the move frames, of the ratio
"error of (c) / error of (a)" over ALL hit pixels; the same means are recorded for the two other sets.  No GPU is involved.

    python tools/reproject_moved_cpu_study.py        # writes profiles/reproject_moved_cpu_study.json (about twenty minutes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptlib  # noqa: E402
import reproject_moved_ref as mref  # noqa: E402
import reproject_ref as ref  # noqa: E402
import reproject_var_ref as rv  # noqa: E402
import test_gpu_aov as aov  # noqa: E402
from reproject_ref import F32  # noqa: E402

W, H = ref.ORBIT_SIZE
SPPS = (ref.ORBIT_SPP, 2)
FRAMES = 5
TRUTH_SPP = 4096
DRAG = (0.1, 0.1, 0.07)  # per frame: about a pixel and a half across and up, a pixel's worth towards the camera
HISTORIES = ("64", "16wt", "8wt", "4wt", "2wt")
THRESHOLD_FACTOR = 3.0
SETS = ("all", "object", "stale")


def scene_at(cam, index, k):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    sc.cam = ref.pt_camera(cam)
    for a in range(3):
        sc.objs[index].position[a] = float(F32(sc.objs[index].position[a]) + F32(k) * F32(DRAG[a]))
    return sc


def truth_of(cam, index, k, seed):
    return ptlib.oracle_render(scene_at(cam, index, k), W, H, TRUTH_SPP, 1000 + seed)[0]


def frame(cam, index, k, seed, spp):
    sc = scene_at(cam, index, k)
    color = ptlib.oracle_render(sc, W, H, spp, seed)[0]
    # test_gpu_aov keeps a scene's primary rays under id(scene), and a scene made here is freed after its frame: a later scene
    # at the same address with the same seed and sample count - the other camera's - would be handed these rays
    aov._ray_cache.clear()
    _, normal, depth, oid = aov.rebuild(sc, W, H, seed, aov.call_pixels(W, H), spp)
    return dict(cam=cam, color=color, normal=normal, depth=depth, oid=oid, obj=mref.object_dict(sc.objs[index]))


def mae(a, b, mask):
    if not mask.any():
        return None
    return float(np.abs(np.asarray(a).reshape(-1, 3)[mask].astype(np.float64) - b[mask]).mean())


def max_history_of(name, spp):
    return 64.0 if name == "64" else float(name[:-2]) * spp


def step(cur, hist, spp, motion=None, max_history=64.0):
    kw = {}
    if hist is not None:
        kw = dict(hist_cam=hist["cam"], hist_color=hist["out"], hist_len=hist["len"], hist_moments=hist["mom"],
                  hist_depth=hist["depth"], hist_object_id=hist["oid"], hist_normal=hist["normal"])
    args = (W, H, cur["cam"], cur["color"], cur["depth"], cur["oid"], cur["normal"])
    if motion is None:
        out, ln, mom, _ = rv.reproject_var(*args, weight=spp, max_history=max_history, **kw)
    else:
        out, ln, mom, _ = mref.reproject_var_moved(*args, weight=spp, max_history=max_history, motion=motion, **kw)
    return dict(cur, out=out, len=ln, mom=mom)


def loop(frames, truths, prevs, index, n_objs, spp):
    rows = []
    hist = {p: None for p in ("dropped", "plain") + HISTORIES}
    for k, cur in enumerate(frames):
        hit = cur["oid"] >= 0
        on = cur["oid"] == index
        row = {"frame": k, "pixels": {"all": int(hit.sum()), "object": int(on.sum())}}
        if k:
            change = np.abs(truths[k].astype(np.float64) - prevs[k]).mean(axis=1)
            floor = float(np.median(change[hit & ~on]))
            stale = hit & ~on & (change > THRESHOLD_FACTOR * floor)
            row["stale_threshold"] = THRESHOLD_FACTOR * floor
            motion = [mref.IDENTITY] * n_objs
            motion[index] = mref.motion_between(cur["obj"], frames[k - 1]["obj"])
        else:
            stale = np.zeros_like(hit)
            motion = None
        row["pixels"]["stale"] = int(stale.sum())
        sets = {"all": hit, "object": on, "stale": stale}
        new = {"dropped": step(cur, None, spp), "plain": step(cur, hist["plain"], spp)}
        for name in HISTORIES:
            new[name] = step(cur, hist[name], spp, motion, max_history_of(name, spp) if k else 64.0)
        for p, f in new.items():
            row[p] = {s: mae(f["out"], truths[k], m) for s, m in sets.items()}
            if p != "dropped":
                row[p]["object_with_history"] = float((f["len"][on] > spp).mean()) if on.any() else None
        rows.append(row)
        hist = new
        print("spp %d frame %d: %s" % (spp, k, json.dumps({p: row[p] for p in new})), flush=True)
    return rows


def main():
    sc0 = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    index = [i for i in range(sc0.n_objs) if sc0.objs[i].kind == ptlib.PT_SPHERE][0]
    base = ref.cam_dict(sc0.cam)
    runs = {}
    for camera, degrees in (("still", 0.0), ("orbit", ref.ORBIT_DEGREES)):
        cams = [ref.orbit(base, k * degrees) if degrees else base for k in range(FRAMES)]
        truths = [truth_of(cams[k], index, k, 11 + k) for k in range(FRAMES)]
        print(camera, "truths rendered", flush=True)
        if degrees:
            prevs = [None] + [truth_of(cams[k], index, k - 1, 511 + k) for k in range(1, FRAMES)]
        else:
            prevs = [None] + truths[:-1]
        runs[camera] = {}
        for spp in SPPS:
            frames = [frame(cams[k], index, k, 11 + k, spp) for k in range(FRAMES)]
            runs[camera][str(spp)] = loop(frames, truths, prevs, index, sc0.n_objs, spp)
    # per max_history and per set: the mean over both cameras, both sample counts and the move frames of (c) / (a)
    summary = {}
    for p in ("plain",) + HISTORIES:
        summary[p] = {}
        for s in SETS:
            ratios = [row[p][s] / row["dropped"][s] for by_spp in runs.values() for rows in by_spp.values() for row in rows[1:]
                      if row[p][s] is not None and row["dropped"][s]]
            summary[p][s] = float(np.mean(ratios))
    pick = min(HISTORIES, key=lambda name: summary[name]["all"])
    loses_on_stale = all(summary[name]["stale"] > 1.0 for name in HISTORIES)
    doc = {
        "command": "python tools/reproject_moved_cpu_study.py",
        "what": "cornell %dx%d, %d frames, the first sphere (object %d) dragged by %r per frame from frame 1 on, under a still camera "
                "and on an orbit of %g degrees per frame, at %s samples per frame; frames = oracle (seeds 11..), guides = oracle first "
                "hits, truth = oracle at %d spp of the edited scene per frame; per frame and policy the mean |reprojected colour - truth| "
                "over all hit pixels, the object's pixels and the stale-light set; policies: dropped = every move frame starts a new "
                "history, plain = pt_ctx_reproject_var with the history kept, and pt_ctx_reproject_var_moved with max_history on move "
                "frames = 64 samples or 16, 8, 4, 2 frames' samples; object_with_history = the share of the object's pixels with "
                "len_out > wt" % (W, H, FRAMES, index, DRAG, ref.ORBIT_DEGREES, " and ".join(map(str, SPPS)), TRUTH_SPP),
        "stale_set": "hit pixels off the object whose truth changed between frame k-1's scene and frame k's under frame k's camera: mean "
                     "over the channels of |difference of the two truths| > %g x its median over the pixels off the object (the "
                     "truths' own noise floor: their seeds are independent)" % THRESHOLD_FACTOR,
        "runs": runs,
        "mean_ratio_to_dropped": summary,
        "table_loses_to_dropped_on_the_stale_set_at_every_max_history": loses_on_stale,
        "chosen": {"move_history_frames": float(pick[:-2]) if pick != "64" else None, "max_history": pick,
                   "by": "the least mean ratio to dropped over all hit pixels"},
    }
    path = os.path.join(ROOT, "profiles", "reproject_moved_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("summary:", json.dumps(summary, indent=1))
    print("chosen:", doc["chosen"], "->", path)


if __name__ == "__main__":
    main()
