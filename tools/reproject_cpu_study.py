#!/usr/bin/env python3
"""The CPU study behind pt_ctx_reproject's defaults and behind the camera move of its end-to-end test.

cornell at 96x64.  The camera orbits the room in STEPS steps of reproject_ref.ORBIT_DEGREES; every frame is an oracle render at
reproject_ref.ORBIT_SPP samples (its own seed) with the oracle's first-hit guides, built the way tests/test_gpu_aov.py builds its
expectation (depth and id of sample 0, the normal the mean over the samples).  The numpy restatement of the contract
(tests/reproject_ref.py) carries the history from frame to frame: frame 0 starts it, every later frame reprojects it.  Truth is
the oracle at 4096 samples per camera.  Over a grid of (max_history, depth_tol, normal_min) the study records, per frame after
the first: the mean absolute error against truth over the hit pixels with history (the output) and without (the frame's own
colour), and the share of hit pixels that find history (len_out > wt).  The chosen point is the grid's minimum of the mean of
the output's error over the frames (a pixel without history counts with its own colour's error).

It also runs the end-to-end test's two frames - A the scene's camera, B one step on, history from A alone - at the chosen point
and records the share and the two errors over the pixels that found history: all of them, and those whose first hit is a
diffuse object.  No GPU is involved.

    python tools/reproject_cpu_study.py            # writes profiles/reproject_cpu_study.json (about three minutes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptlib  # noqa: E402
import reproject_ref as ref  # noqa: E402
import test_gpu_aov as aov  # noqa: E402

W, H = ref.ORBIT_SIZE
SPP = ref.ORBIT_SPP
STEPS = 4
TRUTH_SPP = 4096
MAX_HISTORY = (8.0, 16.0, 32.0, 64.0)
DEPTH_TOL = (0.015625, 0.03125, 0.0625, 0.125, 0.25)
NORMAL_MIN = (0.25, 0.5, 0.75, 0.9)
DIFFUSE = ptlib.abi.PT_DIFFUSE


def scene_at(cam):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    sc.cam = ref.pt_camera(cam)
    return sc


def frame(cam, seed):
    """colour, guides and truth of one camera"""
    sc = scene_at(cam)
    color = ptlib.oracle_render(sc, W, H, SPP, seed)[0]
    pixels = aov.call_pixels(W, H)
    _, normal, depth, oid = aov.rebuild(sc, W, H, seed, pixels, SPP)
    truth = ptlib.oracle_render(sc, W, H, TRUTH_SPP, 1000 + seed)[0]
    diffuse = np.array([sc.objs[i].reflect_type == DIFFUSE for i in range(sc.n_objs)])
    return dict(cam=cam, color=color, normal=normal, depth=depth, oid=oid, truth=truth, hit=oid >= 0,
                diffuse=(oid >= 0) & diffuse[np.maximum(oid, 0)])


def step(cur, hist, P):
    """reproject `hist` (a frame with its out / len) onto `cur`"""
    return ref.reproject(W, H, cur["cam"], cur["color"], cur["depth"], cur["oid"], cur["normal"], hist_cam=hist["cam"],
                         hist_color=hist["out"], hist_len=hist["len"], hist_depth=hist["depth"], hist_object_id=hist["oid"],
                         hist_normal=hist["normal"], weight=SPP, **P)


def mae(a, b, mask):
    return float(np.abs(a[mask].astype(np.float64) - b[mask]).mean())


def chain(frames, P):
    """the orbit under P: per frame after the first, (error with history, error without, share), over the hit pixels"""
    hist = dict(frames[0])
    hist["out"], hist["len"] = ref.reproject(W, H, hist["cam"], hist["color"], hist["depth"], hist["oid"], weight=SPP)
    rows = []
    for cur in frames[1:]:
        out, ln = step(cur, hist, P)
        hit = cur["hit"]
        rows.append({"with": mae(out, cur["truth"], hit), "without": mae(cur["color"], cur["truth"], hit),
                     "share": float((ln[hit] > SPP).mean())})
        hist = dict(cur, out=out, len=ln)
    return rows


def main():
    base = ref.cam_dict(ptlib.load_scene_py(ptlib.scene_path("cornell")).cam)
    frames = []
    for k in range(STEPS + 1):
        frames.append(frame(ref.orbit(base, k * ref.ORBIT_DEGREES), 11 + k))
        print("frame %d rendered" % k, flush=True)
    grid = []
    for mh in MAX_HISTORY:
        for dt in DEPTH_TOL:
            for nm in NORMAL_MIN:
                P = dict(max_history=mh, depth_tol=dt, normal_min=nm)
                rows = chain(frames, P)
                g = dict(P, frames=rows, mean_with=float(np.mean([r["with"] for r in rows])),
                         mean_without=float(np.mean([r["without"] for r in rows])), mean_share=float(np.mean([r["share"] for r in rows])))
                grid.append(g)
                print("max_history %-4g depth_tol %-8g normal_min %-5g with %.5f without %.5f share %.3f" % (
                    mh, dt, nm, g["mean_with"], g["mean_without"], g["mean_share"]), flush=True)
    best = min(grid, key=lambda g: g["mean_with"])
    chosen = {k: best[k] for k in ("max_history", "depth_tol", "normal_min")}
    # the end-to-end test: A, then B one step on, history from A alone
    a, b = frames[0], frames[1]
    a = dict(a)
    a["out"], a["len"] = ref.reproject(W, H, a["cam"], a["color"], a["depth"], a["oid"], weight=SPP)
    out, ln = step(b, a, chosen)
    found = b["hit"] & (ln > SPP)
    found_diffuse = found & b["diffuse"]
    e2e = {"degrees": ref.ORBIT_DEGREES, "spp": SPP, "camera_b": b["cam"], "share": float(found[b["hit"]].mean()),
           "all": {"pixels": int(found.sum()), "with": mae(out, b["truth"], found), "without": mae(b["color"], b["truth"], found)},
           "diffuse": {"pixels": int(found_diffuse.sum()), "with": mae(out, b["truth"], found_diffuse),
                       "without": mae(b["color"], b["truth"], found_diffuse)}}
    doc = {
        "command": "python tools/reproject_cpu_study.py",
        "what": "mean |out - truth| over the hit pixels, with history (out of tests/reproject_ref.py) and without (the frame's own "
                "colour), and the share of hit pixels with len_out > wt; cornell %dx%d, an orbit of %d steps of %g degrees, frames = "
                "oracle at %d spp (seeds 11..), guides = oracle first hits, truth = oracle at %d spp per camera" % (
                    W, H, STEPS, ref.ORBIT_DEGREES, SPP, TRUTH_SPP),
        "grid": grid,
        "chosen": chosen,
        "chosen_result": {k: best[k] for k in ("frames", "mean_with", "mean_without", "mean_share")},
        "end_to_end": e2e,
    }
    path = os.path.join(ROOT, "profiles", "reproject_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("chosen:", chosen, "end to end:", e2e, "->", path)


if __name__ == "__main__":
    main()
