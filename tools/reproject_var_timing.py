#!/usr/bin/env python3
"""HIP-event time of pt_ctx_reproject_var on the GPU, set against pt_ctx_reproject timed in the same run, for DESIGN.md section 4.

The protocol is tools/timing.py's, on a caller's stream.  Both entry points block, so a window holds the host's turn-around
between calls too - for both alike.  The sizes are 1024x768 and 4096x4096, with normals; the inputs are
tools/reproject_timing.py's (one plane, one id, one normal, a history length of 8, the history camera a few pixels to the side:
every tap is taken).  The cases:
  (a) steady state: a history, min_frames = 1, so every pixel is long and every workgroup of the second kernel returns after
      reading its tile's markers.  The call moves 112 B per pixel (32 read of the frame, 36 + 8 of the history, 16 + 8 + 4 + 4
      written) plus the markers read back, against pt_ctx_reproject's 84: the budget is 1.5 times pt_ctx_reproject's time.
  (b) the first frame: no history, the defaults, so every pixel is short and every workgroup stages its tile and runs the
      window.  No budget; recorded.

    python tools/reproject_var_timing.py [out.json]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import kats_camera  # noqa: E402
import ptlib  # noqa: E402
import reproject_ref as ref  # noqa: E402
import reproject_var_ref as rv  # noqa: E402
import timing  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
BUDGET = 1.5
DEPTH = 6.0
WEIGHT = 8


def main():
    L = ptlib.product()
    timing.need_gpu(L, "reproject_var_timing")
    defaults = rv.defaults(L)
    doc = {"command": "python tools/reproject_var_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % timing.WINDOW_MS,
           "inputs": "every pixel on one plane (depth %g, one id, one normal, history length 8, weight %d), the history camera 0.01 "
                     "to the side: every tap is taken; with normals" % (DEPTH, WEIGHT),
           "defaults": defaults, "budget": "steady <= %g x pt_ctx_reproject" % BUDGET, "cases": {}}
    rng = np.random.default_rng(1)
    cam_d = kats_camera.CORNELL_CAM
    hist_d = dict(cam_d, position=(0.01, cam_d["position"][1], cam_d["position"][2]))
    cam, hist_cam = ref.pt_camera(cam_d), ref.pt_camera(hist_d)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        for w, h in SIZES:
            npix = w * h
            planes = dict(color=rng.random(npix * 3, dtype=np.float32), hcolor=rng.random(npix * 3, dtype=np.float32),
                          depth=np.full(npix, DEPTH, dtype=np.float32), hdepth=np.full(npix, DEPTH, dtype=np.float32),
                          oid=np.ones(npix, dtype=np.int32), hoid=np.ones(npix, dtype=np.int32),
                          normal=np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), npix), hlen=np.full(npix, 8.0, dtype=np.float32),
                          hmom=rng.random(npix * 2, dtype=np.float32), out=np.zeros(npix * 3, dtype=np.float32),
                          len=np.zeros(npix, dtype=np.float32), mom=np.zeros(npix * 2, dtype=np.float32), err=np.zeros(npix, dtype=np.float32))
            planes["hnormal"] = planes["normal"]
            B = timing.upload_planes(d, planes)
            del planes
            pp = ptlib.PtReprojectParams(WEIGHT, 0.0, 0.0, 0.0, 0)
            steady_p = ptlib.PtReprojectVarParams(WEIGHT, 0.0, 0.0, 0.0, 1, 0, 0)
            first_p = ptlib.PtReprojectVarParams(WEIGHT, 0.0, 0.0, 0.0, 0, 0, 0)

            def reproject():
                rc = L.pt_ctx_reproject(d.ctx, w, h, C.byref(pp), C.byref(cam), B["color"], B["depth"], B["oid"], B["normal"],
                                        C.byref(hist_cam), B["hcolor"], B["hlen"], B["hdepth"], B["hoid"], B["hnormal"], B["out"], B["len"], stream)
                assert rc == 0, L.pt_last_error()

            def steady():
                rc = L.pt_ctx_reproject_var(d.ctx, w, h, C.byref(steady_p), C.byref(cam), B["color"], B["depth"], B["oid"], B["normal"],
                                            C.byref(hist_cam), B["hcolor"], B["hlen"], B["hmom"], B["hdepth"], B["hoid"], B["hnormal"],
                                            B["out"], B["len"], B["mom"], B["err"], stream)
                assert rc == 0, L.pt_last_error()

            def first():
                rc = L.pt_ctx_reproject_var(d.ctx, w, h, C.byref(first_p), C.byref(cam), B["color"], B["depth"], B["oid"], B["normal"], None,
                                            None, None, None, None, None, None, B["out"], B["len"], B["mom"], B["err"], stream)
                assert rc == 0, L.pt_last_error()

            def share(pred):
                return float(pred(d.download(B["len"], npix)).mean())

            res = {"reproject": ev.measure(reproject)}
            res["steady"] = ev.measure(steady)
            res["steady"]["share_long"] = share(lambda ln: ln >= WEIGHT * 1)
            res["steady"]["share_blended"] = share(lambda ln: ln == 16.0)
            res["first_frame"] = ev.measure(first)
            res["first_frame"]["share_short"] = share(lambda ln: ln < WEIGHT * defaults["min_frames"])
            res["steady_over_reproject"] = res["steady"]["ms_median"] / res["reproject"]["ms_median"]
            res["first_frame_over_reproject"] = res["first_frame"]["ms_median"] / res["reproject"]["ms_median"]
            res["budget"] = "HIT" if res["steady_over_reproject"] <= BUDGET else "MISSES"
            res["steady_GB_per_s"] = npix * 112 / (res["steady"]["ms_median"] * 1e6)
            res["reproject_GB_per_s"] = npix * 84 / (res["reproject"]["ms_median"] * 1e6)
            doc["cases"]["%dx%d" % (w, h)] = res
            timing.report("%dx%d" % (w, h), res)
            timing.free_planes(d, B)
    timing.write(doc, "reproject_var_timing.json")


if __name__ == "__main__":
    main()
