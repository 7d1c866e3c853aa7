#!/usr/bin/env python3
"""HIP-event time of pt_ctx_reproject on the GPU, set against a device-to-device copy of the colour frame, for DESIGN.md section 4.

The cases: 1024x768 and 4096x4096, with and without normals.  The history camera is the frame's camera moved sideways by a few
pixels' worth; every pixel sits on one plane with one object id, one normal and a history length of 8, so every tap is taken: the
call moves all of its compulsory traffic, 84 B per pixel with normals (32 read of the frame, 36 of the history, 16 written) and
60 B without.  A copy of the colour frame moves 24 B per pixel, so the budget is 3.5 copies with normals and 2.5 without.  The
protocol is tools/timing.py's, on a caller's stream; the yardstick is its copy of the colour frame on the same stream, timed
twice: with a stream synchronise after every copy (the like-for-like figure, "copy_sync") and back to back ("copy").

    python tools/reproject_timing.py [out.json]
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
import timing  # noqa: E402

CASES = (("1024x768 with normals", (1024, 768), True, 3.5), ("1024x768 without normals", (1024, 768), False, 2.5),
         ("4096x4096 with normals", (4096, 4096), True, 3.5), ("4096x4096 without normals", (4096, 4096), False, 2.5))
DEPTH = 6.0


def main():
    L = ptlib.product()
    timing.need_gpu(L, "reproject_timing")
    doc = {"command": "python tools/reproject_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % timing.WINDOW_MS,
           "inputs": "every pixel on one plane (depth %g, one id, one normal, history length 8), the history camera 0.01 to the side: "
                     "every tap is taken" % DEPTH,
           "cases": {}}
    rng = np.random.default_rng(1)
    cam_d = kats_camera.CORNELL_CAM
    hist_d = dict(cam_d, position=(0.01, cam_d["position"][1], cam_d["position"][2]))
    cam, hist_cam = ref.pt_camera(cam_d), ref.pt_camera(hist_d)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        B, size = {}, None
        for name, (w, h), normals, budget in CASES:
            npix = w * h
            if size != (w, h):
                timing.free_planes(d, B)
                size = (w, h)
                planes = dict(color=rng.random(npix * 3, dtype=np.float32), hcolor=rng.random(npix * 3, dtype=np.float32),
                              depth=np.full(npix, DEPTH, dtype=np.float32), hdepth=np.full(npix, DEPTH, dtype=np.float32),
                              oid=np.ones(npix, dtype=np.int32), hoid=np.ones(npix, dtype=np.int32),
                              normal=np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), npix), hlen=np.full(npix, 8.0, dtype=np.float32),
                              out=np.zeros(npix * 3, dtype=np.float32), len=np.zeros(npix, dtype=np.float32),
                              copy=np.zeros(npix * 3, dtype=np.float32))
                planes["hnormal"] = planes["normal"]
                B = timing.upload_planes(d, planes)
                del planes
            pp = ptlib.PtReprojectParams(8, 0.0, 0.0, 0.0, 0)

            def reproject():
                rc = L.pt_ctx_reproject(d.ctx, w, h, C.byref(pp), C.byref(cam), B["color"], B["depth"], B["oid"],
                                        B["normal"] if normals else None, C.byref(hist_cam), B["hcolor"], B["hlen"], B["hdepth"], B["hoid"],
                                        B["hnormal"] if normals else None, B["out"], B["len"], stream)
                assert rc == 0, L.pt_last_error()

            copy_sync, copy = timing.copy_yardstick(B["copy"], B["color"], npix * 12, stream)
            res = {"reproject": ev.measure(reproject), "copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy), "budget_in_copies": budget}
            res["share_blended"] = float((d.download(B["len"], npix) == 16.0).mean())  # every pixel but the column that left the history frame
            res["reproject_over_copy_sync"] = res["reproject"]["ms_median"] / res["copy_sync"]["ms_median"]
            res["reproject_over_copy"] = res["reproject"]["ms_median"] / res["copy"]["ms_median"]
            res["budget"] = "HIT" if res["reproject_over_copy_sync"] <= budget else "MISSES"
            res["bytes_moved"] = npix * (84 if normals else 60)
            res["GB_per_s"] = res["bytes_moved"] / (res["reproject"]["ms_median"] * 1e6)
            doc["cases"][name] = res
            timing.report(name, res)
    timing.write(doc, "reproject_timing.json")


if __name__ == "__main__":
    main()
