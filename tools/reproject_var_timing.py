#!/usr/bin/env python3
"""HIP-event time of pt_ctx_reproject_var on the GPU, set against pt_ctx_reproject timed in the same run, for DESIGN.md section 4.

The method is tools/reproject_timing.py's: after a warm-up, N back-to-back calls on a caller's stream are put between two HIP
events, N chosen so that the window is at least 0.25 s, and the window is divided by N; five such windows give the median and
the spread.  Both entry points block, so a window holds the host's turn-around between calls too - for both alike.  The sizes
are 1024x768 and 4096x4096, with normals; the inputs are that tool's (one plane, one id, one normal, a history length of 8, the
history camera a few pixels to the side: every tap is taken).  The cases:
  (a) steady state: a history, min_frames = 1, so every pixel is long and every workgroup of the second kernel returns after
      reading its tile's markers.  The call moves 112 B per pixel (32 read of the frame, 36 + 8 of the history, 16 + 8 + 4 + 4
      written) plus the markers read back, against pt_ctx_reproject's 84: the budget is 1.5 times pt_ctx_reproject's time.
  (b) the first frame: no history, the defaults, so every pixel is short and every workgroup stages its tile and runs the
      window.  No budget; recorded.

    python tools/reproject_var_timing.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import kats_camera  # noqa: E402
import ptlib  # noqa: E402
import reproject_ref as ref  # noqa: E402
import reproject_var_ref as rv  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
BUDGET = 1.5
WINDOW_MS = 250.0
DEPTH = 6.0
WEIGHT = 8


def main(stream):
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "reproject_var_timing needs a GPU: there is nothing to time without one"
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert L.pt_ctx_create(0, C.byref(ctx)) == 0, L.pt_last_error()
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    defaults = rv.defaults(L)
    doc = {"command": "python tools/reproject_var_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % WINDOW_MS,
           "inputs": "every pixel on one plane (depth %g, one id, one normal, history length 8, weight %d), the history camera 0.01 "
                     "to the side: every tap is taken; with normals" % (DEPTH, WEIGHT),
           "defaults": defaults, "budget": "steady <= %g x pt_ctx_reproject" % BUDGET, "cases": {}}
    rng = np.random.default_rng(1)

    def timed(fn, n):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(n):
            fn()
        assert hip.hipEventRecord(e1, stream) == 0
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value

    def measure(fn):
        timed(fn, 20)  # warm-up: code objects
        n = max(20, int(WINDOW_MS / (timed(fn, 50) / 50)) + 1)
        per = [timed(fn, n) / n for _ in range(5)]
        return {"calls_per_window": n, "ms_median": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}

    cam_d = kats_camera.CORNELL_CAM
    hist_d = dict(cam_d, position=(0.01, cam_d["position"][1], cam_d["position"][2]))
    cam, hist_cam = ref.pt_camera(cam_d), ref.pt_camera(hist_d)
    for w, h in SIZES:
        npix = w * h
        planes = dict(color=rng.random(npix * 3, dtype=np.float32), hcolor=rng.random(npix * 3, dtype=np.float32),
                      depth=np.full(npix, DEPTH, dtype=np.float32), hdepth=np.full(npix, DEPTH, dtype=np.float32),
                      oid=np.ones(npix, dtype=np.int32), hoid=np.ones(npix, dtype=np.int32),
                      normal=np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), npix), hlen=np.full(npix, 8.0, dtype=np.float32),
                      hmom=rng.random(npix * 2, dtype=np.float32), out=np.zeros(npix * 3, dtype=np.float32),
                      len=np.zeros(npix, dtype=np.float32), mom=np.zeros(npix * 2, dtype=np.float32), err=np.zeros(npix, dtype=np.float32))
        planes["hnormal"] = planes["normal"]
        B = {}
        for k, v in planes.items():
            B[k] = C.c_void_p()
            assert L.pt_device_malloc(0, v.nbytes, C.byref(B[k])) == 0, L.pt_last_error()
            assert hip.hipMemcpy(B[k], v.ctypes.data_as(C.c_void_p), v.nbytes, 1) == 0
        del planes
        pp = ptlib.PtReprojectParams(WEIGHT, 0.0, 0.0, 0.0, 0)
        steady_p = ptlib.PtReprojectVarParams(WEIGHT, 0.0, 0.0, 0.0, 1, 0, 0)
        first_p = ptlib.PtReprojectVarParams(WEIGHT, 0.0, 0.0, 0.0, 0, 0, 0)

        def reproject():
            rc = L.pt_ctx_reproject(ctx, w, h, C.byref(pp), C.byref(cam), B["color"], B["depth"], B["oid"], B["normal"], C.byref(hist_cam),
                                    B["hcolor"], B["hlen"], B["hdepth"], B["hoid"], B["hnormal"], B["out"], B["len"], stream)
            assert rc == 0, L.pt_last_error()

        def steady():
            rc = L.pt_ctx_reproject_var(ctx, w, h, C.byref(steady_p), C.byref(cam), B["color"], B["depth"], B["oid"], B["normal"],
                                        C.byref(hist_cam), B["hcolor"], B["hlen"], B["hmom"], B["hdepth"], B["hoid"], B["hnormal"],
                                        B["out"], B["len"], B["mom"], B["err"], stream)
            assert rc == 0, L.pt_last_error()

        def first():
            rc = L.pt_ctx_reproject_var(ctx, w, h, C.byref(first_p), C.byref(cam), B["color"], B["depth"], B["oid"], B["normal"], None,
                                        None, None, None, None, None, None, B["out"], B["len"], B["mom"], B["err"], stream)
            assert rc == 0, L.pt_last_error()

        def share(pred):
            ln = np.zeros(npix, dtype=np.float32)
            assert L.pt_device_download(0, ln.ctypes.data_as(C.c_void_p), B["len"], ln.nbytes) == 0
            return float(pred(ln).mean())

        res = {"reproject": measure(reproject)}
        res["steady"] = measure(steady)
        res["steady"]["share_long"] = share(lambda ln: ln >= WEIGHT * 1)
        res["steady"]["share_blended"] = share(lambda ln: ln == 16.0)
        res["first_frame"] = measure(first)
        res["first_frame"]["share_short"] = share(lambda ln: ln < WEIGHT * defaults["min_frames"])
        res["steady_over_reproject"] = res["steady"]["ms_median"] / res["reproject"]["ms_median"]
        res["first_frame_over_reproject"] = res["first_frame"]["ms_median"] / res["reproject"]["ms_median"]
        res["budget"] = "HIT" if res["steady_over_reproject"] <= BUDGET else "MISSES"
        res["steady_GB_per_s"] = npix * 112 / (res["steady"]["ms_median"] * 1e6)
        res["reproject_GB_per_s"] = npix * 84 / (res["reproject"]["ms_median"] * 1e6)
        doc["cases"]["%dx%d" % (w, h)] = res
        print("%dx%d" % (w, h), json.dumps(res), flush=True)
        for p in B.values():
            L.pt_device_free(0, p)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reproject_var_timing.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
