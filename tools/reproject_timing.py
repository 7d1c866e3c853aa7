#!/usr/bin/env python3
"""HIP-event time of pt_ctx_reproject on the GPU, set against a device-to-device copy of the colour frame, for DESIGN.md section 4.

The cases: 1024x768 and 4096x4096, with and without normals.  The history camera is the frame's camera moved sideways by a few
pixels' worth; every pixel sits on one plane with one object id, one normal and a history length of 8, so every tap is taken: the
call moves all of its compulsory traffic, 84 B per pixel with normals (32 read of the frame, 36 of the history, 16 written) and
60 B without.  A copy of the colour frame moves 24 B per pixel, so the budget is 3.5 copies with normals and 2.5 without.  A call
is far below a millisecond at the small size, so one call is not timed: after a warm-up, N back-to-back calls on a caller's stream
are put between two HIP events, N chosen so that the window is at least 0.25 s, and the window is divided by N; five such windows
give the median and the spread.  pt_ctx_reproject blocks (it ends in a stream synchronise), so its window holds the host's
turn-around between calls too.  The yardstick is hipMemcpyAsync, device to device, of the colour frame on the same stream,
timed twice: with a stream synchronise after every copy (the like-for-like figure, "copy_sync") and back to back ("copy").

    python tools/reproject_timing.py [out.json]
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

CASES = (("1024x768 with normals", (1024, 768), True, 3.5), ("1024x768 without normals", (1024, 768), False, 2.5),
         ("4096x4096 with normals", (4096, 4096), True, 3.5), ("4096x4096 without normals", (4096, 4096), False, 2.5))
WINDOW_MS = 250.0
DEPTH = 6.0


def main(stream):
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "reproject_timing needs a GPU: there is nothing to time without one"
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert L.pt_ctx_create(0, C.byref(ctx)) == 0, L.pt_last_error()
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    doc = {"command": "python tools/reproject_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % WINDOW_MS,
           "inputs": "every pixel on one plane (depth %g, one id, one normal, history length 8), the history camera 0.01 to the side: "
                     "every tap is taken" % DEPTH,
           "cases": {}}
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
    bufs = {}
    size = None
    for name, (w, h), normals, budget in CASES:
        npix = w * h
        if size != (w, h):
            for p in bufs.values():
                L.pt_device_free(0, p)
            bufs, size = {}, (w, h)
            planes = dict(color=rng.random(npix * 3, dtype=np.float32), hcolor=rng.random(npix * 3, dtype=np.float32),
                          depth=np.full(npix, DEPTH, dtype=np.float32), hdepth=np.full(npix, DEPTH, dtype=np.float32),
                          oid=np.ones(npix, dtype=np.int32), hoid=np.ones(npix, dtype=np.int32),
                          normal=np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), npix), hlen=np.full(npix, 8.0, dtype=np.float32),
                          out=np.zeros(npix * 3, dtype=np.float32), len=np.zeros(npix, dtype=np.float32),
                          copy=np.zeros(npix * 3, dtype=np.float32))
            planes["hnormal"] = planes["normal"]
            for k, v in planes.items():
                bufs[k] = C.c_void_p()
                assert L.pt_device_malloc(0, v.nbytes, C.byref(bufs[k])) == 0, L.pt_last_error()
                assert hip.hipMemcpy(bufs[k], v.ctypes.data_as(C.c_void_p), v.nbytes, 1) == 0
            del planes
        pp = ptlib.PtReprojectParams(8, 0.0, 0.0, 0.0, 0)
        B = bufs

        def reproject():
            rc = L.pt_ctx_reproject(ctx, w, h, C.byref(pp), C.byref(cam), B["color"], B["depth"], B["oid"],
                                    B["normal"] if normals else None, C.byref(hist_cam), B["hcolor"], B["hlen"], B["hdepth"], B["hoid"],
                                    B["hnormal"] if normals else None, B["out"], B["len"], stream)
            assert rc == 0, L.pt_last_error()

        def copy():
            assert hip.hipMemcpyAsync(B["copy"], B["color"], npix * 12, 3, stream) == 0  # device to device

        def copy_sync():
            copy()
            assert hip.hipStreamSynchronize(stream) == 0

        res = {"reproject": measure(reproject), "copy_sync": measure(copy_sync), "copy": measure(copy), "budget_in_copies": budget}
        ln = np.zeros(npix, dtype=np.float32)
        assert L.pt_device_download(0, ln.ctypes.data_as(C.c_void_p), B["len"], ln.nbytes) == 0
        res["share_blended"] = float((ln == 16.0).mean())  # every pixel but the column that left the history frame
        res["reproject_over_copy_sync"] = res["reproject"]["ms_median"] / res["copy_sync"]["ms_median"]
        res["reproject_over_copy"] = res["reproject"]["ms_median"] / res["copy"]["ms_median"]
        res["budget"] = "HIT" if res["reproject_over_copy_sync"] <= budget else "MISSES"
        res["bytes_moved"] = npix * (84 if normals else 60)
        res["GB_per_s"] = res["bytes_moved"] / (res["reproject"]["ms_median"] * 1e6)
        doc["cases"][name] = res
        print(name, json.dumps(res), flush=True)
    for p in bufs.values():
        L.pt_device_free(0, p)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reproject_timing.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
