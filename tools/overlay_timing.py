#!/usr/bin/env python3
"""HIP-event time of pt_ctx_overlay on the GPU, set against a device-to-device copy of the colour frame measured in the same run,
for the README's bullet and DESIGN.md section 4.

Sizes: 1024x768 and 4096x4096.  Cases: nothing selected, in place (the pass then costs the id plane: 4 B per pixel); one object - a
disc covering about 4 % of the frame - selected, out of place, at R = 2 and at R = 8 (4 B of ids, 12 B read, 12 B written: 28 B);
sky and grid both on over the same planes, out of place (the depth plane too: 32 B).  The yardstick copies 24 B per pixel, so a
case's budget is its compulsory bytes / 24 of the copy's time.  A call is far below a millisecond, so one call is not timed: after
a warm-up of the same shape, N back-to-back calls are put between two HIP events - on the null stream: the call takes no stream,
and as it blocks, everything it issued is complete when the second event is recorded - N chosen so that the window is at least
0.25 s, and the window is divided by N; five such windows give the median and the spread.  pt_ctx_overlay ends in a
stream synchronise, so its window holds the host's turn-around between calls too: the like-for-like yardstick is the copy with a
stream synchronise after each ("copy_sync"); the back-to-back copy ("copy") is recorded beside it.

    python tools/overlay_timing.py [out.json]
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
import overlay_ref as ref  # noqa: E402
import ptlib  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
WINDOW_MS = 250.0
COPY_BYTES = 24
CAM = dict(position=(0.5, 3.0, 4.0), direction=(-0.1, -0.6, -0.79), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)


def main():
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "overlay_timing needs a GPU: there is nothing to time without one"
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    doc = {"command": "python tools/overlay_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the ratio is "
                     "against the copy with a stream synchronise after each, the budget is compulsory bytes / %d" % (WINDOW_MS, COPY_BYTES),
           "cases": {}}
    rng = np.random.default_rng(1)

    def timed(fn, n):
        assert hip.hipEventRecord(e0, None) == 0
        for _ in range(n):
            fn()
        assert hip.hipEventRecord(e1, None) == 0
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value

    def measure(fn):
        timed(fn, 20)
        n = max(20, int(WINDOW_MS / (timed(fn, 50) / 50)) + 1)
        per = [timed(fn, n) / n for _ in range(5)]
        return {"calls_per_window": n, "ms_median": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}

    with gpudev.Device(L) as d:
        cam = ref.pt_camera(CAM)
        for w, h in SIZES:
            n = w * h
            d_rgb, d_out, d_id, d_z = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 4)
            d.upload(d_rgb, rng.random(n * 3, dtype=np.float32))
            yy, xx = np.mgrid[0:h, 0:w]
            disc = (xx - w // 2) ** 2 + (yy - h // 2) ** 2 <= int(0.04 * n / np.pi)  # one object over about 4 % of the frame
            oid = np.where(disc, 1, 0).astype(np.int32)
            oid[: h // 4, :] = -1  # a quarter of the frame is sky
            d.upload(d_id, oid.reshape(n))
            d.upload(d_z, np.where(oid.reshape(n) < 0, np.float32(np.inf), (4.0 + 8.0 * rng.random(n)).astype(np.float32)).astype(np.float32))
            base = ref.defaults(L, CAM)

            def copy_sync():
                assert hip.hipMemcpyAsync(d_out, d_rgb, n * 12, 3, None) == 0  # device to device
                assert hip.hipStreamSynchronize(None) == 0

            def copy():
                assert hip.hipMemcpyAsync(d_out, d_rgb, n * 12, 3, None) == 0

            yard = {"copy_sync": measure(copy_sync), "copy": measure(copy)}
            cases = (("nothing selected, in place", dict(base, selected=(7,)), d_rgb, 4),
                     ("one object, out of place, R = 2", dict(base, selected=(1,), radius=2), d_out, 28),
                     ("one object, out of place, R = 8", dict(base, selected=(1,), radius=8), d_out, 28),
                     ("sky and grid, out of place", dict(base, flags=ref.SKY | ref.GRID, selected=(1,)), d_out, 32))
            for name, p, out, nbytes in cases:
                s = ref.struct(p)

                def overlay():
                    assert L.pt_ctx_overlay(d.ctx, w, h, C.byref(s), C.byref(cam), d_rgb, d_id, d_z, out) == 0, L.pt_last_error()

                res = {"overlay": measure(overlay), "compulsory_bytes_per_pixel": nbytes, "budget_in_copies": nbytes / COPY_BYTES}
                res.update(yard)
                res["overlay_over_copy_sync"] = res["overlay"]["ms_median"] / yard["copy_sync"]["ms_median"]
                res["overlay_over_copy"] = res["overlay"]["ms_median"] / yard["copy"]["ms_median"]
                res["within_budget"] = res["overlay_over_copy_sync"] <= res["budget_in_copies"]
                doc["cases"]["%dx%d %s" % (w, h, name)] = res
                print("%dx%d %s" % (w, h, name), "%.4f ms, %.2f copies (budget %.2f): %s" % (
                    res["overlay"]["ms_median"], res["overlay_over_copy_sync"], res["budget_in_copies"],
                    "HIT" if res["within_budget"] else "MISS"), flush=True)
            for p in (d_rgb, d_out, d_id, d_z):
                d.free(p)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "overlay_timing.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
