#!/usr/bin/env python3
"""HIP-event time of pt_ctx_overlay on the GPU, set against a device-to-device copy of the colour frame measured in the same run,
for the README's bullet and DESIGN.md section 4.

Sizes: 1024x768 and 4096x4096.  Cases: nothing selected, in place (the pass then costs the id plane: 4 B per pixel); one object - a
disc covering about 4 % of the frame - selected, out of place, at R = 2 and at R = 8 (4 B of ids, 12 B read, 12 B written: 28 B);
sky and grid both on over the same planes, out of place (the depth plane too: 32 B).  The yardstick copies 24 B per pixel, so a
case's budget is its compulsory bytes / 24 of the copy's time.  The protocol is tools/timing.py's, on the null stream: the call
takes no stream, and as it blocks, everything it issued is complete when the second event is recorded.  The like-for-like yardstick
is the copy with a stream synchronise after each ("copy_sync"); the back-to-back copy ("copy") is recorded beside it.

    python tools/overlay_timing.py [out.json]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import overlay_ref as ref  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
COPY_BYTES = 24
CAM = dict(position=(0.5, 3.0, 4.0), direction=(-0.1, -0.6, -0.79), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)


def main():
    L = ptlib.product()
    timing.need_gpu(L, "overlay_timing")
    doc = {"command": "python tools/overlay_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the ratio is "
                     "against the copy with a stream synchronise after each, the budget is compulsory bytes / %d" % (timing.WINDOW_MS, COPY_BYTES),
           "cases": {}}
    rng = np.random.default_rng(1)
    with timing.Events() as ev, gpudev.Device(L) as d:
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
            copy_sync, copy = timing.copy_yardstick(d_out, d_rgb, n * 12)
            yard = {"copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy)}
            cases = (("nothing selected, in place", dict(base, selected=(7,)), d_rgb, 4),
                     ("one object, out of place, R = 2", dict(base, selected=(1,), radius=2), d_out, 28),
                     ("one object, out of place, R = 8", dict(base, selected=(1,), radius=8), d_out, 28),
                     ("sky and grid, out of place", dict(base, flags=ref.SKY | ref.GRID, selected=(1,)), d_out, 32))
            for name, p, out, nbytes in cases:
                s = ref.struct(p)

                def overlay():
                    assert L.pt_ctx_overlay(d.ctx, w, h, C.byref(s), C.byref(cam), d_rgb, d_id, d_z, out) == 0, L.pt_last_error()

                res = {"overlay": ev.measure(overlay), "compulsory_bytes_per_pixel": nbytes, "budget_in_copies": nbytes / COPY_BYTES}
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
    timing.write(doc, "overlay_timing.json")


if __name__ == "__main__":
    main()
