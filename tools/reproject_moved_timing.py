#!/usr/bin/env python3
"""HIP-event time of pt_ctx_reproject_moved and pt_ctx_reproject_var_moved on the GPU, set against pt_ctx_reproject and
pt_ctx_reproject_var in the same run, for DESIGN.md section 4.

tools/reproject_timing.py's inputs, at 1024x768 and 4096x4096, with normals: every pixel on one plane with one normal and a
history length of 8, the history camera 0.01 to the side, so every tap is taken.  The protocol is tools/timing.py's, on a caller's
stream.  The calls block, so a window holds the host's turn-around too - the yardstick's as much as the moved call's, which also
holds the copy of the table (16 B per record, host to device, on the stream).

The yardstick is the plain call (its code is unchanged).  Three cases per size and call:
  identity    every record IDENTITY: the call delegates to the plain launch and copies nothing - expected ratio 1
  one-object  an object of about 5 % of the pixels (a rectangle in the middle of the frame, object id 2) moved by three pixels'
              worth; every other record IDENTITY
  all-moved   every pixel's object moved by 0.4 of a pixel's worth
The moved kernels have the plain kernels' compulsory bytes plus 16 B x n_motion once, so the budget of the two moved cases is
1.10 x the yardstick; HIT or MISS is recorded beside each case and gates nothing.

    python tools/reproject_moved_timing.py [out.json]
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
import reproject_moved_ref as mref  # noqa: E402
import reproject_ref as ref  # noqa: E402
import timing  # noqa: E402
from reproject_moved_ref import IDENTITY  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
DEPTH = 6.0
BUDGET = 1.10


def main():
    L = ptlib.product()
    timing.need_gpu(L, "reproject_moved_timing")
    doc = {"command": "python tools/reproject_moved_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the yardstick "
                     "(the plain call) is timed in the same run, before the three cases" % timing.WINDOW_MS,
           "inputs": "tools/reproject_timing.py's: every pixel on one plane (depth %g, one normal, history length 8), the history "
                     "camera 0.01 to the side; with normals; object id 1 everywhere but a rectangle of about 5 %% of the pixels in the "
                     "middle, id 2; n_motion 3" % DEPTH,
           "budget": "moved cases: %.2f x the plain call of the same run; identity: delegation, expected ratio 1" % BUDGET,
           "cases": {}}
    rng = np.random.default_rng(1)
    cam_d = kats_camera.CORNELL_CAM
    hist_d = dict(cam_d, position=(0.01, cam_d["position"][1], cam_d["position"][2]))
    cam, hist_cam = ref.pt_camera(cam_d), ref.pt_camera(hist_d)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        for w, h in SIZES:
            npix = w * h
            oid = np.ones((h, w), dtype=np.int32)
            bw, bh = int(w * 0.224), int(h * 0.224)  # 0.224^2 = 5 % of the frame
            oid[(h - bh) // 2:(h + bh) // 2, (w - bw) // 2:(w + bw) // 2] = 2
            planes = dict(color=rng.random(npix * 3, dtype=np.float32), hcolor=rng.random(npix * 3, dtype=np.float32),
                          depth=np.full(npix, DEPTH, dtype=np.float32), oid=oid.reshape(-1),
                          normal=np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), npix), hlen=np.full(npix, 8.0, dtype=np.float32),
                          hmom=rng.random(npix * 2, dtype=np.float32), out=np.zeros(npix * 3, dtype=np.float32),
                          len=np.zeros(npix, dtype=np.float32), mom=np.zeros(npix * 2, dtype=np.float32), err=np.zeros(npix, dtype=np.float32))
            B = timing.upload_planes(d, planes)
            share = float((oid == 2).mean())
            del planes
            pixel = DEPTH * cam_d["sensor_width"] / cam_d["focal_length"] / w  # a pixel's width on the plane
            tables = {"identity": [IDENTITY] * 3, "one-object": [IDENTITY, IDENTITY, (3.0 * pixel, 0.0, 0.0, 1.0)],
                      "all-moved": [IDENTITY, (0.4 * pixel, 0.0, 0.0, 1.0), (0.4 * pixel, 0.0, 0.0, 1.0)]}
            pp = ptlib.PtReprojectParams(8, 0.0, 0.0, 0.0, 0)
            pv = ptlib.PtReprojectVarParams(8, 0.0, 0.0, 0.0, 0, 0, 0)
            guides = (B["color"], B["depth"], B["oid"], B["normal"])

            def plain():
                rc = L.pt_ctx_reproject(d.ctx, w, h, C.byref(pp), C.byref(cam), *guides, C.byref(hist_cam), B["hcolor"], B["hlen"], B["depth"],
                                        B["oid"], B["normal"], B["out"], B["len"], stream)
                assert rc == 0, L.pt_last_error()

            def plain_var():
                rc = L.pt_ctx_reproject_var(d.ctx, w, h, C.byref(pv), C.byref(cam), *guides, C.byref(hist_cam), B["hcolor"], B["hlen"],
                                            B["hmom"], B["depth"], B["oid"], B["normal"], B["out"], B["len"], B["mom"], B["err"], stream)
                assert rc == 0, L.pt_last_error()

            def moved(t):
                def call():
                    rc = L.pt_ctx_reproject_moved(d.ctx, w, h, C.byref(pp), C.byref(cam), *guides, C.byref(hist_cam), B["hcolor"], B["hlen"],
                                                  B["depth"], B["oid"], B["normal"], B["out"], B["len"], t, 3, stream)
                    assert rc == 0, L.pt_last_error()
                return call

            def moved_var(t):
                def call():
                    rc = L.pt_ctx_reproject_var_moved(d.ctx, w, h, C.byref(pv), C.byref(cam), *guides, C.byref(hist_cam), B["hcolor"],
                                                      B["hlen"], B["hmom"], B["depth"], B["oid"], B["normal"], B["out"], B["len"], B["mom"],
                                                      B["err"], t, 3, stream)
                    assert rc == 0, L.pt_last_error()
                return call

            for family, yard, make in (("pt_ctx_reproject_moved", plain, moved), ("pt_ctx_reproject_var_moved", plain_var, moved_var)):
                res = {"yardstick": ev.measure(yard), "share_of_object_2": share}
                for case, records in tables.items():
                    m = ev.measure(make(mref.table(records)))
                    m["share_blended"] = float((d.download(B["len"], npix) == 16.0).mean())
                    m["over_yardstick"] = m["ms_median"] / res["yardstick"]["ms_median"]
                    if case == "identity":
                        m["expected"] = "1 (delegation)"
                    else:
                        m["budget"] = "HIT" if m["over_yardstick"] <= BUDGET else "MISS"
                    res[case] = m
                name = "%dx%d %s" % (w, h, family)
                doc["cases"][name] = res
                timing.report(name, res)
            timing.free_planes(d, B)
    timing.write(doc, "reproject_moved_timing.json")


if __name__ == "__main__":
    main()
