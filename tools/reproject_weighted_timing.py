#!/usr/bin/env python3
"""HIP-event time of pt_ctx_reproject_var_weighted and pt_ctx_spp_plane on the GPU, set against pt_ctx_reproject_var in the same
run and process, for DESIGN.md section 4.

tools/reproject_moved_timing.py's inputs, at 1024x768 and 4096x4096, with normals: every pixel on one plane with one normal and a
history length of 32 samples (so that a pixel of every count used here ends long), the history camera 0.01 to the side, so every
tap is taken.  The protocol is tools/timing.py's, on a caller's stream.

The yardstick is pt_ctx_reproject_var at weight 8 (its code is unchanged).  Per size:
  steady-constant   a plane that holds 8 everywhere: the yardstick's arithmetic and its bytes plus the plane's 4 B per pixel
  steady-mixed      counts 4, 8, 16 and 32 by tiles of 8 x 8 pixels, a twentieth of the tiles 0 ("not traced this frame")
The two are the steady state - every pixel with samples ends long, kernel B returns everywhere - and carry the budget of 1.10 x
the yardstick, the factor the moved forms were given: the compulsory bytes grow from 112 to 116 B per pixel.  HIT or MISS is
recorded beside each and gates nothing.  Without a budget:
  first-frame       no history, constant plane, against pt_ctx_reproject_var's first frame: every pixel is short, kernel B stages
                    four planes where the yardstick's stages three
  moved             steady-mixed with a table that moves every pixel's object by 0.4 of a pixel's worth
  spp-plane         pt_ctx_spp_plane with a mask (5 % ones) and without one, against a synchronised device-to-device copy of the
                    colour frame: 5 B (4 B) per pixel against 24

    python tools/reproject_weighted_timing.py [out.json]
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
    timing.need_gpu(L, "reproject_weighted_timing")
    doc = {"command": "python tools/reproject_weighted_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the yardstick "
                     "(pt_ctx_reproject_var, weight 8) is timed in the same run and process, before the cases" % timing.WINDOW_MS,
           "inputs": "tools/reproject_moved_timing.py's: every pixel on one plane (depth %g, one normal, history length 32), the "
                     "history camera 0.01 to the side; with normals; object id 1; planes: 8 everywhere, and 4/8/16/32 by tiles of "
                     "8 x 8 with a twentieth of the tiles 0" % DEPTH,
           "budget": "steady-constant and steady-mixed: %.2f x the yardstick of the same run; the others carry none" % BUDGET,
           "cases": {}}
    rng = np.random.default_rng(1)
    cam_d = kats_camera.CORNELL_CAM
    hist_d = dict(cam_d, position=(0.01, cam_d["position"][1], cam_d["position"][2]))
    cam, hist_cam = ref.pt_camera(cam_d), ref.pt_camera(hist_d)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        for w, h in SIZES:
            npix = w * h
            tiles = rng.choice(np.array([4, 8, 16, 32, 0], dtype=np.uint32), size=((h + 7) // 8, (w + 7) // 8), p=[0.2375] * 4 + [0.05])
            mixed = np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:h, :w]
            planes = dict(color=rng.random(npix * 3, dtype=np.float32), hcolor=rng.random(npix * 3, dtype=np.float32),
                          depth=np.full(npix, DEPTH, dtype=np.float32), oid=np.ones(npix, dtype=np.int32),
                          normal=np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), npix), hlen=np.full(npix, 32.0, dtype=np.float32),
                          hmom=rng.random(npix * 2, dtype=np.float32), out=np.zeros(npix * 3, dtype=np.float32),
                          len=np.zeros(npix, dtype=np.float32), mom=np.zeros(npix * 2, dtype=np.float32), err=np.zeros(npix, dtype=np.float32),
                          constant=np.full(npix, 8, dtype=np.uint32), mixed=np.ascontiguousarray(mixed).reshape(-1),
                          built=np.zeros(npix, dtype=np.uint32), mask=(rng.random(npix) < 0.05).astype(np.uint8))
            B = timing.upload_planes(d, planes)
            share_empty = float((planes["mixed"] == 0).mean())
            del planes
            pixel = DEPTH * cam_d["sensor_width"] / cam_d["focal_length"] / w  # a pixel's width on the plane
            moved_table = mref.table([IDENTITY, (0.4 * pixel, 0.0, 0.0, 1.0)])
            pv = ptlib.PtReprojectVarParams(8, 0.0, 0.0, 0.0, 0, 0, 0)
            guides = (B["color"], B["depth"], B["oid"], B["normal"])
            history = (C.byref(hist_cam), B["hcolor"], B["hlen"], B["hmom"], B["depth"], B["oid"], B["normal"])
            outs = (B["out"], B["len"], B["mom"], B["err"])

            def yardstick(hist=history):
                def call():
                    rc = L.pt_ctx_reproject_var(d.ctx, w, h, C.byref(pv), C.byref(cam), *guides, *hist, *outs, stream)
                    assert rc == 0, L.pt_last_error()
                return call

            def weighted(plane, hist=history, table=None, n_motion=0):
                def call():
                    rc = L.pt_ctx_reproject_var_weighted(d.ctx, w, h, C.byref(pv), C.byref(cam), *guides, B[plane], *hist, *outs, table,
                                                         n_motion, stream)
                    assert rc == 0, L.pt_last_error()
                return call

            def spp_plane(mask):
                def call():
                    rc = L.pt_ctx_spp_plane(d.ctx, w, h, 8, mask, 32, B["built"], stream)
                    assert rc == 0, L.pt_last_error()
                return call

            def shares():
                ln, err = d.download(B["len"], npix), d.download(B["err"], npix)
                return {"mean_len": float(ln.mean()), "share_finite_error": float(np.isfinite(err).mean())}

            copy_sync, _ = timing.copy_yardstick(B["out"], B["color"], npix * 12, stream)
            none = (None,) * 7
            res = {"yardstick": ev.measure(yardstick()), "share_of_count_0": share_empty}
            for case, fn, budget in (("steady-constant", weighted("constant"), True), ("steady-mixed", weighted("mixed"), True),
                                     ("moved", weighted("mixed", table=moved_table, n_motion=2), False)):
                m = ev.measure(fn)
                m.update(shares())
                m["over_yardstick"] = m["ms_median"] / res["yardstick"]["ms_median"]
                if budget:
                    m["budget"] = "HIT" if m["over_yardstick"] <= BUDGET else "MISS"
                res[case] = m
            first = {"yardstick": ev.measure(yardstick(none)), "weighted": ev.measure(weighted("constant", none))}
            first["over_yardstick"] = first["weighted"]["ms_median"] / first["yardstick"]["ms_median"]
            res["first-frame"] = first
            plane = {"copy_of_the_colour_frame": ev.measure(copy_sync), "with_mask": ev.measure(spp_plane(B["mask"])),
                     "without_mask": ev.measure(spp_plane(None))}
            for k in ("with_mask", "without_mask"):
                plane[k]["copies"] = plane[k]["ms_median"] / plane["copy_of_the_colour_frame"]["ms_median"]
            plane["bytes_allow_copies"] = {"with_mask": 5.0 / 24.0, "without_mask": 4.0 / 24.0}
            res["spp-plane"] = plane
            name = "%dx%d" % (w, h)
            doc["cases"][name] = res
            timing.report(name, res)
            timing.free_planes(d, B)
    timing.write(doc, "reproject_weighted_timing.json")


if __name__ == "__main__":
    main()
