#!/usr/bin/env python3
"""HIP-event time of pt_ctx_solid on the GPU, set against a device-to-device copy of the colour frame measured in the same run,
for the README's bullet and DESIGN.md section 4 - in the style of tools/overlay_timing.py - and what the view buys: the wall
time of a frame of the solid loop beside the traced loop's front end.

The pass.  Sizes: 1024x768 and 4096x4096.  Cases: with albedo, out of place (12 B albedo, 12 B normal, 4 B depth, 4 B id read,
12 B written: 44 B per pixel); without albedo (32 B); in place on the albedo (44 B); a frame that is all misses (the ids read,
the background written: 16 B - the yardstick's convention counts its 12 B written against the copy's 24 B, a budget of 0.5
copies).  The planes are synthetic: a disc of one object over a floor of another, a quarter of the frame sky, a table of three
records.  The yardstick copies 24 B per pixel, so a case's budget is its compulsory bytes / 24 of the copy's time.  The protocol
is tools/timing.py's, on the null stream; the like-for-like yardstick is the copy with a stream synchronise after each
("copy_sync"), the back-to-back copy ("copy") is recorded beside it.

The loop.  On cornell and mesh.json at 1024x768, wall time per frame (timing.wall), median of 30, of
  solid:  pt_ctx_render_aov(1 spp) + pt_ctx_solid + pt_ctx_overlay (sky, grid, one object selected) + pt_ctx_present
  traced: pt_ctx_render(8 spp) + pt_ctx_render_aov(8 spp) - the front end of the traced loop, as tools/upsample_timing.py's
          "full" chain makes it, before any reprojection, denoiser, overlay or present.

    python tools/solid_timing.py [out.json]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import overlay_ref  # noqa: E402
import ptlib  # noqa: E402
import solid_ref as ref  # noqa: E402
import timing  # noqa: E402
from ptlib import PtConfig, PtPresentParams, PtStats  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
COPY_BYTES = 24
CAM = dict(position=(0.5, 3.0, 4.0), direction=(-0.1, -0.6, -0.79), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
LOOKS = [((0.0, 0.0, 0.0), ref.DIFFUSE), ((0.0, 0.0, 0.0), ref.SPECULAR), ((2.0, 2.0, 2.0), ref.DIFFUSE)]
LOOP_SCENES, LOOP_SIZE, LOOP_SPP, FRAMES = ("cornell", "mesh"), (1024, 768), 8, 30


def main():
    L = ptlib.product()
    timing.need_gpu(L, "solid_timing")
    doc = {"command": "python tools/solid_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the ratio is "
                     "against the copy with a stream synchronise after each, the budget is compulsory bytes / %d; the loop: wall time "
                     "per frame, median of %d after a warm-up" % (timing.WINDOW_MS, COPY_BYTES, FRAMES),
           "cases": {}, "loop": {}}
    rng = np.random.default_rng(1)
    with timing.Events() as ev, gpudev.Device(L) as d:
        cam = ref.pt_camera(CAM)
        looks = ref.looks_array(LOOKS)
        s = ref.struct(ref.params(flags=ref.HEADLIGHT | ref.REFLECT_SKY))
        for w, h in SIZES:
            n = w * h
            d_alb, d_n, d_out, d_id, d_z, d_miss = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 4), d.alloc(n * 4)
            d.upload(d_alb, rng.random(n * 3, dtype=np.float32))
            d.upload(d_n, rng.random(n * 3, dtype=np.float32) - np.float32(0.5))
            yy, xx = np.mgrid[0:h, 0:w]
            disc = (xx - w // 2) ** 2 + (yy - h // 2) ** 2 <= int(0.04 * n / np.pi)  # a mirror over about 4 % of the frame
            oid = np.where(disc, 1, 0).astype(np.int32)
            oid[: h // 4, :] = -1  # a quarter of the frame is sky
            oid[h - h // 8:, : w // 8] = 2  # a lamp in a corner
            d.upload(d_id, oid.reshape(n))
            d.upload(d_miss, np.full(n, -1, dtype=np.int32))
            d.upload(d_z, np.where(oid.reshape(n) < 0, np.float32(np.inf), (4.0 + 8.0 * rng.random(n)).astype(np.float32)).astype(np.float32))
            copy_sync, copy = timing.copy_yardstick(d_out, d_alb, n * 12)
            yard = {"copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy)}
            cases = (("with albedo, out of place", d_alb, d_id, d_out, 44),
                     ("without albedo, out of place", None, d_id, d_out, 32),
                     ("all misses, out of place", d_alb, d_miss, d_out, 12),
                     ("with albedo, in place on the albedo", d_alb, d_id, d_alb, 44))  # last: it overwrites the albedo
            for name, alb, ids, out, nbytes in cases:

                def solid():
                    rc = L.pt_ctx_solid(d.ctx, w, h, C.byref(s), C.byref(cam), alb, d_n, d_z, ids, looks, len(LOOKS), out, None)
                    assert rc == 0, L.pt_last_error()

                res = {"solid": ev.measure(solid), "compulsory_bytes_per_pixel": nbytes, "budget_in_copies": nbytes / COPY_BYTES}
                res.update(yard)
                res["solid_over_copy_sync"] = res["solid"]["ms_median"] / yard["copy_sync"]["ms_median"]
                res["solid_over_copy"] = res["solid"]["ms_median"] / yard["copy"]["ms_median"]
                res["within_budget"] = res["solid_over_copy_sync"] <= res["budget_in_copies"]
                res["verdict"] = "HIT" if res["within_budget"] else "MISS"
                doc["cases"]["%dx%d %s" % (w, h, name)] = res
                print("%dx%d %s" % (w, h, name), "%.4f ms, %.2f copies (budget %.2f): %s" % (
                    res["solid"]["ms_median"], res["solid_over_copy_sync"], res["budget_in_copies"], res["verdict"]), flush=True)
            for p in (d_alb, d_n, d_out, d_id, d_z, d_miss):
                d.free(p)

        # ---- the loop: wall time per frame of the solid view and of the traced loop's front end
        W, H = LOOP_SIZE
        n = W * H
        for sid in LOOP_SCENES:
            sc = ptlib.load_scene_py(ptlib.scene_path(sid))
            d.set_scene(sc)
            P = {k: d.alloc(n * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4), ("shown", 12), ("px", 4))}
            table = ref.looks_array([(tuple(sc.objs[i].emission), int(sc.objs[i].reflect_type)) for i in range(sc.n_objs)])
            op = overlay_ref.struct(dict(overlay_ref.defaults(L), flags=overlay_ref.SKY | overlay_ref.GRID, selected=(1,)))
            pp = PtPresentParams(0, 0, 0.0, ptlib.abi.PT_PRESENT_RGBA8, 0)
            st = PtStats()
            seed = [100]

            def guides(spp):
                cfg = PtConfig(W, H, spp, 0, seed[0], 0, 0, 0, 0)
                assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), P["albedo"], P["normal"], P["depth"], P["oid"], None) == 0, L.pt_last_error()

            def solid_chain():
                seed[0] += 1
                guides(1)
                rc = L.pt_ctx_solid(d.ctx, W, H, C.byref(s), C.byref(sc.cam), P["albedo"], P["normal"], P["depth"], P["oid"], table, sc.n_objs,
                                    P["shown"], None)
                assert rc == 0, L.pt_last_error()
                assert L.pt_ctx_overlay(d.ctx, W, H, C.byref(op), C.byref(sc.cam), P["shown"], P["oid"], P["depth"], P["shown"]) == 0, L.pt_last_error()
                assert L.pt_ctx_present(d.ctx, W, H, C.byref(pp), P["shown"], P["px"], None) == 0, L.pt_last_error()

            def traced_front_end():
                seed[0] += 1
                cfg = PtConfig(W, H, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
                assert L.pt_ctx_render(d.ctx, C.byref(cfg), P["color"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
                guides(LOOP_SPP)

            res = {"solid": timing.wall(solid_chain, FRAMES), "traced_front_end": timing.wall(traced_front_end, FRAMES)}
            res["traced_over_solid"] = res["traced_front_end"]["ms_median"] / res["solid"]["ms_median"]
            key = "%s %dx%d: solid at 1 spp of guides, traced at %d spp" % (sid, W, H, LOOP_SPP)
            doc["loop"][key] = res
            timing.report(key, res)
            for p in P.values():
                d.free(p)
    timing.write(doc, "solid_timing.json")


if __name__ == "__main__":
    main()
