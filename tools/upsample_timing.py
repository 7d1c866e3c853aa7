#!/usr/bin/env python3
"""What pt_ctx_upsample costs, and what tracing at half the resolution gains a viewport's loop: for DESIGN.md section 4.

The call.  1024x768 <- 512x384 and 4096x4096 <- 2048x2048, each with normals, without normals, and with normals and albedo.  Every
pixel of both frames sits on one plane with one object id and one normal, so every tap is taken and the call moves all of its
compulsory bytes.  Per frame pixel those are: its own guides (id 4, depth 4, normal 12, albedo 12), the colour written (12), and a
low-resolution pixel's planes (colour 12, id 4, depth 4, normal 12, albedo 12) divided by the frame pixels per low-resolution
pixel.  A device-to-device copy of the full-size colour frame moves 24 B per pixel: the budget of a case is its bytes over 24, in
copies - the rule that gave pt_ctx_reproject its 3.5.  The protocol is tools/timing.py's, on a caller's stream; the yardstick is
its copy of the colour frame on the same stream with a stream synchronise after every copy ("copy_sync"), and back to back ("copy").

The loop.  On cornell and mesh.json at 1024x768 and 4096x4096, n = 8 samples, wall time per frame of the two chains, in this
process (timing.wall), the median of FRAMES frames:
  full:  pt_ctx_render(n spp, full) + pt_ctx_render_aov(full)
  half:  pt_ctx_render(n spp, half) + pt_ctx_render_aov(half) + pt_ctx_render_aov(full) + pt_ctx_upsample (normals and albedo)

    python tools/upsample_timing.py [out.json]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402
from ptlib import PtConfig, PtStats  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
FORMS = (("with normals", True, False), ("without normals", False, False), ("with normals and albedo", True, True))
DEPTH = 6.0
LOOP_SCENES = ("cornell", "mesh")
LOOP_SPP = 8
FRAMES = 7
COPY_BYTES = 24


def compulsory_bytes(W, H, w, h, normals, albedo):
    """per frame pixel"""
    own = 8 + (12 if normals else 0) + (12 if albedo else 0)
    lo = 20 + (12 if normals else 0) + (12 if albedo else 0)
    return own + 12 + lo * (w * h) / (W * H)


def main():
    L = ptlib.product()
    timing.need_gpu(L, "upsample_timing")
    doc = {"command": "python tools/upsample_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % timing.WINDOW_MS,
           "inputs": "every pixel of both frames on one plane (depth %g, one id, one normal, albedo 0.5): every tap is taken" % DEPTH,
           "budget_rule": "compulsory bytes per frame pixel / %d (a device-to-device copy of the colour frame)" % COPY_BYTES,
           "cases": {}, "loop": {}}
    rng = np.random.default_rng(1)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        ctx = d.ctx
        for W, H in SIZES:
            w, h = W // 2, H // 2
            n, nl = W * H, w * h
            planes = {}
            for side, cnt in (("", n), ("l", nl)):
                planes.update({side + "depth": np.full(cnt, DEPTH, dtype=np.float32), side + "oid": np.ones(cnt, dtype=np.int32),
                               side + "normal": np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), cnt),
                               side + "albedo": np.full(cnt * 3, 0.5, dtype=np.float32)})
            planes["lcolor"] = rng.random(nl * 3, dtype=np.float32)
            B = timing.upload_planes(d, planes)
            del planes
            B["out"], B["copy"], B["weight"] = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 4)
            copy_sync, copy = timing.copy_yardstick(B["copy"], B["out"], n * 12, stream)
            copies = {"copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy)}
            for form, normals, albedo in FORMS:
                def upsample(weight=None):
                    rc = L.pt_ctx_upsample(ctx, W, H, w, h, None, B["lcolor"], B["ldepth"], B["loid"], B["lnormal"] if normals else None,
                                           B["lalbedo"] if albedo else None, B["depth"], B["oid"], B["normal"] if normals else None,
                                           B["albedo"] if albedo else None, B["out"], weight, stream)
                    assert rc == 0, L.pt_last_error()

                upsample(B["weight"])  # once with the weight plane: every pixel found every tap
                wg = d.download(B["weight"], n)
                per_pixel = compulsory_bytes(W, H, w, h, normals, albedo)
                res = {"upsample": ev.measure(upsample), "bytes_per_frame_pixel": per_pixel, "budget_in_copies": per_pixel / COPY_BYTES,
                       "share_all_taps": float((np.abs(wg - 1.0) <= 2.0 ** -20).mean())}
                res.update(copies)
                res["upsample_over_copy_sync"] = res["upsample"]["ms_median"] / copies["copy_sync"]["ms_median"]
                res["upsample_over_copy"] = res["upsample"]["ms_median"] / copies["copy"]["ms_median"]
                res["budget"] = "HIT" if res["upsample_over_copy_sync"] <= res["budget_in_copies"] else "MISSES"
                res["GB_per_s"] = per_pixel * n / (res["upsample"]["ms_median"] * 1e6)
                name = "%dx%d <- %dx%d %s" % (W, H, w, h, form)
                doc["cases"][name] = res
                timing.report(name, res)
            timing.free_planes(d, B)

        # ---- the loop: wall time per frame of the two chains
        for sid in LOOP_SCENES:
            d.set_scene(ptlib.load_scene_py(ptlib.scene_path(sid)))
            for W, H in SIZES:
                w, h = W // 2, H // 2
                n, nl = W * H, w * h
                F = {k: d.alloc(n * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4), ("out", 12))}
                Lo = {k: d.alloc(nl * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4))}
                st = PtStats()
                seed = [100]

                def trace(wd, ht, P):
                    seed[0] += 1
                    cfg = PtConfig(wd, ht, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
                    assert L.pt_ctx_render(ctx, C.byref(cfg), P["color"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()

                def guides(wd, ht, P):
                    cfg = PtConfig(wd, ht, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
                    assert L.pt_ctx_render_aov(ctx, C.byref(cfg), P["albedo"], P["normal"], P["depth"], P["oid"], None) == 0, L.pt_last_error()

                def full_chain():
                    trace(W, H, F)
                    guides(W, H, F)

                def half_chain():
                    trace(w, h, Lo)
                    guides(w, h, Lo)
                    guides(W, H, F)
                    rc = L.pt_ctx_upsample(ctx, W, H, w, h, None, Lo["color"], Lo["depth"], Lo["oid"], Lo["normal"], Lo["albedo"], F["depth"],
                                           F["oid"], F["normal"], F["albedo"], F["out"], None, None)
                    assert rc == 0, L.pt_last_error()

                res = {}
                for name, chain in (("full", full_chain), ("half", half_chain)):
                    res[name] = dict(timing.wall(chain, FRAMES), ray_bounces=int(st.ray_bounces))  # the last frame's
                res["half_over_full"] = res["half"]["ms_median"] / res["full"]["ms_median"]
                key = "%s %dx%d @ %d spp" % (sid, W, H, LOOP_SPP)
                doc["loop"][key] = res
                timing.report(key, res)
                timing.free_planes(d, F, Lo)
    timing.write(doc, "upsample_timing.json")


if __name__ == "__main__":
    main()
