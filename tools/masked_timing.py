#!/usr/bin/env python3
"""What pt_ctx_select_pixels and pt_ctx_render_masked cost, and what --retrace's two calls add to the half-resolution loop: for
DESIGN.md section 4.  One process on one GPU.

Select and compaction.  1024x768 and 4096x4096, a weight plane with 1 % of its pixels 0 at random places (the rest 1) and a
length plane that selects none.  The protocol is tools/timing.py's, on a caller's stream; the yardstick is its copy of the colour
frame (24 B per pixel moved) on the same stream with a stream synchronise after every copy ("copy_sync").  The budget of a case is
its compulsory bytes per pixel over 24, in copies.  pt_ctx_select_pixels: 4 B read per plane and 1 B written.  The compaction has
no entry point of its own; it is timed as pt_ctx_render_masked with the cancel byte raised, which makes the list - the mask read
(1 B per pixel), 4 B written per selected pixel, the length's round trip - and returns PT_CANCELLED before the first launch of the
trace; and as the same call on an all-zero mask, which returns after the list too.

All ones.  cornell 1024x768 @ 8: pt_ctx_render_masked with every pixel selected against pt_ctx_render with
PT_BACKEND_MEGAKERNEL and the same cfg, wall time in this process after two warm-up calls (timing.wall), the median of FRAMES: the
ratio is the price of the list's indirection and the scatter.

The loop.  cornell and mesh.json at 1024x768 @ 8, wall time per frame, the median of FRAMES, both chains in this run:
  half:     pt_ctx_render + pt_ctx_render_aov at half size, pt_ctx_render_aov at full size, pt_ctx_upsample (normals and albedo)
  retrace:  the same with a weight plane, then pt_ctx_select_pixels(weight_max 0) and pt_ctx_render_masked at the same spp

    python tools/masked_timing.py [out.json]
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
from ptlib import PtConfig, PtSelectParams, PtStats  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
SHARE = 0.01
LOOP_SCENES = ("cornell", "mesh")
LOOP_SIZE = (1024, 768)
LOOP_SPP = 8
FRAMES = 7
COPY_BYTES = 24
PT_CANCELLED = ptlib.abi.PT_CANCELLED
MEGAKERNEL = ptlib.abi.PT_BACKEND_MEGAKERNEL


def wall(chain):
    chain()  # with timing.wall's own, two warm-up calls: scratch, code objects, the rounds' rate
    return timing.wall(chain, FRAMES)


def main():
    L = ptlib.product()
    timing.need_gpu(L, "masked_timing")
    doc = {"command": "python tools/masked_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % timing.WINDOW_MS,
           "inputs": "a weight plane with %g of its pixels 0 at random places, the rest 1; a length plane of 64 against len_max 8" % SHARE,
           "budget_rule": "compulsory bytes per pixel / %d (a device-to-device copy of the colour frame)" % COPY_BYTES,
           "cases": {}, "all_ones": {}, "loop": {}}
    rng = np.random.default_rng(1)
    scenes = {sid: ptlib.load_scene_py(ptlib.scene_path(sid)) for sid in LOOP_SCENES}

    def against(res, copies, per_pixel):
        res.update(bytes_per_pixel=per_pixel, budget_in_copies=per_pixel / COPY_BYTES,
                   over_copy_sync=res["ms_median"] / copies["copy_sync"]["ms_median"], over_copy=res["ms_median"] / copies["copy"]["ms_median"])
        res["budget"] = "HIT" if res["over_copy_sync"] <= res["budget_in_copies"] else "MISSES"
        return res

    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        ctx = d.ctx
        # ---- select and compaction
        d.set_scene(scenes["cornell"])  # pt_ctx_render_masked wants a scene; nothing of it is traced here
        for W, H in SIZES:
            n = W * H
            weight = np.ones(n, dtype=np.float32)
            weight[rng.random(n) < SHARE] = 0.0
            ones = int((weight == 0).sum())
            B = {k: d.alloc(n * b) for k, b in (("weight", 4), ("len", 4), ("mask", 1), ("zero", 1), ("out", 12), ("copy", 12))}
            d.upload(B["weight"], weight)
            d.upload(B["len"], np.full(n, 64.0, dtype=np.float32))
            d.upload(B["zero"], np.zeros(n, dtype=np.uint8))
            del weight
            copy_sync, copy = timing.copy_yardstick(B["copy"], B["out"], n * 12, stream)
            copies = {"copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy)}
            p, count = PtSelectParams(0.0, 8.0, 0), C.c_uint32(0)

            def select(both, counted=True):
                rc = L.pt_ctx_select_pixels(ctx, W, H, C.byref(p), B["weight"], B["len"] if both else None, B["mask"],
                                            C.byref(count) if counted else None, stream)
                assert rc == 0, L.pt_last_error()

            cfg, raised, traced = PtConfig(W, H, 1, MEGAKERNEL, 1, 0, 0, 0, 0), (C.c_uint8 * 1)(1), C.c_uint32(0)

            def compact(mask, want, cancel):
                rc = L.pt_ctx_render_masked(ctx, C.byref(cfg), mask, B["out"], stream, cancel, None, C.byref(traced))
                assert rc == want, (rc, L.pt_last_error())

            res = {"pixels": n, "selected": ones}
            res.update(copies)
            select(True)
            assert count.value == ones, (count.value, ones)
            res["select, weight plane"] = against(ev.measure(lambda: select(False)), copies, 5.0)
            res["select, both planes"] = against(ev.measure(lambda: select(True)), copies, 9.0)
            res["select, both planes, no count read back"] = against(ev.measure(lambda: select(True, False)), copies, 9.0)
            compact(B["mask"], PT_CANCELLED, C.cast(raised, C.c_void_p))
            assert traced.value == ones, (traced.value, ones)
            res["compaction (cancelled call)"] = against(ev.measure(lambda: compact(B["mask"], PT_CANCELLED, C.cast(raised, C.c_void_p))),
                                                         copies, 1.0 + 4.0 * ones / n)
            res["compaction (all-zero mask)"] = against(ev.measure(lambda: compact(B["zero"], 0, None)), copies, 1.0)
            name = "%dx%d" % (W, H)
            doc["cases"][name] = res
            timing.report(name, res)
            timing.free_planes(d, B)

        # ---- every pixel selected against the frame call
        W, H = LOOP_SIZE
        n = W * H
        F = {"a": d.alloc(n * 12), "b": d.alloc(n * 12), "mask": d.alloc(n)}
        d.upload(F["mask"], np.ones(n, dtype=np.uint8))
        st, cfg, traced = PtStats(), PtConfig(W, H, LOOP_SPP, MEGAKERNEL, 7, 0, 0, 0, 0), C.c_uint32(0)

        def frame_call():
            assert L.pt_ctx_render(ctx, C.byref(cfg), F["a"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()

        def masked_call():
            assert L.pt_ctx_render_masked(ctx, C.byref(cfg), F["mask"], F["b"], None, None, C.byref(st), C.byref(traced)) == 0, L.pt_last_error()

        res = {"pt_ctx_render": wall(frame_call)}
        b0 = st.ray_bounces
        res["pt_ctx_render_masked"] = wall(masked_call)
        b1 = st.ray_bounces
        a, b = d.download(F["a"], n * 3), d.download(F["b"], n * 3)
        res.update(ray_bounces=int(b0), same_bounces=bool(b0 == b1), same_bytes=bool(a.tobytes() == b.tobytes()), pixels=int(traced.value),
                   masked_over_render=res["pt_ctx_render_masked"]["ms_median"] / res["pt_ctx_render"]["ms_median"])
        doc["all_ones"]["cornell %dx%d @ %d spp" % (W, H, LOOP_SPP)] = res
        timing.report("all ones", res)
        timing.free_planes(d, F)

        # ---- the loop's front end with and without the retrace
        w, h = W // 2, H // 2
        nl = w * h
        for sid in LOOP_SCENES:
            d.set_scene(scenes[sid])
            F = {k: d.alloc(n * b) for k, b in (("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4), ("out", 12), ("weight", 4), ("mask", 1))}
            Lo = {k: d.alloc(nl * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4))}
            seed = [100]
            sel, traced = PtSelectParams(0.0, 0.0, 0), C.c_uint32(0)

            def half_chain(retrace):
                seed[0] += 1
                lo, full = PtConfig(w, h, LOOP_SPP, 0, seed[0], 0, 0, 0, 0), PtConfig(W, H, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
                assert L.pt_ctx_render(ctx, C.byref(lo), Lo["color"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
                assert L.pt_ctx_render_aov(ctx, C.byref(lo), Lo["albedo"], Lo["normal"], Lo["depth"], Lo["oid"], None) == 0, L.pt_last_error()
                assert L.pt_ctx_render_aov(ctx, C.byref(full), F["albedo"], F["normal"], F["depth"], F["oid"], None) == 0, L.pt_last_error()
                rc = L.pt_ctx_upsample(ctx, W, H, w, h, None, Lo["color"], Lo["depth"], Lo["oid"], Lo["normal"], Lo["albedo"], F["depth"],
                                       F["oid"], F["normal"], F["albedo"], F["out"], F["weight"] if retrace else None, None)
                assert rc == 0, L.pt_last_error()
                if retrace:
                    assert L.pt_ctx_select_pixels(ctx, W, H, C.byref(sel), F["weight"], None, F["mask"], None, None) == 0, L.pt_last_error()
                    assert L.pt_ctx_render_masked(ctx, C.byref(full), F["mask"], F["out"], None, None, None, C.byref(traced)) == 0, L.pt_last_error()

            res = {"half": wall(lambda: half_chain(False)), "retrace": wall(lambda: half_chain(True))}
            pixels = traced.value
            res.update(retraced_pixels=int(pixels), retraced_share=pixels / n,
                       retrace_over_half=res["retrace"]["ms_median"] / res["half"]["ms_median"],
                       added_ms=res["retrace"]["ms_median"] - res["half"]["ms_median"])
            key = "%s %dx%d @ %d spp" % (sid, W, H, LOOP_SPP)
            doc["loop"][key] = res
            timing.report(key, res)
            timing.free_planes(d, F, Lo)
    timing.write(doc, "masked_timing.json")


if __name__ == "__main__":
    main()
