#!/usr/bin/env python3
"""What pt_ctx_select_pixels and pt_ctx_render_masked cost, and what --retrace's two calls add to the half-resolution loop: for
DESIGN.md section 4.  One process on one GPU.

Select and compaction.  1024x768 and 4096x4096, a weight plane with 1 % of its pixels 0 at random places (the rest 1) and a
length plane that selects none.  tools/upsample_timing.py's method: after a warm-up, N back-to-back calls on a caller's stream
between two HIP events, N chosen so that the window is at least 0.25 s; five windows give the median.  Both calls block, so a
window holds the host's turn-around too; the yardstick is hipMemcpyAsync of the colour frame (24 B per pixel moved) on the same
stream with a stream synchronise after every copy ("copy_sync").  The budget of a case is its compulsory bytes per pixel over 24,
in copies.  pt_ctx_select_pixels: 4 B read per plane and 1 B written.  The compaction has no entry point of its own; it is
timed as pt_ctx_render_masked with the cancel byte raised, which makes the list - the mask read (1 B per pixel), 4 B written per
selected pixel, the length's round trip - and returns PT_CANCELLED before the first launch of the trace; and as the same call on
an all-zero mask, which returns after the list too.

All ones.  cornell 1024x768 @ 8: pt_ctx_render_masked with every pixel selected against pt_ctx_render with
PT_BACKEND_MEGAKERNEL and the same cfg, wall time in this process after a warm-up, the median of FRAMES: the ratio is the
price of the list's indirection and the scatter.

The loop.  cornell and mesh.json at 1024x768 @ 8, wall time per frame, the median of FRAMES, both chains in this run:
  half:     pt_ctx_render + pt_ctx_render_aov at half size, pt_ctx_render_aov at full size, pt_ctx_upsample (normals and albedo)
  retrace:  the same with a weight plane, then pt_ctx_select_pixels(weight_max 0) and pt_ctx_render_masked at the same spp

    python tools/masked_timing.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import masked_ref as ref  # noqa: E402
import ptlib  # noqa: E402
import upsample_ref  # noqa: E402
from ptlib import PtConfig, PtSelectParams, PtStats  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
WINDOW_MS = 250.0
SHARE = 0.01
LOOP_SCENES = ("cornell", "mesh")
LOOP_SIZE = (1024, 768)
LOOP_SPP = 8
FRAMES = 7
COPY_BYTES = 24
PT_CANCELLED = ptlib.abi.PT_CANCELLED
MEGAKERNEL = ptlib.abi.PT_BACKEND_MEGAKERNEL


def main(stream):
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "masked_timing needs a GPU: there is nothing to time without one"
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert L.pt_ctx_create(0, C.byref(ctx)) == 0, L.pt_last_error()
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    doc = {"command": "python tools/masked_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % WINDOW_MS,
           "inputs": "a weight plane with %g of its pixels 0 at random places, the rest 1; a length plane of 64 against len_max 8" % SHARE,
           "budget_rule": "compulsory bytes per pixel / %d (a device-to-device copy of the colour frame)" % COPY_BYTES,
           "cases": {}, "all_ones": {}, "loop": {}}
    rng = np.random.default_rng(1)
    scenes = {sid: ptlib.load_scene_py(ptlib.scene_path(sid)) for sid in LOOP_SCENES}

    def set_scene(sid):
        sc = scenes[sid]
        assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0, L.pt_last_error()

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
        timed(fn, 20)  # warm-up: code objects, scratch
        n = max(20, int(WINDOW_MS / (timed(fn, 50) / 50)) + 1)
        per = [timed(fn, n) / n for _ in range(5)]
        return {"calls_per_window": n, "ms_median": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}

    def alloc(nbytes):
        p = C.c_void_p()
        assert L.pt_device_malloc(0, nbytes, C.byref(p)) == 0, L.pt_last_error()
        return p

    def put(p, host):
        assert hip.hipMemcpy(p, host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0

    def against(res, copies, per_pixel):
        res.update(bytes_per_pixel=per_pixel, budget_in_copies=per_pixel / COPY_BYTES,
                   over_copy_sync=res["ms_median"] / copies["copy_sync"]["ms_median"], over_copy=res["ms_median"] / copies["copy"]["ms_median"])
        res["budget"] = "HIT" if res["over_copy_sync"] <= res["budget_in_copies"] else "MISSES"
        return res

    # ---- select and compaction
    set_scene("cornell")  # pt_ctx_render_masked wants a scene; nothing of it is traced here
    for W, H in SIZES:
        n = W * H
        weight = np.ones(n, dtype=np.float32)
        weight[rng.random(n) < SHARE] = 0.0
        ones = int((weight == 0).sum())
        B = {"weight": alloc(n * 4), "len": alloc(n * 4), "mask": alloc(n), "zero": alloc(n), "out": alloc(n * 12), "copy": alloc(n * 12)}
        put(B["weight"], weight)
        put(B["len"], np.full(n, 64.0, dtype=np.float32))
        put(B["zero"], np.zeros(n, dtype=np.uint8))
        del weight

        def copy():
            assert hip.hipMemcpyAsync(B["copy"], B["out"], n * 12, 3, stream) == 0  # device to device

        def copy_sync():
            copy()
            assert hip.hipStreamSynchronize(stream) == 0

        copies = {"copy_sync": measure(copy_sync), "copy": measure(copy)}
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
        res["select, weight plane"] = against(measure(lambda: select(False)), copies, 5.0)
        res["select, both planes"] = against(measure(lambda: select(True)), copies, 9.0)
        res["select, both planes, no count read back"] = against(measure(lambda: select(True, False)), copies, 9.0)
        compact(B["mask"], PT_CANCELLED, C.cast(raised, C.c_void_p))
        assert traced.value == ones, (traced.value, ones)
        res["compaction (cancelled call)"] = against(measure(lambda: compact(B["mask"], PT_CANCELLED, C.cast(raised, C.c_void_p))), copies,
                                                     1.0 + 4.0 * ones / n)
        res["compaction (all-zero mask)"] = against(measure(lambda: compact(B["zero"], 0, None)), copies, 1.0)
        name = "%dx%d" % (W, H)
        doc["cases"][name] = res
        print(name, json.dumps(res), flush=True)
        for q in B.values():
            L.pt_device_free(0, q)

    # ---- every pixel selected against the frame call
    W, H = LOOP_SIZE
    n = W * H
    F = {"a": alloc(n * 12), "b": alloc(n * 12), "mask": alloc(n)}
    put(F["mask"], np.ones(n, dtype=np.uint8))
    st, cfg, traced = PtStats(), PtConfig(W, H, LOOP_SPP, MEGAKERNEL, 7, 0, 0, 0, 0), C.c_uint32(0)

    def frame_call():
        assert L.pt_ctx_render(ctx, C.byref(cfg), F["a"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
        return st.ray_bounces

    def masked_call():
        assert L.pt_ctx_render_masked(ctx, C.byref(cfg), F["mask"], F["b"], None, None, C.byref(st), C.byref(traced)) == 0, L.pt_last_error()
        return st.ray_bounces

    def wall(chain):
        chain()
        chain()  # warm-up: scratch, code objects, the rounds' rate
        times, last = [], 0
        for _ in range(FRAMES):
            t0 = time.perf_counter()
            last = chain()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times)}, last

    res = {}
    res["pt_ctx_render"], b0 = wall(frame_call)
    res["pt_ctx_render_masked"], b1 = wall(masked_call)
    a, b = np.zeros(n * 3, dtype=np.float32), np.zeros(n * 3, dtype=np.float32)
    assert L.pt_device_download(0, a.ctypes.data_as(C.c_void_p), F["a"], a.nbytes) == 0
    assert L.pt_device_download(0, b.ctypes.data_as(C.c_void_p), F["b"], b.nbytes) == 0
    res.update(ray_bounces=int(b0), same_bounces=bool(b0 == b1), same_bytes=bool(a.tobytes() == b.tobytes()), pixels=int(traced.value),
               masked_over_render=res["pt_ctx_render_masked"]["ms_median"] / res["pt_ctx_render"]["ms_median"])
    doc["all_ones"]["cornell %dx%d @ %d spp" % (W, H, LOOP_SPP)] = res
    print("all ones", json.dumps(res), flush=True)
    for q in F.values():
        L.pt_device_free(0, q)

    # ---- the loop's front end with and without the retrace
    w, h = W // 2, H // 2
    nl = w * h
    for sid in LOOP_SCENES:
        set_scene(sid)
        F = {k: alloc(n * b) for k, b in (("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4), ("out", 12), ("weight", 4), ("mask", 1))}
        Lo = {k: alloc(nl * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4))}
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
            return traced.value

        res = {}
        res["half"], _ = wall(lambda: half_chain(False))
        res["retrace"], pixels = wall(lambda: half_chain(True))
        res.update(retraced_pixels=int(pixels), retraced_share=pixels / n, retrace_over_half=res["retrace"]["ms_median"] / res["half"]["ms_median"],
                   added_ms=res["retrace"]["ms_median"] - res["half"]["ms_median"])
        key = "%s %dx%d @ %d spp" % (sid, W, H, LOOP_SPP)
        doc["loop"][key] = res
        print(key, json.dumps(res), flush=True)
        for q in list(F.values()) + list(Lo.values()):
            L.pt_device_free(0, q)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "masked_timing.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
