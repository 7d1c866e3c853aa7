#!/usr/bin/env python3
"""What pt_ctx_upsample costs, and what tracing at half the resolution gains a viewport's loop: for DESIGN.md section 4.

The call.  1024x768 <- 512x384 and 4096x4096 <- 2048x2048, each with normals, without normals, and with normals and albedo.  Every
pixel of both frames sits on one plane with one object id and one normal, so every tap is taken and the call moves all of its
compulsory bytes.  Per frame pixel those are: its own guides (id 4, depth 4, normal 12, albedo 12), the colour written (12), and a
low-resolution pixel's planes (colour 12, id 4, depth 4, normal 12, albedo 12) divided by the frame pixels per low-resolution
pixel.  A device-to-device copy of the full-size colour frame moves 24 B per pixel: the budget of a case is its bytes over 24, in
copies - the rule that gave pt_ctx_reproject its 3.5.  The method is tools/reproject_timing.py's: after a warm-up, N back-to-back
calls on a caller's stream between two HIP events, N chosen so that the window is at least 0.25 s; five windows give the median.
pt_ctx_upsample blocks, so its window holds the host's turn-around too; the yardstick is hipMemcpyAsync of the colour frame on the
same stream with a stream synchronise after every copy ("copy_sync"), and back to back ("copy").

The loop.  On cornell and mesh.json at 1024x768 and 4096x4096, n = 8 samples, wall time per frame of the two chains, in this
process after a warm-up, the median of FRAMES frames:
  full:  pt_ctx_render(n spp, full) + pt_ctx_render_aov(full)
  half:  pt_ctx_render(n spp, half) + pt_ctx_render_aov(half) + pt_ctx_render_aov(full) + pt_ctx_upsample (normals and albedo)

    python tools/upsample_timing.py [out.json]
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
import ptlib  # noqa: E402
import upsample_ref as ref  # noqa: E402
from ptlib import PtConfig, PtStats  # noqa: E402

SIZES = ((1024, 768), (4096, 4096))
FORMS = (("with normals", True, False), ("without normals", False, False), ("with normals and albedo", True, True))
WINDOW_MS = 250.0
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


def main(stream):
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "upsample_timing needs a GPU: there is nothing to time without one"
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert L.pt_ctx_create(0, C.byref(ctx)) == 0, L.pt_last_error()
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    doc = {"command": "python tools/upsample_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % WINDOW_MS,
           "inputs": "every pixel of both frames on one plane (depth %g, one id, one normal, albedo 0.5): every tap is taken" % DEPTH,
           "budget_rule": "compulsory bytes per frame pixel / %d (a device-to-device copy of the colour frame)" % COPY_BYTES,
           "cases": {}, "loop": {}}
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

    def alloc(nbytes):
        p = C.c_void_p()
        assert L.pt_device_malloc(0, nbytes, C.byref(p)) == 0, L.pt_last_error()
        return p

    def put(p, host):
        assert hip.hipMemcpy(p, host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0

    for W, H in SIZES:
        w, h = W // 2, H // 2
        n, nl = W * H, w * h
        B = {}
        for side, cnt in (("", n), ("l", nl)):
            for k, v in (("depth", np.full(cnt, DEPTH, dtype=np.float32)), ("oid", np.ones(cnt, dtype=np.int32)),
                         ("normal", np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), cnt)),
                         ("albedo", np.full(cnt * 3, 0.5, dtype=np.float32))):
                B[side + k] = alloc(v.nbytes)
                put(B[side + k], v)
        lcolor = rng.random(nl * 3, dtype=np.float32)
        B["lcolor"] = alloc(lcolor.nbytes)
        put(B["lcolor"], lcolor)
        del lcolor
        B["out"], B["copy"], B["weight"] = alloc(n * 12), alloc(n * 12), alloc(n * 4)

        def copy():
            assert hip.hipMemcpyAsync(B["copy"], B["out"], n * 12, 3, stream) == 0  # device to device

        def copy_sync():
            copy()
            assert hip.hipStreamSynchronize(stream) == 0

        copies = {"copy_sync": measure(copy_sync), "copy": measure(copy)}
        for form, normals, albedo in FORMS:
            def upsample(weight=None):
                rc = L.pt_ctx_upsample(ctx, W, H, w, h, None, B["lcolor"], B["ldepth"], B["loid"], B["lnormal"] if normals else None,
                                       B["lalbedo"] if albedo else None, B["depth"], B["oid"], B["normal"] if normals else None,
                                       B["albedo"] if albedo else None, B["out"], weight, stream)
                assert rc == 0, L.pt_last_error()

            upsample(B["weight"])  # once with the weight plane: every pixel found every tap
            wg = np.zeros(n, dtype=np.float32)
            assert L.pt_device_download(0, wg.ctypes.data_as(C.c_void_p), B["weight"], wg.nbytes) == 0
            per_pixel = compulsory_bytes(W, H, w, h, normals, albedo)
            res = {"upsample": measure(upsample), "bytes_per_frame_pixel": per_pixel, "budget_in_copies": per_pixel / COPY_BYTES,
                   "share_all_taps": float((np.abs(wg - 1.0) <= 2.0 ** -20).mean())}
            res.update(copies)
            res["upsample_over_copy_sync"] = res["upsample"]["ms_median"] / copies["copy_sync"]["ms_median"]
            res["upsample_over_copy"] = res["upsample"]["ms_median"] / copies["copy"]["ms_median"]
            res["budget"] = "HIT" if res["upsample_over_copy_sync"] <= res["budget_in_copies"] else "MISSES"
            res["GB_per_s"] = per_pixel * n / (res["upsample"]["ms_median"] * 1e6)
            name = "%dx%d <- %dx%d %s" % (W, H, w, h, form)
            doc["cases"][name] = res
            print(name, json.dumps(res), flush=True)
        for p in B.values():
            L.pt_device_free(0, p)

    # ---- the loop: wall time per frame of the two chains
    for sid in LOOP_SCENES:
        sc = ptlib.load_scene_py(ptlib.scene_path(sid))
        assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0, L.pt_last_error()
        for W, H in SIZES:
            w, h = W // 2, H // 2
            n, nl = W * H, w * h
            F = {k: alloc(n * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4), ("out", 12))}
            Lo = {k: alloc(nl * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4))}
            st = PtStats()
            seed = [100]

            def trace(wd, ht, P):
                seed[0] += 1
                cfg = PtConfig(wd, ht, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
                assert L.pt_ctx_render(ctx, C.byref(cfg), P["color"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
                return st.ray_bounces

            def guides(wd, ht, P):
                cfg = PtConfig(wd, ht, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
                assert L.pt_ctx_render_aov(ctx, C.byref(cfg), P["albedo"], P["normal"], P["depth"], P["oid"], None) == 0, L.pt_last_error()

            def full_chain():
                b = trace(W, H, F)
                guides(W, H, F)
                return b

            def half_chain():
                b = trace(w, h, Lo)
                guides(w, h, Lo)
                guides(W, H, F)
                rc = L.pt_ctx_upsample(ctx, W, H, w, h, None, Lo["color"], Lo["depth"], Lo["oid"], Lo["normal"], Lo["albedo"], F["depth"],
                                       F["oid"], F["normal"], F["albedo"], F["out"], None, None)
                assert rc == 0, L.pt_last_error()
                return b

            res = {}
            for name, chain in (("full", full_chain), ("half", half_chain)):
                chain()  # warm-up: scratch, code objects
                times, bounces = [], 0
                for _ in range(FRAMES):
                    t0 = time.perf_counter()
                    bounces = chain()
                    times.append((time.perf_counter() - t0) * 1e3)
                res[name] = {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "ray_bounces": int(bounces)}
            res["half_over_full"] = res["half"]["ms_median"] / res["full"]["ms_median"]
            key = "%s %dx%d @ %d spp" % (sid, W, H, LOOP_SPP)
            doc["loop"][key] = res
            print(key, json.dumps(res), flush=True)
            for p in list(F.values()) + list(Lo.values()):
                L.pt_device_free(0, p)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "upsample_timing.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
