#!/usr/bin/env python3
"""HIP-event time of pt_ctx_denoise on the GPU, per level count and per kernel form, for DESIGN.md section 4.

A call is far below a millisecond, so one call is not timed: after a warm-up, N back-to-back calls on a caller's stream are
put between two HIP events, N chosen so that the window is at least 0.25 s, and the window is divided by N; five such windows
give the median and the spread.  The frame is cornell at 1024x768, 16 samples, guides at 16; pt_stats.ms_device of that
render on the same context is what the denoiser is set against.  The form is chosen per context through PT_DN_LDS_MAXSTEP
(0 = every level loads its taps from global memory, 128 = every level stages them in LDS); level i alone is the time at
i + 1 levels minus the time at i levels (the prepare pass is in every figure, the finish is folded into the last level).

    python tools/denoise_timing.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref  # noqa: E402
import gpudev  # noqa: E402
import ptlib  # noqa: E402
from ptlib import PtConfig, PtStats  # noqa: E402

W, H, SPP = 1024, 768, 16


def main(stream):
    L = ptlib.product()
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    npix = W * H
    doc = {"frame": "cornell %dx%d, %d spp, guides at %d" % (W, H, SPP, SPP), "isa_hash": L.pt_kernel_isa_hash().decode(),
           "command": "python tools/denoise_timing.py", "forms": {}}
    for form, maxstep in (("direct", "0"), ("lds", "128"), ("default", None)):
        if maxstep is None:
            os.environ.pop("PT_DN_LDS_MAXSTEP", None)
        else:
            os.environ["PT_DN_LDS_MAXSTEP"] = maxstep
        ctx = C.c_void_p()
        assert L.pt_ctx_create(0, C.byref(ctx)) == 0
        assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0
        bufs = []
        for k in (3, 3, 3, 1, 3):
            p = C.c_void_p()
            assert L.pt_device_malloc(0, npix * k * 4, C.byref(p)) == 0
            bufs.append(p)
        color, albedo, normal, depth, out = bufs
        cfg = PtConfig(W, H, SPP, 0, 1, 0, 0, 0, 0)
        st = PtStats()
        for _ in range(3):  # the last of three: the pass rate is measured by then
            assert L.pt_ctx_render(ctx, C.byref(cfg), color, None, None, None, None, C.byref(st)) == 0
        assert L.pt_ctx_render_aov(ctx, C.byref(cfg), albedo, normal, depth, None, None) == 0
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

        def window(levels, n):
            p = ptlib.PtDenoiseParams(levels, 0, 0, 0, 0)
            assert hip.hipEventRecord(e0, stream) == 0
            for _ in range(n):
                assert L.pt_ctx_denoise(ctx, W, H, C.byref(p), color, albedo, normal, depth, out, stream) == 0
            assert hip.hipEventRecord(e1, stream) == 0
            assert hip.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            return ms.value

        res = {"render_ms_device": st.ms_device, "levels": {}}
        for levels in range(1, 9):
            window(levels, 50)
            n = max(50, int(250.0 / (window(levels, 200) / 200)) + 1)
            per = [window(levels, n) / n for _ in range(5)]
            res["levels"][str(levels)] = {"calls_per_window": n, "ms_median": statistics.median(per), "ms_min": min(per),
                                          "ms_max": max(per)}
            print(form, levels, n, "%.4f ms (%.4f..%.4f)" % (statistics.median(per), min(per), max(per)), flush=True)
        doc["forms"][form] = res
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        for p in bufs:
            L.pt_device_free(0, p)
        L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_timing_1024x768.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
