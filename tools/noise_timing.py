#!/usr/bin/env python3
"""Two measurements of noise tracking on the GPU, for DESIGN.md section 4.

1. HIP-event time of pt_ctx_accum_noise on cornell 1024x768 (64 samples held, 32 + 32): a call is microseconds, so N
   back-to-back blocking calls on a caller's stream go between two HIP events, N chosen so that the window is at least 0.25 s,
   and the window is divided by N; five windows give the median and the spread (as tools/denoise_timing.py).  With and
   without the per-pixel map.  The figure is set against the call's bytes, 52 B per pixel.
2. The cost of tracking: cornell 1024x768 @4096 as eight pt_ctx_accumulate calls of 512 samples, tracking on against tracking
   off on the same build, three repetitions each, interleaved; wall time of the eight calls and the sums of pt_stats.

    python tools/noise_timing.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
from ptlib import PtConfig, PtNoiseStats, PtStats  # noqa: E402

W, H = 1024, 768


def context(L, sc, tracked):
    ctx = C.c_void_p()
    assert L.pt_ctx_create(0, C.byref(ctx)) == 0
    assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0
    assert L.pt_ctx_accum_track_noise(ctx, 1 if tracked else 0) == 0
    return ctx


def main(stream):
    L = ptlib.product()
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    npix = W * H
    out, err = C.c_void_p(), C.c_void_p()
    assert L.pt_device_malloc(0, npix * 12, C.byref(out)) == 0 and L.pt_device_malloc(0, npix * 4, C.byref(err)) == 0
    doc = {"frame": "cornell %dx%d" % (W, H), "isa_hash": L.pt_kernel_isa_hash().decode(), "command": "python tools/noise_timing.py"}

    # 1. pt_ctx_accum_noise
    ctx = context(L, sc, True)
    st, ns = PtStats(), PtNoiseStats()
    cfg = PtConfig(W, H, 64, 0, 1, 0, 0, 0, 0)
    assert L.pt_ctx_accumulate(ctx, C.byref(cfg), out, None, None, None, None, C.byref(st)) == 0
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    def window(d_err, n):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(n):
            assert L.pt_ctx_accum_noise(ctx, C.byref(cfg), d_err, C.byref(ns), stream) == 0
        assert hip.hipEventRecord(e1, stream) == 0
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value

    doc["accum_noise"] = {"bytes_per_pixel": 52, "bytes": 52 * npix, "us_at_6.29_TB_per_s": 52 * npix / 6.29e12 * 1e6}
    for name, d_err in (("with_map", err), ("stats_only", None)):
        window(d_err, 50)
        n = max(50, int(250.0 / (window(d_err, 200) / 200)) + 1)
        per = [window(d_err, n) / n * 1e3 for _ in range(5)]
        doc["accum_noise"][name] = {"calls_per_window": n, "us_median": statistics.median(per), "us_min": min(per), "us_max": max(per)}
        print("pt_ctx_accum_noise %s: %d calls per window, %.2f us (%.2f..%.2f)" % (name, n, statistics.median(per), min(per), max(per)),
              flush=True)
    doc["accum_noise"]["mean_error"] = ns.mean_error
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.pt_ctx_destroy(ctx)

    # 2. eight calls of 512 samples, tracking on / off interleaved
    ctxs = {"off": context(L, sc, False), "on": context(L, sc, True)}
    runs = {"off": [], "on": []}
    for rep in range(4):  # the first repetition warms both contexts up (pass rates, allocations) and is dropped
        for name in ("off", "on"):
            assert L.pt_ctx_accum_reset(ctxs[name]) == 0
            tot = {"passes": 0, "ms_device": 0.0, "samples": 0, "ray_bounces": 0}
            t0 = time.perf_counter()
            for k in range(1, 9):
                c = PtConfig(W, H, 512 * k, 0, 1, 0, 0, 0, 0)
                assert L.pt_ctx_accumulate(ctxs[name], C.byref(c), out, None, None, None, None, C.byref(st)) == 0
                tot["passes"] += st.passes
                tot["ms_device"] += st.ms_device
                tot["samples"] += st.samples
                tot["ray_bounces"] += st.ray_bounces
            tot["ms_wall"] = (time.perf_counter() - t0) * 1e3
            if rep:
                runs[name].append(tot)
            print("tracking %-3s rep %d: %.2f ms wall, %.2f ms device, %d passes" % (name, rep, tot["ms_wall"], tot["ms_device"], tot["passes"]),
                  flush=True)
    assert runs["on"][0]["ray_bounces"] == runs["off"][0]["ray_bounces"] and runs["on"][0]["samples"] == runs["off"][0]["samples"]
    doc["tracking_cost"] = {"what": "cornell %dx%d @4096 as eight pt_ctx_accumulate calls of 512 samples" % (W, H), "runs": runs}
    for ctx in ctxs.values():
        L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "noise_timing_1024x768.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
