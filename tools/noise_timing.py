#!/usr/bin/env python3
"""Two measurements of noise tracking on the GPU, for DESIGN.md section 4.

1. HIP-event time of pt_ctx_accum_noise on cornell 1024x768 (64 samples held, 32 + 32): a call is microseconds, so it is
   measured by tools/timing.py's protocol on a caller's stream, with tools/denoise_timing.py's counts.  With and without the
   per-pixel map.  The figure is set against the call's bytes, 52 B per pixel.
2. The cost of tracking: cornell 1024x768 @4096 as eight pt_ctx_accumulate calls of 512 samples, tracking on against tracking
   off on the same build, three repetitions each, interleaved; wall time of the eight calls and the sums of pt_stats.

    python tools/noise_timing.py [out.json]
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402
from denoise_timing import COUNTS  # noqa: E402
from ptlib import PtConfig, PtNoiseStats, PtStats  # noqa: E402

W, H = 1024, 768


def context(L, sc, tracked):
    d = gpudev.Device(L, sc)
    assert L.pt_ctx_accum_track_noise(d.ctx, 1 if tracked else 0) == 0
    return d


def main():
    L = ptlib.product()
    timing.need_gpu(L, "noise_timing")
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    npix = W * H
    doc = {"frame": "cornell %dx%d" % (W, H), "isa_hash": L.pt_kernel_isa_hash().decode(), "command": "python tools/noise_timing.py"}
    st, ns = PtStats(), PtNoiseStats()

    # 1. pt_ctx_accum_noise
    with gpudev.stream() as stream, context(L, sc, True) as d, timing.Events(stream) as ev:
        out, err = d.alloc(npix * 12), d.alloc(npix * 4)
        cfg = PtConfig(W, H, 64, 0, 1, 0, 0, 0, 0)
        assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg), out, None, None, None, None, C.byref(st)) == 0
        doc["accum_noise"] = {"bytes_per_pixel": 52, "bytes": 52 * npix, "us_at_6.29_TB_per_s": 52 * npix / 6.29e12 * 1e6}
        for name, d_err in (("with_map", err), ("stats_only", None)):
            def accum_noise():
                assert L.pt_ctx_accum_noise(d.ctx, C.byref(cfg), d_err, C.byref(ns), stream) == 0

            m = ev.measure(accum_noise, **COUNTS)
            us = doc["accum_noise"][name] = {"calls_per_window": m["calls_per_window"], "us_median": m["ms_median"] * 1e3,
                                             "us_min": m["ms_min"] * 1e3, "us_max": m["ms_max"] * 1e3}
            print("pt_ctx_accum_noise %s: %d calls per window, %.2f us (%.2f..%.2f)" % (
                name, us["calls_per_window"], us["us_median"], us["us_min"], us["us_max"]), flush=True)
        doc["accum_noise"]["mean_error"] = ns.mean_error

    # 2. eight calls of 512 samples, tracking on / off interleaved
    with context(L, sc, False) as off, context(L, sc, True) as on:
        out = off.alloc(npix * 12)
        runs = {"off": [], "on": []}
        for rep in range(4):  # the first repetition warms both contexts up (pass rates, allocations) and is dropped
            for name, d in (("off", off), ("on", on)):
                assert L.pt_ctx_accum_reset(d.ctx) == 0
                tot = {"passes": 0, "ms_device": 0.0, "samples": 0, "ray_bounces": 0}
                t0 = time.perf_counter()
                for k in range(1, 9):
                    c = PtConfig(W, H, 512 * k, 0, 1, 0, 0, 0, 0)
                    assert L.pt_ctx_accumulate(d.ctx, C.byref(c), out, None, None, None, None, C.byref(st)) == 0
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
    timing.write(doc, "noise_timing_1024x768.json")


if __name__ == "__main__":
    main()
