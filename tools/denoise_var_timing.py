#!/usr/bin/env python3
"""HIP-event time of pt_ctx_denoise_var next to pt_ctx_denoise on the GPU - same build, same frame, same session - per level
count and per kernel form, for DESIGN.md section 4.

The protocol and its counts are tools/denoise_timing.py's (tools/timing.py with a warm-up of 50, a probe of 200, at least 50).
The frame is cornell at 1024x768: a noise-tracked pt_ctx_accumulate frame at 16 samples, its pt_ctx_accum_noise map, guides
at 16.  The form is chosen per context through PT_DN_LDS_MAXSTEP (0 = every level loads its taps from global memory, 128 =
every level stages them in LDS, unset = the default mix); level i alone is the time at i + 1 levels minus the time at i.
The guided call has one launch more than the fixed one (the 3x3 prefilter of the variance).

    python tools/denoise_var_timing.py [out.json]
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402
from denoise_timing import COUNTS, FORMS  # noqa: E402
from ptlib import PtConfig, PtNoiseStats, PtStats  # noqa: E402

W, H, SPP = 1024, 768, 16


def main():
    L = ptlib.product()
    timing.need_gpu(L, "denoise_var_timing")
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    npix = W * H
    doc = {"frame": "cornell %dx%d, tracked frame at %d spp, its noise map, guides at %d" % (W, H, SPP, SPP),
           "isa_hash": L.pt_kernel_isa_hash().decode(), "command": "python tools/denoise_var_timing.py", "forms": {}}
    os.environ.pop("PT_DN_LDS_MAXSTEP", None)  # "default" is the variable unset
    with gpudev.stream() as stream:
        for form, env in FORMS:
            with gpudev.Device(L, sc, env=env) as d, timing.Events(stream) as ev:
                assert L.pt_ctx_accum_track_noise(d.ctx, 1) == 0
                color, error, albedo, normal, depth, out = (d.alloc(npix * k * 4) for k in (3, 1, 3, 3, 1, 3))
                cfg = PtConfig(W, H, SPP, 0, 1, 0, 0, 0, 0)
                st, ns = PtStats(), PtNoiseStats()
                assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg), color, None, None, None, None, C.byref(st)) == 0
                assert L.pt_ctx_accum_noise(d.ctx, C.byref(cfg), error, C.byref(ns), None) == 0
                assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), albedo, normal, depth, None, None) == 0
                res = {"mean_error": ns.mean_error, "denoise": {}, "denoise_var": {}}
                for levels in range(1, 9):
                    def denoise():  # (the parameters are made per call, as a host would: inside the window for both)
                        p = ptlib.PtDenoiseParams(levels, 0, 0, 0, 0)
                        assert L.pt_ctx_denoise(d.ctx, W, H, C.byref(p), color, albedo, normal, depth, out, stream) == 0

                    def denoise_var():
                        p = ptlib.PtDenoiseVarParams(levels, 0, 0, 0)
                        assert L.pt_ctx_denoise_var(d.ctx, W, H, C.byref(p), color, error, albedo, normal, depth, out, stream) == 0

                    for which, call in (("denoise", denoise), ("denoise_var", denoise_var)):  # interleaved: the two share whatever the clocks do
                        m = res[which][str(levels)] = ev.measure(call, **COUNTS)
                        print(form, which, levels, m["calls_per_window"], "%.4f ms (%.4f..%.4f)" % (m["ms_median"], m["ms_min"], m["ms_max"]),
                              flush=True)
                doc["forms"][form] = res
    timing.write(doc, "denoise_var_timing_1024x768.json")


if __name__ == "__main__":
    main()
