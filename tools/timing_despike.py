#!/usr/bin/env python3
"""HIP-event time of pt_ctx_despike on the GPU, set against a device-to-device copy of the colour frame measured in the same run,
for the README's bullet and DESIGN.md section 4, in the style of tools/timing_tone.py; and what the pass adds to a frame of the
traced loop.

The pass.  Sizes: 1024x768 and 4096x4096.  The yardstick copies 24 B per pixel, so a case's budget is its compulsory bytes / 24 of
the copy's time: 24 B plain (1.0), 28 B with ids (1.17), 1 B more with the mask (+0.04).  Cases: a frame with no pixel above the
floor (every wave takes the early-out), a noise frame in which every wave runs the window at radius 1 and at radius 2, the noise
frame with ids and the flag, with the mask, and with the stats asked for (a clear and a download beside the kernel: part of the
call's time).  The protocol is tools/timing.py's, on the null stream; the like-for-like yardstick is the copy with a stream
synchronise after each ("copy_sync"), the back-to-back copy ("copy") is recorded beside it.  The budget says what the bytes allow;
it is no prediction.

The loop.  On cornell at 1024x768, 8 samples per pixel, wall time per call (timing.wall), median of 20, of
  hdr:      pt_ctx_accum_reset + pt_ctx_accumulate + pt_ctx_accum_hdr   - the traced frame the pass works on
  despike:  pt_ctx_despike at its defaults, with the stats                - what the pass adds
  tonemap:  pt_ctx_tonemap at its defaults, in place                      - the neighbour it is set beside

    python tools/timing_despike.py [out.json]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptlib  # noqa: E402  (first: it puts the repository on the path)
import despike_ref as ref  # noqa: E402
import gpudev  # noqa: E402
import timing  # noqa: E402
from ptlib import PtConfig, PtStats  # noqa: E402

da = ref.despike_abi
SIZES = ((1024, 768), (4096, 4096))
COPY_BYTES = 24
LOOP_SIZE, LOOP_SPP, FRAMES = (1024, 768), 8, 20


def main():
    L = ptlib.product()
    timing.need_gpu(L, "timing_despike")
    doc = {"command": "python tools/timing_despike.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the ratio is "
                     "against the copy with a stream synchronise after each, the budget is compulsory bytes / %d; the loop: wall time "
                     "per call, median of %d after a warm-up" % (timing.WINDOW_MS, COPY_BYTES, FRAMES),
           "cases": {}, "loop": {}}
    rng = np.random.default_rng(1)
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    with timing.Events() as ev, gpudev.Device(L, sc) as d:
        stats = da.pt_despike_stats()
        for w, h in SIZES:
            n = w * h
            d_rgb, d_dim, d_out, d_id, d_mask = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 4), d.alloc(n)
            # noise over some nine octaves above the floor: every pixel is a candidate, every wave runs its window
            d.upload(d_rgb, np.float32(1.5) + (rng.random(n * 3, dtype=np.float32) * np.float32(6.0)) ** 3)
            d.upload(d_dim, rng.random(n * 3, dtype=np.float32) * np.float32(0.2))  # no pixel above the defaults' floor of 0.25
            d.upload(d_id, ref.voronoi_ids(w, h, 3))
            copy_sync, copy = timing.copy_yardstick(d_out, d_rgb, n * 12)
            yard = {"copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy)}

            def despike(rgb, radius, flag=0, mask=None, st=None):
                p = da.pt_despike_params(radius, 3, flag, 2.0, 0.25)  # the defaults but for the radius and the flag
                return lambda: L.pt_ctx_despike(d.ctx, w, h, C.byref(p), rgb, d_id if flag else None, d_out, mask,
                                                C.byref(st) if st is not None else None, None)

            cases = (("early-out, nothing above the floor", despike(d_dim, 1), 24),
                     ("noise, radius 1", despike(d_rgb, 1), 24),
                     ("noise, radius 2", despike(d_rgb, 2), 24),
                     ("noise, radius 1, ids and the flag", despike(d_rgb, 1, flag=1), 28),
                     ("noise, radius 1, mask", despike(d_rgb, 1, mask=d_mask), 25),
                     ("noise, radius 1, stats", despike(d_rgb, 1, st=stats), 24))
            for name, call, nbytes in cases:

                def run():
                    rc = call()
                    assert rc == 0, L.pt_last_error()

                res = {"pass": ev.measure(run), "compulsory_bytes_per_pixel": nbytes}
                res.update(yard)
                res["pass_over_copy_sync"] = res["pass"]["ms_median"] / yard["copy_sync"]["ms_median"]
                res["pass_over_copy"] = res["pass"]["ms_median"] / yard["copy"]["ms_median"]
                res["budget_in_copies"] = nbytes / COPY_BYTES
                res["within_budget"] = res["pass_over_copy_sync"] <= res["budget_in_copies"]
                res["verdict"] = "HIT" if res["within_budget"] else "MISS"
                if "stats" in name:
                    res["spikes"], res["pixels"] = int(stats.spikes), int(stats.pixels)
                doc["cases"]["%dx%d %s" % (w, h, name)] = res
                print("%dx%d %s" % (w, h, name), "%.4f ms, %.2f copies (budget %.2f): %s" % (
                    res["pass"]["ms_median"], res["pass_over_copy_sync"], res["budget_in_copies"], res["verdict"]), flush=True)
            for p in (d_rgb, d_dim, d_out, d_id, d_mask):
                d.free(p)

        # ---- the loop: what the pass adds to a traced frame
        W, H = LOOP_SIZE
        n = W * H
        d_rgb, d_out = d.alloc(n * 12), d.alloc(n * 12)
        st = PtStats()
        seed = [100]

        def hdr():
            seed[0] += 1
            cfg = PtConfig(W, H, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)
            assert L.pt_ctx_accum_reset(d.ctx) == 0
            assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg), d_rgb, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
            assert L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), d_rgb, None) == 0, L.pt_last_error()

        def despike_call():
            assert L.pt_ctx_despike(d.ctx, W, H, None, d_rgb, None, d_out, None, C.byref(stats), None) == 0, L.pt_last_error()

        def tonemap():
            assert L.pt_ctx_tonemap(d.ctx, W, H, None, d_out, d_out, None) == 0, L.pt_last_error()

        res = {"hdr": timing.wall(hdr, FRAMES)}
        hdr()  # (the frame the two passes work on)
        res["despike"] = timing.wall(despike_call, FRAMES)
        res["spikes"], res["nonfinite"], res["pixels"] = int(stats.spikes), int(stats.nonfinite), int(stats.pixels)
        res["tonemap"] = timing.wall(tonemap, FRAMES)
        res["despike_adds_ms"] = res["despike"]["ms_median"]
        key = "cornell %dx%d at %d spp" % (W, H, LOOP_SPP)
        doc["loop"][key] = res
        print(key, "hdr %.3f ms, despike %.3f ms (%d spikes), tonemap %.3f ms" % (
            res["hdr"]["ms_median"], res["despike"]["ms_median"], res["spikes"], res["tonemap"]["ms_median"]), flush=True)
    timing.write(doc, "despike_timing.json")


if __name__ == "__main__":
    main()
