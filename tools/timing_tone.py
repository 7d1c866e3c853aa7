#!/usr/bin/env python3
"""HIP-event time of the tone stage on the GPU - pt_ctx_tonemap, pt_ctx_meter, pt_ctx_accum_hdr - set against a device-to-device
copy of the colour frame measured in the same run, for the README's bullet and DESIGN.md section 4, in the style of
tools/solid_timing.py; and what the stage adds to a frame of the traced loop.

The passes.  Sizes: 1024x768 and 4096x4096.  The yardstick copies 24 B per pixel, so a case's budget is its compulsory bytes / 24
of the copy's time: tonemap 24 B (1.0), in place 24 B (1.0), the meter 12 B (0.5; 16 B with ids: 0.67), pt_ctx_accum_hdr 36 B
(1.5).  The meter's worst case for its LDS atomics, a frame of one colour, is timed beside a noise frame and carries no budget.
pt_ctx_accum_hdr needs a held frame: cornell accumulated at 1 sample per pixel at that size.  The protocol is tools/timing.py's, on
the null stream; the like-for-like yardstick is the copy with a stream synchronise after each ("copy_sync"), the back-to-back
copy ("copy") is recorded beside it.  The meter's call also clears and downloads its counters: that is part of its time.

The loop.  On cornell at 1024x768, 8 samples per pixel, wall time per frame (timing.wall), median of 20, of
  render:   pt_ctx_render                                                  - what the loop traced before
  hdr:      pt_ctx_accum_reset + pt_ctx_accumulate + pt_ctx_accum_hdr      - what it traces with a tone option
  tone:     pt_ctx_meter + pt_meter_exposure + pt_meter_adapt + pt_ctx_tonemap, in place
The stage adds (hdr - render) + tone per frame.

    python tools/timing_tone.py [out.json]
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
import tone_ref as ref  # noqa: E402
from ptlib import PtConfig, PtStats  # noqa: E402

ta = ref.tone_abi
SIZES = ((1024, 768), (4096, 4096))
COPY_BYTES = 24
LOOP_SIZE, LOOP_SPP, FRAMES = (1024, 768), 8, 20


def main():
    L = ptlib.product()
    timing.need_gpu(L, "timing_tone")
    doc = {"command": "python tools/timing_tone.py", "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up; the ratio is "
                     "against the copy with a stream synchronise after each, the budget is compulsory bytes / %d; the loop: wall time "
                     "per frame, median of %d after a warm-up" % (timing.WINDOW_MS, COPY_BYTES, FRAMES),
           "cases": {}, "loop": {}}
    rng = np.random.default_rng(1)
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    with timing.Events() as ev, gpudev.Device(L, sc) as d:
        aces = ta.pt_tonemap_params(ref.ACES, 0, 0.7, 4.0)
        luma = ta.pt_tonemap_params(ref.REINHARD, ref.LUMA, 0.7, 4.0)
        stats = ta.pt_meter_stats()
        skip = ta.pt_meter_params(ta.PT_METER_SKIP_MISSES, 0, 0, 0, 0)
        for w, h in SIZES:
            n = w * h
            d_rgb, d_out, d_flat, d_id = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 4)
            d.upload(d_rgb, (rng.random(n * 3, dtype=np.float32) * np.float32(6.0)) ** 3)  # noise over some nine octaves
            d.upload(d_flat, np.tile(np.array((0.5, 0.25, 2.0), dtype=np.float32), n))
            ids = np.zeros((h, w), dtype=np.int32)
            ids[: h // 4, :] = -1  # a quarter of the frame is sky
            d.upload(d_id, ids.reshape(n))
            cfg = PtConfig(w, h, 1, 0, 7, 0, 0, 0, 0)
            st = PtStats()
            assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg), d_out, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
            copy_sync, copy = timing.copy_yardstick(d_out, d_rgb, n * 12)
            yard = {"copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy)}

            def tonemap(p, out):
                return lambda: L.pt_ctx_tonemap(d.ctx, w, h, C.byref(p), d_rgb, out, None)

            def meter(rgb, par, ids_p):
                return lambda: L.pt_ctx_meter(d.ctx, w, h, C.byref(par) if par is not None else None, rgb, ids_p, C.byref(stats), None)

            cases = (("tonemap aces, out of place", tonemap(aces, d_out), 24, True),
                     ("tonemap reinhard luma, out of place", tonemap(luma, d_out), 24, True),
                     ("meter, noise frame", meter(d_rgb, None, None), 12, True),
                     ("meter, noise frame, ids", meter(d_rgb, skip, d_id), 16, True),
                     ("meter, one colour", meter(d_flat, None, None), 12, False),
                     ("accum_hdr", lambda: L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), d_out, None), 36, True),
                     ("tonemap aces, in place", tonemap(aces, d_rgb), 24, True))  # last: it overwrites the frame
            for name, call, nbytes, budgeted in cases:

                def run():
                    rc = call()
                    assert rc == 0, L.pt_last_error()

                res = {"pass": ev.measure(run), "compulsory_bytes_per_pixel": nbytes}
                res.update(yard)
                res["pass_over_copy_sync"] = res["pass"]["ms_median"] / yard["copy_sync"]["ms_median"]
                res["pass_over_copy"] = res["pass"]["ms_median"] / yard["copy"]["ms_median"]
                if budgeted:
                    res["budget_in_copies"] = nbytes / COPY_BYTES
                    res["within_budget"] = res["pass_over_copy_sync"] <= res["budget_in_copies"]
                    res["verdict"] = "HIT" if res["within_budget"] else "MISS"
                doc["cases"]["%dx%d %s" % (w, h, name)] = res
                print("%dx%d %s" % (w, h, name), "%.4f ms, %.2f copies%s" % (
                    res["pass"]["ms_median"], res["pass_over_copy_sync"],
                    " (budget %.2f): %s" % (res["budget_in_copies"], res["verdict"]) if budgeted else " (no budget)"), flush=True)
            assert L.pt_ctx_accum_reset(d.ctx) == 0
            for p in (d_rgb, d_out, d_flat, d_id):
                d.free(p)

        # ---- the loop: what the stage adds to a traced frame
        W, H = LOOP_SIZE
        n = W * H
        d_rgb = d.alloc(n * 12)
        st = PtStats()
        seed = [100]
        state = {"exposure": 1.0}

        def cfg_now():
            seed[0] += 1
            return PtConfig(W, H, LOOP_SPP, 0, seed[0], 0, 0, 0, 0)

        def render():
            assert L.pt_ctx_render(d.ctx, C.byref(cfg_now()), d_rgb, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()

        def hdr():
            cfg = cfg_now()
            assert L.pt_ctx_accum_reset(d.ctx) == 0
            assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg), d_rgb, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
            assert L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), d_rgb, None) == 0, L.pt_last_error()

        def tone():
            e, nxt = C.c_float(), C.c_float()
            assert L.pt_ctx_meter(d.ctx, W, H, None, d_rgb, None, C.byref(stats), None) == 0, L.pt_last_error()
            assert L.pt_meter_exposure(C.byref(stats), None, C.byref(e)) == 0
            assert L.pt_meter_adapt(state["exposure"], e.value, 1.0 / 30, 0.5, C.byref(nxt)) == 0
            state["exposure"] = nxt.value
            p = ta.pt_tonemap_params(ref.ACES, 0, nxt.value, 4.0)
            assert L.pt_ctx_tonemap(d.ctx, W, H, C.byref(p), d_rgb, d_rgb, None) == 0, L.pt_last_error()

        res = {"render": timing.wall(render, FRAMES), "hdr": timing.wall(hdr, FRAMES)}
        hdr()  # (the frame the tone step works on)
        res["tone"] = timing.wall(tone, FRAMES)
        res["stage_adds_ms"] = res["hdr"]["ms_median"] - res["render"]["ms_median"] + res["tone"]["ms_median"]
        key = "cornell %dx%d at %d spp" % (W, H, LOOP_SPP)
        doc["loop"][key] = res
        timing.report(key, res)
        print("the stage adds %.3f ms per frame" % res["stage_adds_ms"], flush=True)
    timing.write(doc, "tone_timing.json")


if __name__ == "__main__":
    main()
