#!/usr/bin/env python3
"""What pt_ctx_render_aov_ex with PT_AOV_THROUGH_DELTA costs against pt_ctx_render_aov: for DESIGN.md section 4.  One process on
one GPU, both calls in the same run, alternating.

Per scene (cornell, mesh) and spp (8, 1) at 1024x768, with all four guide buffers (and the chain plane for the chain call):
after a warm-up of both calls, ROUNDS rounds of [a window of N plain calls, a window of N chain calls], each an event window of
tools/timing.py on a caller's stream, N chosen so that a window is at least WINDOW_MS.  Both calls block, so a window holds the
host's turn-around per call too - the same for both.  Reported per call: the median over the rounds, the extremes, and
chain_over_plain = the median of the per-round ratios.

mesh.json has no mirror or glass surface: the chain call does the plain call's intersections plus one reflect-type test per hit,
and its planes must be the plain call's bit for bit (checked here at the timed size).  Its budget is the plain call's time times
BUDGET; the margin is for the chain loop's registers.  cornell has no budget: the chain call traces more rays there.  What bounds
it is recorded with it - the mean of the chain plane (sample 0's extra rays per pixel) and the mean over waves of a wave's
maximum (a wave loops until its longest chain ends; lanes are consecutive samples of one pixel at spp 8 and 8 pixels per wave,
64 consecutive pixels per wave at spp 1, so the chain plane's maximum over those pixels stands for the wave's).

    python tools/aov_chain_timing.py [out.json]
"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402
from ptlib import PtAovParams, PtConfig  # noqa: E402

W, H = 1024, 768
SPPS = (8, 1)
SCENES = ("mesh", "cornell")
BUDGET = 1.10
BUDGETED = ("mesh",)
WINDOW_MS = timing.WINDOW_MS
ROUNDS = 5
THROUGH_DELTA = ptlib.abi.PT_AOV_THROUGH_DELTA


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    L = ptlib.product()
    timing.need_gpu(L, "aov_chain_timing")
    n = W * H
    sizes = (n * 12, n * 12, n * 4, n * 4, n * 4)
    doc = {"command": "python tools/aov_chain_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(), "size": [W, H],
           "method": "%d rounds of [N plain calls, N chain calls], each window between two HIP events on one stream (window >= %.0f ms), "
                     "after a warm-up of both; ms per call; chain_over_plain = median of the per-round ratios" % (ROUNDS, WINDOW_MS),
           "budget_rule": "scenes without a delta surface (%s): chain <= %.2f x plain" % (", ".join(BUDGETED), BUDGET),
           "max_chain": 8, "cases": {}}
    on = PtAovParams(THROUGH_DELTA, 0)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        bufs = {side: [d.alloc(nbytes) for nbytes in sizes] for side in ("plain", "chain")}

        def download(side):
            return [d.download(p, nbytes // 4, np.uint32) for p, nbytes in zip(bufs[side], sizes)]

        for sid in SCENES:
            d.set_scene(ptlib.load_scene_py(ptlib.scene_path(sid)))
            for spp in SPPS:
                cfg = PtConfig(W, H, spp, 0, 7, 0, 0, 0, 0)

                def plain():
                    assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), *bufs["plain"][:4], stream) == 0, L.pt_last_error()

                def chain():
                    assert L.pt_ctx_render_aov_ex(d.ctx, C.byref(cfg), C.byref(on), *bufs["chain"], stream) == 0, L.pt_last_error()

                ev.window(plain, 10)
                ev.window(chain, 10)
                calls = max(10, int(WINDOW_MS / (max(ev.window(chain, 20), ev.window(plain, 20)) / 20)) + 1)
                rounds = [(ev.window(plain, calls) / calls, ev.window(chain, calls) / calls) for _ in range(ROUNDS)]
                ratios = [r[1] / r[0] for r in rounds]
                a, b = download("plain"), download("chain")
                plane = b[4]
                group = 64 // min(spp, 64)  # pixels per wave
                per_wave = plane[:n - n % group].reshape(-1, group).max(axis=1)
                res = {"calls_per_window": calls, "plain_ms": spread([r[0] for r in rounds]), "chain_ms": spread([r[1] for r in rounds]),
                       "chain_over_plain": statistics.median(ratios), "ratio_min": min(ratios), "ratio_max": max(ratios),
                       "chain_plane_mean": float(plane.mean()), "chain_plane_max": int(plane.max()),
                       "chain_plane_mean_of_wave_max": float(per_wave.mean()),
                       "same_bits_as_plain": bool(all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])))}
                if sid in BUDGETED:
                    assert res["same_bits_as_plain"] and res["chain_plane_max"] == 0, "a scene without delta surfaces must give the plain bits"
                    res["budget"] = BUDGET
                    res["verdict"] = "HIT" if res["chain_over_plain"] <= BUDGET else "MISS"
                key = "%s %dx%d @ %d spp" % (sid, W, H, spp)
                doc["cases"][key] = res
                timing.report(key, res)
    timing.write(doc, "aov_chain_timing.json")


if __name__ == "__main__":
    main()
