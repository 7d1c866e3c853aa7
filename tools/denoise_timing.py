#!/usr/bin/env python3
"""HIP-event time of pt_ctx_denoise on the GPU, per level count and per kernel form, for DESIGN.md section 4.

The protocol is tools/timing.py's, on a caller's stream, with this tool's own counts: a warm-up of 50 calls, a probe of 200, at
least 50 calls a window.  The frame is cornell at 1024x768, 16 samples, guides at 16; pt_stats.ms_device of that
render on the same context is what the denoiser is set against.  The form is chosen per context through PT_DN_LDS_MAXSTEP
(0 = every level loads its taps from global memory, 128 = every level stages them in LDS); level i alone is the time at
i + 1 levels minus the time at i levels (the prepare pass is in every figure, the finish is folded into the last level).

    python tools/denoise_timing.py [out.json]
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402
from ptlib import PtConfig, PtStats  # noqa: E402

W, H, SPP = 1024, 768, 16
COUNTS = dict(warm=50, probe=200, floor=50)
FORMS = (("direct", {"PT_DN_LDS_MAXSTEP": "0"}), ("lds", {"PT_DN_LDS_MAXSTEP": "128"}), ("default", None))


def main():
    L = ptlib.product()
    timing.need_gpu(L, "denoise_timing")
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    npix = W * H
    doc = {"frame": "cornell %dx%d, %d spp, guides at %d" % (W, H, SPP, SPP), "isa_hash": L.pt_kernel_isa_hash().decode(),
           "command": "python tools/denoise_timing.py", "forms": {}}
    os.environ.pop("PT_DN_LDS_MAXSTEP", None)  # "default" is the variable unset
    with gpudev.stream() as stream:
        for form, env in FORMS:
            with gpudev.Device(L, sc, env=env) as d, timing.Events(stream) as ev:
                color, albedo, normal, depth, out = (d.alloc(npix * k * 4) for k in (3, 3, 3, 1, 3))
                cfg = PtConfig(W, H, SPP, 0, 1, 0, 0, 0, 0)
                st = PtStats()
                for _ in range(3):  # the last of three: the pass rate is measured by then
                    assert L.pt_ctx_render(d.ctx, C.byref(cfg), color, None, None, None, None, C.byref(st)) == 0
                assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), albedo, normal, depth, None, None) == 0
                res = {"render_ms_device": st.ms_device, "levels": {}}
                for levels in range(1, 9):
                    p = ptlib.PtDenoiseParams(levels, 0, 0, 0, 0)

                    def denoise():
                        assert L.pt_ctx_denoise(d.ctx, W, H, C.byref(p), color, albedo, normal, depth, out, stream) == 0

                    m = res["levels"][str(levels)] = ev.measure(denoise, **COUNTS)
                    print(form, levels, m["calls_per_window"], "%.4f ms (%.4f..%.4f)" % (m["ms_median"], m["ms_min"], m["ms_max"]), flush=True)
                doc["forms"][form] = res
    timing.write(doc, "denoise_timing_1024x768.json")


if __name__ == "__main__":
    main()
