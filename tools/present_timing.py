#!/usr/bin/env python3
"""HIP-event time of pt_ctx_present on the GPU, set against a device-to-device copy of the same frame, for DESIGN.md section 4.

The cases: 1024x768 at its own size, 4096x4096 -> 1024x1024 and 4096x4096 -> 720x720, and - because a 1024x768 frame is so
small that a call is mostly its launch and its synchronise - 4096x4096 at its own size; RGBA8 in display order.  The frame is
uniform noise in [-0.1, 1.1) (the time does not depend on the values: the search is branch-free).  The protocol is
tools/timing.py's, on a caller's stream; the yardstick is its copy of the same source frame on the same stream, timed twice: with a
stream synchronise after every copy (the like-for-like figure, "copy_sync") and back to back ("copy").  The budget: the
same-size form within the copy (it reads the same bytes and writes a third), the resampling form within twice the copy.
Beside them the one-core host time of what the device call replaces: pt_to_int_with_gamma_correction over every value of the
frame (a C loop, compiled here with cc; a quarter of the 4096x4096 frame, times four), and pt_present_quantize_host over the same.

    python tools/present_timing.py [out.json]
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import present_ref  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402

CASES = (("1024x768 same size", (1024, 768), (0, 0), 1.0), ("4096x4096 same size", (4096, 4096), (0, 0), 1.0),
         ("4096x4096 -> 1024x1024", (4096, 4096), (1024, 1024), 2.0),
         ("4096x4096 -> 720x720", (4096, 4096), (720, 720), 2.0))

HOST_LOOP = r"""
#include <stddef.h>
#include <stdint.h>
uint32_t pt_to_int_with_gamma_correction(float x);
uint64_t gamma_loop(const float *v, size_t n) {
    uint64_t s = 0;
    for (size_t i = 0; i < n; ++i) s += pt_to_int_with_gamma_correction(v[i]);
    return s;
}
"""


def host_loop(tmp):
    """the C loop over pt_to_int_with_gamma_correction, or None if no C compiler is at hand"""
    src, so = os.path.join(tmp, "gamma_loop.c"), os.path.join(tmp, "gamma_loop.so")
    open(src, "w").write(HOST_LOOP)
    try:
        subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, src, "-L", ptlib.PKG, "-lptrace_hip",
                               "-Wl,-rpath," + ptlib.PKG])
    except (OSError, subprocess.CalledProcessError):
        return None
    lib = C.CDLL(so)
    lib.gamma_loop.argtypes = [C.c_void_p, C.c_size_t]
    lib.gamma_loop.restype = C.c_uint64
    return lib.gamma_loop


def main():
    L = ptlib.product()
    timing.need_gpu(L, "present_timing")
    tmp = tempfile.mkdtemp()
    gamma_loop = host_loop(tmp)
    doc = {"command": "python tools/present_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(), "format": "RGBA8, display order",
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % timing.WINDOW_MS,
           "cases": {}}
    rng = np.random.default_rng(1)
    with gpudev.stream() as stream, gpudev.Device(L) as d, timing.Events(stream) as ev:
        for name, (w, h), (ow, oh), budget in CASES:
            npix = w * h
            frame = (rng.random(npix * 3, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
            d_rgb, d_copy, d_out = d.alloc(npix * 12), d.alloc(npix * 12), d.alloc((ow or w) * (oh or h) * 4)
            d.upload(d_rgb, frame)
            pp = ptlib.PtPresentParams(ow, oh, 0.0, present_ref.RGBA8, 0)

            def present():
                assert L.pt_ctx_present(d.ctx, w, h, C.byref(pp), d_rgb, d_out, stream) == 0, L.pt_last_error()

            copy_sync, copy = timing.copy_yardstick(d_copy, d_rgb, npix * 12, stream)
            res = {"present": ev.measure(present), "copy_sync": ev.measure(copy_sync), "copy": ev.measure(copy), "budget_in_copies": budget}
            res["present_over_copy_sync"] = res["present"]["ms_median"] / res["copy_sync"]["ms_median"]
            res["present_over_copy"] = res["present"]["ms_median"] / res["copy"]["ms_median"]
            res["within_budget"] = res["present_over_copy_sync"] <= budget
            res["bytes_read"] = npix * 12
            res["bytes_downloaded_by_the_host"] = (ow or w) * (oh or h) * 4
            # the host's side of the same step, one core
            share = 4 if npix > 1 << 22 else 1
            part = frame[:frame.size // share]
            if gamma_loop:
                t0 = time.perf_counter()
                gamma_loop(part.ctypes.data_as(C.c_void_p), part.size)
                res["host_gamma_ms"] = (time.perf_counter() - t0) * 1e3 * share
            else:
                res["host_gamma_ms"] = None  # not measured: no C compiler
            out = np.zeros(part.size, dtype=np.uint8)
            t0 = time.perf_counter()
            assert L.pt_present_quantize_host(part.ctypes.data_as(C.c_void_p), part.size, 0.0, out.ctypes.data_as(C.c_void_p)) == 0
            res["host_table_ms"] = (time.perf_counter() - t0) * 1e3 * share
            res["host_share_measured"] = "1/%d of the frame, scaled" % share
            doc["cases"][name] = res
            timing.report(name, res)
            for p in (d_rgb, d_copy, d_out):
                d.free(p)
    timing.write(doc, "present_timing.json")


if __name__ == "__main__":
    main()
