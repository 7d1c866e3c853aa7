#!/usr/bin/env python3
"""HIP-event time of pt_ctx_present on the GPU, set against a device-to-device copy of the same frame, for DESIGN.md section 4.

The cases: 1024x768 at its own size, 4096x4096 -> 1024x1024 and 4096x4096 -> 720x720, and - because a 1024x768 frame is so
small that a call is mostly its launch and its synchronise - 4096x4096 at its own size; RGBA8 in display order.  The frame is
uniform noise in [-0.1, 1.1) (the time does not depend on the values: the search is branch-free).  A call is far below a
millisecond, so one call is not timed: after a warm-up of the same shape, N back-to-back calls on a caller's stream are put between
two HIP events, N chosen so that the window is at least 0.25 s, and the window is divided by N; five such windows give the median
and the spread.  pt_ctx_present blocks (it ends in a stream synchronise), so its window holds the host's turn-around between
calls too.  The yardstick is hipMemcpyAsync, device to device, of the same source frame on the same stream, timed twice: with a
stream synchronise after every copy (the like-for-like figure, "copy_sync") and back to back ("copy").  The budget: the
same-size form within the copy (it reads the same bytes and writes a third), the resampling form within twice the copy.
Beside them the one-core host time of what the device call replaces: pt_to_int_with_gamma_correction over every value of the
frame (a C loop, compiled here with cc; a quarter of the 4096x4096 frame, times four), and pt_present_quantize_host over the same.

    python tools/present_timing.py [out.json]
"""
import ctypes as C
import json
import os
import statistics
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

CASES = (("1024x768 same size", (1024, 768), (0, 0), 1.0), ("4096x4096 same size", (4096, 4096), (0, 0), 1.0),
         ("4096x4096 -> 1024x1024", (4096, 4096), (1024, 1024), 2.0),
         ("4096x4096 -> 720x720", (4096, 4096), (720, 720), 2.0))
WINDOW_MS = 250.0

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


def main(stream):
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "present_timing needs a GPU: there is nothing to time without one"
    hip = gpudev.hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert L.pt_ctx_create(0, C.byref(ctx)) == 0, L.pt_last_error()
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    tmp = tempfile.mkdtemp()
    gamma_loop = host_loop(tmp)
    doc = {"command": "python tools/present_timing.py", "isa_hash": L.pt_kernel_isa_hash().decode(), "format": "RGBA8, display order",
           "method": "median of 5 HIP-event windows of N back-to-back calls (window >= %.0f ms) / N, after a warm-up" % WINDOW_MS,
           "cases": {}}
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
        timed(fn, 20)  # warm-up: code objects, the table, the scratch
        n = max(20, int(WINDOW_MS / (timed(fn, 50) / 50)) + 1)
        per = [timed(fn, n) / n for _ in range(5)]
        return {"calls_per_window": n, "ms_median": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}

    for name, (w, h), (ow, oh), budget in CASES:
        npix = w * h
        frame = (rng.random(npix * 3, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
        d_rgb, d_copy, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p, nbytes in ((d_rgb, npix * 12), (d_copy, npix * 12), (d_out, (ow or w) * (oh or h) * 4)):
            assert L.pt_device_malloc(0, nbytes, C.byref(p)) == 0, L.pt_last_error()
        assert hip.hipMemcpy(d_rgb, frame.ctypes.data_as(C.c_void_p), frame.nbytes, 1) == 0
        pp = ptlib.PtPresentParams(ow, oh, 0.0, present_ref.RGBA8, 0)

        def present():
            assert L.pt_ctx_present(ctx, w, h, C.byref(pp), d_rgb, d_out, stream) == 0, L.pt_last_error()

        def copy():
            assert hip.hipMemcpyAsync(d_copy, d_rgb, npix * 12, 3, stream) == 0  # device to device

        def copy_sync():
            copy()
            assert hip.hipStreamSynchronize(stream) == 0

        res = {"present": measure(present), "copy_sync": measure(copy_sync), "copy": measure(copy), "budget_in_copies": budget}
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
        print(name, json.dumps(res), flush=True)
        for p in (d_rgb, d_copy, d_out):
            L.pt_device_free(0, p)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.pt_ctx_destroy(ctx)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "present_timing.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)


if __name__ == "__main__":
    with gpudev.stream() as own:
        main(own)
