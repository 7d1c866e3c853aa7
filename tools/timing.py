"""How the tools/*_timing.py tools measure, written down once.  Nothing here knows a feature; a tool is its cases.

A call is often far below a millisecond, so one call is not timed: measure() puts N back-to-back calls between two HIP events
on one stream (Events.window), after a warm-up window of the same shape, with N sized by a probe window so that a window
lasts at least WINDOW_MS; it reports the window divided by N, as the median and the extremes of five windows.  The entry
points block, so a window holds the host's turn-around between calls too; the like-for-like yardstick is therefore a
device-to-device copy with a stream synchronise after each (copy_yardstick's first closure), the back-to-back copy beside it.
A chain of calls that is a frame's worth of work is timed by the wall clock, frame by frame (wall).  Importing this module
loads no library and touches no device."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402

WINDOW_MS = 250.0


def need_gpu(L, tool_name):
    assert L.pt_device_count() >= 1, "%s needs a GPU: there is nothing to time without one" % tool_name


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


class Events:
    """the two HIP events of a window on `stream` (None: the null stream), destroyed on exit"""

    def __init__(self, stream=None):
        self.hip, self.stream, self.e0, self.e1 = gpudev.hip_runtime(), stream, C.c_void_p(), C.c_void_p()

    def __enter__(self):
        assert self.hip.hipEventCreate(C.byref(self.e0)) == 0 and self.hip.hipEventCreate(C.byref(self.e1)) == 0
        return self

    def __exit__(self, *exc):
        rc = self.hip.hipEventDestroy(self.e0), self.hip.hipEventDestroy(self.e1)
        assert rc == (0, 0), rc

    def window(self, fn, n):
        """the elapsed ms of n back-to-back calls of fn"""
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        for _ in range(n):
            fn()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def measure(self, fn, **how):
        return measure(self.window, fn, **how)


def measure(window, fn, *, window_ms=WINDOW_MS, warm=20, probe=50, floor=20, windows=5):
    """ms per call of fn: window(fn, n) is the time of n calls.  A warm-up window (code objects, scratch), a probe window that
    sizes n for windows of at least window_ms, then `windows` of them"""
    window(fn, warm)
    n = max(floor, int(window_ms / (window(fn, probe) / probe)) + 1)
    return dict(calls_per_window=n, **stats([window(fn, n) / n for _ in range(windows)]))


def wall(fn, frames):
    """wall time in ms of one call of fn - a frame's chain, which ends synchronised: one warm-up call, then `frames` calls
    timed one by one"""
    fn()
    ms = []
    for _ in range(frames):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def copy_yardstick(dst, src, nbytes, stream=None):
    """(copy_sync, copy): a device-to-device copy on `stream` followed by a stream synchronise, and the copy alone"""
    hip = gpudev.hip_runtime()

    def copy():
        assert hip.hipMemcpyAsync(dst, src, nbytes, 3, stream) == 0  # device to device

    def copy_sync():
        copy()
        assert hip.hipStreamSynchronize(stream) == 0

    return copy_sync, copy


def upload_planes(d, planes):
    """{name: host array} -> {name: device pointer}, allocated on the gpudev.Device d and filled"""
    B = {}
    for k, v in planes.items():
        B[k] = d.alloc(v.nbytes)
        d.upload(B[k], v)
    return B


def free_planes(d, *dicts):
    for B in dicts:
        for p in B.values():
            d.free(p)


def report(*what):
    """a progress line; a dict is shown as JSON"""
    print(*(json.dumps(x) if isinstance(x, dict) else x for x in what), flush=True)


def write(doc, default_name):
    """the document to the command line's first argument that is no option, or to profiles/<default_name>"""
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", default_name)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("->", path)
