"""tools/timing.py on the device: an event window around the copy yardstick, on the null stream and on a stream of the caller's,
measure() on it, and the events' lifetime.  The arithmetic of measure() is tests/test_timing_tools.py's, without a device."""
import math
import os
import sys

import numpy as np
import pytest

import gpudev
import ptlib
from gpudev import L  # noqa: F401  (fixture)

sys.path.insert(0, os.path.join(ptlib.ROOT, "tools"))
import timing  # noqa: E402

pytestmark = pytest.mark.gpu

NBYTES = 4096


@pytest.fixture(scope="module")
def planes(L):  # noqa: F811
    """a device with a source plane of 4 KiB and a destination of the same size"""
    with gpudev.Device(L) as d:
        src, dst = d.alloc(NBYTES), d.alloc(NBYTES)
        d.upload(src, np.arange(NBYTES // 4, dtype=np.uint32))
        d.upload(dst, np.zeros(NBYTES // 4, dtype=np.uint32))
        yield d, src, dst


def check_window(ev, copy_sync):
    ms = ev.window(copy_sync, 10)
    assert math.isfinite(ms) and ms > 0.0


def test_window_on_the_null_stream_and_the_copy_arrives(planes):
    d, src, dst = planes
    copy_sync, copy = timing.copy_yardstick(dst, src, NBYTES)
    with timing.Events() as ev:
        check_window(ev, copy_sync)
        check_window(ev, copy)  # the second event is synchronised on, so the window is closed without a stream synchronise too
    gpudev.same_bytes(d.download(dst, NBYTES // 4, np.uint32), np.arange(NBYTES // 4, dtype=np.uint32), "the copied plane")


def test_window_on_a_stream_of_the_callers(planes):
    d, src, dst = planes
    with gpudev.stream() as st, timing.Events(st) as ev:
        check_window(ev, timing.copy_yardstick(dst, src, NBYTES, st)[0])


def test_measure_on_the_device(planes):
    d, src, dst = planes
    with gpudev.stream() as st, timing.Events(st) as ev:
        res = ev.measure(timing.copy_yardstick(dst, src, NBYTES, st)[0], window_ms=5.0)
    assert set(res) == {"calls_per_window", "ms_median", "ms_min", "ms_max"}
    assert res["calls_per_window"] >= 20 and 0.0 < res["ms_min"] <= res["ms_median"] <= res["ms_max"]


def test_events_are_destroyed_on_exit_and_made_again(planes):
    d, src, dst = planes
    copy_sync, _ = timing.copy_yardstick(dst, src, NBYTES)
    for _ in range(2):
        with timing.Events() as ev:
            check_window(ev, copy_sync)
            handles = (ev.e0.value, ev.e1.value)
            assert all(handles) and handles[0] != handles[1]
