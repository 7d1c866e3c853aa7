"""tools/timing.py, the measuring protocol of the tools/*_timing.py tools, without a device: the window sizing and the statistics
of measure() against a scripted window function, wall() under a scripted clock, what write() leaves on disk - and that the tools
are on it: each imports without a device, exposes main, and no longer measures, allocates or writes for itself."""
import glob
import importlib
import json
import os
import statistics
import sys

import pytest

import ptlib

TOOLS = os.path.join(ptlib.ROOT, "tools")
sys.path.insert(0, TOOLS)
import timing  # noqa: E402

TIMING_TOOLS = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*_timing.py")))
KEYS = {"calls_per_window", "ms_median", "ms_min", "ms_max"}


def scripted(per_call_ms):
    """a window function that takes per_call_ms per call, and the log of the window lengths it was asked for"""
    log = []

    def window(fn, n):
        log.append(n)
        return n * per_call_ms

    return window, log


def test_the_fifteen_tools():
    assert TIMING_TOOLS == ["aov_chain_timing", "denoise_timing", "denoise_var_timing", "masked_timing", "noise_timing", "overlay_timing",
                            "present_timing", "reproject_moved_timing", "reproject_timing", "reproject_var_timing",
                            "reproject_weighted_timing", "set_camera_timing", "set_object_timing", "solid_timing", "upsample_timing"]


def test_measure_sizes_the_window_by_the_probe():
    window, log = scripted(0.5)
    res = timing.measure(window, None)
    assert log == [20, 50, 501, 501, 501, 501, 501]
    assert set(res) == KEYS and res["calls_per_window"] == 501
    assert res["ms_median"] == res["ms_min"] == res["ms_max"] == 501 * 0.5 / 501


def test_measure_never_goes_below_the_floor():
    window, log = scripted(100.0)
    assert timing.measure(window, None)["calls_per_window"] == 20
    assert log == [20, 50] + [20] * 5


def test_measure_with_the_denoise_tools_counts():
    window, log = scripted(0.5)
    assert timing.measure(window, None, warm=50, probe=200, floor=50)["calls_per_window"] == 501
    assert log == [50, 200] + [501] * 5
    window, log = scripted(100.0)
    timing.measure(window, None, warm=50, probe=200, floor=50)
    assert log == [50, 200] + [50] * 5


def test_measure_window_ms_and_windows():
    window, log = scripted(0.5)
    assert timing.measure(window, None, window_ms=5.0, windows=3)["calls_per_window"] == 20  # 5 / 0.5 + 1 = 11: the floor
    assert log == [20, 50, 20, 20, 20]


def test_measure_reports_ms_per_call_of_the_windows():
    times = iter([1.0, 25.0, 130.0, 110.0, 150.0, 120.0, 140.0])  # warm-up, probe (0.5 ms per call), five windows
    calls = []

    def fn():
        calls.append(1)

    def window(f, n):
        f()
        return next(times)

    res = timing.measure(window, fn)
    per = [t / 501 for t in (130.0, 110.0, 150.0, 120.0, 140.0)]
    assert res == {"calls_per_window": 501, "ms_median": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}
    assert res["ms_median"] == 130.0 / 501 and list(res) == ["calls_per_window", "ms_median", "ms_min", "ms_max"]
    assert len(calls) == 7  # fn is what the window function is given


def test_wall_times_each_frame_after_one_warm_up(monkeypatch):
    # the clock is read twice per timed call and not at all around the warm-up call
    reads = iter([10.0, 10.004, 20.0, 20.001, 30.0, 30.003, 40.0, 40.002])
    events = []

    def clock():
        events.append("clock")
        return next(reads)

    monkeypatch.setattr(timing.time, "perf_counter", clock)
    res = timing.wall(lambda: events.append("call"), 4)
    assert events == ["call"] + ["clock", "call", "clock"] * 4
    ms = [(10.004 - 10.0) * 1e3, (20.001 - 20.0) * 1e3, (30.003 - 30.0) * 1e3, (40.002 - 40.0) * 1e3]
    assert res == {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    assert res["ms_min"] == pytest.approx(1.0) and res["ms_max"] == pytest.approx(4.0) and res["ms_median"] == pytest.approx(2.5)


def test_write_argv_wins_and_the_bytes(tmp_path, monkeypatch, capsys):
    doc = {"command": "python tools/x_timing.py", "cases": {"a b": {"ms_median": 0.25, "verdict": "HIT"}}, "n": [1, 2]}
    out = tmp_path / "out.json"
    monkeypatch.setattr(sys, "argv", ["x_timing.py", str(out), "ignored"])
    timing.write(doc, "x_timing.json")
    assert out.read_bytes() == (json.dumps(doc, indent=1) + "\n").encode()
    assert capsys.readouterr().out == "-> %s\n" % out
    # an option is not the path (set_camera_timing.py and set_object_timing.py take --big in front of it)
    monkeypatch.setattr(sys, "argv", ["x_timing.py", "--big", str(out)])
    timing.write({"other": 1}, "x_timing.json")
    assert out.read_bytes() == b'{\n "other": 1\n}\n'


def test_write_default_is_under_profiles(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["x_timing.py"])
    monkeypatch.setattr(timing, "ROOT", str(tmp_path))
    (tmp_path / "profiles").mkdir()
    timing.write({"a": 1}, "x_timing.json")
    assert (tmp_path / "profiles" / "x_timing.json").read_bytes() == b'{\n "a": 1\n}\n'
    assert capsys.readouterr().out == "-> %s\n" % (tmp_path / "profiles" / "x_timing.json")


def test_need_gpu_names_the_tool():
    class NoDevice:
        @staticmethod
        def pt_device_count():
            return 0

    with pytest.raises(AssertionError, match="x_timing needs a GPU"):
        timing.need_gpu(NoDevice, "x_timing")


@pytest.mark.parametrize("tool", TIMING_TOOLS)
def test_tool_imports_without_a_device_and_has_main(tool):
    assert callable(importlib.import_module(tool).main)


@pytest.mark.parametrize("tool", TIMING_TOOLS)
def test_tool_leaves_the_protocol_to_timing(tool):
    text = open(os.path.join(TOOLS, tool + ".py")).read()
    assert "import timing" in text
    for word in ("hipEvent", "pt_device_malloc", "pt_device_free", "pt_ctx_create", "pt_ctx_destroy", "hipMemcpy(", "json.dump"):
        assert word not in text, "%s.py still has %s" % (tool, word)
