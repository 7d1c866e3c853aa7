"""A wavefront frame's plan (csrc/pt_host.h: first_request, plan_frame, shrink_request) on the CPU.

- THE RECORDING.  tests/golden/frame_plans_parent.json holds, for a grid of frames, what the sizing block of render_wavefront
  gave at the commit the file names - the block that stood in pt_api.hip before the planner existed, run on the CPU with its two
  HIP calls replaced by inputs (mem_avail for hipMemGetInfo; `oom`, a total above which the frame's allocations "fail", for
  DevBuf::ensure).  Per case: the first attempt's spp_pass, m, K, cap, bytes0, bytes1, the taper's n_cut, pieces, extra0, extra1,
  the kPlanRetry answers followed, the return code, and every attempt of the out-of-memory ladder as [spp_pass, K, n_cut].  The
  planner must give the same, compared with ==.  A case's "in" is the planner's input field by field (scene.*: the DevScene
  counts lds_layout reads, those of cornell.json and mesh.json as pt_ctx_set_scene sets them).
  Which case reaches which leg of "longer streams only if the pass and the staging stay the same" (recorded as `long`: 0 not
  tried, 1 tried and passed on to plan_taper, 2 plan_pass refuses the longer streams, 4 the staging changes) was checked with the parent's block:
    * long-staging: 30 objects instead of cornell's 11 put the staging cliff between m = 21 and m = 32: leg 4;
    * long-pass: 640x480 @4096 under 3 GiB - at 683 samples the longer streams make it a small frame, whose shorter streams need
      more stacks than the budget: plan_pass answers kPlanRetry, a pass of other samples: leg 2.  (The comparison of spp_pass
      itself cannot fail once plan_pass says kPlanOk for the same `want`: spp_pass is computed from `want` alone.)
- THE LADDER after failed allocations, from the planner's functions alone: a frame's plan shrunk until nothing smaller is left
  (nobody may exhaust a shared card on purpose: this is where the ladder is tested).  The first step only drops the taper: the
  same request but for try_taper, the same samples and slices.  Where the taper had not brought longer streams (mesh.json's
  frame; knobs set by hand) the PassPlan is the same field by field.  The BENCH frame's default taper comes with streams of
  24 Ki primaries, which go with it - at the parent too: (m, K) = (32, 24576) tapered, (27, 29128) after the step, 4 781 506 560
  bytes before and 4 772 331 520 after.  Every later step asks for passes of half the samples (want = npix x max(1, spp_pass / 2));
  plan_pass makes passes of equal length of that, at most a twentieth longer.  No step raises the bytes."""
import json
import os

import pytest

import ptlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_plans_parent.json")
FIRST = ("spp_pass", "m", "K", "cap", "bytes0", "bytes1", "n_cut", "pieces", "extra0", "extra1", "retries")


def planner(cases, *args):
    """host/frame_plan_probe.cpp on the cases: its lines"""
    text = "".join(" ".join("%s=%d" % kv for kv in c.items()) + "\n" for c in cases)
    return ptlib.host_program("frame_plan_probe")(*args, input=text.encode()).splitlines()


def parse(line):
    """a driver line -> {"rc", the first attempt's figures, "attempts": [[spp_pass, K, n_cut], ..]}"""
    parts = [p.split() for p in line.split("|")]
    out = {"rc": int(parts[0][0])}
    if len(parts) > 1:
        out.update(zip(FIRST, (int(v) for v in parts[1])))
        out["attempts"] = [[int(v) for v in a.split(":")] for a in parts[2]]
    return out


def test_plans_are_the_recorded_ones():
    rec = json.load(open(GOLDEN))
    assert len(rec["commit"]) == 40
    cases = rec["cases"]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) >= 30
    got = planner([c["in"] for c in cases])
    assert len(got) == len(cases)
    for c, line in zip(cases, got):
        want = {k: v for k, v in c["out"].items() if k != "long"}  # (`long` is the recorder's note, see the docstring)
        assert parse(line) == want, (c["name"], line)
    by = {c["name"]: c["out"] for c in cases}
    # what the issue of this recording asked to see in it
    b = by["bench"]
    assert (b["spp_pass"], b["m"], b["K"], b["n_cut"], b["pieces"], b["long"]) == (683, 32, 24576, 1536, 4, 1)  # 24 Ki streams, one round cut
    assert by["bench-mem-ample"] == b and by["bench-mem-binds"]["retries"] >= 1 and by["bench-mem-binds"]["spp_pass"] < 683
    assert by["mesh"]["n_cut"] == 512 and by["mesh"]["long"] == 0 and by["mesh"]["bytes1"] != 0  # half a round, parking areas
    assert by["few-samples"]["m"] == 64 and by["small-frame"]["n_cut"] == 0
    assert by["budget-stack"]["retries"] == 6 and by["budget-stack"]["spp_pass"] == 1
    assert by["long-staging"]["long"] == 4 and by["long-pass"]["long"] == 2
    assert by["bits32-explicit"]["rc"] == -1 and by["bits32-default"]["retries"] >= 1
    assert by["bench-oom-ladder"]["rc"] == 0 and len(by["bench-oom-ladder"]["attempts"]) == 3  # taper dropped, then one halving
    assert by["bench-oom-nothing-fits"]["rc"] == -3 and by["bench-oom-nothing-fits"]["attempts"][-1] == [1, 12288, 0]


@pytest.mark.parametrize("name", ["bench", "mesh", "taper-by-hand"])
def test_the_ladder_after_failed_allocations(name):
    case = {c["name"]: c for c in json.load(open(GOLDEN))["cases"]}[name]
    npix, spp = case["in"]["npix"], case["in"]["spp"]
    steps = [dict(zip(("spp_pass", "m", "K", "cap", "bytes", "n_cut", "want"), (int(v) for v in l.split())))
             for l in planner([case["in"]], "ladder")]
    first, second = steps[0], steps[1]
    assert {k: first[k] for k in ("spp_pass", "m", "K", "cap", "n_cut")} == {k: case["out"][k] for k in ("spp_pass", "m", "K", "cap", "n_cut")}
    # the first step only drops the taper
    assert first["n_cut"] > 0 and second["n_cut"] == 0 and second["want"] == first["want"]
    assert (second["spp_pass"], second["cap"]) == (first["spp_pass"], first["cap"])
    if name == "bench":  # the longer streams came with the default taper and go with it
        assert case["out"]["long"] == 1 and (first["m"], first["K"], second["m"], second["K"]) == (32, 24576, 27, 29128)
        assert (first["bytes"], second["bytes"]) == (4781506560, 4772331520)
    else:
        assert case["out"]["long"] == 0 and (second["m"], second["K"]) == (first["m"], first["K"])
    # every later step asks for passes of half the samples and gets them (equal passes: at most a twentieth longer); no taper again
    for a, b in zip(steps[1:], steps[2:]):
        half = max(1, a["spp_pass"] // 2)
        assert b["want"] == npix * half and 1 <= b["spp_pass"] <= half + half // 20 and b["spp_pass"] < a["spp_pass"] and b["n_cut"] == 0
    # it ends at one sample per pass after a bounded number of steps, and no step raises the bytes
    assert steps[-1]["spp_pass"] == 1 and len(steps) <= 2 + spp.bit_length()
    for a, b in zip(steps, steps[1:]):
        assert b["bytes"] <= a["bytes"], (a, b)
