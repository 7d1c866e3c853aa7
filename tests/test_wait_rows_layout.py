"""k_pass_cand's rows of waiting rays (csrc/pt_layout.h: pass_lds_wait_bytes) and its budget at six workgroups per CU, on the CPU:
what lds_layout decides is asked of the header itself through tests/lds_layouts.py's helper, never restated.

- cornell.json's candidate and shading records stay staged at 1 pixel per stream, at the bench pass's stream length (host::plan_frame
  for 1024x768 @4096 on 256 CUs, before the taper) and at 64, the most plan_pass gives a frame of few samples;
- what a launch asks for never exceeds the header's own budget expression (pass_cand_lds_budget);
- the ladder of tests/lds_layouts.py - its knob ranges were chosen when the budget was a fifth of a CU's LDS - still brackets
  every cliff;
- the rows are k_pass_cand's alone: what k_intersect_cand and the megakernel ask for is what they asked for before the rows
  existed (tests/golden/wait_rows_parent_layouts.json, written from the header of the commit before)."""
import json
import os

import pytest

import lds_layouts
import ptlib

FIELDS = ("isect_staged", "isect_lds", "mega_cand", "mega_depth", "mega_spare_off", "mega_surf_off", "mega_lds")


def read_header():
    """what host/wait_rows_probe.cpp reads from the header"""
    v = [int(x) for x in ptlib.host_program("wait_rows_probe")().split()]
    return dict(zip(("budget", "budget_bvh", "waves", "rows", "rows_bvh", "bench_m", "bench_k"), v))


def test_cornell_stays_staged_within_the_budget():
    header = read_header()
    assert header["waves"] == 6 and header["rows"] == 256 * 16 and header["rows_bvh"] == 0
    assert header["budget"] * 6 <= 160 * 1024 and header["budget_bvh"] * 4 <= 160 * 1024
    resident = 256 * header["waves"]
    assert 16 <= header["bench_m"] <= 32 and -(-header["bench_k"] // resident) * resident - header["bench_k"] < resident // 2
    sc = lds_layouts._cornell()
    for sw in (0, lds_layouts.SW_DEFER):
        got = lds_layouts.layouts(sc, [(m, sw) for m in (1, header["bench_m"], 64)])
        for (L, lines), m in zip(got, (1, header["bench_m"], 64)):
            assert L["pass"] == lds_layouts.PASS_CAND and L["m"] == m and L["defer"] == (1 if sw else 0)
            assert L["staged"] == 1 and L["surf_staged"] == 1, (m, sw, L)
            assert L["pass_lds"] <= header["budget"], (m, sw, L["pass_lds"], header["budget"])
    # and the rows are in what the launch asks for: one stream pixel more costs what it cost, the rows come on top of the
    # per-wave areas and the records (7 pair records, 25 shading records)
    (a, _), (b, _) = lds_layouts.layouts(sc, [(1, 0), (64, 0)])
    assert a["pass_lds"] >= 4 * 4480 + header["rows"] and b["pass_lds"] > a["pass_lds"]


def test_walks_have_no_rows_and_stay_within_their_budget():
    header = read_header()
    sc = ptlib.load_scene_py(ptlib.scene_path("mesh"))
    for m in (1, 22, 64):
        L, _ = lds_layouts.layout(sc, m, 0)
        assert L["pass"] == lds_layouts.PASS_CAND_BVH and L["pass_lds"] <= header["budget_bvh"] + (0 if L["surf_staged"] else 8 * 1024)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_ladder_still_brackets_every_cliff(seed):
    header = read_header()
    rungs = lds_layouts.build(seed)  # (asserts that each knob range holds its cliff)
    assert [r[0] for r in rungs] == [c["name"] for c in lds_layouts.CLIFFS]
    for name, inside, outside in rungs:
        assert outside.knob == inside.knob + 1, name
        for r in (inside, outside):
            if r.L["pass"] == lds_layouts.PASS_CAND and r.L["staged"]:
                assert r.L["pass_lds"] <= header["budget"], (name, r.side, r.L["pass_lds"])


def test_intersect_and_megakernel_layouts_are_the_parents():
    want = json.load(open(os.path.join(ptlib.ROOT, "tests", "golden", "wait_rows_parent_layouts.json")))
    scenes = {"cornell": lds_layouts._cornell(), "mesh": ptlib.load_scene_py(ptlib.scene_path("mesh")),
              "mega2_spheres40_seed0": lds_layouts._mega_depth2_spheres(0, 40)}
    assert sorted(want) == sorted(scenes)
    for name, sc in scenes.items():
        ms = sorted(int(m) for m in want[name])
        for (L, _), m in zip(lds_layouts.layouts(sc, [(m, 0) for m in ms]), ms):
            assert {k: L[k] for k in FIELDS} == want[name][str(m)], (name, m)
