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
import subprocess

import pytest

import ptlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_plans_parent.json")

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "ptrace.h"
#include "pt_host.h"
using namespace pt;
// stdin: one case per line, "field=value ..." of host::FramePlanIn (+ oom).  stdout per case:
//   rc | spp_pass m K cap bytes0 bytes1 n_cut pieces extra0 extra1 retries | spp_pass:K:n_cut of every attempt
// `ladder`: every allocation fails; one line per attempt instead: spp_pass m K cap bytes n_cut want
static size_t frame_bytes(bool one_kernel, const host::FramePlan &p) {  // what render_wavefront's allocations ask for in all
    const size_t K = p.pass.K;
    return p.pass.bytes0 + p.taper.extra0 + (p.pass.bytes1 ? p.pass.bytes1 + p.taper.extra1 : 0u) + (!one_kernel ? K * p.pass.cap * 8u : 0u) +
           13u * K * 4u + 4u + K * 8u + 3u * K * p.pass.m * 8u;
}
int main(int argc, char **argv) {
    const bool ladder = argc > 1 && !strcmp(argv[1], "ladder");
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::map<std::string, std::string> kv;
        std::istringstream is(line);
        std::string tok;
        while (is >> tok) kv[tok.substr(0, tok.find('='))] = tok.substr(tok.find('=') + 1);
        auto g = [&](const char *k, unsigned long long d = 0) { return kv.count(k) ? strtoull(kv[k].c_str(), 0, 10) : d; };
        host::FramePlanIn in;
        in.pass.npix = g("npix");
        in.pass.spp = (uint32_t)g("spp");
        in.pass.stack_form = g("stack_form") != 0;
        in.pass.stack_park = g("stack_park") != 0;
        in.pass.cand_scan = g("scene.cand_scan") != 0;
        in.pass.has_bvh = g("scene.n_bvh_nodes") != 0;
        in.pass.streams = g("streams");
        in.pass.per_stream = (uint32_t)g("per_stream");
        in.pass.wave_stack = (uint32_t)g("wave_stack");
        in.pass.n_cus = (uint32_t)g("n_cus");
        in.rays_per_pass = g("rays_per_pass");
        in.rays_per_pass_tuned = g("rays_per_pass_tuned");
        in.mem_budget = g("mem_budget");
        in.mem_avail = g("mem_avail");
        in.mem_share = (uint32_t)g("mem_share", 1);
        in.probe = g("probe") != 0;
        in.taper_cut = kv.count("taper_cut") ? atoll(kv["taper_cut"].c_str()) : -1;
        in.taper_pieces = (uint32_t)g("taper_pieces");
        in.lds_pad = g("lds_pad");
        in.scene.n_objs = (uint32_t)g("scene.n_objs");
        in.scene.n_tris = (uint32_t)g("scene.n_tris");
        in.scene.n_cand_pairs = (uint32_t)g("scene.n_cand_pairs");
        in.scene.n_bvh_nodes = (uint32_t)g("scene.n_bvh_nodes");
        in.scene.n_bvh_nodes4 = (uint32_t)g("scene.n_bvh_nodes4");
        in.scene.bvh_stack = (uint32_t)g("scene.bvh_stack");
        in.scene.bvh_in_lds = (uint32_t)g("scene.bvh_in_lds");
        in.scene.nodes_in_lds_ok = (uint32_t)g("scene.nodes_in_lds_ok");
        in.scene.glass_defer_ok = (uint32_t)g("scene.glass_defer_ok");
        in.scene.cand_scan = (uint32_t)g("scene.cand_scan");
        const bool one_kernel = g("one_kernel") != 0;
        const size_t oom = ladder ? 1u : g("oom");  // (the ladder: every allocation fails)
        // render_wavefront's loop, the allocation simulated
        host::FrameRequest req = host::first_request(in);
        host::FramePlan plan, first;
        std::string attempts;
        int rc = 0, n = 0;
        for (;; ++n) {
            if (host::plan_frame(in, req, plan) != host::kPlanOk) {
                rc = PT_ERR_INVALID;
                break;
            }
            if (n == 0) first = plan;
            if (ladder)
                printf("%u %u %u %u %zu %u %llu\n", plan.pass.spp_pass, plan.pass.m, plan.pass.K, plan.pass.cap,
                       plan.pass.bytes0 + plan.pass.bytes1 + plan.taper.extra0 + plan.taper.extra1, plan.taper.n_cut, (unsigned long long)req.want);
            attempts += " " + std::to_string(plan.pass.spp_pass) + ":" + std::to_string(plan.pass.K) + ":" + std::to_string(plan.taper.n_cut);
            if (!oom || frame_bytes(one_kernel, plan) <= oom) break;
            if (!host::shrink_request(in, plan, req)) {
                rc = PT_ERR_HIP;
                break;
            }
            if (n > 64) return 3;
        }
        if (ladder) return 0;
        printf("%d", rc);
        if (n || rc == 0 || rc == PT_ERR_HIP)
            printf(" | %u %u %u %u %zu %zu %u %u %zu %zu %d |%s", first.pass.spp_pass, first.pass.m, first.pass.K, first.pass.cap, first.pass.bytes0,
                   first.pass.bytes1, first.taper.n_cut, first.taper.pieces, first.taper.extra0, first.taper.extra1, first.retries, attempts.c_str());
        printf("\n");
    }
    return 0;
}
"""
FIRST = ("spp_pass", "m", "K", "cap", "bytes0", "bytes1", "n_cut", "pieces", "extra0", "extra1", "retries")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_plan")
    src = d / "f.cpp"
    src.write_text(SRC)
    exe = str(d / "f")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])

    def run(cases, *args):
        text = "".join(" ".join("%s=%d" % kv for kv in c.items()) + "\n" for c in cases)
        return subprocess.run([exe] + list(args), input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    return run


def parse(line):
    """a driver line -> {"rc", the first attempt's figures, "attempts": [[spp_pass, K, n_cut], ..]}"""
    parts = [p.split() for p in line.split("|")]
    out = {"rc": int(parts[0][0])}
    if len(parts) > 1:
        out.update(zip(FIRST, (int(v) for v in parts[1])))
        out["attempts"] = [[int(v) for v in a.split(":")] for a in parts[2]]
    return out


def test_plans_are_the_recorded_ones(planner):
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
def test_the_ladder_after_failed_allocations(planner, name):
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
