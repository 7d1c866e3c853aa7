// frame_plan_probe — a wavefront frame's plan (host::first_request, plan_frame, shrink_request) run as render_wavefront's loop runs it,
// the allocation simulated: cases on stdin, plans on stdout, for tests/test_frame_plan.py.
#include "check_common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../csrc/pt_host.h"
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
