// pass_plan_probe — host::plan_pass, once or through host::plan_frame's retries, on the inputs given as arguments: prints the plan for
// tests/test_host_logic.py (test_pass_plan).
#include "check_common.h"
#include <cstdio>
#include <cstdlib>
#include "../csrc/pt_host.h"
using namespace pt;
// argv: npix spp want default(0/1) stack_form stack_park cand_scan has_bvh streams per_stream wave_stack n_cus budget groups_per_cu
// prints OK spp_pass m K cap bytes0 bytes1 retries.  groups_per_cu by hand: plan_pass itself, once (RETRY: it asks for a smaller pass);
// groups_per_cu 0: the library's, through host::plan_frame, which follows plan_pass's retries (no taper)
int main(int argc, char **argv) {
    if (argc != 15) return 2;
    host::PassPlanIn in;
    in.npix = strtoull(argv[1], 0, 10);
    in.spp = (uint32_t)strtoul(argv[2], 0, 10);
    in.want = strtoull(argv[3], 0, 10);
    in.want_is_default = argv[4][0] == '1';
    in.stack_form = argv[5][0] == '1';
    in.stack_park = argv[6][0] == '1';
    in.cand_scan = argv[7][0] == '1';
    in.has_bvh = argv[8][0] == '1';
    in.streams = strtoull(argv[9], 0, 10);
    in.per_stream = (uint32_t)strtoul(argv[10], 0, 10);
    in.wave_stack = (uint32_t)strtoul(argv[11], 0, 10);
    in.n_cus = (uint32_t)strtoul(argv[12], 0, 10);
    in.stack_budget = (size_t)strtoull(argv[13], 0, 10);
    in.groups_per_cu = (uint32_t)strtoul(argv[14], 0, 10);
    host::FramePlan f;
    int rc;
    if (in.groups_per_cu) {
        uint64_t next = in.want;
        rc = host::plan_pass(in, f.pass, &next);
    } else {
        host::FramePlanIn fin;
        fin.pass = in;
        fin.rays_per_pass = in.want_is_default ? 0u : in.want;
        host::FrameRequest req;
        req.want = in.want;
        req.stack_budget = in.stack_budget;
        rc = host::plan_frame(fin, req, f);
    }
    if (rc == host::kPlanTooLarge) { printf("TOOLARGE\n"); return 0; }
    if (rc == host::kPlanRetry) { printf("RETRY\n"); return 0; }
    printf("OK %u %u %u %u %zu %zu %d\n", f.pass.spp_pass, f.pass.m, f.pass.K, f.pass.cap, f.pass.bytes0, f.pass.bytes1, f.retries);
    return 0;
}
