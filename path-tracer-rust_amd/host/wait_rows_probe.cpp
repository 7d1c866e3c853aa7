// wait_rows_probe — k_pass_cand's LDS budget per workgroup, its waves per SIMD and the bytes of its rows of waiting rays as
// csrc/pt_layout.h states them, with the bench pass's stream length and stream count, printed for tests/test_wait_rows_layout.py.
#include "check_common.h"
#include <cstdio>
#include "../csrc/pt_host.h"
#include "../csrc/pt_layout.h"
using namespace pt;
// the budget per workgroup without and with walks, the waves per SIMD, the bytes of the rows, and the bench pass's stream length
int main() {
    host::FramePlanIn in;
    in.pass.npix = 1024u * 768u;
    in.pass.spp = 4096;
    in.pass.stack_form = true;
    in.pass.cand_scan = true;
    in.pass.n_cus = 256;
    host::FrameRequest req;
    req.want = 512ull << 20;
    host::FramePlan f;
    if (host::plan_frame(in, req, f) != host::kPlanOk || f.retries != 0) return 1;
    const host::PassPlan &p = f.pass;
    printf("%zu %zu %d %zu %zu %u %u\n", pass_cand_lds_budget(false), pass_cand_lds_budget(true), (int)PT_CAND_WAVES,
           pass_lds_wait_bytes(false), pass_lds_wait_bytes(true), p.m, p.K);
    return 0;
}
