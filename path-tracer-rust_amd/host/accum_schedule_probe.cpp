// accum_schedule_probe — host::accum_jobs and host::deal_to_a: the jobs of one pt_ctx_accumulate call for the counts given as arguments,
// printed for tests/test_host_logic.py (test_accumulate_schedule_is_the_deal, test_rounds_schedules_and_tiles).
#include "check_common.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;
// argv: spp megakernel total n_parts cnt.. [na..]: the jobs of one pt_ctx_accumulate call that is not cancelled, in order, with the
// half each goes to, the counts following as keep_job moves them (pt_api.hip); then the counts at the end
int main(int argc, char **argv) {
    const uint32_t spp = (uint32_t)atoi(argv[1]);
    const bool mega = atoi(argv[2]) != 0;
    host::FrameCounts f;
    f.total = (uint32_t)atoi(argv[3]);
    f.part_px = host::part_pixels(f.total, true);
    const int n_parts = atoi(argv[4]);
    if ((uint32_t)n_parts != host::part_count(f.total, f.part_px)) return 2;
    for (int i = 0; i < n_parts; ++i) f.cnt.push_back((uint32_t)atoi(argv[5 + i]));
    for (int i = 5 + n_parts; i < argc; ++i) f.na.push_back((uint32_t)atoi(argv[i]));
    for (const host::Job &j : host::accum_jobs(f, spp, mega)) {
        const uint32_t end = j.s_end ? j.s_end : spp;
        if (j.s_first >= end) continue;  // run_frame_call: nothing left to trace here
        const bool to_a = f.tracked() && host::deal_to_a(f.cnt[j.part_lo], f.na[j.part_lo]);
        printf("job %u %u %u %u %d %u %u %.9g %.9g %.9g\n", j.k0, j.n, j.s_first, end, (int)to_a, j.part_lo, j.part_hi, j.base, j.scale,
               j.boundary);
        for (uint32_t i = j.part_lo; i < j.part_hi; ++i) {
            if (to_a) f.na[i] += end - j.s_first;
            f.cnt[i] = end;
        }
    }
    printf("cnt");
    for (uint32_t v : f.cnt) printf(" %u", v);
    printf(" na");
    for (uint32_t v : f.na) printf(" %u", v);
    printf("\n");
    return 0;
}
