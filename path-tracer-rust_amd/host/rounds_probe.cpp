// rounds_probe — the round arithmetic (host::plan_rounds / round_launch), the sample schedules of the calls that render to a noise target,
// and pt_ctx_render_adaptive's refusals, tile geometry and totals: the function named by argv[1] on the arguments after it, printed
// for tests/test_host_logic.py (test_rounds_schedules_and_tiles).
#include "check_common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;
static uint64_t num(const char *s) { return strtoull(s, 0, 0); }
// argv[1] names the function, the rest are its arguments in order; prints its results (a refusal: REFUSED and the message)
int main(int argc, char **argv) {
    const char *f = argv[1];
    auto arg = [&](int i) { return num(argv[1 + i]); };
    if (!strcmp(f, "rounds")) {  // entries spp_left rays_per_pass item_mult n_cus s_here..: the plan, then each launch
        const host::RoundPlan p = host::plan_rounds(arg(1), (uint32_t)arg(2), arg(3), (uint32_t)arg(4), (uint32_t)arg(5));
        printf("%u %u", p.round_spp, p.n_split);
        for (int i = 6; 1 + i < argc; ++i) {
            const host::RoundLaunch l = host::round_launch(arg(1), p.n_split, (uint32_t)arg(i), (uint32_t)arg(5));
            printf(" %u %u %u", l.split, l.lane_spp, l.grid);
        }
        printf("\n");
    } else if (!strcmp(f, "launch")) {  // entries n_split s_here n_cus
        const host::RoundLaunch l = host::round_launch(arg(1), (uint32_t)arg(2), (uint32_t)arg(3), (uint32_t)arg(4));
        printf("%u %u %u\n", l.split, l.lane_spp, l.grid);
    } else if (!strcmp(f, "split")) {  // c T
        printf("%u\n", host::tracked_split((uint32_t)arg(1), (uint32_t)arg(2)));
    } else if (!strcmp(f, "adaptive") || !strcmp(f, "until")) {  // [held] min_spp cap: the counts up to the cap
        const bool ad = f[0] == 'a';
        const uint32_t cap = (uint32_t)arg(ad ? 2 : 3);
        uint32_t t = ad ? host::adaptive_first_level((uint32_t)arg(1), cap) : host::until_first_target((uint32_t)arg(1), (uint32_t)arg(2), cap);
        for (int i = 0; i < 40; ++i, t = host::next_target(t, cap)) {
            printf("%u ", t);
            if (t >= cap) break;
        }
        printf("\n");
    } else if (!strcmp(f, "params")) {  // tile_error tile
        pt_adaptive_params p{(float)atof(argv[2]), (uint32_t)arg(2), 0u};
        uint32_t shift = 99;
        if (host::check_adaptive_params(p, &shift)) printf("REFUSED %s\n", pt_last_error());
        else printf("%u\n", shift);
    } else if (!strcmp(f, "cfg")) {  // width idx_begin idx_end chunk_step flags
        pt_config c{};
        c.width = (uint32_t)arg(1), c.idx_begin = (uint32_t)arg(2), c.idx_end = (uint32_t)arg(3), c.chunk_step = (uint32_t)arg(4), c.flags = (uint32_t)arg(5);
        if (host::check_adaptive_cfg(c)) printf("REFUSED %s\n", pt_last_error());
        else printf("OK\n");
    } else if (!strcmp(f, "target")) {  // mean_error quantile quantile_error
        pt_noise_target t{(float)atof(argv[2]), (float)atof(argv[3]), (float)atof(argv[4]), 0u};
        if (host::check_noise_target(t)) printf("REFUSED %s\n", pt_last_error());
        else printf("OK\n");
    } else if (!strcmp(f, "tiles")) {  // width rows tile_shift [err_sum (spp err)..]: err "-" = no error yet
        host::TileGeometry g{};
        if (host::tile_geometry((uint32_t)arg(1), (uint32_t)arg(2), (uint32_t)arg(3), g)) { printf("REFUSED %s\n", pt_last_error()); return 0; }
        printf("%u %u %u", g.tile_shift, g.tiles_x, g.tiles);
        if (argc > 5) {
            std::vector<uint32_t> spp;
            std::vector<unsigned long long> err;
            for (int i = 5; 1 + i + 1 < argc; i += 2) {
                spp.push_back((uint32_t)arg(i));
                err.push_back(argv[1 + i + 1][0] == '-' ? kTileNoError : arg(i + 1));
            }
            if (spp.size() != g.tiles) return 2;
            const host::TileTotals t = host::tile_totals((uint32_t)arg(1), (uint32_t)arg(2), g, spp.data(), err.data(), arg(4));
            printf(" %llu %llu %.17g", (unsigned long long)t.samples, (unsigned long long)t.est_pixels, t.mean_error);
        }
        printf("\n");
    } else {
        return 2;
    }
    return 0;
}
