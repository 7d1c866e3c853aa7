// taper_plan_check — host::plan_taper and host::taper_piece: coverage, order, the extra bytes and every reason to leave the taper off.
// Judges itself: prints OK, or the check that failed on stderr (tests/test_taper_plan.py).
#include "check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;

static host::PassPlan plan_of(uint32_t K, uint32_t cap, bool park) {
    host::PassPlan p;
    p.spp_pass = 8, p.m = 4, p.K = K, p.cap = cap;
    p.bytes0 = queue_bytes(K, cap);
    p.bytes1 = park ? (size_t)K * 4u * kWaveParkBytes : 0u;
    return p;
}

static int once(const host::PassPlanIn &in, host::PassPlan &p) {  // plan_pass itself (groups_per_cu by hand): its answer
    uint64_t next = in.want;
    return host::plan_pass(in, p, &next);
}

static int follow(const host::PassPlanIn &in, host::PassPlan &p) {  // its retries followed by the library (host::plan_frame, no taper): how many
    host::FramePlanIn fin;
    fin.pass = in;  // (groups_per_cu is plan_frame's to set)
    fin.rays_per_pass = in.want_is_default ? 0u : in.want;
    host::FrameRequest req;
    req.want = in.want;
    req.stack_budget = in.stack_budget;
    host::FramePlan f;
    if (host::plan_frame(fin, req, f) != host::kPlanOk) return -1;
    p = f.pass;
    return f.retries;
}

int main() {
    // 1. coverage and order
    for (uint32_t K = 1; K <= 5; ++K)
        for (uint32_t samples = 1; samples <= 19; ++samples)
            for (uint32_t n_cut = 1; n_cut <= K + 1; ++n_cut)
                for (uint32_t pieces = 2; pieces <= 16; pieces *= 2) {
                    host::TaperIn in;
                    in.n_cut = n_cut, in.pieces = pieces, in.pass_samples = samples, in.forced = true;
                    const host::Taper t = host::plan_taper(plan_of(K, 512, false), in);
                    CHECK(t.on() && t.pieces == pieces && (1u << t.lg_pieces) == pieces);
                    CHECK(t.n_cut == (n_cut < K ? n_cut : K));  // (n_cut > K: every stream)
                    const uint32_t n_whole = K - t.n_cut, grid = t.grid(K);
                    CHECK(grid == n_whole + t.n_cut * pieces);
                    std::vector<int> seen(K * samples, 0);
                    uint32_t last_whole = 0, first_piece = grid;
                    for (uint32_t g = 0; g < grid; ++g) {
                        uint32_t b = g, s0 = 0, n = samples;
                        if (g >= n_whole) {
                            const uint32_t j = g - n_whole;
                            b = n_whole + j / pieces;
                            host::taper_piece(samples, t.lg_pieces, j % pieces, &s0, &n);
                            CHECK(n == samples / pieces || n == samples / pieces + 1u);
                            if (g < first_piece) first_piece = g;
                            if (j % pieces != 0u) {  // contiguous: a piece starts where the one before ended
                                uint32_t ps0, pn;
                                host::taper_piece(samples, t.lg_pieces, j % pieces - 1u, &ps0, &pn);
                                CHECK(ps0 + pn == s0 && pn >= n);
                            } else {
                                CHECK(s0 == 0u);
                            }
                        } else {
                            last_whole = g;
                        }
                        CHECK(b < K && s0 + n <= samples);
                        for (uint32_t s = s0; s < s0 + n; ++s) ++seen[b * samples + s];
                    }
                    for (int v : seen) CHECK(v == 1);
                    CHECK(n_whole == 0u || last_whole < first_piece);
                    CHECK(first_piece == n_whole);
                }
    // pieces that is no power of two is rounded down; more than 64 is 64
    {
        host::TaperIn in;
        in.n_cut = 2, in.pass_samples = 100, in.forced = true;
        in.pieces = 7;
        CHECK(host::plan_taper(plan_of(4, 512, false), in).pieces == 4u);
        in.pieces = 1000;
        CHECK(host::plan_taper(plan_of(4, 512, false), in).pieces == 64u);
    }
    // 2. the extra bytes
    {
        host::TaperIn in;
        in.n_cut = 1536, in.pieces = 4, in.pass_samples = 683, in.resident = 1536;
        host::PassPlan p = plan_of(16384, 4096, false);
        host::Taper t = host::plan_taper(p, in);
        CHECK(t.on() && t.n_cut == 1536u && t.grid(p.K) == 16384u + 3u * 1536u);
        CHECK(t.extra0 == (size_t)1536 * 3u * 4096u * kRayBytes && t.extra1 == 0u);
        CHECK(t.extra0 == queue_bytes(t.grid(p.K), p.cap) - p.bytes0);
        in.stack_park = true;
        p = plan_of(16384, 4096, true);
        t = host::plan_taper(p, in);
        CHECK(t.on() && t.extra1 == (size_t)1536 * 3u * 4u * kWaveParkBytes);
        CHECK(p.bytes1 + t.extra1 == (size_t)t.grid(p.K) * 4u * kWaveParkBytes);
    }
    // 3. off
    {
        const host::PassPlan p = plan_of(16384, 4096, true);
        host::TaperIn ok;
        ok.n_cut = 1536, ok.pieces = 4, ok.pass_samples = 683, ok.resident = 1536, ok.stack_park = true;
        CHECK(host::plan_taper(p, ok).on());
        host::TaperIn in = ok;
        in.n_cut = 0;  // nothing to cut
        CHECK(!host::plan_taper(p, in).on());
        in = ok, in.pieces = 1;
        CHECK(!host::plan_taper(p, in).on());
        in = ok, in.resident = 16384 / host::kTaperMinRounds + 1;  // fewer than kTaperMinRounds rounds
        CHECK(!host::plan_taper(p, in).on());
        in.resident = 16384 / host::kTaperMinRounds;
        CHECK(host::plan_taper(p, in).on());
        in = ok, in.pass_samples = 3;  // fewer samples than pieces
        CHECK(!host::plan_taper(p, in).on());
        in.pass_samples = 4;
        CHECK(host::plan_taper(p, in).on());
        const host::Taper t = host::plan_taper(p, ok);
        in = ok, in.budget = p.bytes0 + p.bytes1 + t.extra0 + t.extra1;  // the budget: to the byte
        CHECK(host::plan_taper(p, in).on());
        in.budget -= 1;
        CHECK(!host::plan_taper(p, in).on());
        in = ok, in.probe = true;
        CHECK(!host::plan_taper(p, in).on());
        // 32-bit slot indices: cap x workgroups <= 2^31 - 1
        const host::PassPlan big = plan_of(400000, 4096, false);
        in = ok, in.stack_park = false, in.n_cut = 400000, in.pieces = 2;
        CHECK((uint64_t)big.cap * big.K <= 0x7fffffffull && !host::plan_taper(big, in).on());
        in.n_cut = 100000;
        CHECK(host::plan_taper(big, in).on());
        // by hand: the rules about speed are lifted, the others are not
        in = ok, in.forced = true, in.resident = 1u << 20, in.pass_samples = 3, in.pieces = 8;
        CHECK(host::plan_taper(p, in).on());
        in.probe = true;
        CHECK(!host::plan_taper(p, in).on());
        in.probe = false, in.budget = 1;
        CHECK(!host::plan_taper(p, in).on());
        // an off taper is the launch as it was
        const host::Taper none = host::plan_taper(p, host::TaperIn{});
        CHECK(none.n_cut == 0u && none.pieces == 1u && none.lg_pieces == 0u && none.extra0 == 0u && none.extra1 == 0u && none.grid(p.K) == p.K);
    }
    // 4. plan_pass is what it was, taper or not: the bench frame and the budget frame (tests/test_host_logic.py's figures)
    {
        host::PassPlanIn in;
        in.npix = 1024u * 768u, in.spp = 4096, in.want = 512u << 20, in.stack_form = true, in.cand_scan = true, in.n_cus = 256, in.groups_per_cu = 5;
        host::PassPlan p, before;
        CHECK(once(in, p) == host::kPlanOk);
        CHECK(p.spp_pass == 683u && p.m == 22u && p.K == 35747u && p.cap == 4096u && p.bytes0 == (size_t)35747 * 4096u * 40u && p.bytes1 == 0u);
        before = p;
        host::TaperIn tin;
        tin.n_cut = 1280, tin.pieces = 4, tin.pass_samples = p.spp_pass, tin.resident = 1280;
        CHECK(host::plan_taper(p, tin).on());
        CHECK(memcmp(&before, &p, sizeof p) == 0);
        host::PassPlan again;
        CHECK(once(in, again) == host::kPlanOk && again.m == 22u && again.K == 35747u && again.bytes0 == before.bytes0);
        in.groups_per_cu = 4;
        CHECK(once(in, p) == host::kPlanOk && p.m == 24u && p.K == 32768u);
        // the budget frame: passes halved six times; a taper that breaks the budget is dropped, the pass is not halved again
        host::PassPlanIn bin;
        bin.npix = 128u * 96u, bin.spp = 64, bin.want = 512u << 20, bin.stack_form = true, bin.cand_scan = true, bin.n_cus = 256;
        bin.stack_budget = 8u << 20;
        CHECK(follow(bin, p) == 6 && p.spp_pass == 1u && p.cap == 512u);
        before = p;
        host::TaperIn tb;
        tb.n_cut = p.K, tb.pieces = 2, tb.pass_samples = 2, tb.budget = bin.stack_budget, tb.forced = true;
        CHECK(!host::plan_taper(p, tb).on());
        tb.budget = 0;
        CHECK(host::plan_taper(p, tb).on());
        CHECK(memcmp(&before, &p, sizeof p) == 0);
        CHECK(follow(bin, again) == 6 && again.spp_pass == 1u && again.K == before.K && again.bytes0 == before.bytes0);
    }
    printf("OK\n");
    return 0;
}
