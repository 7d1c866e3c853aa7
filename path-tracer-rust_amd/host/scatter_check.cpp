// scatter_check — pt_ctx_scatter's host side under a sanitizer, as a program of its own (make scatter-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the refusals of host::check_scatter in the header's
// order over arrays allocated to their exact size, and checks what the validator hands the kernel for the given-surface form: the
// caller's values and, beside each colour, max_reflection and its reciprocal as host::material_reflectance - the routine
// flatten_scene fills a MatRec with - computes them.  A failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_probe.h"

static pt_scatter_item make_item(uint32_t sample, uint32_t depth, uint32_t branch) {
    pt_scatter_item it = {{0, 0, 0}, {0, 0, -1}, {1, 1, 1}, 0xffffffffu, sample, depth, branch};
    return it;
}

int main() {
    using pt::host::check_scatter;
    std::vector<pt::ScatterSurf> given;
    const void *ctx = &given;  // never dereferenced
    const pt_scatter_item good = make_item((1u << 24) - 1u, 11, 7), worst = make_item(1u << 24, 12, 0);
    const pt_scatter_surface glass = {{0, 0, 0}, {0, 0, 1}, {1, 1, 1}, {0, 0, 0}, PT_REFRACT},
                             matte = {{1, 2, 3}, {0, 1, 0}, {0.25f, 0.75f, 0.5f}, {4, 5, 6}, PT_DIFFUSE},
                             black = {{0, 0, 0}, {1, 0, 0}, {0, 0, 0}, {0, 0, 0}, PT_SPECULAR}, unknown = {{0, 0, 0}, {0, 0, 1}, {1, 1, 1}, {0, 0, 0}, 3};
    pt_scatter_out out[3];
    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    CHECK(refused(check_scatter(nullptr, 0x43, nullptr, nullptr, 0, out, given), "items or out"));
    CHECK(refused(check_scatter(nullptr, 0x43, &worst, nullptr, 0, nullptr, given), "items or out"));
    CHECK(refused(check_scatter(nullptr, 0x43, &worst, nullptr, 0, out, given), "n is 0"));
    CHECK(refused(check_scatter(nullptr, 0x40, &worst, nullptr, 1, out, given), "form"));
    CHECK(refused(check_scatter(nullptr, 3, &worst, nullptr, 1, out, given), "form"));
    CHECK(refused(check_scatter(nullptr, PT_SCATTER_BY_ID | PT_SCATTER_DEFER_REFRACT | PT_SCATTER_REFRACT_ONLY, &worst, nullptr, 1, out, given), "form"));
    CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN, &worst, nullptr, 1, out, given), "surfaces is NULL"));
    {
        const std::vector<pt_scatter_item> items = {good, make_item(1u << 24, 0, 1)}, deep = {good, good, make_item(0, 12, 1)},
                                           b0 = {make_item(0, 0, 0)}, b8 = {good, make_item(0, 0, 8)};
        const std::vector<pt_scatter_surface> bad2 = {unknown, unknown}, bad3 = {unknown, unknown, unknown};
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN, items.data(), bad2.data(), 2, out, given), "sample"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN, deep.data(), bad3.data(), 3, out, given), "depth"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_BY_ID, b0.data(), nullptr, 1, out, given), "branch"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_BY_RANK, b8.data(), nullptr, 2, out, given), "branch"));
    }
    {
        const std::vector<pt_scatter_item> items = {good, good, good};
        const std::vector<pt_scatter_surface> kinds = {matte, glass, unknown}, mixed = {glass, glass, black}, all_glass = {glass, glass, glass},
                                              fine = {matte, glass, black};
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN, items.data(), kinds.data(), 3, out, given), "reflect type"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN | PT_SCATTER_REFRACT_ONLY, items.data(), mixed.data(), 3, out, given), "not Refract"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN | PT_SCATTER_REFRACT_ONLY, items.data(), all_glass.data(), 3, out, given), "ctx"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_GIVEN | PT_SCATTER_DEFER_REFRACT, items.data(), fine.data(), 3, out, given), "ctx"));
        CHECK(refused(check_scatter(nullptr, PT_SCATTER_BY_RANK | PT_SCATTER_REFRACT_ONLY, items.data(), nullptr, 3, out, given), "ctx"));
        // ---- what the kernel is handed
        CHECK(check_scatter(ctx, PT_SCATTER_BY_ID, items.data(), nullptr, 3, out, given) == PT_OK && given.empty());
        CHECK(check_scatter(ctx, PT_SCATTER_GIVEN, items.data(), fine.data(), 3, out, given) == PT_OK && given.size() == 3u);
        for (size_t i = 0; i < 3; ++i) {
            const pt_scatter_surface &s = fine[i];
            const pt::ScatterSurf &g = given[i];
            CHECK(!memcmp(g.x, s.x, 12) && !memcmp(g.n, s.n, 12) && !memcmp(g.color, s.color, 12) && !memcmp(g.emission, s.emission, 12));
            float mx, inv;
            pt::host::material_reflectance(s.color, mx, inv);
            CHECK(g.reflect == s.reflect && !memcmp(&g.max_refl, &mx, 4) && !memcmp(&g.inv_max_refl, &inv, 4));
        }
        CHECK(given[0].max_refl == 0.75f && given[0].inv_max_refl == 1.0f / 0.75f && given[1].max_refl == 1.0f && given[1].inv_max_refl == 1.0f);
        CHECK(given[2].max_refl == 0.0f && std::isinf(given[2].inv_max_refl));  // never used: no draw is below 0
    }
    printf("scatter_check: ok\n");
    return 0;
}
