// select_check — pt_ctx_select_pixels' host side under a sanitizer, as a program of its own (make select-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the refusals of host::check_select_pixels in the
// header's order and those of host::check_masked_cfg, and runs the predicate the kernel compiles (select_pixel) over host frames
// allocated to their exact size - the sizes of tests/test_gpu_masked.py - against the contract's expression spelled out here: a
// failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_masked.h"

// a plane in the style of the GPU test: values below, equal to and above `max`, NaN, +inf, -inf and -0
static std::vector<float> make_plane(uint32_t n, float max, uint32_t seed) {
    std::vector<float> v(n);
    uint32_t s = seed;
    for (float &x : v) {
        switch ((lcg(s) >> 16) % 10u) {
            case 0: x = max; break;
            case 1: x = NAN; break;
            case 2: x = INFINITY; break;
            case 3: x = -0.0f; break;
            case 4: x = -INFINITY; break;
            case 5: x = nextafterf(max, INFINITY); break;
            case 6: x = nextafterf(max, -INFINITY); break;
            default: x = 4.0f * unit(s) - 1.0f;
        }
    }
    return v;
}

int main() {
    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        float buf[4];
        uint8_t mbuf[4];
        pt::SelectFrame f;
        const void *ctx = buf;  // never dereferenced
        const pt_select_params nan_w = {NAN, 0.0f, 1}, nan_l = {0.0f, NAN, 1}, bad_flags = {0.0f, 0.0f, 1}, fine = {0.0f, 8.0f, 0},
                               infs = {INFINITY, -INFINITY, 0};
        using pt::host::check_select_pixels;
        CHECK(refused(check_select_pixels(nullptr, 0, 0, &nan_w, nullptr, nullptr, nullptr, f), "NaN"));
        CHECK(refused(check_select_pixels(nullptr, 0, 0, &nan_l, nullptr, nullptr, nullptr, f), "NaN"));
        CHECK(refused(check_select_pixels(nullptr, 0, 0, &bad_flags, nullptr, nullptr, nullptr, f), "flags"));
        CHECK(refused(check_select_pixels(nullptr, 0, 1u << 20, &fine, nullptr, nullptr, nullptr, f), "must be positive"));
        CHECK(refused(check_select_pixels(nullptr, 1u << 20, 0, &fine, nullptr, nullptr, nullptr, f), "must be positive"));
        CHECK(refused(check_select_pixels(nullptr, 1u << 14, (1u << 14) + 1u, &fine, nullptr, nullptr, nullptr, f), "2^28"));
        CHECK(refused(check_select_pixels(nullptr, 2, 2, nullptr, nullptr, nullptr, nullptr, f), "both NULL"));
        CHECK(refused(check_select_pixels(nullptr, 2, 2, nullptr, buf, nullptr, nullptr, f), "d_mask"));
        CHECK(refused(check_select_pixels(nullptr, 2, 2, nullptr, nullptr, buf, nullptr, f), "d_mask"));
        CHECK(refused(check_select_pixels(nullptr, 2, 2, nullptr, buf, buf, mbuf, f), "params"));
        CHECK(refused(check_select_pixels(nullptr, 2, 2, &fine, buf, buf, mbuf, f), "ctx"));
        CHECK(refused(check_select_pixels(nullptr, 1u << 14, 1u << 14, &infs, buf, nullptr, mbuf, f), "ctx"));  // 2^28 and infinities pass
        CHECK(check_select_pixels(ctx, 2, 2, &fine, buf, nullptr, mbuf, f) == PT_OK);
        CHECK(f.npix == 4u && f.weight == buf && !f.len && f.mask == mbuf && f.weight_max == 0.0f && f.len_max == 8.0f && !f.count);
        CHECK(check_select_pixels(ctx, 1u << 14, 1u << 14, &infs, nullptr, buf, mbuf, f) == PT_OK);
        CHECK(f.npix == 1u << 28 && !f.weight && f.len == buf && f.weight_max == INFINITY && f.len_max == -INFINITY);
    }
    // ---- pt_ctx_render_masked's band and flags
    {
        pt_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.width = 7, cfg.height = 5, cfg.spp = 1;
        CHECK(pt::host::check_masked_cfg(cfg) == PT_OK);
        cfg.idx_begin = 14, cfg.idx_end = 35;
        CHECK(pt::host::check_masked_cfg(cfg) == PT_OK);
        cfg.idx_begin = 15, cfg.chunk_step = 2;
        CHECK(refused(pt::host::check_masked_cfg(cfg), "whole image rows"));
        cfg.idx_begin = 14, cfg.idx_end = 34;
        CHECK(refused(pt::host::check_masked_cfg(cfg), "whole image rows"));
        cfg.idx_end = 35;
        CHECK(refused(pt::host::check_masked_cfg(cfg), "chunk_step"));
        cfg.chunk_step = 1, cfg.flags = PT_FLAG_PIPELINES(2);
        CHECK(refused(pt::host::check_masked_cfg(cfg), "PT_FLAG_PIPELINES"));
        cfg.flags = PT_FLAG_NO_BVH;
        CHECK(pt::host::check_masked_cfg(cfg) == PT_OK);
    }
    // ---- the predicate over host frames of exactly their size
    size_t pixels = 0, ones = 0, by_nan = 0;
    const uint32_t sizes[][2] = {{1, 1}, {7, 5}, {257, 3}, {64, 1}, {33, 25}};
    for (const auto &sz : sizes) {
        const uint32_t n = sz[0] * sz[1];
        for (int form = 1; form < 4; ++form) {  // the weight plane: bit 0, the length plane: bit 1
            const pt_select_params p = {0.0f, 8.0f, 0};
            const std::vector<float> weight = make_plane(n, p.weight_max, n * 3u + (uint32_t)form), len = make_plane(n, p.len_max, n * 7u + (uint32_t)form);
            std::vector<uint8_t> mask(n, 9);
            pt::SelectFrame f;
            CHECK(pt::host::check_select_pixels(&f, sz[0], sz[1], &p, form & 1 ? weight.data() : nullptr, form & 2 ? len.data() : nullptr,
                                                mask.data(), f) == PT_OK);
            for (uint32_t i = 0; i < n; ++i) {
                mask[i] = (uint8_t)pt::select_pixel(f, i);
                const bool w_in = (form & 1) && (weight[i] <= p.weight_max || std::isnan(weight[i]));
                const bool l_in = (form & 2) && (len[i] <= p.len_max || std::isnan(len[i]));
                CHECK(mask[i] == (w_in || l_in ? 1 : 0));
                ++pixels;
                ones += mask[i];
                by_nan += ((form & 1) && std::isnan(weight[i])) || ((form & 2) && std::isnan(len[i]));
            }
        }
    }
    CHECK(ones > 0 && ones < pixels && by_nan > 0);
    printf("select_check: ok (%zu pixels, %zu selected, %zu of them hold a NaN)\n", pixels, ones, by_nan);
    return 0;
}
