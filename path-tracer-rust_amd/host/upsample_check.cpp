// upsample_check — pt_ctx_upsample's host side under a sanitizer, as a program of its own (make upsample-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the refusals, pt_upsample_tap_host over whole axes
// against / and %, the multiply-and-shift divisions of csrc/pt_upsample.h against /, and runs the pixel the kernel compiles
// (upsample_pixel) over host frames allocated to their exact size - the sizes of tests/test_gpu_upsample.py - so that the
// sanitizer bounds every tap: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_upsample.h"

struct Guides {
    std::vector<float> color, depth, normal, albedo;
    std::vector<int32_t> id;
};

// random planes in the style of the GPU test: depths on a few planes and +inf, ids -1..2, normals with zero vectors, albedos on
// either side of 2^-6
static Guides make_guides(uint32_t n, uint32_t seed) {
    Guides g;
    uint32_t s = seed;
    const float planes[] = {2.0f, 6.0f, 6.25f, 9.0f, INFINITY};
    g.color.resize(3 * (size_t)n), g.normal.resize(3 * (size_t)n), g.albedo.resize(3 * (size_t)n), g.depth.resize(n), g.id.resize(n);
    auto pick = [&](uint32_t k) { return (lcg(s) >> 16) % k; };  // (the low bits of an LCG repeat after a few draws)
    for (size_t i = 0; i < 3 * (size_t)n; ++i) {
        g.color[i] = unit(s);
        g.normal[i] = pick(8u) ? unit(s) - 0.3f : 0.0f;
        g.albedo[i] = pick(8u) ? unit(s) : 0.01f;
    }
    for (uint32_t i = 0; i < n; ++i) {  // most pixels share an object and a plane, so that every tap of some pixels passes
        g.id[i] = pick(8u) < 5u ? 1 : (int32_t)pick(4u) - 1;
        g.depth[i] = g.id[i] < 0 ? INFINITY : (pick(8u) < 5u ? 6.0f : planes[pick(4u)]);
    }
    return g;
}

int main() {
    const uint32_t MAX = pt::kUpsampleMaxSize;
    // ---- the divisions: n / d for the divisors a call can have, at the numerators where a quotient changes and at the largest
    {
        size_t checked = 0;
        uint32_t s = 5u;
        const uint32_t divisors[] = {1, 2, 3, 5, 6, 7, 10, 14, 33, 66, 257, 514, 1023, 1024, 1025, 2048, 4096, 8192, 16383, 16384,
                                     32766, 32767, 32768};
        for (uint32_t d : divisors) {
            const pt::UpsampleDiv by = pt::upsample_div_make(d);
            CHECK(by.k >= 30u && by.k <= 45u);
            const uint32_t top = (1u << 30) - 1u;
            for (uint32_t n : {0u, 1u, d - 1u, d, d + 1u, top - 1u, top, top / d * d, top / d * d - 1u}) {
                CHECK(pt::upsample_div(n, by) == n / d);
                ++checked;
            }
            for (int k = 0; k < 20000; ++k) {
                const uint32_t m = (lcg(s) >> 2) / d * d;  // a multiple of d below 2^30, and its two neighbours
                for (uint32_t n : {m, m ? m - 1u : 0u, m + 1u < top ? m + 1u : top}) {
                    CHECK(pt::upsample_div(n, by) == n / d);
                    ++checked;
                }
            }
        }
        for (uint32_t d = 1; d <= 2u * MAX; ++d) {  // every divisor, at the largest numerators of a call and a few others
            const pt::UpsampleDiv by = pt::upsample_div_make(d);
            for (uint32_t n : {(1u << 29), (1u << 29) - 1u, (1u << 28) - 1u, (1u << 30) - 1u, d * 3u - 1u, d * 16383u, lcg(s) >> 2}) {
                CHECK(pt::upsample_div(n, by) == n / d);
                ++checked;
            }
        }
        printf("upsample_check: %zu divisions agree with /\n", checked);
    }

    // ---- pt_upsample_tap_host: the refusals, and whole axes against / and %
    {
        int32_t first = -7;
        float frac = -7.0f;
        CHECK(pt_upsample_tap_host(4, 2, 0, nullptr, &frac) == PT_ERR_INVALID);
        CHECK(pt_upsample_tap_host(4, 2, 0, &first, nullptr) == PT_ERR_INVALID);
        CHECK(pt_upsample_tap_host(0, 2, 0, &first, &frac) == PT_ERR_INVALID);
        CHECK(pt_upsample_tap_host(4, 0, 0, &first, &frac) == PT_ERR_INVALID);
        CHECK(pt_upsample_tap_host(MAX + 1u, 2, 0, &first, &frac) == PT_ERR_INVALID);
        CHECK(pt_upsample_tap_host(4, MAX + 1u, 0, &first, &frac) == PT_ERR_INVALID);
        CHECK(pt_upsample_tap_host(4, 2, 4, &first, &frac) == PT_ERR_INVALID);
        CHECK(first == -7 && frac == -7.0f);
        const uint32_t axes[][2] = {{1, 1}, {7, 3}, {3, 7}, {5, 2}, {2, 5}, {257, 129}, {129, 257}, {33, 33}, {33, 16}, {16, 33},
                                    {25, 12}, {12, 25}, {MAX, 1}, {1, MAX}, {MAX, MAX}, {MAX, MAX - 1u}, {MAX - 1u, MAX}, {1024, 512},
                                    {4096, 2048}};
        for (const auto &a : axes) {
            const uint32_t size = a[0], lo = a[1];
            for (uint32_t c = 0; c < size; ++c) {
                CHECK(pt_upsample_tap_host(size, lo, c, &first, &frac) == PT_OK);
                const uint32_t ax = (2u * c + 1u) * lo + size;
                CHECK(first == (int32_t)(ax / (2u * size)) - 1);
                CHECK(frac == (float)(ax % (2u * size)) / (float)(2u * size));
                CHECK(first >= -1 && first <= (int32_t)lo - 1 && frac >= 0.0f && frac < 1.0f);
                if (first < 0) CHECK(frac > 0.0f);                      // the other tap of the axis carries weight
                if (first == (int32_t)lo - 1) CHECK(1.0f - frac > 0.0f);
                if (size == lo) CHECK(first == (int32_t)c && frac == 0.0f);
            }
        }
    }

    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        float buf[4];
        int32_t ibuf[4];
        const float *F = buf;
        const int32_t *I = ibuf;
        pt::UpsampleFrame f;
        const void *ctx = buf;  // never dereferenced
        auto check = [&](const pt_upsample_params *p, uint32_t W, uint32_t H, uint32_t w, uint32_t h, const float *lo, const int32_t *loid,
                         const float *own, const int32_t *id, float *out, const void *cx) {
            return pt::host::check_upsample(cx, W, H, w, h, p, lo, lo, loid, nullptr, nullptr, own, id, nullptr, nullptr, out, nullptr, f);
        };
        const pt_upsample_params bad_dt = {-1.0f, 2.0f, 1}, bad_dt2 = {NAN, 2.0f, 1}, bad_dt3 = {INFINITY, 2.0f, 1}, bad_nm = {0.5f, NAN, 1},
                                 bad_nm2 = {0.5f, -1.5f, 1}, bad_flags = {0.5f, -1.0f, 1}, fine = {0.25f, 1.0f, 0};
        CHECK(refused(check(&bad_dt, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "depth_tol"));
        CHECK(refused(check(&bad_dt2, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "depth_tol"));
        CHECK(refused(check(&bad_dt3, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "depth_tol"));
        CHECK(refused(check(&bad_nm, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "normal_min"));
        CHECK(refused(check(&bad_nm2, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "normal_min"));
        CHECK(refused(check(&bad_flags, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "flags"));
        CHECK(refused(check(&fine, 0, 3, 3, MAX + 1u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "must be positive"));
        CHECK(refused(check(&fine, 3, 3, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "must be positive"));
        CHECK(refused(check(&fine, MAX + 1u, 3, 3, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "2^14"));
        CHECK(refused(check(&fine, 3, 3, 3, MAX + 1u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "2^14"));
        CHECK(refused(check(nullptr, 2, 2, 2, 2, nullptr, I, F, I, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, 2, 2, F, nullptr, F, I, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, 2, 2, F, I, nullptr, I, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, 2, 2, F, I, F, nullptr, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, 2, 2, F, I, F, I, nullptr, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, MAX, MAX, MAX, MAX, F, I, F, I, buf, nullptr), "ctx"));
        // accepted: the defaults are filled in; a guide given on one side only is not a guide
        CHECK(check(nullptr, 2, 2, 1, 1, F, I, F, I, buf, ctx) == PT_OK);
        CHECK(f.depth_tol == pt::kUpsampleDepthTol && f.normal_min == pt::kUpsampleNormalMin && !f.normal && !f.albedo && !f.out_weight);
        CHECK(check(&fine, 2, 2, 1, 1, F, I, F, I, buf, ctx) == PT_OK && f.depth_tol == 0.25f && f.normal_min == 1.0f);
        CHECK(pt::host::check_upsample(ctx, 2, 2, 1, 1, nullptr, F, F, I, F, nullptr, F, I, nullptr, F, buf, buf, f) == PT_OK);
        CHECK(!f.normal && !f.lo_normal && !f.albedo && !f.lo_albedo && f.out_weight == buf);
        CHECK(pt::host::check_upsample(ctx, 2, 2, 1, 1, nullptr, F, F, I, F, F, F, I, F, F, buf, buf, f) == PT_OK);
        CHECK(f.normal && f.lo_normal && f.albedo && f.lo_albedo);
    }

    // ---- the pixel over host frames of exactly their size: every tap inside them, or the sanitizer says so
    size_t pixels = 0, full = 0, partial = 0, fallback = 0;
    const uint32_t cases[][4] = {{1, 1, 1, 1}, {7, 5, 3, 2}, {257, 3, 129, 2}, {33, 25, 16, 12}, {16, 12, 33, 25}, {33, 25, 33, 25},
                                 {2, 1, 1, 2}, {1, 9, 5, 1}, {64, 2, 1, 1}};
    for (const auto &cs : cases) {
        const uint32_t W = cs[0], H = cs[1], w = cs[2], h = cs[3], n = W * H;
        for (int form = 0; form < 4; ++form) {  // normals: bit 0, albedos: bit 1
            const Guides lo = make_guides(w * h, W * 131u + h), hi = make_guides(n, w * 137u + H);
            std::vector<float> out(3 * (size_t)n, -1.0f), weight(n, -1.0f);
            const pt_upsample_params p = {0.05f, 0.5f, 0};
            pt::UpsampleFrame f;
            CHECK(pt::host::check_upsample(&f, W, H, w, h, &p, lo.color.data(), lo.depth.data(), lo.id.data(),
                                           form & 1 ? lo.normal.data() : nullptr, form & 2 ? lo.albedo.data() : nullptr, hi.depth.data(),
                                           hi.id.data(), form & 1 ? hi.normal.data() : nullptr, form & 2 ? hi.albedo.data() : nullptr,
                                           out.data(), weight.data(), f) == PT_OK);
            for (uint32_t i = 0; i < n; ++i) {
                pt::upsample_pixel(f, i, &out[3 * (size_t)i], &weight[i]);
                for (int c = 0; c < 3; ++c) CHECK(out[3 * (size_t)i + c] >= 0.0f && out[3 * (size_t)i + c] <= 1.0f);
                CHECK(weight[i] >= 0.0f && weight[i] <= 1.0f + 1e-6f);
                ++pixels;
                fallback += weight[i] == 0.0f;
                full += weight[i] > 1.0f - 1e-6f;
                partial += weight[i] > 0.0f && weight[i] <= 1.0f - 1e-6f;
            }
        }
        // equal sizes and equal guides: the colour's bytes - a zero normal fails the normal test and takes the fallback, which is
        // the same single tap; with the albedos (c / m) * m may differ from c in the last bits
        if (W == w && H == h) {
            for (int with_albedo = 0; with_albedo < 2; ++with_albedo) {
                const Guides g = make_guides(n, 11u);
                const float *alb = with_albedo ? g.albedo.data() : nullptr;
                std::vector<float> out(3 * (size_t)n, -1.0f), weight(n, -1.0f);
                pt::UpsampleFrame f;
                CHECK(pt::host::check_upsample(&f, W, H, w, h, nullptr, g.color.data(), g.depth.data(), g.id.data(), g.normal.data(), alb,
                                               g.depth.data(), g.id.data(), g.normal.data(), alb, out.data(), weight.data(), f) == PT_OK);
                for (uint32_t i = 0; i < n; ++i) pt::upsample_pixel(f, i, &out[3 * (size_t)i], &weight[i]);
                for (size_t i = 0; i < 3 * (size_t)n; ++i)
                    CHECK(with_albedo ? fabsf(out[i] - g.color[i]) <= g.color[i] * 0x1p-22f : out[i] == g.color[i]);
                for (uint32_t i = 0; i < n; ++i) CHECK(weight[i] == 1.0f || weight[i] == 0.0f);
            }
        }
    }
    CHECK(full > 0 && partial > 0 && fallback > 0);
    printf("upsample_check: ok (%zu pixels: %zu with every tap, %zu with some, %zu fallback)\n", pixels, full, partial, fallback);
    return 0;
}
