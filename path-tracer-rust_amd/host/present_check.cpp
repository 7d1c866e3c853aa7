// present_check — pt_ctx_present's host side under a sanitizer, as a program of its own (make present-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the refusals, the table builder, pt_present_quantize_host,
// pt_write_ppm8 and the footprint arithmetic the kernels share with the host (csrc/pt_present.h), and checks each against its
// definition: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_present.h"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char **argv) {
    uint32_t T[256];
    CHECK(pt_present_thresholds(T) == PT_OK && pt_present_thresholds(nullptr) == PT_ERR_INVALID);
    CHECK(T[0] == 0u && T[255] <= 0x3f800000u);
    for (uint32_t k = 1; k < 256u; ++k) {
        CHECK(T[k] > T[k - 1]);
        CHECK(pt_to_int_with_gamma_correction(from_bits(T[k])) >= k && pt_to_int_with_gamma_correction(from_bits(T[k] - 1u)) < k);
    }
    // the lookup against the function: a stride of bit patterns, the neighbourhood of every threshold, the specials
    std::vector<float> v;
    for (uint32_t b = 0; b <= 0x3f800000u; b += 4099u) v.push_back(from_bits(b));
    for (uint32_t k = 1; k < 256u; ++k)
        for (int d = -64; d <= 64; ++d) v.push_back(from_bits(T[k] + (uint32_t)d));
    const float specials[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1e-39f, 0x1p-33f, 1.0f, 1.0000001f, 2.0f, -1.0f, INFINITY, -INFINITY, NAN, 3e38f};
    v.insert(v.end(), specials, specials + sizeof specials / sizeof *specials);
    std::vector<uint8_t> q(v.size());
    for (float e : {0.0f, 1.0f, 2.0f, 0.5f, 1e30f}) {
        CHECK(pt_present_quantize_host(v.data(), v.size(), e, q.data()) == PT_OK);
        const float mul = e == 0.0f ? 1.0f : e;
        for (size_t i = 0; i < v.size(); ++i) CHECK(q[i] == pt_to_int_with_gamma_correction(v[i] * mul));
    }
    CHECK(pt_present_quantize_host(v.data(), 0, 1.0f, nullptr) == PT_OK);
    CHECK(pt_present_quantize_host(v.data(), 1, -1.0f, q.data()) == PT_ERR_INVALID);
    CHECK(pt_present_quantize_host(v.data(), 1, NAN, q.data()) == PT_ERR_INVALID);
    CHECK(pt_present_quantize_host(nullptr, 1, 1.0f, q.data()) == PT_ERR_INVALID);
    // the footprints: a cell's weights sum to the source size, a source pixel is handed out whole, the spans stay inside
    const uint32_t sizes[][2] = {{7, 3}, {5, 2}, {8, 4}, {7, 7}, {5, 11}, {3, 7}, {67, 1}, {33, 1}, {130, 64}, {257, 100}, {129, 50},
                                 {4096, 720}, {1u << 28, 1}, {1, 1u << 28}, {1u << 14, (1u << 14) - 1u}};
    for (const auto &s : sizes) {
        const uint32_t n = s[0], on = s[1];
        const uint32_t cells[] = {0u, 1u % on, on / 2u, on - 1u};
        for (uint32_t X : cells) {
            const pt::PresentSpan sp = pt::present_span(X, n, on);
            CHECK(sp.first < sp.last && sp.last <= n);
            if (sp.last - sp.first > 4096u) continue;  // (the one-cell cases: their sum is the line below's, by the same formula)
            uint64_t sum = 0;
            for (uint32_t x = sp.first; x < sp.last; ++x) {
                const uint32_t w = pt::present_weight(X, x, n, on);
                CHECK(w >= 1u && w <= (n < on ? n : on));
                sum += w;
            }
            CHECK(sum == n);
        }
        if ((uint64_t)n * on > (1u << 16)) continue;
        std::vector<uint64_t> given(n, 0);
        for (uint32_t X = 0; X < on; ++X) {
            const pt::PresentSpan sp = pt::present_span(X, n, on);
            for (uint32_t x = sp.first; x < sp.last; ++x) given[x] += pt::present_weight(X, x, n, on);
        }
        for (uint32_t x = 0; x < n; ++x) CHECK(given[x] == on);
    }
    // the fixed point and the mean: a constant frame comes back
    for (uint32_t b : {0u, 1u, T[1], T[128], T[255], 0x3f7fffffu, 0x3f800000u}) {
        const float c = pt::present_clamp(from_bits(b), 1.0f);
        const uint64_t fx = pt::present_fixed(c);
        CHECK(fx <= (1ull << 32));
        const float m = pt::present_mean(fx * 35u, 35.0 * 4294967296.0);
        CHECK(m == (float)((double)fx / 4294967296.0));
        if (c >= 0x1p-8f) CHECK(m == c);
    }
    // the refusals, in the header's order: each call breaks one rule and every rule after it; then what an accepted call fills in
    {
        float rgb[1];
        uint8_t out[1];
        const uint32_t BIG = 1u << 15;  // BIG * BIG = 2^30 > 2^28
        pt::PresentFrame f;
        auto check = [&](uint32_t w, uint32_t h, const pt_present_params *p, const float *d_rgb, uint8_t *d_out, const void *cx = nullptr) {
            return pt::host::check_present(cx, w, h, p, d_rgb, d_out, f);
        };
        using P = pt_present_params;
        const P neg = {3, 0, -1.0f, 7, 6}, inf = {3, 0, INFINITY, 7, 6}, nan = {3, 0, NAN, 7, 6}, fmt = {3, 0, 1.0f, 2, 6},
                flags = {3, 0, 1.0f, 1, 2}, w_alone = {3, 0, 1.0f, 1, 1}, w_alone0 = {3, 0, 0.0f, 0, 0}, w_only = {3, 0, 1.0f, 0, 0},
                h_only = {0, 3, 1.0f, 0, 0}, small = {2, 2, 1.0f, 0, 0}, big_out = {BIG, BIG, 1.0f, 0, 0}, fine = {2, 2, 2.0f, 1, 1};
        for (const P *p : {&neg, &inf, &nan}) CHECK(refused(check(0, 0, p, nullptr, nullptr), "exposure"));
        CHECK(refused(check(0, 0, &fmt, nullptr, nullptr), "format"));
        CHECK(refused(check(0, 0, &flags, nullptr, nullptr), "flags"));
        CHECK(refused(check(0, 5, &w_alone, nullptr, nullptr), "width and height"));
        CHECK(refused(check(5, 0, &w_alone0, nullptr, nullptr), "width and height"));
        CHECK(refused(check(BIG, BIG, &w_only, nullptr, nullptr), "0 alone"));
        CHECK(refused(check(BIG, BIG, &h_only, nullptr, nullptr), "0 alone"));
        CHECK(refused(check(BIG, BIG, &small, nullptr, nullptr), "2^28"));
        CHECK(refused(check(BIG, BIG, nullptr, nullptr, nullptr), "2^28"));
        CHECK(refused(check(4, 4, &big_out, nullptr, nullptr), "2^28"));
        CHECK(refused(check(4, 4, &small, nullptr, nullptr), "d_rgb"));
        CHECK(refused(check(4, 4, nullptr, rgb, nullptr), "d_out"));
        CHECK(refused(check(4, 4, &fine, rgb, out), "ctx"));
        CHECK(refused(check(1u << 14, 1u << 14, nullptr, rgb, out), "ctx"));  // 2^28 pixels exactly are allowed
        const void *ctx = rgb;  // never dereferenced
        CHECK(check(1u << 14, 1u << 14, nullptr, rgb, out, ctx) == PT_OK);
        CHECK(f.rgb == rgb && f.out == out && f.width == 1u << 14 && f.out_width == 1u << 14 && f.out_height == 1u << 14 && f.bpp == 4u &&
              f.flip && f.exposure == 1.0f && !f.table && !f.mid && !f.resamples());
        CHECK(check(4, 4, &fine, rgb, out, ctx) == PT_OK);
        CHECK(f.out_width == 2u && f.out_height == 2u && f.bpp == 3u && !f.flip && f.exposure == 2.0f && f.resamples());
    }
    // the file
    const std::string path = std::string(argc > 1 ? argv[1] : "/tmp") + "/present_check.ppm";
    std::vector<uint8_t> px(5 * 3 * 3);
    for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 37u);
    CHECK(pt_write_ppm8(path.c_str(), px.data(), 5, 3) == PT_OK);
    FILE *f = fopen(path.c_str(), "rb");
    CHECK(f);
    char buf[128];
    const size_t got = fread(buf, 1, sizeof buf, f);
    fclose(f);
    remove(path.c_str());
    CHECK(got == 11 + px.size() && !memcmp(buf, "P6\n5 3\n255\n", 11) && !memcmp(buf + 11, px.data(), px.size()));
    CHECK(pt_write_ppm8(nullptr, px.data(), 5, 3) == PT_ERR_INVALID && pt_write_ppm8(path.c_str(), px.data(), 0, 3) == PT_ERR_INVALID);
    CHECK(pt_write_ppm8((path + "/no/such").c_str(), px.data(), 5, 3) == PT_ERR_IO);
    printf("present_check: ok (%zu values, 255 thresholds)\n", v.size());
    return 0;
}
