// denoise_check — pt_ctx_denoise's and pt_ctx_denoise_var's host side under a sanitizer, as a program of its own (make
// denoise-check builds it with -fsanitize=address,undefined and runs it; no device, no Python).  It drives both filters' refusals
// in the header's order, the limits they accept, and the levels' schedule (csrc/pt_denoise.h: DenoiseCall) against the formula as
// tests/denoise_ref.py states it, bit for bit: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_denoise.h"

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
    float buf[1];
    float *const B = buf, *const N = nullptr;
    const void *ctx = buf;  // never dereferenced
    pt::DenoiseCall call;
    const uint32_t MAX = 16384u;

    // ---- pt_ctx_denoise's refusals, in the header's order; the context is the last thing checked
    {
        using P = pt_denoise_params;
        auto check = [&](const P *p, uint32_t w, uint32_t h, const float *color, float *out, const void *cx = nullptr) {
            return pt::host::check_denoise(cx, w, h, p, color, B, B, B, out, call);
        };
        const P levels = {9, 0, 0, 0, 0}, s_neg = {5, -1.0f, 0, 0, 0}, s_nan = {5, NAN, 0, 0, 0}, s_inf = {5, INFINITY, 0, 0, 0},
                d_neg = {5, 0, 0, -0.5f, 0}, d_nan = {5, 0, 0, NAN, 0}, d_inf = {5, 0, 0, INFINITY, 0}, pow1 = {5, 0, 1.0f, 0, 0},
                pow_nan = {5, 0, NAN, 0, 0}, flags = {5, 0, 0, 0, 2}, flags2 = {5, 0, 0, 0, 0x80000001u}, limits = {8, 1.0f, 0, 1.0f, 1};
        CHECK(refused(check(&levels, 8, 8, B, B), "levels"));
        for (const P *p : {&s_neg, &s_nan, &s_inf, &d_neg, &d_nan, &d_inf}) CHECK(refused(check(p, 8, 8, B, B), "sigma"));
        CHECK(refused(check(&pow1, 8, 8, B, B), "sigma_normal_pow"));
        CHECK(refused(check(&pow_nan, 8, 8, B, B), "sigma_normal_pow"));
        CHECK(refused(check(&flags, 8, 8, B, B), "flags"));
        CHECK(refused(check(&flags2, 8, 8, B, B), "flags"));
        CHECK(refused(check(nullptr, 0, 8, B, B), "width"));
        CHECK(refused(check(nullptr, 8, 0, B, B), "width"));
        CHECK(refused(check(nullptr, MAX + 1u, MAX, B, B), "2^28"));
        CHECK(refused(check(nullptr, 0xffffffffu, 0xffffffffu, B, B), "2^28"));
        CHECK(refused(check(nullptr, 8, 8, N, B), "d_color"));
        CHECK(refused(check(nullptr, 8, 8, B, N), "d_out"));
        CHECK(refused(check(nullptr, 8, 8, B, B), "ctx"));  // everything valid but the context
        CHECK(refused(check(&limits, 8, 8, B, B), "ctx"));  // the limits themselves are accepted
        CHECK(refused(check(nullptr, MAX, MAX, B, B), "ctx"));
        // accepted: the limits, the defaults filled in, the scratch left to the caller
        CHECK(check(&limits, MAX, MAX, B, B, ctx) == PT_OK);
        CHECK(call.levels == 8u && call.f.width == MAX && call.f.height == MAX && call.f.color == B && call.f.out == B);
        CHECK(!call.f.albedo && call.f.normal == B && call.f.depth == B && !call.f.error && !call.f.guide && !call.f.u[0] && !call.f.u[1]);
        CHECK(check(nullptr, 8, 8, B, B, ctx) == PT_OK && call.levels == pt::kDenoiseDefaults.levels && call.f.albedo == B);
    }

    // ---- pt_ctx_denoise_var's, with the order: an earlier field wins over every later one
    {
        using P = pt_denoise_var_params;
        auto check = [&](const P *p, uint32_t w, uint32_t h, const float *color, const float *error, float *out, const void *cx = nullptr) {
            return pt::host::check_denoise_var(cx, w, h, p, color, error, B, B, B, out, call);
        };
        const P levels = {9, 0, 0, 0}, s_neg = {5, -1.0f, 0, 0}, s_nan = {5, NAN, 0, 0}, s_inf = {5, INFINITY, 0, 0}, d_neg = {5, 0, -0.5f, 0},
                d_nan = {5, 0, NAN, 0}, d_inf = {5, 0, INFINITY, 0}, flags = {5, 0, 0, 2}, flags2 = {5, 0, 0, 0x80000001u},
                limits = {8, 1.0f, 1.0f, 1}, all9 = {9, -1.0f, 0, 2}, all8 = {8, -1.0f, 0, 2}, all_flags = {8, 1.0f, 0, 2};
        CHECK(refused(check(&levels, 8, 8, B, B, B), "levels"));
        for (const P *p : {&s_neg, &s_nan, &s_inf, &d_neg, &d_nan, &d_inf}) CHECK(refused(check(p, 8, 8, B, B, B), "sigma"));
        CHECK(refused(check(&flags, 8, 8, B, B, B), "flags"));
        CHECK(refused(check(&flags2, 8, 8, B, B, B), "flags"));
        CHECK(refused(check(nullptr, 0, 8, B, B, B), "width"));
        CHECK(refused(check(nullptr, 8, 0, B, B, B), "width"));
        CHECK(refused(check(nullptr, MAX + 1u, MAX, B, B, B), "2^28"));
        CHECK(refused(check(nullptr, 0xffffffffu, 0xffffffffu, B, B, B), "2^28"));
        CHECK(refused(check(nullptr, 8, 8, N, B, B), "d_color"));
        CHECK(refused(check(nullptr, 8, 8, B, N, B), "d_error"));
        CHECK(refused(check(nullptr, 8, 8, B, B, N), "d_out"));
        CHECK(refused(check(nullptr, 8, 8, B, B, B), "ctx"));
        CHECK(refused(check(&limits, 8, 8, B, B, B), "ctx"));
        CHECK(refused(check(nullptr, MAX, MAX, B, B, B), "ctx"));
        CHECK(refused(check(&all9, 0, 8, N, N, N), "levels"));
        CHECK(refused(check(&all8, 0, 8, N, N, N), "sigma"));
        CHECK(refused(check(&all_flags, 0, 8, N, N, N), "flags"));
        CHECK(refused(check(nullptr, 0, 0, N, N, N), "width"));
        CHECK(refused(check(nullptr, MAX + 1u, MAX, N, N, N), "2^28"));
        CHECK(refused(check(nullptr, 8, 8, N, N, N), "d_color"));
        CHECK(refused(check(nullptr, 8, 8, B, N, N), "d_error"));
        CHECK(check(&limits, MAX, MAX, B, B, B, ctx) == PT_OK);
        CHECK(call.levels == 8u && call.f.width == MAX && call.f.height == MAX && call.f.error == B && !call.f.albedo && !call.f.guide);
        CHECK(check(nullptr, 8, 8, B, B, B, ctx) == PT_OK && call.levels == pt::kDenoiseVarDefaults.levels && call.f.albedo == B);
    }

    // ---- the schedule, levels 1..8: sc = sigma * 2^-i, rc = 1 / (sc * sc) - or kv = sigma * sigma with an error map - and
    // sds = sigma_depth * 2^i, each one binary32 operation on an exact power of two
    size_t entries = 0;
    const float sigmas[][2] = {{0.0f, 0.0f}, {0.7f, 0.3f}};  // 0: the filter's default
    for (const auto &sg : sigmas) {
        for (uint32_t levels = 1; levels <= 8u; ++levels) {
            for (int var = 0; var < 2; ++var) {
                const pt_denoise_params p = {levels, sg[0], 0.0f, sg[1], 0};
                const pt_denoise_var_params q = {levels, sg[0], sg[1], 0};
                CHECK((var ? pt::host::check_denoise_var(ctx, 8, 8, &q, B, B, B, B, B, B, call)
                           : pt::host::check_denoise(ctx, 8, 8, &p, B, B, B, B, B, call)) == PT_OK);
                const float sigma = sg[0] != 0.0f ? sg[0] : var ? pt::kDenoiseVarDefaults.sigma_var : pt::kDenoiseDefaults.sigma_color;
                const float sigma_depth = sg[1] != 0.0f ? sg[1] : var ? pt::kDenoiseVarDefaults.sigma_depth : pt::kDenoiseDefaults.sigma_depth;
                CHECK(call.levels == levels);
                for (uint32_t i = 0; i < levels; ++i, ++entries) {
                    const float sc = sigma * ldexpf(1.0f, -(int)i);
                    CHECK(same_bits(call.rc[i], var ? sigma * sigma : 1.0f / (sc * sc)));
                    CHECK(same_bits(call.sds[i], sigma_depth * ldexpf(1.0f, (int)i)));
                }
            }
        }
    }
    printf("denoise_check: ok (%zu schedule entries)\n", entries);
    return 0;
}
