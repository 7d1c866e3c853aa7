// sincos_check — csrc/pt_math.h's sincos_f32 (the fused, sign-outside form) against the UNFUSED form it replaced, as a program
// of its own (make sincos-check builds it with -fsanitize=address,undefined and runs it; no device, no Python).  The unfused
// form is restated here from glibc's sinf / cosf (ARM optimized-routines): every product and every sum rounded on its own
// (this file is compiled with -ffp-contract=off like every unit of the library), the quadrant's sign carried by x and by a
// negated cosine table.  All 2^24 arguments the path tracer can reach - r1 = fl(2 pi) * (k * 2^-24), k = 0 .. 2^24 - 1 - are
// compared bit for bit, sine and cosine; the two mismatch counts are printed and a non-zero one ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_math.h"

namespace unfused {
constexpr double kHpiInv = 0x1.45F306DC9C883p+23, kHpi = 0x1.921FB54442D18p0;
constexpr double kC0 = 0x1p0, kC1 = -0x1.ffffffd0c621cp-2, kC2 = 0x1.55553e1068f19p-5, kC3 = -0x1.6c087e89a359dp-10,
                 kC4 = 0x1.99343027bf8c3p-16;
constexpr double kS1 = -0x1.555545995a603p-3, kS2 = 0x1.1107605230bc4p-7, kS3 = -0x1.994eb3774cf24p-13;

static float sin_poly(double x, double x2) {
    const double x3 = x * x2;
    const double s1 = kS2 + x2 * kS3;
    const double x7 = x3 * x2;
    const double s = x + x3 * kS1;
    return (float)(s + x7 * s1);
}
static float cos_poly(double x2, bool flip) {
    const double g = flip ? -1.0 : 1.0;
    const double x4 = x2 * x2;
    const double c2 = g * kC3 + x2 * (g * kC4);
    const double c1 = g * kC1 + x2 * (g * kC2);
    const double x6 = x4 * x2;
    const double c = g * kC0 + x2 * c1;
    return (float)(c + x6 * c2);
}
static void sincos(float y, float *s_out, float *c_out) {
    double x = (double)y;
    const double r = x * kHpiInv;
    const int n = ((int32_t)r + 0x800000) >> 24;
    x = x - (double)n * kHpi;
    const int q = n & 3;
    const double sgn = (q == 1 || q == 2) ? -1.0 : 1.0;
    const float sp = sin_poly(x * sgn, x * x);
    const float cp = cos_poly(x * x, (n & 2) != 0);
    const bool even = (n & 1) == 0;
    *s_out = even ? sp : cp;
    *c_out = even ? cp : sp;
}
}  // namespace unfused

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main() {
    unsigned long long bad_sin = 0, bad_cos = 0;
    uint32_t quadrants = 0;
    for (uint32_t k = 0; k < (1u << 24); ++k) {
        const float r1 = (2.0f * 3.141592653589793f) * pt::unit_f32(k << 8);
        float s, c, ws, wc;
        pt::sincos_f32(r1, &s, &c);
        unfused::sincos(r1, &ws, &wc);
        bad_sin += bits(s) != bits(ws);
        bad_cos += bits(c) != bits(wc);
        quadrants |= 1u << (((int32_t)((double)r1 * unfused::kHpiInv) + 0x800000) >> 24);
    }
    CHECK(quadrants == 0x1fu);  // the sweep reached n = 0 .. 4
    printf("sincos_check: %u arguments, sin mismatches %llu, cos mismatches %llu\n", 1u << 24, bad_sin, bad_cos);
    if (bad_sin != 0 || bad_cos != 0) return 1;
    printf("sincos_check: ok\n");
    return 0;
}
