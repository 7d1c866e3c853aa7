// solid_check — pt_ctx_solid's host side under a sanitizer, as a program of its own (make solid-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the validator's refusals in the header's order,
// pt_solid_defaults, pt_solid_look_of, and pt_solid_pixel_host - the pixel the kernel compiles - on pixels whose values are worked
// out by hand below: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_solid.h"

// A 1 x 1 frame: sx = sy = (0 + 0.5) / 1 - 0.5 = 0, so S = C and g = L - C = direction * 0.5: dot(g, g) = 0.25, its root 0.5,
// 1 / 0.5 = 2, and d = direction exactly.  With C = -4.5 * direction the lens centre is L = -4 * direction, and at depth 4 the
// pixel sees P = L + d * 4 = (0, 0, 0), with v = -d.
static pt_camera toward_origin(float dx, float dy, float dz) {
    pt_camera c = {{-4.5f * dx, -4.5f * dy, -4.5f * dz}, {dx, dy, dz}, 0.5f, 0.036f, 1.5f};
    return c;
}

static bool is(const float got[3], float r, float g, float b) {
    const float want[3] = {r, g, b};
    return memcmp(got, want, sizeof want) == 0;  // the bits
}

int main() {
    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        float buf[4];
        int32_t ibuf[4];
        const float *F = buf;
        const int32_t *I = ibuf;
        const void *ctx = buf;  // never dereferenced
        pt::SolidFrame f;
        const pt_camera cam = camera(0.5f, 3.0f, 4.0f, -0.1f, -0.6f, -0.79f);
        pt_camera far_cam = cam;
        far_cam.position[0] = INFINITY;
        const pt_solid_look good[2] = {{{0.0f, 0.0f, 0.0f}, PT_SPECULAR}, {{2.0f, 2.0f, 2.0f}, PT_DIFFUSE}};
        const pt_solid_look odd[2] = {{{0.0f, 0.0f, 0.0f}, PT_REFRACT}, {{0.0f, 0.0f, 0.0f}, 3u}};
        const pt_solid_look dim[1] = {{{0.0f, -1.0f, 0.0f}, PT_DIFFUSE}};
        const pt_solid_look hot[1] = {{{0.0f, 0.0f, INFINITY}, PT_DIFFUSE}};
        auto check = [&](const pt_solid_params *p, uint32_t w, uint32_t h, const pt_camera *c, const float *n, const float *z, const int32_t *id,
                         float *out, const pt_solid_look *looks, uint32_t n_looks, const void *cx) {
            return pt::host::check_solid(cx, w, h, p, c, nullptr, n, z, id, looks, n_looks, out, f);
        };
        const uint32_t many = (1u << 20) + 1u;
        pt_solid_params p = pt::kSolidDefaults;
        p.flags = 4u, p.shininess_log2 = 11u, p.ambient = -1.0f, p.light[1] = NAN, p.background[2] = -1.0f;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "flags"));
        p.flags = PT_SOLID_REFLECT_SKY;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "shininess_log2"));
        p.shininess_log2 = 10u;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "ambient"));
        p.ambient = 0.0f, p.specular = NAN;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "specular"));
        p.specular = 0.0f;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "light"));
        p.flags |= PT_SOLID_HEADLIGHT;  // the light is not read
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "colour"));
        p.background[2] = 0.0f, p.sky_top[0] = INFINITY;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "colour"));
        p.sky_top[0] = 0.0f;
        CHECK(refused(check(&p, 0, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "must be positive"));
        CHECK(refused(check(&p, 1u << 15, 1u << 15, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "2^28"));
        CHECK(refused(check(&p, 2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "cam is NULL"));
        CHECK(refused(check(&p, 2, 2, &far_cam, nullptr, nullptr, nullptr, nullptr, nullptr, many, nullptr), "lens centre"));
        CHECK(refused(check(&p, 2, 2, &cam, nullptr, F, I, buf, nullptr, many, nullptr), "d_normal"));
        CHECK(refused(check(&p, 2, 2, &cam, F, nullptr, I, buf, nullptr, many, nullptr), "d_depth"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, nullptr, buf, nullptr, many, nullptr), "d_object_id"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, nullptr, nullptr, many, nullptr), "d_out"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, nullptr, many, nullptr), "2^20"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, nullptr, 1u << 20, nullptr), "looks is NULL"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, odd, 2, nullptr), "reflect_type"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, dim, 1, nullptr), "emission"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, hot, 1, nullptr), "emission"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, good, 2, nullptr), "ctx"));
        CHECK(refused(check(&p, 2, 2, &cam, F, F, I, buf, odd, 1, nullptr), "ctx"));  // the odd record lies beyond n_looks
        CHECK(refused(check(nullptr, 1u << 14, 1u << 14, &cam, F, F, I, buf, nullptr, 0, nullptr), "ctx"));
        // accepted: NULL params are the defaults; a table of no records is no table
        CHECK(check(nullptr, 2, 2, &cam, F, F, I, buf, good, 0, ctx) == PT_OK);
        CHECK(memcmp(&f.p, &pt::kSolidDefaults, sizeof f.p) == 0 && !f.looks && !f.n_looks && !f.albedo && f.normal == F && f.out == buf);
        CHECK(check(&p, 2, 2, &cam, F, F, I, buf, good, 2, ctx) == PT_OK && f.looks == good && f.n_looks == 2u && f.p.shininess_log2 == 10u);
        CHECK(f.width == 2u && f.height == 2u && f.L.y == cam.position[1] + cam.direction[1] * cam.focal_length);
        // the wide form: every plane handed over 16-byte aligned, and a whole group of four pixels
        alignas(16) float planes[64];
        f.albedo = nullptr, f.normal = planes, f.depth = planes + 16, f.object_id = (const int32_t *)(planes + 32), f.out = planes + 48;
        CHECK(pt::host::solid_wide(f));
        f.albedo = planes + 1;
        CHECK(!pt::host::solid_wide(f));
        f.albedo = planes, f.out = planes + 3;
        CHECK(!pt::host::solid_wide(f));
        f.out = planes, f.width = 3u, f.height = 1u;
        CHECK(!pt::host::solid_wide(f));
    }

    // ---- pt_solid_defaults, pt_solid_look_of
    {
        pt_solid_params d;
        CHECK(pt_solid_defaults(nullptr) == PT_ERR_INVALID);
        CHECK(pt_solid_defaults(&d) == PT_OK);
        CHECK(d.flags == PT_SOLID_HEADLIGHT && d.ambient == 0.1f && d.diffuse == 1.0f && d.specular == 0.5f && d.shininess_log2 == 5u);
        CHECK(is(d.light, 0.0f, 0.0f, 0.0f) && is(d.background, 0.0f, 0.0f, 0.0f));
        CHECK(is(d.sky_top, 0.25f, 0.5f, 0.75f) && is(d.sky_bottom, 0.75f, 0.75f, 0.75f));
        pt_solid_params filled;
        CHECK(pt::host::check_solid_params(&d, filled) == PT_OK && pt::host::check_solid_params(nullptr, filled) == PT_OK);
        pt_object o;
        memset(&o, 0, sizeof o);
        o.emission[0] = 2.0f, o.emission[2] = 0.125f, o.reflect_type = PT_REFRACT, o.color[0] = 0.5f;
        pt_solid_look look = {{9.0f, 9.0f, 9.0f}, 9u};
        CHECK(pt_solid_look_of(&o, &look) == PT_OK && is(look.emission, 2.0f, 0.0f, 0.125f) && look.reflect_type == PT_REFRACT);
        CHECK(pt_solid_look_of(nullptr, &look) == PT_ERR_INVALID && pt_solid_look_of(&o, nullptr) == PT_ERR_INVALID);
    }

    // ---- the pixel, by hand.  ambient 0.125, diffuse 0.5, specular 0.25, exponent 2^1; albedo A = (0.5, 1, 0.25).
    {
        const pt_camera along_z = toward_origin(0.0f, 0.0f, -1.0f);  // d = (0, 0, -1), v = (0, 0, 1), L = (0, 0, 4)
        pt_solid_params p = pt::kSolidDefaults;
        p.flags = 0u, p.ambient = 0.125f, p.diffuse = 0.5f, p.specular = 0.25f, p.shininess_log2 = 1u;
        p.background[0] = 0.25f, p.background[1] = -0.0f, p.background[2] = 3.0f;
        const float A[3] = {0.5f, 1.0f, 0.25f}, n[3] = {0.0f, 0.0f, 2.0f}, none[3] = {0.0f, 0.0f, 0.0f};  // N(n) = (0, 0, 1): 2 / sqrt(4)
        float o[3];
        auto at = [&](const pt_camera &cam, float lx, float ly, float lz, const float *albedo, const float *normal, const pt_solid_look *look,
                      int32_t id = 0, float depth = 4.0f) {
            p.light[0] = lx, p.light[1] = ly, p.light[2] = lz;
            return pt_solid_pixel_host(&cam, 1, 1, &p, 0, id, depth, albedo, normal, look, o);
        };
        // light along the normal, Q = (0, 0, 2): lv = (0, 0, 2), ll = 2, ld = lv * 0.5 = (0, 0, 1); ndl = 1, dif = 1;
        // r = N * 2 - ld = (0, 0, 1); dot(v, r) = 1, s = 1 * 1 = 1; k = (0.125 + 0.5 * 1) + 0.25 * 1 = 0.875; out = A * 0.875
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, A, n, nullptr) == PT_OK && is(o, 0.4375f, 0.875f, 0.21875f));
        // ... and without an albedo plane: (1, 1, 1) * 0.875
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, nullptr, n, nullptr) == PT_OK && is(o, 0.875f, 0.875f, 0.875f));
        // at grazing incidence, Q = (2, 0, 0): ld = (1, 0, 0), ndl = 0: dif = 0, and s = 0 because ndl > 0 fails; k = 0.125
        CHECK(at(along_z, 2.0f, 0.0f, 0.0f, A, n, nullptr) == PT_OK && is(o, 0.0625f, 0.125f, 0.03125f));
        // behind the surface, Q = (0, 0, -2): ld = (0, 0, -1), ndl = -1: dif = pos(-1) = 0, s = 0; k = 0.125
        CHECK(at(along_z, 0.0f, 0.0f, -2.0f, A, n, nullptr) == PT_OK && is(o, 0.0625f, 0.125f, 0.03125f));
        // a zero normal under the light of the first case: N = (0, 0, 0), ndl = 0; k = 0.125
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, A, none, nullptr) == PT_OK && is(o, 0.0625f, 0.125f, 0.03125f));
        // ll == 0, the light in the point itself, Q = P = (0, 0, 0): ld = (0, 0, 0), ndl = 0; k = 0.125
        CHECK(at(along_z, 0.0f, 0.0f, 0.0f, A, n, nullptr) == PT_OK && is(o, 0.0625f, 0.125f, 0.03125f));
        // ... and a headlight at depth 0: P = L = Q
        p.flags = PT_SOLID_HEADLIGHT;
        CHECK(at(along_z, NAN, NAN, NAN, A, n, nullptr, 0, 0.0f) == PT_OK && is(o, 0.0625f, 0.125f, 0.03125f));
        // the headlight at depth 4: Q = L = (0, 0, 4), lv = (0, 0, 4), ld = lv * 0.25 = (0, 0, 1): the first case again
        CHECK(at(along_z, NAN, NAN, NAN, A, n, nullptr) == PT_OK && is(o, 0.4375f, 0.875f, 0.21875f));
        p.flags = 0u;
        // a miss: the background's bits, not clamped (3 stays 3, -0 stays -0), and nothing else is looked at
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, nullptr, none, nullptr, -1, NAN) == PT_OK && is(o, 0.25f, -0.0f, 3.0f));
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, nullptr, none, nullptr, INT32_MIN, NAN) == PT_OK && is(o, 0.25f, -0.0f, 3.0f));
        // an emitter that saturates the clamp: the first case, (0.4375, 0.875, 0.21875), + (2, 0.5, 0) = (2.4375, 1.375, 0.21875)
        const pt_solid_look lamp = {{2.0f, 0.5f, 0.0f}, PT_DIFFUSE};
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, A, n, &lamp) == PT_OK && is(o, 1.0f, 1.0f, 0.21875f));
        // a mirror without PT_SOLID_REFLECT_SKY, and a glass with it, are shaded as the first case
        const pt_solid_look mirror = {{0.0f, 0.0f, 0.0f}, PT_SPECULAR}, glass = {{0.0f, 0.0f, 0.0f}, PT_REFRACT};
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, A, n, &mirror) == PT_OK && is(o, 0.4375f, 0.875f, 0.21875f));
        p.flags = PT_SOLID_HEADLIGHT | PT_SOLID_REFLECT_SKY;
        CHECK(at(along_z, 0.0f, 0.0f, 2.0f, A, n, &glass) == PT_OK && is(o, 0.4375f, 0.875f, 0.21875f));
        // a mirror looking straight up: the camera looks down, d = (0, -1, 0), N = (0, 1, 0).  Headlight: lv = (0, 4, 0), ld = (0, 1, 0),
        // ndl = 1, r = (0, 1, 0) = v, s = 1, specular * s = 0.25.  dn = -1; m_y = -1 - 1 * (2 * -1) = 1; t = clamp(1 * 0.5 + 0.5) = 1:
        // mix = sky_bottom + (sky_top - sky_bottom) * 1 = sky_top = (0.25, 0.5, 0.75); b = A * sky_top + 0.25 = (0.375, 0.75, 0.4375)
        const pt_camera down = toward_origin(0.0f, -1.0f, 0.0f), up = toward_origin(0.0f, 1.0f, 0.0f);
        const float floor_n[3] = {0.0f, 1.0f, 0.0f}, ceiling_n[3] = {0.0f, -1.0f, 0.0f};
        CHECK(at(down, NAN, NAN, NAN, A, floor_n, &mirror) == PT_OK && is(o, 0.375f, 0.75f, 0.4375f));
        // ... and straight down: the camera looks up, d = (0, 1, 0), N = (0, -1, 0): ld = (0, -1, 0), ndl = 1, s = 1.  dn = -1;
        // m_y = 1 - (-1) * (2 * -1) = -1; t = clamp(-1 * 0.5 + 0.5) = 0: mix = sky_bottom = (0.75, 0.75, 0.75);
        // b = A * 0.75 + 0.25 = (0.625, 1, 0.4375)
        CHECK(at(up, NAN, NAN, NAN, A, ceiling_n, &mirror) == PT_OK && is(o, 0.625f, 1.0f, 0.4375f));
        // the same mirror as a lamp: + (2, 0.5, 0) = (2.625, 1.5, 0.4375), clamped
        const pt_solid_look bright_mirror = {{2.0f, 0.5f, 0.0f}, PT_SPECULAR};
        CHECK(at(up, NAN, NAN, NAN, A, ceiling_n, &bright_mirror) == PT_OK && is(o, 1.0f, 1.0f, 0.4375f));
        // refused: what pt_ctx_solid refuses, an idx outside the frame, NULL normal or rgb_out, a bad record
        const pt_solid_look odd = {{0.0f, 0.0f, 0.0f}, 3u};
        CHECK(pt_solid_pixel_host(&up, 1, 1, &p, 1, 0, 4.0f, A, n, nullptr, o) == PT_ERR_INVALID);
        CHECK(pt_solid_pixel_host(&up, 1, 1, &p, 0, 0, 4.0f, A, nullptr, nullptr, o) == PT_ERR_INVALID);
        CHECK(pt_solid_pixel_host(&up, 1, 1, &p, 0, 0, 4.0f, A, n, nullptr, nullptr) == PT_ERR_INVALID);
        CHECK(pt_solid_pixel_host(&up, 1, 1, &p, 0, 0, 4.0f, A, n, &odd, o) == PT_ERR_INVALID);
        CHECK(pt_solid_pixel_host(nullptr, 1, 1, &p, 0, 0, 4.0f, A, n, nullptr, o) == PT_ERR_INVALID);
        CHECK(pt_solid_pixel_host(&up, 0, 1, &p, 0, 0, 4.0f, A, n, nullptr, o) == PT_ERR_INVALID);
        p.shininess_log2 = 11u;
        CHECK(pt_solid_pixel_host(&up, 1, 1, &p, 0, 0, 4.0f, A, n, nullptr, o) == PT_ERR_INVALID);
    }

    // ---- the pixel over whole frames allocated to their exact size: every read stays inside (the sanitizer's part), a miss is the
    // background, every hit lies in [0, 1] or is a NaN its albedo brought
    size_t pixels = 0, misses = 0, lit = 0;
    {
        const pt_camera cam = camera(0.5f, 3.0f, 4.0f, -0.1f, -0.6f, -0.79f);
        const pt_solid_look looks[3] = {{{0.0f, 0.0f, 0.0f}, PT_DIFFUSE}, {{0.0f, 0.0f, 0.0f}, PT_SPECULAR}, {{2.0f, 2.0f, 2.0f}, PT_DIFFUSE}};
        const uint32_t sizes[][2] = {{1, 1}, {5, 1}, {31, 7}, {33, 9}};
        for (const auto &sz : sizes)
            for (uint32_t flags = 0; flags < 4u; ++flags) {
                const uint32_t W = sz[0], H = sz[1], n = W * H;
                uint32_t s = W * 977u + flags;
                pt_solid_params p = pt::kSolidDefaults;
                p.flags = flags, p.light[1] = 5.0f, p.shininess_log2 = flags * 3u, p.background[1] = 0.5f;
                std::vector<float> albedo(3 * (size_t)n), normal(3 * (size_t)n), depth(n), out(3 * (size_t)n, -1.0f);
                std::vector<int32_t> id(n);
                for (float &v : albedo) v = unit(s);
                for (float &v : normal) v = unit(s) - 0.5f;
                for (uint32_t i = 0; i < n; ++i) id[i] = (int32_t)((lcg(s) >> 16) % 6u) - 1, depth[i] = 1.0f + 12.0f * unit(s);
                for (uint32_t i = 0; i < n; ++i) {
                    const pt_solid_look *look = (uint32_t)id[i] < 3u ? &looks[id[i]] : nullptr;
                    CHECK(pt_solid_pixel_host(&cam, W, H, &p, i, id[i], depth[i], flags & 1u ? &albedo[3 * (size_t)i] : nullptr, &normal[3 * (size_t)i],
                                              look, &out[3 * (size_t)i]) == PT_OK);
                    const float *o = &out[3 * (size_t)i];
                    if (id[i] < 0) CHECK(is(o, p.background[0], p.background[1], p.background[2]));
                    else CHECK(o[0] >= 0.0f && o[0] <= 1.0f && o[1] >= 0.0f && o[1] <= 1.0f && o[2] >= 0.0f && o[2] <= 1.0f);
                    ++pixels;
                    misses += id[i] < 0;
                    lit += id[i] >= 0 && o[0] > p.ambient;
                }
            }
    }
    CHECK(misses > 0 && lit > 0);
    printf("solid_check: ok (%zu pixels: %zu missed, %zu lit)\n", pixels, misses, lit);
    return 0;
}
