// overlay_check — pt_ctx_overlay's host side under a sanitizer, as a program of its own (make overlay-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the validator's refusals in the header's order,
// pt_overlay_defaults against its rule, and pt_overlay_pixel_host - the pixel the kernel compiles - over whole frames allocated to
// their exact size, with the window of step 6 taken from the definition: a failed check or a sanitizer report ends it with a
// non-zero status.
#include "check_common.h"
#include "../csrc/pt_overlay.h"

static pt_overlay_params with_grid(uint32_t flags) {
    pt_overlay_params p;
    memset(&p, 0, sizeof p);
    p.flags = flags;
    p.grid_spacing = 0.5f, p.grid_half_width = 0.04f, p.grid_extent = 6.0f;
    return p;
}

int main() {
    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        float buf[4];
        int32_t ibuf[4];
        const float *F = buf;
        const int32_t *I = ibuf;
        const void *ctx = buf;  // never dereferenced
        pt::OverlayFrame f;
        const pt_camera cam = camera(0.5f, 3.0f, 4.0f, -0.1f, -0.6f, -0.79f);
        pt_camera far_cam = cam;
        far_cam.position[0] = INFINITY;
        auto check = [&](const pt_overlay_params *p, uint32_t w, uint32_t h, const pt_camera *c, const float *rgb, const int32_t *id,
                         const float *z, float *out, const void *cx) { return pt::host::check_overlay(cx, w, h, p, c, rgb, id, z, out, f); };
        pt_overlay_params p = with_grid(4u);
        p.n_selected = 17u, p.radius = 9u, p.outline_alpha = 2.0f, p.grid_spacing = -1.0f;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "flags"));
        p.flags = 3u;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "n_selected"));
        p.n_selected = 2u, p.selected[1] = -1;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "negative"));
        p.selected[1] = 5, p.selected[2] = -1;  // beyond n_selected: not listed, not looked at
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "radius"));
        p.radius = 8u, p.sky_bottom[2] = NAN;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "colour"));
        p.sky_bottom[2] = 0.0f;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "alpha"));
        p.outline_alpha = 1.0f, p.fill_alpha = NAN;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "alpha"));
        p.fill_alpha = 0.5f;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "grid"));
        p.grid_spacing = 0.5f, p.grid_y = NAN;
        CHECK(refused(check(&p, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "grid_y"));
        p.grid_y = 0.0f;
        CHECK(refused(check(&p, 0, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "must be positive"));
        CHECK(refused(check(&p, 1u << 15, 1u << 15, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "2^28"));
        CHECK(refused(check(&p, 2, 2, nullptr, nullptr, nullptr, nullptr, buf, nullptr), "d_rgb"));
        CHECK(refused(check(&p, 2, 2, nullptr, F, nullptr, nullptr, nullptr, nullptr), "d_out"));
        CHECK(refused(check(&p, 2, 2, nullptr, F, nullptr, nullptr, buf, nullptr), "d_object_id"));
        CHECK(refused(check(&p, 2, 2, nullptr, F, I, nullptr, buf, nullptr), "d_depth"));
        CHECK(refused(check(&p, 2, 2, nullptr, F, I, F, buf, nullptr), "cam is NULL"));
        CHECK(refused(check(&p, 2, 2, &far_cam, F, I, F, buf, nullptr), "lens centre"));
        CHECK(refused(check(&p, 2, 2, &cam, F, I, F, buf, nullptr), "ctx"));
        CHECK(refused(check(nullptr, 1u << 14, 1u << 14, nullptr, F, nullptr, nullptr, buf, nullptr), "ctx"));
        // accepted: the defaults are filled in, and a plane the call does not need is not handed on
        CHECK(check(nullptr, 2, 2, &far_cam, F, I, F, buf, ctx) == PT_OK);
        CHECK(f.p.radius == pt::kOverlayRadius && f.p.outline_alpha == 1.0f && f.p.grid_alpha == 1.0f && f.p.fill_alpha == 0.0f);
        CHECK(!f.object_id && !f.depth && f.rgb == F && f.out == buf && f.width == 2u && f.height == 2u);
        CHECK(check(&p, 2, 2, &cam, F, I, F, buf, ctx) == PT_OK && f.p.radius == 8u && f.object_id == I && f.depth == F);
        const pt_overlay_params grid_only = with_grid(PT_OVERLAY_GRID);
        CHECK(check(&grid_only, 2, 2, &cam, F, I, F, buf, ctx) == PT_OK && !f.object_id && f.depth == F && f.L.y == cam.position[1] + cam.direction[1] * cam.focal_length);
    }

    // ---- pt_overlay_defaults
    {
        pt_overlay_params d;
        CHECK(pt_overlay_defaults(nullptr, nullptr) == PT_ERR_INVALID);
        CHECK(pt_overlay_defaults(nullptr, &d) == PT_OK);
        CHECK(d.flags == 0u && d.n_selected == 0u && d.radius == 2u && d.outline_color[1] == 1.0f && d.outline_alpha == 1.0f && d.fill_alpha == 0.0f);
        CHECK(d.grid_y == 0.0f && d.grid_spacing == 1.0f && d.grid_half_width == 0.01f && d.grid_extent == 5.0f && d.grid_color[0] == 0.5f);
        const float dist[] = {0.0f, 1.0f, 5.0f, 20.0f, 50.0f, 250.0f, 1000.0f, 5000.0f};
        for (float r : dist) {
            const pt_camera cam = camera(0.6f * r, 0.0f, -0.8f * r, 0.0f, 0.0f, 1.0f);
            CHECK(pt_overlay_defaults(&cam, &d) == PT_OK);
            const double x = cam.position[0], z = cam.position[2], zoom = sqrt(x * x + z * z) / 5.0;
            const double spacing = pow(10.0, floor(log10(zoom * 1.2 + 1.0)));
            CHECK(d.grid_spacing == (float)spacing && d.grid_half_width == (float)(0.01 * zoom) && d.grid_extent == (float)(5.0 * spacing));
            d.flags = PT_OVERLAY_SKY | PT_OVERLAY_GRID;
            pt_overlay_params filled;
            CHECK(r == 0.0f || pt::host::check_overlay_params(&d, filled) == PT_OK);  // (at the origin the half width is 0)
        }
        pt_camera bad = camera(1.0f, 2.0f, 3.0f, 0.0f, 0.0f, 1.0f);
        bad.position[2] = NAN;
        CHECK(pt_overlay_defaults(&bad, &d) == PT_ERR_INVALID);
    }

    // ---- the pixel over whole frames: planes of exactly the frame's size, the window from the definition
    size_t pixels = 0, sky = 0, lines = 0, filled = 0, outlined_n = 0, same = 0;
    const uint32_t sizes[][2] = {{1, 1}, {31, 7}, {33, 9}, {48, 32}};
    const pt_camera cams[] = {camera(0.5f, 3.0f, 4.0f, -0.1f, -0.6f, -0.79f), camera(0.5f, -3.0f, 4.0f, 0.0f, -0.2f, -0.97f),
                              camera(1.0f, 0.25f, 6.0f, -0.15f, 0.0f, -0.98f)};
    for (const auto &sz : sizes) {
        const uint32_t W = sz[0], H = sz[1], n = W * H;
        for (const pt_camera &cam : cams) {
            for (uint32_t flags = 0; flags < 4u; ++flags) {
                uint32_t s = W * 131u + flags;
                std::vector<float> rgb(3 * (size_t)n), depth(n), out(3 * (size_t)n, -1.0f);
                std::vector<int32_t> id(n);
                for (float &v : rgb) v = unit(s);
                for (uint32_t i = 0; i < n; ++i) {
                    id[i] = (int32_t)((lcg(s) >> 16) % 5u) - 1;
                    depth[i] = id[i] < 0 ? INFINITY : 1.0f + 12.0f * unit(s);
                }
                rgb[0] = -0.0f, rgb[n > 1 ? 4 : 1] = NAN;
                pt_overlay_params p = with_grid(flags);
                p.n_selected = 2u, p.selected[0] = 2, p.selected[1] = 70000, p.radius = 1u + (W + flags) % 8u;
                p.outline_color[1] = 1.0f, p.fill_color[0] = 1.0f, p.fill_alpha = flags & 1u ? 0.25f : 0.0f;
                p.sky_top[2] = 0.75f, p.sky_bottom[0] = 0.75f, p.grid_color[1] = 0.5f, p.grid_alpha = 0.5f;
                const int32_t R = (int32_t)p.radius;
                for (uint32_t i = 0; i < n; ++i) {
                    const int32_t x = (int32_t)(i % W), r = (int32_t)(i / W);
                    const bool m = id[i] == 2;
                    bool near = false;
                    for (int32_t j = -R; j <= R; ++j)
                        for (int32_t k = -R; k <= R; ++k) {
                            const int32_t qx = x + k, qr = r + j;
                            if (qx >= 0 && qx < (int32_t)W && qr >= 0 && qr < (int32_t)H) near = near || id[(size_t)qr * W + qx] == 2;
                        }
                    CHECK(pt_overlay_pixel_host(&cam, W, H, &p, i, id[i], depth[i], m, near && !m, &rgb[3 * (size_t)i], &out[3 * (size_t)i]) == PT_OK);
                    const bool untouched = memcmp(&out[3 * (size_t)i], &rgb[3 * (size_t)i], 12) == 0;
                    const bool is_sky = (flags & PT_OVERLAY_SKY) && id[i] < 0;
                    if (!is_sky && !(flags & PT_OVERLAY_GRID) && !(m && p.fill_alpha != 0.0f) && !(near && !m)) CHECK(untouched);
                    if (near && !m && !is_sky && !(flags & PT_OVERLAY_GRID) && i != 0 && i != 1)
                        CHECK(out[3 * (size_t)i] == 0.0f && out[3 * (size_t)i + 1] == 1.0f && out[3 * (size_t)i + 2] == 0.0f);  // alpha 1: the colour itself
                    ++pixels;
                    sky += is_sky;
                    filled += m && p.fill_alpha != 0.0f;
                    outlined_n += near && !m;
                    same += untouched;
                    lines += (flags == PT_OVERLAY_GRID) && !untouched && !m && !(near && !m);
                }
            }
        }
    }
    CHECK(sky > 0 && lines > 0 && filled > 0 && outlined_n > 0 && same > 0);
    // in place: rgb_out may be rgb_in
    {
        float v[3] = {0.25f, 0.5f, 0.75f};
        pt_overlay_params p = with_grid(0u);
        p.fill_alpha = 1.0f, p.fill_color[0] = 1.0f;
        CHECK(pt_overlay_pixel_host(nullptr, 4, 4, &p, 3, 0, 1.0f, 1, 0, v, v) == PT_OK && v[0] == 1.0f && v[1] == 0.0f && v[2] == 0.0f);
        CHECK(pt_overlay_pixel_host(nullptr, 4, 4, &p, 16, 0, 1.0f, 1, 0, v, v) == PT_ERR_INVALID);
    }
    printf("overlay_check: ok (%zu pixels: %zu sky, %zu on a grid line, %zu filled, %zu outlined, %zu untouched)\n", pixels, sky, lines,
           filled, outlined_n, same);
    return 0;
}
