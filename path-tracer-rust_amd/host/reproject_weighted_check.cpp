// reproject_weighted_check — pt_ctx_reproject_var_weighted's and pt_ctx_spp_plane's host side under a sanitizer, as a program of
// its own (make reproject-weighted-check builds it with -fsanitize=address,undefined and runs it; no device, no Python).  It
// drives the refusals of both calls in the header's order, and runs the very pixel the weighted kernels compile
// (csrc/pt_reproject.h: reproject_var_pixel<MOVED, true>, then reproject_var_short_pixel<Src, true>) over host frames, a plane of
// counts and a motion table allocated to their exact size, so that the sanitizer bounds every tap, every window read and every
// count read.  On the way it checks the contract's consequence - a constant plane gives the uniform call's bits - and what a
// pixel without samples ends as: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_masked.h"
#include "../csrc/pt_reproject.h"

struct HostSrc {
    const float *s, *z;
    const int32_t *id;
    const uint32_t *c;
    int32_t W;
    void operator()(int32_t qx, int32_t qr, float &so, int32_t &ido, float &zo) const {
        const size_t q = (size_t)qr * (size_t)W + (size_t)qx;
        so = s[q];
        ido = id[q];
        zo = z[q];
    }
    uint32_t count(int32_t qx, int32_t qr) const { return c[(size_t)qr * (size_t)W + (size_t)qx]; }
};

static bool same_bits(const void *a, const void *b, size_t bytes) { return memcmp(a, b, bytes) == 0; }

int main() {
    const pt_camera cam = camera(0.0f, -0.2f, 7.8f, 0.0f, -0.06f, -1.0f);
    const pt_camera near_cam = camera(0.3f, -0.2f, 7.7f, -0.04f, -0.06f, -1.0f);
    const pt_camera aside = camera(4.0f, -0.2f, 3.0f, -1.0f, -0.06f, -0.2f);
    const pt_object_motion I = {{0.0f, 0.0f, 0.0f}, 1.0f};

    // ---- the refusals: pt_ctx_reproject_var_moved's in its order, whatever d_spp is; then pt_ctx_spp_plane's
    {
        float buf[4];
        int32_t ibuf[4];
        uint32_t ubuf[4];
        const float *F = buf;
        const int32_t *Ii = ibuf;
        const void *ctx = buf;  // never dereferenced
        pt::ReprojectCall rc;
        pt::ReprojectVarFrame &v = rc.v;
        pt::ReprojectWeights &wts = rc.wts;
        int &how = rc.how;
        const pt_object_motion bad[2] = {I, {{0.0f, INFINITY, 0.0f}, -2.0f}}, fine[2] = {I, {{0.5f, 0.0f, 0.0f}, 1.0f}};
        pt_reproject_var_params p = {};
        auto call = [&](const void *cx, uint32_t w, const pt_reproject_var_params *pp, const uint32_t *spp, float *err,
                        const pt_object_motion *m, uint32_t n) {
            pt::ReprojectArgs a{};
            a.ctx = cx, a.var = true, a.width = w, a.height = 2, a.var_params = pp, a.cam = &cam, a.hist_cam = &near_cam;
            a.color = F, a.depth = F, a.object_id = Ii, a.spp = spp;
            a.hist_color = F, a.hist_len = F, a.hist_moments = F, a.hist_depth = F, a.hist_object_id = Ii;
            a.out_color = buf, a.out_len = buf, a.out_moments = buf, a.error = err, a.motion = m, a.n_motion = n;
            return pt::host::check_reproject(a, rc);
        };
        for (const uint32_t *spp : {(const uint32_t *)nullptr, (const uint32_t *)ubuf}) {
            p = {};
            p.max_history = -1.0f;
            CHECK(refused(call(nullptr, 0, &p, spp, nullptr, bad, 2), "max_history"));
            p = {};
            p.radius = 4u;
            CHECK(refused(call(nullptr, 0, &p, spp, nullptr, bad, 2), "radius"));
            CHECK(refused(call(nullptr, 0, nullptr, spp, nullptr, bad, 2), "width and height"));
            CHECK(refused(call(nullptr, 2, nullptr, spp, nullptr, bad, 2), "d_error is NULL"));
            CHECK(refused(call(nullptr, 2, nullptr, spp, buf, bad, 2), "ctx"));
            CHECK(refused(call(ctx, 2, nullptr, spp, buf, nullptr, (1u << 20) + 1u), "2^20"));
            CHECK(refused(call(ctx, 2, nullptr, spp, buf, nullptr, 2), "motion is NULL"));
            CHECK(refused(call(ctx, 2, nullptr, spp, buf, bad, 2), "finite scale"));
            CHECK(call(ctx, 2, nullptr, spp, buf, nullptr, 0) == PT_OK && how == pt::host::kMotionPlain);
            CHECK(wts.spp == spp && wts.min_frames == (float)pt::kReprojectVarMinFrames && v.f.wt == 1.0f);
            p = {};
            p.weight = 4u, p.min_frames = 3u;
            CHECK(call(ctx, 2, &p, spp, buf, fine, 2) == PT_OK && how == pt::host::kMotionTable);
            CHECK(wts.spp == spp && wts.min_frames == 3.0f && v.f.wt == 4.0f && v.long_len == 12.0f);
        }
        using pt::host::check_spp_plane;
        CHECK(refused(check_spp_plane(nullptr, 0, 1u << 20, nullptr), "must be positive"));
        CHECK(refused(check_spp_plane(nullptr, 1u << 20, 0, nullptr), "must be positive"));
        CHECK(refused(check_spp_plane(nullptr, 1u << 14, (1u << 14) + 1u, nullptr), "2^28"));
        CHECK(refused(check_spp_plane(nullptr, 1u << 14, 1u << 14, nullptr), "d_spp"));
        CHECK(refused(check_spp_plane(nullptr, 2, 2, ubuf), "ctx"));
        CHECK(check_spp_plane(ctx, 1u << 14, 1u << 14, ubuf) == PT_OK);
        CHECK(pt::spp_plane_value(0u, 8u, 32u) == 8u && pt::spp_plane_value(1u, 8u, 32u) == 32u && pt::spp_plane_value(255u, 8u, 0u) == 0u);
    }

    // ---- the weighted pixel over host frames of exactly width * height, a plane of exactly as many counts and a table of two
    size_t pixels = 0, empty_px = 0, empty_kept = 0, short_px = 0, moved_px = 0;
    const uint32_t frames[][2] = {{1, 1}, {7, 5}, {257, 3}, {33, 25}};
    const uint32_t counts[] = {0u, 1u, 2u, 4u, 8u, 16u, 100u};
    for (const auto &sz : frames) {
        const uint32_t w = sz[0], h = sz[1], n = w * h;
        for (const pt_camera *hc : {&cam, &near_cam, &aside}) {
            for (int form = 0; form < 4; ++form) {  // bit 0: normals; bit 1: a motion table
                Frames fr = make_frames(n, w * 131u + h, true);
                Frames un = fr;  // the uniform call's outputs on the same inputs
                std::vector<pt_object_motion> table = {I, {{0.02f, -0.01f, 0.03f}, 0.98f}};
                const pt::ReprojectMotion m = {table.data(), (uint32_t)table.size()};
                const pt_reproject_var_params p = {4, 64.0f, 0.05f, 0.5f, 2u, 2u, 0};
                std::vector<uint32_t> plane(n);
                uint32_t seed = n + (uint32_t)form;
                pt::ReprojectCall call;
                pt::ReprojectArgs a = frames_args(fr, w, h, &cam, hc, true, form & 1);
                a.var_params = &p, a.spp = plane.data(), a.motion = form & 2 ? table.data() : nullptr, a.n_motion = form & 2 ? m.n : 0u;
                CHECK(pt::host::check_reproject(a, call) == PT_OK);
                pt::ReprojectVarFrame &v = call.v;
                pt::ReprojectVarFrame vu;
                const pt::ReprojectWeights &wts = call.wts;
                const int how = call.how;
                CHECK(how == (form & 2 ? pt::host::kMotionTable : pt::host::kMotionPlain) && wts.spp == plane.data());
                v.s_plane = fr.splane.data();
                vu = v;
                vu.f.out_color = un.out.data(), vu.f.out_len = un.len.data();
                vu.out_moments = reinterpret_cast<pt::ReprojectMom *>(un.mom.data());
                vu.error = un.err.data(), vu.s_plane = un.splane.data();
                auto run = [&](bool weighted) {
                    const pt::ReprojectVarFrame &x = weighted ? v : vu;
                    Frames &o = weighted ? fr : un;
                    for (uint32_t i = 0; i < n; ++i) {
                        if (weighted && (form & 2))
                            pt::reproject_var_pixel<true, true>(x, i, &m, &wts);
                        else if (weighted)
                            pt::reproject_var_pixel<false, true>(x, i, nullptr, &wts);
                        else if (form & 2)
                            pt::reproject_var_pixel<true>(x, i, &m);
                        else
                            pt::reproject_var_pixel(x, i);
                    }
                    const HostSrc src = {x.s_plane, x.f.depth, x.f.object_id, plane.data(), (int32_t)w};
                    for (uint32_t i = 0; i < n; ++i) {
                        if (o.err[i] != pt::kReprojectVarShort) continue;
                        o.err[i] = weighted ? pt::reproject_var_short_pixel<HostSrc, true>(x, src, i) : pt::reproject_var_short_pixel(x, src, i);
                    }
                };
                // the consequence: the constant plane 4 is the uniform call with weight 4, on all four outputs
                std::fill(plane.begin(), plane.end(), 4u);
                run(true);
                run(false);
                CHECK(same_bits(fr.out.data(), un.out.data(), 12 * (size_t)n) && same_bits(fr.len.data(), un.len.data(), 4 * (size_t)n));
                CHECK(same_bits(fr.mom.data(), un.mom.data(), 8 * (size_t)n) && same_bits(fr.err.data(), un.err.data(), 4 * (size_t)n));
                CHECK(same_bits(fr.splane.data(), un.splane.data(), 4 * (size_t)n));
                // a mixed plane, with a NaN colour under every pixel without samples
                for (uint32_t i = 0; i < n; ++i) {
                    plane[i] = counts[lcg(seed) % 7u];
                    if (plane[i] == 0u) fr.color[3 * (size_t)i + (lcg(seed) % 3u)] = NAN;
                }
                fr.err.assign(n, -2.0f);
                run(true);
                for (uint32_t i = 0; i < n; ++i) {
                    const float wp = (float)plane[i];
                    ++pixels;
                    if (form & 2 && fr.id[i] == 1) ++moved_px;
                    CHECK(fr.err[i] != pt::kReprojectVarShort && !(fr.err[i] < 0.0f));
                    if (plane[i] == 0u) {
                        ++empty_px;
                        if (fr.len[i] > 0.0f) {  // the history as it is: no NaN came in, and the length is at most the cap
                            ++empty_kept;
                            CHECK(fr.out[3 * (size_t)i] == fr.out[3 * (size_t)i] && fr.out[3 * (size_t)i + 1] == fr.out[3 * (size_t)i + 1] &&
                                  fr.out[3 * (size_t)i + 2] == fr.out[3 * (size_t)i + 2] && fr.len[i] <= 64.0f);
                            CHECK(fr.len[i] >= 8.0f ? fr.err[i] <= 12.0f : fr.err[i] == INFINITY);
                        } else {  // step 1: the colour as stored, no samples, no estimate
                            CHECK(same_bits(&fr.out[3 * (size_t)i], &fr.color[3 * (size_t)i], 12) && fr.len[i] == 0.0f && fr.err[i] == INFINITY);
                        }
                    } else {
                        CHECK(fr.len[i] >= wp && (fr.len[i] <= 64.0f || fr.len[i] == wp));
                        if (fr.len[i] < 2.0f * wp) ++short_px;
                    }
                }
            }
        }
    }
    CHECK(empty_px > pixels / 10 && empty_kept > 0 && empty_kept < empty_px && short_px > 0 && moved_px > 0);
    printf("reproject_weighted_check: ok (%zu pixels, %zu without samples, %zu of them kept their history, %zu short, %zu on a moved object)\n",
           pixels, empty_px, empty_kept, short_px, moved_px);
    return 0;
}
