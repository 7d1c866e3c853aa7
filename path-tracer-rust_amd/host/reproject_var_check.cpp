// reproject_var_check — pt_ctx_reproject_var's host side under a sanitizer, as a program of its own (make reproject-var-check
// builds it with -fsanitize=address,undefined and runs it; no device, no Python).  It drives the refusals in the header's order,
// and runs the whole pixel the kernels compile (csrc/pt_reproject.h: reproject_var_pixel - projection and gather with moments -
// then reproject_var_short_pixel - the spatial window) over host frames allocated to their exact size, so that the sanitizer
// bounds every tap and every window read: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_reproject.h"

// the frame as kernel B's window sees it: global planes, every read inside them or the sanitizer says so
struct HostSrc {
    const float *s, *z;
    const int32_t *id;
    int32_t W;
    void operator()(int32_t qx, int32_t qr, float &so, int32_t &ido, float &zo) const {
        const size_t q = (size_t)qr * (size_t)W + (size_t)qx;
        so = s[q];
        ido = id[q];
        zo = z[q];
    }
};

// both kernels' work over the whole frame, in their order: every pixel of A before any of B.  Returns the number of short pixels.
static size_t run(const pt::ReprojectVarFrame &v) {
    const uint32_t n = v.f.width * v.f.height;
    for (uint32_t i = 0; i < n; ++i) pt::reproject_var_pixel(v, i);
    const HostSrc src = {v.s_plane, v.f.depth, v.f.object_id, (int32_t)v.f.width};
    size_t shorts = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (v.error[i] == pt::kReprojectVarShort) {
            v.error[i] = pt::reproject_var_short_pixel(v, src, i);
            ++shorts;
        }
    return shorts;
}

int main() {
    const pt_camera cam = camera(0.0f, -0.2f, 7.8f, 0.0f, -0.06f, -1.0f);
    const pt_camera near_cam = camera(0.3f, -0.2f, 7.7f, -0.04f, -0.06f, -1.0f);
    const pt_camera back = camera(0.0f, -0.2f, 7.8f, 0.0f, 0.06f, 1.0f);
    const pt_camera aside = camera(4.0f, -0.2f, 3.0f, -1.0f, -0.06f, -0.2f);  // part of the frame behind its lens, part outside
    const pt_camera zero = camera(0.0f, -0.2f, 7.8f, 0.0f, 0.0f, 0.0f);

    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        float buf[4];
        int32_t ibuf[4];
        const float *F = buf;
        const int32_t *I = ibuf;
        pt::ReprojectCall call;
        pt::ReprojectVarFrame &v = call.v;
        const void *ctx = buf;  // never dereferenced
        // col: the frame's own planes; hc / hl / hm: history colour (with depth and id) / length / moments; out: colour and
        // length; om / er: moments and error
        auto check = [&](const pt_reproject_var_params *p, uint32_t w, uint32_t h, const pt_camera *c, const float *col, const float *hc,
                         const float *hl, const float *hm, const pt_camera *hcam, float *out, float *om, float *er, const void *cx) {
            pt::ReprojectArgs a{};
            a.ctx = cx, a.var = true, a.width = w, a.height = h, a.var_params = p, a.cam = c, a.hist_cam = hcam;
            a.color = col, a.depth = col ? F : nullptr, a.object_id = col ? I : nullptr;
            a.hist_color = hc, a.hist_len = hl, a.hist_moments = hm, a.hist_depth = hc, a.hist_object_id = hc ? I : nullptr;
            a.out_color = out, a.out_len = out, a.out_moments = om, a.error = er;
            return pt::host::check_reproject(a, call);
        };
        const pt_reproject_var_params bad_mh = {0, -1.0f, NAN, 2.0f, 0, 4, 1}, bad_dt = {0, 1.0f, INFINITY, 2.0f, 0, 4, 1},
                                      bad_nm = {0, 1.0f, 1.0f, NAN, 0, 4, 1}, bad_nm2 = {0, 1.0f, 1.0f, -1.5f, 0, 4, 1},
                                      bad_r = {0, 1.0f, 1.0f, -1.0f, 0, 4, 1}, bad_flags = {0, 1.0f, 1.0f, -1.0f, 9, 3, 1},
                                      fine = {3, 8.0f, 0.1f, 1.0f, 2, 1, 0};
        float *N = nullptr;
        CHECK(refused(check(&bad_mh, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "max_history or depth_tol"));
        CHECK(refused(check(&bad_dt, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "max_history or depth_tol"));
        CHECK(refused(check(&bad_nm, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "normal_min"));
        CHECK(refused(check(&bad_nm2, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "normal_min"));
        CHECK(refused(check(&bad_r, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "radius"));
        CHECK(refused(check(&bad_flags, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "flags"));
        CHECK(refused(check(&fine, 0, 3, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "width and height"));
        CHECK(refused(check(&fine, 1u << 15, 1u << 15, nullptr, nullptr, F, nullptr, nullptr, nullptr, N, N, N, nullptr), "2^28"));
        CHECK(refused(check(nullptr, 2, 2, nullptr, F, F, nullptr, nullptr, nullptr, buf, buf, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, nullptr, F, nullptr, nullptr, nullptr, buf, buf, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, nullptr, nullptr, nullptr, N, buf, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, nullptr, nullptr, nullptr, buf, N, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, nullptr, nullptr, nullptr, buf, buf, N, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, nullptr, nullptr, nullptr, buf, buf, buf, nullptr), "history"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, nullptr, F, nullptr, nullptr, buf, buf, buf, nullptr), "history"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, nullptr, nullptr, F, nullptr, buf, buf, buf, nullptr), "history"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, F, nullptr, nullptr, buf, buf, buf, nullptr), "history"));  // no moments
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, F, F, nullptr, buf, buf, buf, nullptr), "hist_cam"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, F, F, &cam, buf, buf, buf, nullptr), "ctx"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, nullptr, nullptr, nullptr, nullptr, buf, buf, buf, nullptr), "ctx"));
        // accepted: the defaults are filled in, the first frame carries no history
        CHECK(check(nullptr, 2, 2, &cam, F, F, F, F, &near_cam, buf, buf, buf, ctx) == PT_OK);
        CHECK(v.f.wt == 1.0f && v.f.max_history == pt::kReprojectMaxHistory && v.f.depth_tol == pt::kReprojectDepthTol &&
              v.f.normal_min == pt::kReprojectNormalMin && v.f.view.same == 0u && v.f.hist_color == F);
        CHECK(v.radius == pt::kReprojectVarRadius && v.long_len == (float)pt::kReprojectVarMinFrames && v.s_plane == nullptr);
        CHECK((const void *)v.hist_moments == (const void *)F && (void *)v.out_moments == (void *)buf && v.error == buf);
        CHECK(check(&fine, 2, 2, &cam, F, F, F, F, &cam, buf, buf, buf, ctx) == PT_OK);
        CHECK(v.f.wt == 3.0f && v.f.max_history == 8.0f && v.f.depth_tol == 0.1f && v.f.normal_min == 1.0f && v.f.view.same == 1u);
        CHECK(v.radius == 1u && v.long_len == 6.0f);
        CHECK(check(&fine, 2, 2, &cam, F, nullptr, nullptr, nullptr, nullptr, buf, buf, buf, ctx) == PT_OK && v.f.hist_color == nullptr &&
              v.hist_moments == nullptr);
    }

    // ---- the whole pixel over host frames of exactly width * height: every tap and every window read inside them
    size_t pixels = 0, blended = 0, shorts = 0, none = 0;
    const uint32_t frames[][2] = {{1, 1}, {7, 5}, {257, 3}, {33, 25}};
    for (const auto &s : frames) {
        const uint32_t w = s[0], h = s[1], n = w * h;
        for (const pt_camera *hc : {&cam, &near_cam, &aside, &back, &zero}) {
            for (uint32_t radius = 1; radius <= 3; ++radius) {
                for (int with_normals = 0; with_normals < 2; ++with_normals) {
                    Frames fr = make_frames(n, w * 131u + h, true);
                    const pt_reproject_var_params p = {4, 64.0f, 0.05f, 0.5f, with_normals ? 4u : 1u, radius, 0};
                    pt::ReprojectCall call;
                    pt::ReprojectArgs a = frames_args(fr, w, h, &cam, hc, true, with_normals);
                    a.var_params = &p;
                    CHECK(pt::host::check_reproject(a, call) == PT_OK);
                    pt::ReprojectVarFrame &v = call.v;
                    v.s_plane = fr.splane.data();
                    shorts += run(v);
                    for (uint32_t i = 0; i < n; ++i) {
                        const float sum = (fr.color[3 * (size_t)i] + fr.color[3 * (size_t)i + 1]) + fr.color[3 * (size_t)i + 2];
                        CHECK(fr.splane[i] == sum);
                        CHECK(fr.len[i] >= 4.0f && fr.len[i] <= 64.0f);
                        CHECK(fr.mom[2 * (size_t)i] >= 0.0f && fr.mom[2 * (size_t)i] <= 3.0f + 1e-5f && fr.mom[2 * (size_t)i + 1] >= 0.0f);
                        CHECK((fr.err[i] >= 0.0f && fr.err[i] <= 12.0f) || (std::isinf(fr.err[i]) && fr.err[i] > 0.0f));
                        if (std::isinf(fr.err[i])) ++none;
                        if (fr.len[i] > 4.0f) {
                            CHECK(fr.id[i] >= 0);
                            ++blended;
                        } else {
                            CHECK(fr.mom[2 * (size_t)i] == sum && fr.mom[2 * (size_t)i + 1] == sum * sum);
                            if (with_normals) CHECK(n == 1 ? std::isinf(fr.err[i]) : true);  // short, and a window of one pixel
                        }
                        ++pixels;
                    }
                    if (hc == &back || hc == &zero)
                        for (uint32_t i = 0; i < n; ++i) CHECK(fr.len[i] == 4.0f);
                }
            }
        }
        // the first frame, in place: every pixel short, the colour unchanged, the moments (s, s*s)
        Frames fr = make_frames(n, 7u, true);
        pt::ReprojectCall call;
        pt::ReprojectArgs a{};
        a.ctx = &fr, a.var = true, a.width = w, a.height = h, a.cam = &cam, a.color = fr.color.data(), a.depth = fr.depth.data();
        a.object_id = fr.id.data(), a.out_color = fr.color.data(), a.out_len = fr.len.data(), a.out_moments = fr.mom.data();
        a.error = fr.err.data();
        CHECK(pt::host::check_reproject(a, call) == PT_OK);
        pt::ReprojectVarFrame &v = call.v;
        v.s_plane = fr.splane.data();
        const std::vector<float> before = fr.color;
        CHECK(run(v) == n);
        CHECK(fr.color == before);
        for (uint32_t i = 0; i < n; ++i) {
            CHECK(fr.len[i] == 1.0f && fr.mom[2 * (size_t)i] == fr.splane[i]);
            CHECK(fr.err[i] >= 0.0f);
        }
        if (n == 1) CHECK(std::isinf(fr.err[0]));
    }
    CHECK(blended > pixels / 50 && shorts > pixels / 50 && shorts < pixels && none > 0);
    printf("reproject_var_check: ok (%zu pixels, %zu blended, %zu short, %zu without an estimate)\n", pixels, blended, shorts, none);
    return 0;
}
