// reproject_check — pt_ctx_reproject's host side under a sanitizer, as a program of its own (make reproject-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives pt_reproject_project_host and the refusals over
// edge inputs, and runs the pixel the kernel compiles (csrc/pt_reproject.h: reproject_pixel) over host frames allocated to their
// exact size, so that the sanitizer bounds every tap of the gather: a failed check or a sanitizer report ends it with a non-zero
// status.
#include "check_common.h"
#include "../csrc/pt_reproject.h"

int main() {
    const pt_camera cam = camera(0.0f, -0.2f, 7.8f, 0.0f, -0.06f, -1.0f);
    const pt_camera near_cam = camera(0.3f, -0.2f, 7.7f, -0.04f, -0.06f, -1.0f);
    const pt_camera back = camera(0.0f, -0.2f, 7.8f, 0.0f, 0.06f, 1.0f);
    const pt_camera aside = camera(4.0f, -0.2f, 3.0f, -1.0f, -0.06f, -0.2f);  // part of the frame behind its lens, part outside
    const pt_camera down = camera(0.5f, 6.0f, -0.25f, 0.0f, -1.0f, 0.0f);
    const pt_camera zero = camera(0.0f, -0.2f, 7.8f, 0.0f, 0.0f, 0.0f);
    float px = -7.0f, pr = -7.0f, z = -7.0f;

    // ---- pt_reproject_project_host
    CHECK(pt_reproject_project_host(nullptr, &cam, 4, 4, 0, 1.0f, &px, &pr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, nullptr, 4, 4, 0, 1.0f, &px, &pr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 4, 4, 0, 1.0f, nullptr, &pr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 4, 4, 0, 1.0f, &px, nullptr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 4, 4, 0, 1.0f, &px, &pr, nullptr) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 0, 4, 0, 1.0f, &px, &pr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 4, 0, 0, 1.0f, &px, &pr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 4, 4, 16, 1.0f, &px, &pr, &z) == PT_ERR_INVALID);
    CHECK(pt_reproject_project_host(&cam, &cam, 1u << 15, 1u << 15, 0, 1.0f, &px, &pr, &z) == PT_ERR_INVALID);
    CHECK(px == -7.0f && pr == -7.0f && z == -7.0f);
    const uint32_t sizes[][2] = {{1, 1}, {7, 5}, {450, 300}, {1024, 768}, {1u << 14, 1u << 14}};
    for (const auto &s : sizes) {
        const uint32_t w = s[0], h = s[1], last = w * h - 1u;
        for (uint32_t idx : {0u, w - 1u, last - (w - 1u), last, (h / 2u) * w + w / 2u}) {
            // a point behind the history lens, a zero direction on either side, depths that are not distances
            CHECK(pt_reproject_project_host(&cam, &back, w, h, idx, 4.0f, &px, &pr, &z) == 1);
            CHECK(pt_reproject_project_host(&cam, &zero, w, h, idx, 4.0f, &px, &pr, &z) == 1);
            CHECK(pt_reproject_project_host(&zero, &cam, w, h, idx, 4.0f, &px, &pr, &z) == 1);
            CHECK(pt_reproject_project_host(&cam, &near_cam, w, h, idx, NAN, &px, &pr, &z) == 1);
            CHECK(pt_reproject_project_host(&cam, &near_cam, w, h, idx, INFINITY, &px, &pr, &z) == 1);
            CHECK(pt_reproject_project_host(&cam, &near_cam, w, h, idx, -INFINITY, &px, &pr, &z) == 1);
            CHECK(px == -7.0f && pr == -7.0f && z == -7.0f);  // "no position" writes nothing
            for (float depth : {0.125f, 1.0f, 8.0f, 64.0f, 0.0f, -1.0f, 1e-30f, 3e38f}) {
                for (const pt_camera *hc : {&cam, &near_cam, &aside, &down}) {
                    float x = -7.0f, r = -7.0f, d = -7.0f;
                    const int rc = pt_reproject_project_host(&cam, hc, w, h, idx, depth, &x, &r, &d);
                    CHECK(rc == PT_OK || rc == 1);
                    if (rc == PT_OK) CHECK(x > -1.0f && x < (float)w && r > -1.0f && r < (float)h && d >= 0.0f);
                }
            }
            // the same camera sees the pixel where it is
            CHECK(pt_reproject_project_host(&cam, &cam, w, h, idx, 8.0f, &px, &pr, &z) == PT_OK);
            CHECK(fabsf(px - (float)(idx % w)) < 0.25f && fabsf(pr - (float)(idx / w)) < 0.25f && fabsf(z - 8.0f) < 1e-4f);
            px = pr = z = -7.0f;
        }
    }

    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        float buf[4];
        int32_t ibuf[4];
        const float *F = buf;
        const int32_t *I = ibuf;
        pt::ReprojectCall call;
        pt::ReprojectFrame &f = call.v.f;
        const void *ctx = buf;  // never dereferenced
        // col: the frame's own planes; hc / hl: history colour (with depth and id) / length; out: colour and length
        auto check = [&](const pt_reproject_params *p, uint32_t w, uint32_t h, const pt_camera *c, const float *col, const float *hc,
                         const float *hl, const pt_camera *hcam, float *out, const void *cx) {
            pt::ReprojectArgs a{};
            a.ctx = cx, a.width = w, a.height = h, a.params = p, a.cam = c, a.hist_cam = hcam;
            a.color = col, a.depth = col ? F : nullptr, a.object_id = col ? I : nullptr;
            a.hist_color = hc, a.hist_len = hl, a.hist_depth = hc, a.hist_object_id = hc ? I : nullptr;
            a.out_color = out, a.out_len = out;
            return pt::host::check_reproject(a, call);
        };
        const pt_reproject_params bad_mh = {0, -1.0f, NAN, 2.0f, 1}, bad_dt = {0, 1.0f, INFINITY, 2.0f, 1}, bad_nm = {0, 1.0f, 1.0f, NAN, 1},
                                  bad_nm2 = {0, 1.0f, 1.0f, -1.5f, 1}, bad_flags = {0, 1.0f, 1.0f, -1.0f, 1}, fine = {3, 8.0f, 0.1f, 1.0f, 0};
        CHECK(refused(check(&bad_mh, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "max_history or depth_tol"));
        CHECK(refused(check(&bad_dt, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "max_history or depth_tol"));
        CHECK(refused(check(&bad_nm, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "normal_min"));
        CHECK(refused(check(&bad_nm2, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "normal_min"));
        CHECK(refused(check(&bad_flags, 0, 0, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "flags"));
        CHECK(refused(check(&fine, 0, 3, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "width and height"));
        CHECK(refused(check(&fine, 1u << 15, 1u << 15, nullptr, nullptr, F, nullptr, nullptr, nullptr, nullptr), "2^28"));
        CHECK(refused(check(nullptr, 2, 2, nullptr, F, F, nullptr, nullptr, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, nullptr, F, nullptr, nullptr, buf, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, nullptr, nullptr, nullptr, nullptr), "is NULL"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, nullptr, nullptr, buf, nullptr), "history"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, nullptr, F, nullptr, buf, nullptr), "history"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, F, nullptr, buf, nullptr), "hist_cam"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, F, F, &cam, buf, nullptr), "ctx"));
        CHECK(refused(check(nullptr, 2, 2, &cam, F, nullptr, nullptr, nullptr, buf, nullptr), "ctx"));
        // accepted: the defaults are filled in, the first frame carries no history
        CHECK(check(nullptr, 2, 2, &cam, F, F, F, &near_cam, buf, ctx) == PT_OK);
        CHECK(f.wt == 1.0f && f.max_history == pt::kReprojectMaxHistory && f.depth_tol == pt::kReprojectDepthTol &&
              f.normal_min == pt::kReprojectNormalMin && f.view.same == 0u && f.hist_color == F);
        CHECK(check(&fine, 2, 2, &cam, F, F, F, &cam, buf, ctx) == PT_OK);
        CHECK(f.wt == 3.0f && f.max_history == 8.0f && f.depth_tol == 0.1f && f.normal_min == 1.0f && f.view.same == 1u);
        CHECK(check(&fine, 2, 2, &cam, F, nullptr, nullptr, nullptr, buf, ctx) == PT_OK && f.hist_color == nullptr);
    }

    // ---- the pixel over host frames of exactly width * height: every tap inside them, or the sanitizer says so
    size_t pixels = 0, blended = 0;
    const uint32_t frames[][2] = {{1, 1}, {2, 1}, {1, 2}, {7, 5}, {257, 3}, {33, 25}};
    for (const auto &s : frames) {
        const uint32_t w = s[0], h = s[1], n = w * h;
        for (const pt_camera *hc : {&cam, &near_cam, &aside, &back, &zero}) {
            for (int with_normals = 0; with_normals < 2; ++with_normals) {
                Frames fr = make_frames(n, w * 131u + h, false);
                const pt_reproject_params p = {4, 64.0f, 0.05f, 0.5f, 0};
                pt::ReprojectCall call;
                pt::ReprojectArgs a = frames_args(fr, w, h, &cam, hc, false, with_normals);
                a.params = &p;
                CHECK(pt::host::check_reproject(a, call) == PT_OK);
                const pt::ReprojectFrame &f = call.v.f;
                for (uint32_t i = 0; i < n; ++i) {
                    pt::reproject_pixel(f, i, &fr.out[3 * (size_t)i], &fr.len[i]);
                    CHECK(fr.len[i] >= 4.0f && fr.len[i] <= 64.0f);
                    for (int c = 0; c < 3; ++c) CHECK(fr.out[3 * (size_t)i + c] >= -1e-6f && fr.out[3 * (size_t)i + c] <= 1.0f + 1e-6f);
                    if (fr.len[i] > 4.0f) {
                        CHECK(fr.id[i] >= 0);
                        ++blended;
                    } else {
                        for (int c = 0; c < 3; ++c) CHECK(fr.out[3 * (size_t)i + c] == fr.color[3 * (size_t)i + c]);
                    }
                    ++pixels;
                }
                if (hc == &back || hc == &zero)
                    for (uint32_t i = 0; i < n; ++i) CHECK(fr.len[i] == 4.0f);
            }
        }
        // the first frame, and in place
        Frames fr = make_frames(n, 7u, false);
        pt::ReprojectCall call;
        pt::ReprojectArgs a{};
        a.ctx = &fr, a.width = w, a.height = h, a.cam = &cam, a.color = fr.color.data(), a.depth = fr.depth.data();
        a.object_id = fr.id.data(), a.out_color = fr.color.data(), a.out_len = fr.len.data();
        CHECK(pt::host::check_reproject(a, call) == PT_OK);
        const pt::ReprojectFrame &f = call.v.f;
        const std::vector<float> before = fr.color;
        for (uint32_t i = 0; i < n; ++i) pt::reproject_pixel(f, i, &fr.color[3 * (size_t)i], &fr.len[i]);
        CHECK(fr.color == before);
        for (uint32_t i = 0; i < n; ++i) CHECK(fr.len[i] == 1.0f);
    }
    CHECK(blended > pixels / 50);
    printf("reproject_check: ok (%zu pixels, %zu blended)\n", pixels, blended);
    return 0;
}
