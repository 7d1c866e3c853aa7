// reproject_moved_check — pt_ctx_reproject_moved's and pt_ctx_reproject_var_moved's host side under a sanitizer, as a program of
// its own (make reproject-moved-check builds it with -fsanitize=address,undefined and runs it; no device, no Python).  It drives
// pt_object_motion_between and pt_reproject_project_moved_host over edge inputs and the table's refusals in the header's order,
// and runs the very pixel the moved kernels compile (csrc/pt_reproject.h: reproject_pixel_moved, reproject_var_pixel<true>, then
// reproject_var_short_pixel) over host frames and a motion table allocated to their exact size, so that the sanitizer bounds every
// tap, every window read and every record read: a failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_reproject.h"

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

static bool same_bits(const void *a, const void *b, size_t bytes) { return memcmp(a, b, bytes) == 0; }

static bool is_marker(const pt_object_motion &r) { return r.scale == 0.0f; }
static bool is_identity(const pt_object_motion &r) {
    const pt_object_motion I = {{0.0f, 0.0f, 0.0f}, 1.0f};
    return same_bits(&r, &I, sizeof r);
}

int main() {
    const pt_camera cam = camera(0.0f, -0.2f, 7.8f, 0.0f, -0.06f, -1.0f);
    const pt_camera near_cam = camera(0.3f, -0.2f, 7.7f, -0.04f, -0.06f, -1.0f);
    const pt_camera back = camera(0.0f, -0.2f, 7.8f, 0.0f, 0.06f, 1.0f);
    const pt_camera aside = camera(4.0f, -0.2f, 3.0f, -1.0f, -0.06f, -0.2f);
    const pt_object_motion I = {{0.0f, 0.0f, 0.0f}, 1.0f}, M = {{0.0f, 0.0f, 0.0f}, 0.0f};
    static_assert(sizeof(pt_object_motion) == 16, "the record is 16 bytes");

    // ---- pt_object_motion_between
    {
        pt_object s = {};
        s.kind = PT_SPHERE;
        s.position[0] = 1.0f, s.position[1] = -2.0f, s.position[2] = 0.5f;
        s.radius = 1.5f;
        s.color[0] = 0.5f;
        pt_object_motion r;
        CHECK(pt_object_motion_between(nullptr, &s, &r) == PT_ERR_INVALID);
        CHECK(pt_object_motion_between(&s, nullptr, &r) == PT_ERR_INVALID);
        CHECK(pt_object_motion_between(&s, &s, nullptr) == PT_ERR_INVALID);
        CHECK(pt_object_motion_between(&s, &s, &r) == PT_OK && is_identity(r));
        pt_object t = s;
        t.position[0] = 1.25f;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && r.scale == 1.0f && r.offset[0] == -0.25f && r.offset[1] == 0.0f);
        t.radius = -3.0f;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && r.scale == 0.5f && r.offset[0] == 1.0f - 1.25f * 0.5f);
        t.radius = 0.0f;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        CHECK(pt_object_motion_between(&s, &t, &r) == PT_OK && is_marker(r));  // before.radius 0: scale 0
        t = s, t.radius = NAN;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        t = s, t.position[2] = INFINITY;
        CHECK(pt_object_motion_between(&s, &t, &r) == PT_OK && is_marker(r));
        t = s, t.color[0] = 0.25f;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        t = s, t.emission[2] = 1.0f;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        t = s, t.reflect_type = 2u;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        t = s, t.kind = PT_MESH;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        t = s, t.tri_count = 3u;
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        t = s, t.position[1] = 3e38f, s.position[1] = -1e38f;  // the offset leaves the finite numbers
        CHECK(pt_object_motion_between(&t, &s, &r) == PT_OK && is_marker(r));
        pt_object m = {};
        m.kind = PT_MESH;
        m.tri_count = 12u;
        m.radius = 0.0f;  // not read for a mesh
        pt_object n = m;
        n.position[0] = 2.0f, n.bs_radius = 9.0f;
        CHECK(pt_object_motion_between(&n, &m, &r) == PT_OK && r.scale == 1.0f && r.offset[0] == -2.0f);
        n.position[0] = 0.0f;
        CHECK(pt_object_motion_between(&n, &m, &r) == PT_OK && is_identity(r));
        n.position[0] = -0.0f;  // a difference of -0 is stored as +0
        CHECK(pt_object_motion_between(&m, &n, &r) == PT_OK && is_identity(r));
    }

    // ---- pt_reproject_project_moved_host
    {
        float px, pr, z, qx, qr, qz;
        const pt_object_motion tr = {{0.05f, -0.02f, 0.1f}, 1.0f}, sc = {{0.1f, 0.0f, -0.3f}, 0.75f}, neg = {{0.0f, 0.0f, 0.0f}, -1.0f},
                               nan_off = {{NAN, 0.0f, 0.0f}, 2.0f}, inf_s = {{0.0f, 0.0f, 0.0f}, INFINITY};
        CHECK(pt_reproject_project_moved_host(nullptr, &cam, 4, 4, 0, 1.0f, &tr, &px, &pr, &z) == PT_ERR_INVALID);
        CHECK(pt_reproject_project_moved_host(&cam, &cam, 4, 4, 0, 1.0f, nullptr, &px, &pr, &z) == PT_ERR_INVALID);
        CHECK(pt_reproject_project_moved_host(&cam, &cam, 4, 4, 0, 1.0f, &tr, nullptr, &pr, &z) == PT_ERR_INVALID);
        CHECK(pt_reproject_project_moved_host(&cam, &cam, 4, 4, 16, 1.0f, &tr, &px, &pr, &z) == PT_ERR_INVALID);
        CHECK(pt_reproject_project_moved_host(&cam, &cam, 0, 4, 0, 1.0f, &tr, &px, &pr, &z) == PT_ERR_INVALID);
        for (const pt_object_motion *bad : {&M, &neg, &nan_off, &inf_s})
            CHECK(pt_reproject_project_moved_host(&cam, &cam, 4, 4, 0, 1.0f, bad, &px, &pr, &z) == PT_ERR_INVALID);
        const uint32_t sizes[][2] = {{1, 1}, {7, 5}, {33, 25}};
        for (const auto &s : sizes)
            for (uint32_t idx = 0; idx < s[0] * s[1]; ++idx)
                for (const pt_camera *hc : {&cam, &near_cam, &back, &aside})
                    for (float depth : {0.0f, 4.0f, 8.0f, 1e30f, NAN, INFINITY}) {
                        // IDENTITY: the plain projection, bit for bit
                        const int a = pt_reproject_project_host(&cam, hc, s[0], s[1], idx, depth, &px, &pr, &z);
                        const int b = pt_reproject_project_moved_host(&cam, hc, s[0], s[1], idx, depth, &I, &qx, &qr, &qz);
                        CHECK(a == b && (a == 0 || a == 1));
                        if (a == 0) CHECK(same_bits(&px, &qx, 4) && same_bits(&pr, &qr, 4) && same_bits(&z, &qz, 4));
                        for (const pt_object_motion *rec : {&tr, &sc}) {
                            const int rc = pt_reproject_project_moved_host(&cam, hc, s[0], s[1], idx, depth, rec, &qx, &qr, &qz);
                            CHECK(rc == 0 || rc == 1);
                            if (rc == 0) CHECK(qx > -1.0f && qx < (float)s[0] && qr > -1.0f && qr < (float)s[1] && qz >= 0.0f);
                        }
                    }
    }

    // ---- the table's refusals, after the plain call's own and in the header's order: each breaks one rule and every one after it
    {
        float buf[4];
        int32_t ibuf[4];
        const float *F = buf;
        const int32_t *Ii = ibuf;
        const void *ctx = buf;  // never dereferenced
        pt::ReprojectCall pc, vc;
        pt::ReprojectFrame &f = pc.v.f;
        pt::ReprojectVarFrame &v = vc.v;
        int how = -1;  // the verdict of the last call that passed
        const pt_object_motion bad[3] = {I, M, {{0.0f, INFINITY, 0.0f}, -2.0f}}, neg[1] = {{{0.0f, 0.0f, 0.0f}, -1.0f}},
                               nan_s[1] = {{{0.0f, 0.0f, 0.0f}, NAN}}, inf_o[2] = {I, {{0.0f, 0.0f, -INFINITY}, 1.0f}},
                               fine[4] = {I, {{0.5f, 0.0f, 0.0f}, 1.0f}, M, {{0.0f, 0.0f, 0.0f}, 2.0f}}, idents[2] = {I, I},
                               marked[2] = {I, {{NAN, NAN, NAN}, -0.0f}};
        auto run = [&](bool is_var, pt::ReprojectCall &call, const void *cx, const pt_object_motion *m, uint32_t n) {
            pt::ReprojectArgs a{};
            a.ctx = cx, a.var = is_var, a.width = 2, a.height = 2, a.cam = &cam, a.hist_cam = &near_cam;
            a.color = F, a.depth = F, a.object_id = Ii, a.hist_color = F, a.hist_len = F, a.hist_depth = F, a.hist_object_id = Ii;
            a.out_color = buf, a.out_len = buf, a.motion = m, a.n_motion = n;
            if (is_var) a.hist_moments = F, a.out_moments = buf, a.error = buf;
            const int rc = pt::host::check_reproject(a, call);
            if (rc == PT_OK) how = call.how;
            return rc;
        };
        auto plain = [&](const void *cx, const pt_object_motion *m, uint32_t n) { return run(false, pc, cx, m, n); };
        auto var = [&](const void *cx, const pt_object_motion *m, uint32_t n) { return run(true, vc, cx, m, n); };
        // the plain call's last refusal comes first
        CHECK(refused(plain(nullptr, nullptr, (1u << 20) + 1u), "ctx") && refused(var(nullptr, nullptr, (1u << 20) + 1u), "ctx"));
        CHECK(refused(plain(ctx, nullptr, (1u << 20) + 1u), "2^20") && refused(var(ctx, nullptr, (1u << 20) + 1u), "2^20"));
        CHECK(refused(plain(ctx, nullptr, 3), "motion is NULL") && refused(var(ctx, nullptr, 3), "motion is NULL"));
        CHECK(refused(plain(ctx, bad, 3), "finite scale") && refused(var(ctx, bad, 3), "finite scale"));
        CHECK(refused(plain(ctx, neg, 1), "finite scale") && refused(plain(ctx, nan_s, 1), "finite scale"));
        CHECK(refused(plain(ctx, inf_o, 2), "finite scale") && refused(var(ctx, inf_o, 2), "finite scale"));
        CHECK(plain(ctx, bad, 2) == PT_OK && how == pt::host::kMotionTable);  // the bad record lies beyond n_motion
        // accepted, and which launch it is
        CHECK(plain(ctx, nullptr, 0) == PT_OK && how == pt::host::kMotionPlain);
        CHECK(plain(ctx, fine, 0) == PT_OK && how == pt::host::kMotionPlain);
        CHECK(plain(ctx, idents, 2) == PT_OK && how == pt::host::kMotionPlain);
        CHECK(var(ctx, idents, 2) == PT_OK && how == pt::host::kMotionPlain);
        CHECK(plain(ctx, marked, 2) == PT_OK && how == pt::host::kMotionTable);
        CHECK(plain(ctx, fine, 4) == PT_OK && how == pt::host::kMotionTable && f.hist_color == F && f.view.same == 0u);
        CHECK(var(ctx, fine, 4) == PT_OK && how == pt::host::kMotionTable && v.f.hist_color == F);
    }

    // ---- the moved pixel over host frames of exactly width * height and a table of exactly n_motion records
    size_t pixels = 0, blended = 0, moved_blended = 0, marked_px = 0, beyond = 0;
    const uint32_t frames[][2] = {{1, 1}, {7, 5}, {257, 3}, {33, 25}};
    for (const auto &s : frames) {
        const uint32_t w = s[0], h = s[1], n = w * h;
        for (const pt_camera *hc : {&cam, &near_cam, &aside, &back}) {
            for (int with_normals = 0; with_normals < 2; ++with_normals) {
                Frames fr = make_frames(n, w * 131u + h, true);
                Frames pl = fr;  // the plain call's outputs on the same inputs
                // ids -1..2 in the frames: records for 0 and 1 only, so that id 2 lies beyond the table; and a second pass with a
                // marker in the table
                for (int pass = 0; pass < 2; ++pass) {
                    std::vector<pt_object_motion> table = {{{0.0f, 0.0f, 0.0f}, 1.0f}, {{0.02f, -0.01f, 0.03f}, pass ? 0.0f : 0.98f}};
                    const pt::ReprojectMotion m = {table.data(), (uint32_t)table.size()};
                    const pt_reproject_var_params p = {4, 64.0f, 0.05f, 0.5f, 2u, 2u, 0};
                    pt::ReprojectCall call;
                    pt::ReprojectArgs a = frames_args(fr, w, h, &cam, hc, true, with_normals);
                    a.var_params = &p, a.motion = table.data(), a.n_motion = m.n;
                    CHECK(pt::host::check_reproject(a, call) == PT_OK);
                    pt::ReprojectVarFrame &v = call.v;
                    pt::ReprojectVarFrame vp;
                    const int how = call.how;
                    CHECK(how == pt::host::kMotionTable);
                    v.s_plane = fr.splane.data();
                    vp = v;
                    vp.f.out_color = pl.out.data(), vp.f.out_len = pl.len.data();
                    vp.out_moments = reinterpret_cast<pt::ReprojectMom *>(pl.mom.data());
                    vp.error = pl.err.data(), vp.s_plane = pl.splane.data();
                    for (uint32_t i = 0; i < n; ++i) pt::reproject_var_pixel<true>(v, i, &m);
                    for (uint32_t i = 0; i < n; ++i) pt::reproject_var_pixel(vp, i);
                    const HostSrc src = {v.s_plane, v.f.depth, v.f.object_id, (int32_t)w};
                    for (uint32_t i = 0; i < n; ++i) {
                        if (fr.err[i] == pt::kReprojectVarShort) fr.err[i] = pt::reproject_var_short_pixel(v, src, i);
                        if (pl.err[i] == pt::kReprojectVarShort) pl.err[i] = pt::reproject_var_short_pixel(vp, src, i);
                    }
                    // the colour-only pixel gives the var pixel's colour and length
                    for (uint32_t i = 0; i < n; ++i) {
                        float out[3], len;
                        pt::reproject_pixel_moved(v.f, m, i, out, &len);
                        CHECK(same_bits(out, &fr.out[3 * (size_t)i], 12) && same_bits(&len, &fr.len[i], 4));
                    }
                    for (uint32_t i = 0; i < n; ++i) {
                        const int32_t id = fr.id[i];
                        const bool plain_px = id != 1;  // no hit, IDENTITY, or beyond the table
                        if (plain_px) {
                            CHECK(same_bits(&fr.out[3 * (size_t)i], &pl.out[3 * (size_t)i], 12) && same_bits(&fr.len[i], &pl.len[i], 4));
                            CHECK(same_bits(&fr.mom[2 * (size_t)i], &pl.mom[2 * (size_t)i], 8) && same_bits(&fr.err[i], &pl.err[i], 4));
                            if (id == 2) ++beyond;
                        } else if (pass) {  // the marker: (color, wt)
                            CHECK(same_bits(&fr.out[3 * (size_t)i], &fr.color[3 * (size_t)i], 12) && fr.len[i] == 4.0f);
                            ++marked_px;
                        } else if (fr.len[i] > 4.0f)
                            ++moved_blended;
                        CHECK(fr.len[i] >= 4.0f && fr.len[i] <= 64.0f);
                        if (fr.len[i] > 4.0f) ++blended;
                        ++pixels;
                    }
                }
            }
        }
    }
    CHECK(blended > pixels / 50 && moved_blended > 0 && marked_px > 0 && beyond > 0);
    printf("reproject_moved_check: ok (%zu pixels, %zu blended, %zu of them on a moved object, %zu marked, %zu beyond the table)\n", pixels,
           blended, moved_blended, marked_px, beyond);
    return 0;
}
