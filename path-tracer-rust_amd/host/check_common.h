// check_common.h — what the stand-alone host programs under host/ share (<name>_check judges itself, <name>_probe and <name>_dump
// print what a test asks for; the Makefile's one rule builds each with -fsanitize=address,undefined; no device, no Python): the
// library's error channel, which lives in csrc/pt_api.hip and so is not linked here, CHECK, the refusal test, the random numbers, and
// the cameras and frames of the reproject programs.  Each program is one translation unit of its own, linked against
// host/scene_io.cpp and csrc/pt_host.cpp compiled once for all of them: the definitions below are its.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptrace.h"
#include "../csrc/pt_reproject.h"

namespace pt {
static std::string g_error;
void set_error(const std::string &m) { g_error = m; }
}  // namespace pt
extern "C" const char *pt_last_error(void) { return pt::g_error.c_str(); }

// a failed check ends main with a non-zero status
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

// the call was refused, and the message names `word`
static bool refused(int rc, const char *word) { return rc == PT_ERR_INVALID && pt::g_error.find(word) != std::string::npos; }

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

static pt_camera camera(float px, float py, float pz, float dx, float dy, float dz) {
    const float l = sqrtf(dx * dx + dy * dy + dz * dz);
    pt_camera c = {{px, py, pz}, {dx, dy, dz}, 0.035f, 0.036f, 1.5f};
    if (l > 0.0f)
        for (float &v : c.direction) v /= l;
    return c;
}

// a frame and its history for pt_ctx_reproject; hmom, mom, err and splane are pt_ctx_reproject_var's and empty without it
struct Frames {
    std::vector<float> color, depth, normal, hcolor, hlen, hmom, hdepth, hnormal, out, len, mom, err, splane;
    std::vector<int32_t> id, hid;
};

// Random frames in the style of the GPU tests: depths on a few planes and +inf, ids -1..2, normals with zero vectors, lengths
// with zeros.  `var` (pt_ctx_reproject_var): depths, ids and lengths in blocks, so that some stretches are all long and some all
// short, and moments of a colour sum in [0, 3].
static Frames make_frames(uint32_t n, uint32_t seed, bool var) {
    Frames f;
    uint32_t s = seed;
    const float planes[] = {2.0f, 6.0f, 6.25f, 9.0f, INFINITY};
    auto fill = [&](std::vector<float> &v, size_t k) {
        v.resize(k);
        for (float &x : v) x = unit(s);
    };
    fill(f.color, 3 * (size_t)n);
    fill(f.hcolor, 3 * (size_t)n);
    fill(f.normal, 3 * (size_t)n);
    fill(f.hnormal, 3 * (size_t)n);
    for (size_t i = 0; i < 3 * (size_t)n; ++i) {
        f.normal[i] -= 0.5f;
        f.hnormal[i] = lcg(s) % 8u ? f.normal[i] : 0.0f;
    }
    f.depth.resize(n), f.hdepth.resize(n), f.hlen.resize(n), f.id.resize(n), f.hid.resize(n);
    if (var) f.hmom.resize(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        f.depth[i] = planes[!var || (i / 5u) % 4u == 3u ? lcg(s) % 5u : (i / 5u) % 4u];
        f.hdepth[i] = lcg(s) % 4u ? f.depth[i] : planes[lcg(s) % 5u];
        f.id[i] = var && lcg(s) % 6u ? (int32_t)((i / 7u) % 3u) : (int32_t)(lcg(s) % 4u) - 1;
        f.hid[i] = lcg(s) % 4u ? f.id[i] : (int32_t)(lcg(s) % 4u) - 1;
        f.hlen[i] = var && (i / 40u) % 3u == 0u ? 32.0f : (float)(lcg(s) % 5u) * 4.0f;
        if (var) {
            const float m1 = 3.0f * unit(s);
            f.hmom[2 * (size_t)i] = m1;
            f.hmom[2 * (size_t)i + 1] = m1 * m1 + unit(s);
        }
    }
    f.out.assign(3 * (size_t)n, -1.0f);
    f.len.assign(n, -1.0f);
    if (var) {
        f.mom.assign(2 * (size_t)n, -1.0f);
        f.err.assign(n, -2.0f);
        f.splane.assign(n, -1.0f);
    }
    return f;
}

// The reproject call over such frames: the frame, its whole history and the outputs - `var`: the moments and the error too;
// `normals`: both normal planes.  ctx is the frames' address; params, spp and the table are the caller's to set.
static pt::ReprojectArgs frames_args(Frames &fr, uint32_t w, uint32_t h, const pt_camera *cam, const pt_camera *hist_cam, bool var,
                                     bool normals) {
    pt::ReprojectArgs a{};
    a.ctx = &fr, a.var = var, a.width = w, a.height = h, a.cam = cam, a.hist_cam = hist_cam;
    a.color = fr.color.data(), a.depth = fr.depth.data(), a.object_id = fr.id.data(), a.normal = normals ? fr.normal.data() : nullptr;
    a.hist_color = fr.hcolor.data(), a.hist_len = fr.hlen.data(), a.hist_depth = fr.hdepth.data(), a.hist_object_id = fr.hid.data();
    a.hist_normal = normals ? fr.hnormal.data() : nullptr, a.out_color = fr.out.data(), a.out_len = fr.len.data();
    if (var) a.hist_moments = fr.hmom.data(), a.out_moments = fr.mom.data(), a.error = fr.err.data();
    return a;
}
