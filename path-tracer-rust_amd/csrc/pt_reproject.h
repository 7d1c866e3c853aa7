// pt_reproject.h — pt_ctx_reproject (pt_reproject.hip): last frame's colour carried into this frame's pixels through the depth
// and object-id guides, and blended with this frame's colour by the history length (the temporal half of SVGF, Schied et al.
// 2017).  The arithmetic is the contract in include/ptrace.h ("THE ARITHMETIC" of pt_ctx_reproject), operation for operation.
// Steps 3 to 5 - and the pixel that strings them together - are stated once, below, for host and device:
// pt_reproject_project_host (host/scene_io.cpp) is the host instantiation of the projection the kernel compiles, as
// pt_present_quantize_host is of pt_present.h.  pt_ctx_reproject_moved and pt_ctx_reproject_var_moved - history carried through
// pt_ctx_set_object's edits by a per-object motion table - are the same functions with MOVED compiled in, and
// pt_ctx_reproject_var_weighted - a plane of per-pixel sample counts in place of the one weight - with WEIGHTED.  Around the
// kernels the five entry points are one call, at the end of this file: ReprojectArgs names what the caller passed,
// host::check_reproject (pt_host.cpp) refuses or fills a ReprojectCall, launch_reproject (pt_reproject.hip) picks the kernels.
// A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace.h"
#include "pt_math.h"

namespace pt {

// the values a zero field of pt_reproject_params stands for: what the CPU study picked (profiles/reproject_cpu_study.json)
constexpr float kReprojectMaxHistory = 64.0f, kReprojectDepthTol = 0.125f, kReprojectNormalMin = 0.9f;

// What step 3 needs of the two cameras, computed on the host in binary32 (host::reproject_view, pt_host.cpp): pt_camera_basis of
// both, and the history camera's constants - each the one binary32 operation sequence the contract names, so a pixel that
// computed them itself would hold the same bits.
struct ReprojectView {
    vec3 C, L, su, sv;           // cam: position, lens centre, sensor axes
    vec3 hL, hD, hDf, hsu, hsv;  // hist_cam: lens centre L', direction D' as stored, D' * f', sensor axes
    float hfdd, hsuu, hsvv;      // f' * dot(D', D'), dot(su', su'), dot(sv', sv')
    uint32_t same;               // step 2: all nine floats of the two cameras are bitwise equal
};

// The call's whole frames.  Host pointers on the host, device pointers on the device.
struct ReprojectFrame {
    uint32_t width, height;
    const float *color, *depth, *normal;  // normal may be NULL
    const int32_t *object_id;
    const float *hist_color, *hist_len, *hist_depth, *hist_normal;  // hist_color NULL: no history; hist_normal may be NULL
    const int32_t *hist_object_id;
    float *out_color, *out_len;
    float wt, max_history, depth_tol, normal_min;  // defaults filled in; wt = (float)weight
    ReprojectView view;
};

// pt_ctx_reproject_var: the values a zero min_frames / radius stands for - what its CPU study picked
// (profiles/reproject_var_cpu_study.json) - the marker kernel A leaves in d_error for a pixel whose history is short (an
// estimate is never negative), and kernel B's tile (pt_denoise.hip's shape)
constexpr uint32_t kReprojectVarMinFrames = 2u, kReprojectVarRadius = 3u, kReprojectVarMaxRadius = 3u;
constexpr float kReprojectVarShort = -1.0f;
constexpr uint32_t kReprojectVarTileW = 32u, kReprojectVarTileH = 8u;

// a pixel's temporal moments (m1, m2) of s = (r + g) + b: one 8-byte load or store
struct alignas(8) ReprojectMom {
    float m1, m2;
};

// pt_ctx_reproject_var's call: pt_ctx_reproject's, the moments planes, the error map and the context's plane of s values
struct ReprojectVarFrame {
    ReprojectFrame f;
    const ReprojectMom *hist_moments;  // NULL with f.hist_color
    ReprojectMom *out_moments;
    float *error, *s_plane;
    float long_len;   // (float)min_frames * wt: a history of at least this many samples is long
    uint32_t radius;  // the spatial window is (2 * radius + 1)^2
};

struct ReprojectPos {
    float px, pr, zexp;
};

// ---- pt_ctx_reproject_moved: the per-object motion table ("THE RECORD" in include/ptrace.h).  Device memory on the device (the
// context's scratch, 16-byte aligned), the caller's array on the host.
struct ReprojectMotion {
    const pt_object_motion *table;
    uint32_t n;
};
PT_HD uint32_t reproject_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
// IDENTITY by its bits: scale 1.0f, the three offsets +0.0f
PT_HD bool reproject_rec_identity(const pt_object_motion &r) {
    return reproject_bits(r.scale) == 0x3f800000u && (reproject_bits(r.offset[0]) | reproject_bits(r.offset[1]) | reproject_bits(r.offset[2])) == 0u;
}
// the MARKER: scale == 0 (either sign)
PT_HD bool reproject_rec_marker(const pt_object_motion &r) { return r.scale == 0.0f; }
// the record of object `id` (>= 0): an id beyond the table reads nothing and stands for IDENTITY.  One 16-byte load.
PT_HD pt_object_motion reproject_rec(const ReprojectMotion &m, int32_t id) {
    pt_object_motion r = {{0.0f, 0.0f, 0.0f}, 1.0f};
    if ((uint32_t)id < m.n) {
#if defined(__HIP_DEVICE_COMPILE__)
        const float4 q = *reinterpret_cast<const float4 *>(m.table + (uint32_t)id);
        r.offset[0] = q.x, r.offset[1] = q.y, r.offset[2] = q.z, r.scale = q.w;
#else
        r = m.table[(uint32_t)id];
#endif
    }
    return r;
}

// ---- pt_ctx_reproject_var_weighted: the plane of per-pixel sample counts ("THE ARITHMETIC" of pt_ctx_reproject_var_weighted in
// include/ptrace.h).  A kernel argument of its own, as the motion table is: ReprojectFrame and ReprojectVarFrame stay what they
// are.  The uniform value w0 is the frame's f.wt, and (float)min_frames * w0 its long_len.  spp NULL: the uniform call.
struct ReprojectWeights {
    const uint32_t *spp;  // width * height counts; 0: the pixel holds no samples this frame
    float min_frames;     // (float)min_frames: a pixel with count c > 0 is long from min_frames * (float)c samples on
};

// Step 3's first lines, stated once: the unit direction of the ray through the centre of the pixel in column x and camera row y
// (y = H-1-r), made as render_pixel makes it - sx, sy, S, g = L - S, d = g * (1 / sqrt(dot(g, g))).  C, L, su, sv: the camera's
// position and its pt_camera_basis.  pt_ctx_overlay's step 1 (pt_overlay.h) is this function too.
PT_HD vec3 reproject_ray(vec3 C, vec3 L, vec3 su, vec3 sv, uint32_t W, uint32_t H, uint32_t x, uint32_t y) {
    const float fw = (float)W, fh = (float)H;
    const float sx = ((float)x + 0.5f) / fw - 0.5f;
    const float sy = ((float)y + 0.5f) / fh - 0.5f;
    const vec3 S = (C + su * sx) + sv * sy;
    const vec3 g = L - S;
    return g * (1.0f / __builtin_sqrtf(dot(g, g)));
}

// step 3 up to the reject test: where the point pixel idx sees at `depth` lies in the history frame.  false: no position.
// MOVED (pt_ctx_reproject_moved): the point goes through the object's record first - Pm[a] = P[a]*scale + offset[a], two
// operations per component - unless the record is IDENTITY, which leaves P's bits alone.
template <bool MOVED = false>
PT_HD bool reproject_project(const ReprojectView &V, uint32_t W, uint32_t H, uint32_t idx, float depth, ReprojectPos &o,
                             const pt_object_motion *rec = nullptr) {
    const uint32_t x = idx % W, r = idx / W, y = H - 1u - r;
    vec3 P = V.L + reproject_ray(V.C, V.L, V.su, V.sv, W, H, x, y) * depth;
    const float fw = (float)W, fh = (float)H;
    if constexpr (MOVED) {
        const vec3 Pm = mk(P.x * rec->scale + rec->offset[0], P.y * rec->scale + rec->offset[1], P.z * rec->scale + rec->offset[2]);
        if (!reproject_rec_identity(*rec)) P = Pm;
    }
    const vec3 v = P - V.hL;
    const float a = dot(v, V.hD);
    if (!(a > 0.0f)) return false;
    const float t = a / V.hfdd;
    const vec3 w = V.hDf - v / t;
    const float sxh = dot(w, V.hsu) / V.hsuu;
    const float syh = dot(w, V.hsv) / V.hsvv;
    o.px = (sxh + 0.5f) * fw - 0.5f;
    const float py = (syh + 0.5f) * fh - 0.5f;
    o.pr = (float)(H - 1u) - py;
    if (!(o.px > -1.0f && o.px < fw && o.pr > -1.0f && o.pr < fh)) return false;  // a NaN rejects
    o.zexp = __builtin_sqrtf(dot(v, v));
    return true;
}

// N(.): pt_ctx_denoise's normalised normal
PT_HD vec3 reproject_normal(const float *n) {
    const float nx = n[0], ny = n[1], nz = n[2];
    const float l = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
    return l > 0.0f ? mk(nx / l, ny / l, nz / l) : mk(0.0f, 0.0f, 0.0f);
}

// step 4 without the normals: is history pixel q (length, id, depth) the surface pixel idx sees?
PT_HD bool reproject_tap_ok(float hist_len, int32_t hist_id, int32_t id, float zexp, float hist_depth, float depth_tol) {
    if (!(hist_len > 0.0f) || hist_id != id) return false;
    const float zm = zexp > hist_depth ? zexp : hist_depth;
    return __builtin_fabsf(zexp - hist_depth) <= depth_tol * zm;
}

// One tap of step 4: history pixel q (clamped into the frame, so that it can be read before anything is known about it), its
// bilinear weight b, and whether the tap lies inside the frame at all.
struct ReprojectTap {
    uint32_t q;
    float b;
    bool inside;
};

// Steps 4 and 5 over NT taps (1: the same camera; 4: the bilinear footprint, in the contract's order).  Written for the
// memory system: everything the taps may need - guides, normals, colours - is read before the first tap is tested, so a lane has
// all of its history reads in flight at once instead of up to three dependent round trips per tap, one tap after the other.  A
// tap that fails its test has been read for nothing - its neighbours want the same lines - and adds nothing: the sums are the
// contract's, in its order.  false: bsum > 0 does not hold (step 1).
// MOM (pt_ctx_reproject_var): the taps' moments ride along - read with the rest, summed with the same b over the same taps, and
// blended with the same k as the colour; `mom` holds (s, s*s) on entry and (m1, m2) on return.  Without MOM nothing of it is
// compiled.
// WEIGHTED (pt_ctx_reproject_var_weighted): wp, the pixel's own count as a float, stands in for f.wt; `empty` (count 0) carries
// the history through as it is - the values themselves, not a blend by 0, so that the pixel's colour never enters them.
template <int NT, bool MOM = false, bool WEIGHTED = false>
PT_HD bool reproject_gather(const ReprojectFrame &f, const ReprojectTap (&tap)[NT], float zexp, int32_t id, bool normals, vec3 N,
                            const float col[3], float out[3], float *len_out, const ReprojectMom *hist_moments = nullptr,
                            ReprojectMom *mom = nullptr, float wp = 0.0f, bool empty = false) {
    float hlen[NT], hdepth[NT];
    int32_t hid[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        hlen[t] = f.hist_len[tap[t].q];
        hid[t] = f.hist_object_id[tap[t].q];
        hdepth[t] = f.hist_depth[tap[t].q];
    }
    float hc[NT][3], hn[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t q3 = (size_t)tap[t].q * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hc[t][c] = f.hist_color[q3 + c];
            hn[t][c] = normals ? f.hist_normal[q3 + c] : 0.0f;
        }
    }
    ReprojectMom hm[NT];
    if constexpr (MOM) {
#pragma unroll
        for (int t = 0; t < NT; ++t) hm[t] = hist_moments[tap[t].q];
    }
    float s[3] = {0.0f, 0.0f, 0.0f}, nsum = 0.0f, bsum = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        bool take = tap[t].inside && reproject_tap_ok(hlen[t], hid[t], id, zexp, hdepth[t], f.depth_tol);
        if (normals) take = take && dot(N, reproject_normal(hn[t])) >= f.normal_min;
        const float b = tap[t].b;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = take ? s[c] + hc[t][c] * b : s[c];
        if constexpr (MOM) {
            a1 = take ? a1 + hm[t].m1 * b : a1;
            a2 = take ? a2 + hm[t].m2 * b : a2;
        }
        nsum = take ? nsum + hlen[t] * b : nsum;
        bsum = take ? bsum + b : bsum;
    }
    if (!(bsum > 0.0f)) return false;
    float wt = f.wt;
    if constexpr (WEIGHTED) {
        wt = wp;
        if (empty) {
            float n = nsum / bsum;
            if (n > f.max_history) n = f.max_history;
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = s[c] / bsum;
            if constexpr (MOM) {
                mom->m1 = a1 / bsum;
                mom->m2 = a2 / bsum;
            }
            *len_out = n;
            return true;
        }
    }
    float n = nsum / bsum + wt;
    if (n > f.max_history) n = f.max_history;
    if (n < wt) n = wt;
    const float k = wt / n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float h = s[c] / bsum;
        out[c] = h + (col[c] - h) * k;
    }
    if constexpr (MOM) {
        const float h1 = a1 / bsum, h2 = a2 / bsum;
        mom->m1 = h1 + (mom->m1 - h1) * k;
        mom->m2 = h2 + (mom->m2 - h2) * k;
    }
    *len_out = n;
    return true;
}

// a value of the pixel's own planes: read once by one lane, so the device keeps it out of the L1 the taps live in
PT_HD float reproject_own(const float *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
PT_HD int32_t reproject_own(const int32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
PT_HD uint32_t reproject_own(const uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// steps 1 to 5 for pixel idx (< width * height): the colour and the length it ends with.  The pixel's own colour is read before
// anything is returned, so the caller may store into color[idx].  MOM: pt_ctx_reproject_var's moments too - *s_out is the
// pixel's s = (r + g) + b of the input colour, *mom its (m1, m2).
// MOVED (pt_ctx_reproject_moved): the object's record, read as soon as the id is known, decides - the marker ends at step 1,
// IDENTITY runs the steps as they are, any other record maps the point and never takes step 2.  Under a still camera a wave then
// holds one-tap and four-tap lanes: both go through the ONE four-tap gather, the one-tap lanes with their own pixel as tap 0
// (b = 1) and three taps that are outside (never taken, so the sums are the one-tap sums bit for bit; they read the lane's own
// history pixel again, a line it has in flight already).  No lane waits for another's second gather.  Without MOVED nothing of it
// is compiled.
// WEIGHTED (pt_ctx_reproject_var_weighted): the pixel's count - one more of its own loads, issued with the colour's - is handed
// back in *count_out; as a float it is the pixel's wt in every step, and a count of 0 takes the history as it is.  Without
// WEIGHTED nothing of it is compiled.
template <bool MOM, bool MOVED = false, bool WEIGHTED = false>
PT_HD void reproject_pixel_t(const ReprojectFrame &f, uint32_t idx, float out[3], float *len_out, const ReprojectMom *hist_moments,
                             ReprojectMom *mom, float *s_out, const ReprojectMotion *motion = nullptr,
                             const ReprojectWeights *weights = nullptr, uint32_t *count_out = nullptr) {
    const size_t i3 = (size_t)idx * 3u;
    float col[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = col[c] = reproject_own(f.color + i3 + c);
    float wp = 0.0f;
    bool empty = false;
    if constexpr (WEIGHTED) {
        const uint32_t count = reproject_own(weights->spp + idx);
        *count_out = count;
        wp = (float)count;
        empty = count == 0u;
        *len_out = wp;
    } else {
        *len_out = f.wt;
    }
    if constexpr (MOM) {
        const float s = (col[0] + col[1]) + col[2];
        *s_out = s;
        mom->m1 = s;
        mom->m2 = s * s;
    }
    if (!f.hist_color) return;
    const int32_t id = reproject_own(f.object_id + idx);
    if (id < 0) return;
    pt_object_motion rec = {{0.0f, 0.0f, 0.0f}, 1.0f};
    if constexpr (MOVED) rec = reproject_rec(*motion, id);
    const float depth = reproject_own(f.depth + idx);
    const bool normals = f.normal && f.hist_normal;
    vec3 N = mk(0.0f, 0.0f, 0.0f);
    if (normals) {
        const float n[3] = {reproject_own(f.normal + i3), reproject_own(f.normal + i3 + 1), reproject_own(f.normal + i3 + 2)};
        N = reproject_normal(n);
    }
    if constexpr (MOVED) {
        if (reproject_rec_marker(rec)) return;
    } else if (f.view.same) {
        const ReprojectTap tap[1] = {{idx, 1.0f, true}};
        reproject_gather<1, MOM, WEIGHTED>(f, tap, depth, id, normals, N, col, out, len_out, hist_moments, mom, wp, empty);
        return;
    }
    ReprojectTap tap[4];
    float zexp;
    if (MOVED && f.view.same && reproject_rec_identity(rec)) {  // step 2 in the four-tap gather's shape
        tap[0] = {idx, 1.0f, true};
#pragma unroll
        for (int t = 1; t < 4; ++t) tap[t] = {idx, 0.0f, false};
        zexp = depth;
    } else {
        ReprojectPos p;
        if (!reproject_project<MOVED>(f.view, f.width, f.height, idx, depth, p, &rec)) return;
        const float flx = __builtin_floorf(p.px), flr = __builtin_floorf(p.pr);
        const int32_t x0 = (int32_t)flx, r0 = (int32_t)flr;  // in [-1, width - 1] and [-1, height - 1]
        const float fx = p.px - flx, fr = p.pr - flr;
        const int32_t xmax = (int32_t)f.width - 1, rmax = (int32_t)f.height - 1;
#pragma unroll
        for (int32_t j = 0; j < 2; ++j) {
#pragma unroll
            for (int32_t i = 0; i < 2; ++i) {
                const int32_t qx = x0 + i, qr = r0 + j;
                ReprojectTap &t = tap[j * 2 + i];
                t.inside = qx >= 0 && qr >= 0 && qx <= xmax && qr <= rmax;
                const int32_t cx = qx < 0 ? 0 : (qx > xmax ? xmax : qx), cr = qr < 0 ? 0 : (qr > rmax ? rmax : qr);
                t.q = (uint32_t)cr * f.width + (uint32_t)cx;
                t.b = (i ? fx : 1.0f - fx) * (j ? fr : 1.0f - fr);
            }
        }
        zexp = p.zexp;
    }
    reproject_gather<4, MOM, WEIGHTED>(f, tap, zexp, id, normals, N, col, out, len_out, hist_moments, mom, wp, empty);
}
PT_HD void reproject_pixel(const ReprojectFrame &f, uint32_t idx, float out[3], float *len_out) {
    reproject_pixel_t<false>(f, idx, out, len_out, nullptr, nullptr, nullptr);
}
PT_HD void reproject_pixel_moved(const ReprojectFrame &f, const ReprojectMotion &m, uint32_t idx, float out[3], float *len_out) {
    reproject_pixel_t<false, true>(f, idx, out, len_out, nullptr, nullptr, nullptr, &m);
}

// ---- pt_ctx_reproject_var: the variance and the error map ("THE ARITHMETIC" of pt_ctx_reproject_var in include/ptrace.h)
PT_HD float reproject_pos(float v) { return v > 0.0f ? v : 0.0f; }
// vt = pos(m2 - m1*m1)
PT_HD float reproject_var_temporal(const ReprojectMom &m) { return reproject_pos(m.m2 - m.m1 * m.m1); }
// e = sqrt(v*k) / sqrt(2^-6 + ((out[0] + out[1]) + out[2])), at most 12 (a NaN gives 12)
PT_HD float reproject_var_error(float v, float k, const float out[3]) {
    const float e = __builtin_sqrtf(v * k) / __builtin_sqrtf(0.015625f + ((out[0] + out[1]) + out[2]));
    return e < 12.0f ? e : 12.0f;
}

// Kernel A's pixel: pt_ctx_reproject's colour and length, the moments, the s plane, and d_error - final where the history is
// long, kReprojectVarShort where the spatial estimate has to stand in.  Everything the pixel reads of planes it may share with
// an output (its own colour) is read before the first store.
// WEIGHTED: a pixel with a count is long from min_frames * wp samples on, the product formed here, and its k is wp / len; a
// pixel without one is long by the frame's long_len, its k is w0 / len, and it is never marked: no spatial estimate without a colour.
template <bool MOVED = false, bool WEIGHTED = false>
PT_HD void reproject_var_pixel(const ReprojectVarFrame &v, uint32_t idx, const ReprojectMotion *motion = nullptr,
                               const ReprojectWeights *weights = nullptr) {
    float out[3], len, s;
    ReprojectMom mom;
    uint32_t count = 0u;
    reproject_pixel_t<true, MOVED, WEIGHTED>(v.f, idx, out, &len, v.hist_moments, &mom, &s, motion, weights, &count);
    float *o = v.f.out_color + (size_t)idx * 3u;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    v.f.out_len[idx] = len;
    v.out_moments[idx] = mom;
    v.s_plane[idx] = s;
    if constexpr (WEIGHTED) {
        const float wp = (float)count, vt = reproject_var_temporal(mom);
        if (count == 0u)
            v.error[idx] = len >= v.long_len ? reproject_var_error(vt, v.f.wt / len, out) : __builtin_inff();
        else
            v.error[idx] = len >= weights->min_frames * wp ? reproject_var_error(vt, wp / len, out) : kReprojectVarShort;
    } else {
        v.error[idx] = len >= v.long_len ? reproject_var_error(reproject_var_temporal(mom), v.f.wt / len, out) : kReprojectVarShort;
    }
}

// The spatial estimate of the pixel at column x, row r: the window of s values around it, in the contract's tap order (dy outside,
// dx inside; taps outside the frame skipped, the centre always taken).  src(qx, qr, s, id, depth) reads a pixel of the frame:
// global planes on the host, the staged tile on the device.  false: fewer than two taps, no estimate.
// WEIGHTED: src.count(qx, qr) is a pixel's count, and a q other than the centre is taken only when its count is the centre's - a
// neighbour with another count holds values of another variance, one with count 0 holds no data.
template <class Src, bool WEIGHTED = false>
PT_HD bool reproject_var_spatial(const Src &src, int32_t W, int32_t H, int32_t R, float depth_tol, int32_t x, int32_t r, float *vs) {
    float s0, z0;
    int32_t id0;
    src(x, r, s0, id0, z0);
    uint32_t c0 = 0u;
    if constexpr (WEIGHTED) c0 = src.count(x, r);
    float S1 = 0.0f, S2 = 0.0f;
    uint32_t cnt = 0;
    for (int32_t dy = -R; dy <= R; ++dy) {
        const int32_t qr = r + dy;
        if (qr < 0 || qr >= H) continue;
        for (int32_t dx = -R; dx <= R; ++dx) {
            const int32_t qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            float sq, zq;
            int32_t idq;
            src(qx, qr, sq, idq, zq);
            bool take = idq == id0;
            if (id0 >= 0) {
                const float zm = z0 > zq ? z0 : zq;
                take = take && __builtin_fabsf(z0 - zq) <= depth_tol * zm;
            }
            if constexpr (WEIGHTED) take = take && src.count(qx, qr) == c0;
            take = take || (dx == 0 && dy == 0);
            S1 = take ? S1 + sq : S1;
            S2 = take ? S2 + sq * sq : S2;
            cnt += take ? 1u : 0u;
        }
    }
    if (cnt < 2u) return false;
    const float fc = (float)cnt, mean = S1 / fc;
    *vs = reproject_pos(S2 / fc - mean * mean);
    return true;
}

// Kernel B's pixel, for one kernel A marked short: e from max(vs, vt), or +inf without a spatial estimate.  It reads the pixel's
// own outputs of kernel A and writes d_error[idx] alone.  WEIGHTED: k = wp / len_out, wp the pixel's own count (> 0: it is marked).
template <class Src, bool WEIGHTED = false>
PT_HD float reproject_var_short_pixel(const ReprojectVarFrame &v, const Src &src, uint32_t idx) {
    const int32_t W = (int32_t)v.f.width, H = (int32_t)v.f.height;
    const int32_t x = (int32_t)(idx % v.f.width), r = (int32_t)(idx / v.f.width);
    float vs;
    if (!reproject_var_spatial<Src, WEIGHTED>(src, W, H, (int32_t)v.radius, v.f.depth_tol, x, r, &vs)) return __builtin_inff();
    const float vt = reproject_var_temporal(v.out_moments[idx]);
    const float *o = v.f.out_color + (size_t)idx * 3u;
    const float out[3] = {o[0], o[1], o[2]};
    float wt = v.f.wt;
    if constexpr (WEIGHTED) wt = (float)src.count(x, r);
    return reproject_var_error(vs > vt ? vs : vt, wt / v.f.out_len[idx], out);
}

// ---- A call of any of the five entry points.  They are ONE call with three optional parts: the moments planes make it a _var
// call, a motion table that is not all IDENTITY a _moved one, a plane of counts the _weighted one.
namespace host {
// How a call runs its table.  kMotionPlain: motion NULL, n_motion 0 or every record IDENTITY - the plain kernels, unchanged.
// kMotionTable: the moved kernels.
constexpr int kMotionPlain = 0, kMotionTable = 1;
constexpr uint32_t kReprojectMaxMotion = 1u << 20;
}  // namespace host

// What the caller passed, by name: the arguments of include/ptrace.h without their d_ prefix.  An entry point leaves what it
// does not take at zero.  Host pointers on the host, device pointers on the device.
struct ReprojectArgs {
    const void *ctx;  // tested against NULL, never dereferenced: the host programs pass any address
    bool var;         // a pt_ctx_reproject_var* entry point: var_params and its messages, the moments and error are compulsory
    uint32_t width, height;
    const pt_reproject_params *params;          // without var
    const pt_reproject_var_params *var_params;  // with var
    const pt_camera *cam, *hist_cam;
    const float *color, *depth, *normal;
    const int32_t *object_id;
    const float *hist_color, *hist_len, *hist_moments, *hist_depth, *hist_normal;
    const int32_t *hist_object_id;
    float *out_color, *out_len, *out_moments, *error;
    const uint32_t *spp;  // the plane of counts; NULL: the uniform call.  Never refused.
    const pt_object_motion *motion;
    uint32_t n_motion;
};

// The call once it has passed: the frames with the defaults filled in, and which kernels it takes
struct ReprojectCall {
    ReprojectVarFrame v;   // without var, v.f alone; v.s_plane is the caller's to set
    ReprojectWeights wts;  // the plane and (float)min_frames
    bool var, weighted;    // weighted: var with a plane
    int how;               // host::kMotionPlain or host::kMotionTable: what the table's records say
    // the moved kernels and the table's upload: something moved, and there is a history for it to move in
    bool moved() const { return how == host::kMotionTable && v.f.hist_color; }
};

namespace host {
// the view of a camera pair; hist_cam NULL: the first frame, nothing of the history is set
void reproject_view(const pt_camera &cam, const pt_camera *hist_cam, ReprojectView &out);
// The refusals of all five entry points, each test made once and in the header's order (PT_ERR_INVALID + message; the
// params struct a message names is the entry point's): the params, the size, the compulsory pointers, the history, ctx, then
// the table's (check_reproject_motion).  PT_OK: `call` holds the call.  No device is touched.
int check_reproject(const ReprojectArgs &a, ReprojectCall &call);
// the table's own refusals, in the header's order, after the rest of the call has passed (rc_plain is that verdict and is
// returned when not PT_OK); PT_OK: *how is kMotionPlain or kMotionTable.  O(n_motion) on the host, no device.
int check_reproject_motion(int rc_plain, const pt_object_motion *motion, uint32_t n_motion, int *how);
}  // namespace host

#if defined(__HIPCC__)
// The kernels of a call that has passed: colour only - one lane per pixel; with moments - kernel A, one lane per pixel, then
// kernel B, one workgroup per tile of 32 x 8.  `table` (device memory, 16-byte aligned) is read when call.moved().
void launch_reproject(hipStream_t st, const ReprojectCall &call, const ReprojectMotion *table);
#endif

}  // namespace pt
