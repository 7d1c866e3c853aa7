// pt_upsample.h — pt_ctx_upsample (pt_upsample.hip): a frame traced at low resolution filled in at full resolution through the
// first-hit guides of both sizes - a joint bilateral upsampler (Kopf et al. 2007) whose tap tests are pt_ctx_reproject's (object
// id, relative depth, normal cosine).  The arithmetic is the contract in include/ptrace.h ("THE ARITHMETIC" of pt_ctx_upsample),
// operation for operation, stated once, below, for host and device: pt_upsample_tap_host (host/scene_io.cpp) is the host
// instantiation of the tap position the kernel compiles.  A translation unit of its own: pt_kernels.s, and so
// pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace.h"
#include "pt_math.h"
#include "pt_reproject.h"  // reproject_normal (N(.)), reproject_own (the non-temporal load of a pixel's own planes)

namespace pt {

// the values a zero field of pt_upsample_params stands for: what the CPU study picked (profiles/upsample_cpu_study.json)
constexpr float kUpsampleDepthTol = 0.25f, kUpsampleNormalMin = 0.95f;
// the largest size of an axis, of either frame: (2x + 1) * w + W is then at most 2^29, and (float)e / (float)(2W) is below 1
constexpr uint32_t kUpsampleMaxSize = 1u << 14;

// n / d for every n < 2^30 as one 64-bit product and a shift.  With L = ceil(log2 d), k = 30 + L and m = floor(2^k / d) + 1:
// m * d = 2^k + e with 0 < e <= d <= 2^L, so n * m / 2^k = n / d + n * e / (d * 2^k) with n * e < 2^30 * 2^L = 2^k - the excess is
// below 1 / d and the floor is that of n / d.  m <= 2^31 + 1 (d > 2^(L-1)), so n * m < 2^62.  The divisors of a call are W, 2W and
// 2H, the same for every pixel: the host makes the three pairs once, a lane spends a multiply instead of a division.
struct UpsampleDiv {
    uint32_t m, k;
};
PT_HD uint32_t upsample_div(uint32_t n, UpsampleDiv d) { return (uint32_t)(((uint64_t)n * d.m) >> d.k); }
inline UpsampleDiv upsample_div_make(uint32_t d) {  // 1 <= d <= 2^15
    uint32_t L = 0;
    while ((1u << L) < d) ++L;
    const uint32_t k = 30u + L;
    return {(uint32_t)((1ull << k) / d) + 1u, k};
}

// The call's whole frames.  Host pointers on the host, device pointers on the device.
struct UpsampleFrame {
    uint32_t width, height, lo_width, lo_height;
    const float *lo_color, *lo_depth, *lo_normal, *lo_albedo;  // lo_normal / lo_albedo NULL unless BOTH normals / albedos are given
    const int32_t *lo_object_id;
    const float *depth, *normal, *albedo;  // normal / albedo NULL likewise
    const int32_t *object_id;
    float *out_color, *out_weight;  // out_weight may be NULL
    float depth_tol, normal_min;    // defaults filled in
    UpsampleDiv div_w, div_2w, div_2h;
};

// step 1 for one coordinate of one axis: a = (2 * coord + 1) * lo + size; first = (int)(a / (2 * size)) - 1; frac =
// (float)(a % (2 * size)) / (float)(2 * size).  `by` divides by 2 * size.
PT_HD void upsample_tap(uint32_t size, uint32_t lo, UpsampleDiv by, uint32_t coord, int32_t &first, float &frac) {
    const uint32_t a = (2u * coord + 1u) * lo + size, d = 2u * size;
    const uint32_t q = upsample_div(a, by);
    first = (int32_t)q - 1;
    frac = (float)(a - q * d) / (float)d;
}

// m_c(.): pt_ctx_denoise's demodulation factor of one channel
PT_HD float upsample_demod(float albedo) { return albedo > 0.015625f ? albedo : 1.0f; }

// Steps 1 to 5 for frame pixel idx (< width * height): the colour, and the sum of the bilinear weights of the taps that passed (0
// where the fallback was used).  Written for the memory system, as reproject_gather is: the four taps are clamped into the
// low-resolution frame, so that everything they may need - guides, normals, albedos, colours - is read before the first is tested:
// one round trip.  A tap that fails its test has been read for nothing - its neighbours want the same lines - and adds nothing: the
// sums are the contract's, in its order.  The pixel's own guides are read once by one lane (reproject_own); a low-resolution pixel
// is read by about 4 * (W/w) * (H/h) lanes and stays on the default policy.  NORMALS and DEMOD say whether f holds both normal
// planes and both albedo planes: compile-time, so that no load waits behind a branch on a pointer.
template <bool NORMALS, bool DEMOD>
PT_HD void upsample_pixel_t(const UpsampleFrame &f, uint32_t idx, float out[3], float *weight) {
    const uint32_t r = upsample_div(idx, f.div_w), x = idx - r * f.width;
    int32_t x0, r0;
    float fx, fr;
    upsample_tap(f.width, f.lo_width, f.div_2w, x, x0, fx);
    upsample_tap(f.height, f.lo_height, f.div_2h, r, r0, fr);
    constexpr bool normals = NORMALS, demod = DEMOD;
    const size_t i3 = (size_t)idx * 3u;
    const int32_t id = reproject_own(f.object_id + idx);
    const float depth = reproject_own(f.depth + idx);
    float n[3] = {0.0f, 0.0f, 0.0f}, m[3] = {1.0f, 1.0f, 1.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (normals) n[c] = reproject_own(f.normal + i3 + c);
        if constexpr (demod) m[c] = reproject_own(f.albedo + i3 + c);
    }
    const int32_t xmax = (int32_t)f.lo_width - 1, rmax = (int32_t)f.lo_height - 1;
    uint32_t q[4];
    float b[4];
    bool inside[4];
#pragma unroll
    for (int32_t j = 0; j < 2; ++j) {
#pragma unroll
        for (int32_t i = 0; i < 2; ++i) {
            const int32_t qx = x0 + i, qr = r0 + j, t = j * 2 + i;
            inside[t] = qx >= 0 && qr >= 0 && qx <= xmax && qr <= rmax;
            const int32_t cx = qx < 0 ? 0 : (qx > xmax ? xmax : qx), cr = qr < 0 ? 0 : (qr > rmax ? rmax : qr);
            q[t] = (uint32_t)cr * f.lo_width + (uint32_t)cx;
            b[t] = (i ? fx : 1.0f - fx) * (j ? fr : 1.0f - fr);
        }
    }
    int32_t lid[4];
    float lz[4], lc[4][3], ln[4][3], la[4][3];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        lid[t] = f.lo_object_id[q[t]];
        lz[t] = f.lo_depth[q[t]];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const size_t q3 = (size_t)q[t] * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lc[t][c] = f.lo_color[q3 + c];
            if constexpr (normals) ln[t][c] = f.lo_normal[q3 + c];
            if constexpr (demod) la[t][c] = f.lo_albedo[q3 + c];
        }
    }
    // m(idx); u_q = lo_color[q] / m^lo(q)
    if constexpr (demod) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = upsample_demod(m[c]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int c = 0; c < 3; ++c) lc[t][c] = lc[t][c] / upsample_demod(la[t][c]);
        }
    }
    vec3 N = mk(0.0f, 0.0f, 0.0f);
    if constexpr (normals) N = reproject_normal(n);
    float s[3] = {0.0f, 0.0f, 0.0f}, bsum = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        bool take = inside[t] && lid[t] == id;
        if (id >= 0) {
            const float zm = depth > lz[t] ? depth : lz[t];
            take = take && __builtin_fabsf(depth - lz[t]) <= f.depth_tol * zm;
            if constexpr (normals) take = take && dot(N, reproject_normal(ln[t])) >= f.normal_min;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = take ? s[c] + lc[t][c] * b[t] : s[c];
        bsum = take ? bsum + b[t] : bsum;
    }
    *weight = bsum;
    if (!(bsum > 0.0f)) {  // the fallback: every tap inside the low-resolution frame; its bsum is > 0 (step 1)
        s[0] = s[1] = s[2] = bsum = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = inside[t] ? s[c] + lc[t][c] * b[t] : s[c];
            bsum = inside[t] ? bsum + b[t] : bsum;
        }
        *weight = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (s[c] / bsum) * m[c];
        out[c] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    }
}

// the pixel for whatever planes f holds
PT_HD void upsample_pixel(const UpsampleFrame &f, uint32_t idx, float out[3], float *weight) {
    if (f.normal)
        f.albedo ? upsample_pixel_t<true, true>(f, idx, out, weight) : upsample_pixel_t<true, false>(f, idx, out, weight);
    else
        f.albedo ? upsample_pixel_t<false, true>(f, idx, out, weight) : upsample_pixel_t<false, false>(f, idx, out, weight);
}

namespace host {
// pt_ctx_upsample's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call with the defaults and
// the divisions filled in.  No device is touched.
int check_upsample(const void *ctx, uint32_t width, uint32_t height, uint32_t lo_width, uint32_t lo_height,
                   const pt_upsample_params *params, const float *d_lo_color, const float *d_lo_depth, const int32_t *d_lo_object_id,
                   const float *d_lo_normal, const float *d_lo_albedo, const float *d_depth, const int32_t *d_object_id,
                   const float *d_normal, const float *d_albedo, float *d_out_color, float *d_out_weight, UpsampleFrame &f);
}  // namespace host

#if defined(__HIPCC__)
// one lane per frame pixel
void launch_upsample(hipStream_t st, const UpsampleFrame &f);
#endif

}  // namespace pt
