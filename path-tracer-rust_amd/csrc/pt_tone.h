// pt_tone.h — the tone stage (pt_tone.hip): pt_ctx_accum_hdr, the held frame resolved without the clamp; pt_ctx_meter, a luminance
// histogram of a float frame; pt_ctx_tonemap, exposure and a curve into [0, 1].  The arithmetic is the contract in
// include/ptrace_tone.h, operation for operation.  What happens to one value - the luminance, the meter's bin, the curve, a
// tonemapped pixel, the resolve of one sum - is stated once, below, for host and device: pt_meter_bin_host and
// pt_tonemap_pixel_host (host/scene_io.cpp) are the host instantiations of the source the kernels compile, as pt_solid_pixel_host
// is of pt_solid.h.  A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace_tone.h"
#include "pt_math.h"

namespace pt {

// what a NULL params stands for and the pt_*_defaults write out
constexpr pt_tonemap_params kTonemapDefaults = {PT_TONE_ACES, 0u, 1.0f, 4.0f};
constexpr pt_meter_exposure_params kMeterExposureDefaults = {0.18f, 0.05f, 0.02f, 0.00390625f, 256.0f};
// the kernels' units: a workgroup of 256 lanes (four waves); in the wide forms a lane owns four consecutive pixels
constexpr uint32_t kToneBlock = 256u, kToneLanePixels = 4u;
// the meter's bins: k = bits(Y) >> 20 from kMeterKLo (2^-20) to kMeterKHi (the last eighth of an octave below 2^12)
constexpr uint32_t kMeterKLo = 856u, kMeterKHi = 1111u;
// the meter's counters on the device and a wave's row of them in LDS: the bins, then the dark pixels, then the maximum's bits
constexpr uint32_t kMeterDark = PT_METER_BINS, kMeterMax = PT_METER_BINS + 1u, kMeterWords = PT_METER_BINS + 4u;
constexpr uint32_t kMeterMaxBlocks = 2048u;  // the meter's grid is capped: a workgroup walks the frame and flushes once

PT_HD uint32_t tone_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
PT_HD float tone_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the meter's slot for one luminance: a bin, or kMeterDark for !(Y > 0) (a NaN among them) and Y < 2^-20
PT_HD uint32_t meter_slot(float Y) {
    if (!(Y > 0.0f) || Y < 9.5367431640625e-07f) return kMeterDark;
    const uint32_t k = tone_bits(Y) >> 20;
    return (k < kMeterKHi ? k : kMeterKHi) - kMeterKLo;
}
// what max_luminance takes the integer maximum of: the bits of a Y > 0 (not NaN), else 0
PT_HD uint32_t meter_max_bits(float Y) { return Y > 0.0f ? tone_bits(Y) : 0u; }

PT_HD float tone_clamp01(float v) { return v > 0.0f ? (v > 1.0f ? 1.0f : v) : 0.0f; }  // a NaN gives 0
// x = v * exposure, held to [0, 2^32]: NaN and -0 give +0, +inf gives 2^32
PT_HD float tone_expose(float v, float exposure) {
    const float x = v * exposure;
    return x > 0.0f ? (x > 4294967296.0f ? 4294967296.0f : x) : 0.0f;
}
// f(x); `curve` is the same for every value of a call (a uniform branch on the device).  iw2 = 1 / (white * white)
PT_HD float tone_curve(uint32_t curve, float iw2, float x) {
    if (curve == PT_TONE_REINHARD) return (x * (1.0f + x * iw2)) / (1.0f + x);
    if (curve == PT_TONE_ACES) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return x;
}

// The call once it has passed: a kernel argument as it stands.
struct ToneFrame {
    uint32_t width, height;
    const float *rgb;
    float *out;  // may be rgb
    uint32_t curve;
    bool luma;
    float exposure, iw2;
};

// one pixel of pt_ctx_tonemap but for the loads and the stores
PT_HD void tone_pixel(const ToneFrame &f, const float v[3], float out[3]) {
    const float x[3] = {tone_expose(v[0], f.exposure), tone_expose(v[1], f.exposure), tone_expose(v[2], f.exposure)};
    if (f.luma) {
        const float Y = tone_luma(x[0], x[1], x[2]);
        const float s = Y > 0.0f ? tone_curve(f.curve, f.iw2, Y) / Y : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = tone_clamp01(x[c] * s);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = tone_clamp01(tone_curve(f.curve, f.iw2, x[c]));
    }
}

// pt_ctx_accum_hdr's value: k_resolve's conversion of a 32.32 sum over n samples, without the clamp; n = 0 gives 0
PT_HD float hdr_value(unsigned long long S, uint32_t n) {
    const double sum = (double)S * (1.0 / 4294967296.0);
    return n ? (float)sum / (float)n : 0.0f;
}

// pt_ctx_meter once it has passed.  The pixels looked at are `rows` runs of `span` consecutive pixels, the r-th from pixel
// first + r * pitch: a rectangle's rows, or ONE run for a rectangle as wide as the frame (the whole frame among them).
struct MeterFrame {
    const float *rgb;
    const int32_t *object_id;  // NULL: no pixel is skipped
    uint32_t npix;             // of the frame: no access goes to a pixel at or beyond it
    uint32_t first, span, pitch, rows;
    uint32_t row_groups;  // groups of four aligned pixels a run can touch: (span + 3) / 4 + 1
    uint32_t *counters;   // kMeterWords on the device, cleared before the launch
};

// pt_ctx_accum_hdr once it has passed: the held planes, [3] of `total` u64, and each pixel's count by its part
struct HdrFrame {
    const unsigned long long *sums;
    float *out;
    uint32_t total, part_px;
    uint32_t count;          // with counts == NULL (one part): every pixel's
    const uint32_t *counts;  // on the device, one per part
};

namespace host {
// pt_ctx_tonemap's refusals about params alone, in the header's order (its first four); PT_OK: f holds curve, luma, exposure, iw2
int check_tonemap_params(const pt_tonemap_params *params, ToneFrame &f);
// pt_ctx_tonemap's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call.  No device is touched.
int check_tonemap(const void *ctx, uint32_t width, uint32_t height, const pt_tonemap_params *params, const float *d_rgb, float *d_out,
                  ToneFrame &f);
// pt_ctx_meter's likewise; f.counters is the caller's to fill in
int check_meter(const void *ctx, uint32_t width, uint32_t height, const pt_meter_params *params, const float *d_rgb,
                const int32_t *d_object_id, const pt_meter_stats *out, MeterFrame &f);
// pt_meter_exposure's refusals about params; PT_OK: P holds them, the defaults for a NULL
int check_meter_exposure(const pt_meter_exposure_params *params, pt_meter_exposure_params &P);
// kept[b] of the header, and the two sums
void meter_weights(const pt_meter_stats &s, const pt_meter_exposure_params &P, double kept[PT_METER_BINS], double *sum_w, double *sum_wl);
// the wide forms are valid: every plane handed over is 16-byte aligned (the held planes: each of the three) and there is a whole
// group of four pixels
bool tone_wide(const ToneFrame &f);
bool meter_wide(const MeterFrame &f);
bool hdr_wide(const HdrFrame &f);
// the counters as the device left them into *out
void meter_stats_of(const uint32_t counters[kMeterWords], pt_meter_stats *out);
}  // namespace host

#if defined(__HIPCC__)
// one lane per four consecutive pixels, then one per pixel of the rest; one lane per pixel throughout where !tone_wide(f)
void launch_tonemap(hipStream_t st, const ToneFrame &f);
void launch_hdr(hipStream_t st, const HdrFrame &f);
// adds the frame's pixels to f.counters; a capped grid of workgroups, each with a histogram per wave in LDS
void launch_meter(hipStream_t st, const MeterFrame &f);
#endif

}  // namespace pt
