// pt_despike.h — the firefly stage (pt_despike.hip): pt_ctx_despike scales a pixel far brighter than its neighbourhood down to a
// limit the neighbourhood sets.  The arithmetic is the contract in include/ptrace_despike.h, operation for operation.  What
// happens to one value - a neighbour's luminance or its marker, one step of the running top-`rank`, the centre's verdict - is
// stated once, below, for host and device: pt_despike_frame_host (host/scene_io.cpp) is the host instantiation of the source the
// kernel compiles, as pt_tonemap_pixel_host is of pt_tone.h.  A translation unit of its own: pt_kernels.s, and so
// pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace_despike.h"
#include "pt_math.h"

namespace pt {

// what a NULL params stands for and pt_despike_defaults writes out: the grid's minimum in profiles/despike_study.json ("chosen")
constexpr pt_despike_params kDespikeDefaults = {1u, 3u, 0u, 2.0f, 0.25f};
constexpr uint32_t kDespikeMaxRadius = 2u, kDespikeMaxRank = 4u;
// the kernel's unit: a workgroup of 256 lanes (four waves) per tile of 32 x 8 pixels, one lane per pixel, a wave two rows
constexpr uint32_t kDespikeTileW = 32u, kDespikeTileH = 8u;
// the mask's values
constexpr uint32_t kDespikeCopied = 0u, kDespikeSpike = 1u, kDespikeNonfinite = 2u;
// what stands for a neighbour that does not count (outside the frame, non-finite, another object): below every y(q) >= 0
constexpr float kDespikeNone = -1.0f;

PT_HD uint32_t despike_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
PT_HD bool despike_nonfinite(float r, float g, float b) {
    return (despike_bits(r) & 0x7f800000u) == 0x7f800000u || (despike_bits(g) & 0x7f800000u) == 0x7f800000u ||
           (despike_bits(b) & 0x7f800000u) == 0x7f800000u;
}
PT_HD float despike_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// y(q) of a pixel inside the frame, or the marker for a non-finite one.  (Finite channels give no NaN: each product is finite.)
PT_HD float despike_y(float r, float g, float b) {
    if (despike_nonfinite(r, g, b)) return kDespikeNone;
    const float Y = despike_luma(r, g, b);
    return Y > 0.0f ? Y : 0.0f;
}

// One value into the running top-RANK: t[0] >= t[1] >= ... hold the RANK largest seen, kDespikeNone where fewer were seen.  A
// maximum and a minimum per register, no index that depends on a lane; v is never a NaN and never -0, so max and min are exact.
template <int RANK>
PT_HD void despike_push(float (&t)[RANK], float v) {
#pragma unroll
    for (int k = 0; k < RANK; ++k) {
        const float hi = __builtin_fmaxf(t[k], v);
        v = __builtin_fminf(t[k], v);
        t[k] = hi;
    }
}

// The call once it has passed: a kernel argument as it stands.
struct DespikeFrame {
    uint32_t width, height;
    const float *rgb;
    const int32_t *object_id;  // NULL without PT_DESPIKE_SAME_OBJECT
    float *out;                // never rgb
    uint8_t *mask;             // may be NULL
    unsigned long long *counters;  // [0] spikes, [1] non-finite: on the device, cleared before the launch; NULL: nothing is counted
    uint32_t radius, rank;
    float threshold, floor;
};

// Steps 2-4 of the contract for a pixel that is not non-finite: R = the rank-th largest y among the valid neighbours, or
// kDespikeNone where there are fewer (m < rank).  Returns the mask's value.
PT_HD uint32_t despike_verdict(float threshold, float floor, float R, const float v[3], float out[3]) {
    out[0] = v[0], out[1] = v[1], out[2] = v[2];
    if (R < 0.0f) return kDespikeCopied;
    const float L = (threshold * R) + floor;
    const float Y = despike_luma(v[0], v[1], v[2]);
    if (!(Y > L)) return kDespikeCopied;
    const float s = L / Y;
    out[0] = v[0] * s, out[1] = v[1] * s, out[2] = v[2] * s;
    return kDespikeSpike;
}

namespace host {
// pt_ctx_despike's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call but its counters.  No
// device is touched.  (pt_despike_frame_host has no context to refuse and hands over any non-NULL pointer.)
int check_despike(const void *ctx, uint32_t width, uint32_t height, const pt_despike_params *params, const float *d_rgb,
                  const int32_t *d_object_id, float *d_out, uint8_t *d_mask, DespikeFrame &f);
// the whole frame on the host, from the source above; counts[0] spikes, counts[1] non-finite
void despike_frame(const DespikeFrame &f, unsigned long long counts[2]);
}  // namespace host

#if defined(__HIPCC__)
// one workgroup per tile of kDespikeTileW x kDespikeTileH, a grid of one dimension
void launch_despike(hipStream_t st, const DespikeFrame &f);
#endif

}  // namespace pt
