// pt_denoise.h — the edge-avoiding a-trous filter behind pt_ctx_denoise (pt_denoise.hip): prepare packs the guides and the
// demodulated colour, one launch per level ping-pongs the colour plane, the last level multiplies the albedo back and clamps.
// The arithmetic is the contract in include/ptrace.h, operation for operation.  A translation unit of its own: pt_kernels.s,
// and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ptrace.h"

namespace pt {

// the values a zero field of pt_denoise_params / pt_denoise_var_params stands for: the minima of the CPU studies
// (profiles/denoise_cpu_study.json, profiles/denoise_var_cpu_study.json)
constexpr pt_denoise_params kDenoiseDefaults = {5u, 2.0f, 0.0f, 0.03125f, 0u};
constexpr pt_denoise_var_params kDenoiseVarDefaults = {5u, 1.0f, 0.125f, 0u};
constexpr uint32_t kDenoiseMaxLevels = 8u;

struct DenoiseFrame {
    uint32_t width, height;
    const float *color, *albedo, *normal, *depth;  // albedo: NULL also under PT_DENOISE_NO_DEMODULATE
    const float *error;                            // pt_ctx_denoise_var's noise estimate per pixel; NULL selects pt_ctx_denoise
    float4 *guide;                                 // (N.xyz, depth) per pixel; depth 0 without a depth buffer (every pixel a hit)
    float4 *u[2];                                  // the colour planes, (r, g, b, V); V is 0 and unread without `error`
    float *out;
};

// u[0] and guide from the caller's buffers; with `error` also V_0 into u[0].w (Vraw through u[1].w, then one 3x3 launch)
void launch_dn_prepare(hipStream_t st, const DenoiseFrame &f);
// level i: u[i & 1] -> u[(i + 1) & 1], or -> f.out (times m, clamped) when `last`.  rc = 1 / sc_i^2, sds = sigma_depth * 2^i
// (host binary32).  lds: the workgroup stages its taps in LDS (any step: the tile is dense in x up to step 4, a lattice of
// the step beyond, and always a lattice in y); otherwise every tap is a global load.  Same results.
// With `error`, rc is kv = sigma_var^2 and each pixel scales its colour term by 1 / (kv * V(p) + 2^-20); V goes on to the
// next plane as sum(V(q) w^2) / wsum^2.
void launch_dn_level(hipStream_t st, const DenoiseFrame &f, uint32_t i, float rc, float sds, bool last, bool lds);

// A checked call of either filter: the frame, and per level i < levels the rc and sds launch_dn_level receives - host binary32,
// sc_i = sigma * 2^-i with 2^-i as the running product of 0.5f, rc = 1 / (sc_i * sc_i) or, with an error map, kv = sigma * sigma
// at every level; sds = sigma_depth * (float)(1 << i).
struct DenoiseCall {
    DenoiseFrame f;
    uint32_t levels;
    float rc[kDenoiseMaxLevels], sds[kDenoiseMaxLevels];
};

namespace host {
// pt_ctx_denoise's and pt_ctx_denoise_var's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `call` holds the
// call with the defaults filled in, but for f.guide and f.u[], which the caller owns.  No device is touched.
int check_denoise(const void *ctx, uint32_t width, uint32_t height, const pt_denoise_params *params, const float *d_color,
                  const float *d_albedo, const float *d_normal, const float *d_depth, float *d_out, DenoiseCall &call);
int check_denoise_var(const void *ctx, uint32_t width, uint32_t height, const pt_denoise_var_params *params, const float *d_color,
                      const float *d_error, const float *d_albedo, const float *d_normal, const float *d_depth, float *d_out,
                      DenoiseCall &call);
}  // namespace host

}  // namespace pt
