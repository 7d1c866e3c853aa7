/* ptrace_despike.h — fireflies clipped before the denoiser: pt_ctx_despike.  C ABI of libptrace_hip.so. */
#ifndef PTRACE_DESPIKE_H
#define PTRACE_DESPIKE_H

#include "ptrace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the firefly stage: a pixel far brighter than its neighbourhood is scaled down to a limit the neighbourhood sets ----------
 * A header of its own beside ptrace.h, which it includes, for the reason ptrace_tone.h is one: tests/test_abi.py holds ptrace.h
 * and abi.py to 22 structs, tests/test_streams_abi.py holds every hip_stream prototype of ptrace.h to a table of cases, and this
 * stage adds two structs and one such prototype without changing either.  The symbols are libptrace_hip.so's like all others
 * (PT_ABI_VERSION stays 5: symbols are only added); path-tracer-rust_amd/despike_abi.py describes this header to Python.
 *
 * The frame pt_ctx_accum_hdr hands out is not clamped: one sample that found the lamp through the glass sphere leaves a pixel at
 * 30 or 300 where the clamped resolve left it at 1.  pt_ctx_denoise weighs colours by absolute difference and keeps such a pixel
 * as a dot or smears it, pt_ctx_meter reports it as max_luminance.  This pass stands in front of them:
 *   accumulate -> accum_hdr -> despike -> [denoise] -> meter -> tonemap -> overlay -> present.
 *
 * pt_ctx_despike: a float frame to a float frame, 3 floats per pixel each, framebuffer order, width * height pixels.
 * - `hip_stream` obeys the paragraph of ptrace.h that begins "`hip_stream` is a hipStream_t": NULL is the context's own stream;
 *   the clear, the kernel and the copy of the call are ordered on that stream, behind what the caller queued there, and
 *   everything is complete when the call returns.  Blocking.  No scene is needed.  The call changes no state of the context but
 *   its own scratch, 16 bytes of counters, which grows on demand, is freed by pt_ctx_destroy and is shared with nothing.  Every
 *   refusal is made before any device is touched and leaves every output as it was.
 * - Every field of pt_despike_params is taken as it stands: there is no "0 = default".  params == NULL stands for the defaults.
 * - d_out may NOT be d_rgb: the pass gathers, a pixel reads its neighbours' source values.  Equal pointers are refused; any other
 *   overlap is the caller's error.
 * - d_object_id (may be NULL without the flag): width * height int32, read only with PT_DESPIKE_SAME_OBJECT.
 * - d_mask (may be NULL): width * height bytes in pixel order, one per pixel: 0 copied, 1 a spike that was scaled down, 2 a
 *   non-finite pixel written as 0.  Zero or not is the convention pt_ctx_render_masked and pt_ctx_spp_plane read, so a host can
 *   retrace the spikes with more samples (that loop is not part of this stage).
 * - out (host, may be NULL): pixels = width * height, spikes = the pixels with mask 1, nonfinite = those with mask 2.  Integer
 *   counts: they do not depend on the order in which lanes run.  With out == NULL the call clears, counts and downloads nothing.
 * THE ARITHMETIC.  pt_ctx_tonemap's rules: IEEE binary32 * + /, correctly rounded, never contracted, in the order the parentheses
 * give.
 *   Y(p) = (0.2126f*r + 0.7152f*g) + 0.0722f*b          (pt_ctx_meter's coefficients and order)
 *   A pixel is NON-FINITE if a channel has all exponent bits set: (bits & 0x7f800000) == 0x7f800000.
 *   A neighbour q of p is VALID if it lies within `radius` of p in both axes and is not p, lies inside the frame, is not
 *   non-finite and, with PT_DESPIKE_SAME_OBJECT, id(q) == id(p).  Its luminance is y(q) = Y(q) > 0 ? Y(q) : 0.
 *   m = the number of valid neighbours.  R = the rank-th LARGEST of their y; equal values count separately: R is element rank-1
 *   of the descending sort.  The limit is L = (threshold * R) + floor.
 *   Per pixel, in this order:
 *   1. p is non-finite: out = (+0, +0, +0), mask 2, counted in `nonfinite`.
 *   2. m < rank: out has p's bits, mask 0.
 *   3. Y(p) > L: s = L / Y(p), out_c = rgb_c * s, mask 1, counted in `spikes`.
 *   4. otherwise out has p's bits exactly (a -0 stays -0), mask 0.
 * What follows from it:
 * - A 1x1 frame is copied (m = 0).  A pixel on an edge or in a corner has fewer neighbours, never other ones.
 * - A pixel with Y <= floor is never a spike: L >= floor, because threshold * R >= 0 and the sum is rounded monotonically.
 * - With rank 2 two touching fireflies are both clipped (each sees the other as the largest and the background as the second),
 *   and a one-pixel-wide bright line survives except at its ends: an inner pixel of it has two bright neighbours.  With rank 1
 *   a touching pair survives.
 * - R = +inf makes L = +inf, so nothing is clipped: a finite pixel whose luminance overflows shields its neighbours.
 * - A spike keeps its colour ratios and lands on luminance L to the rounding of the products.
 * - PT_ERR_INVALID, in this order: a radius that is not 1 or 2; a rank that is 0, above 4 or above the neighbour count
 *   (2*radius+1)^2 - 1; unknown flag bits; a threshold that is not finite or below 1; a floor that is not finite or negative;
 *   width or height 0; width * height above 2^28; NULL d_rgb; NULL d_out; d_out == d_rgb; PT_DESPIKE_SAME_OBJECT with a NULL
 *   d_object_id; NULL ctx.  PT_ERR_HIP: a HIP call failed.
 * - pt_despike_defaults: radius 1, rank 3, no flags, threshold 2, floor 0.25: the setting tools/despike_study.py chose
 *   (profiles/despike_study.json, "chosen": the smallest mean RMSE ratio with pt_ctx_denoise behind the pass, over radius {1, 2} x
 *   rank {1, 2, 3} x threshold {2, 4, 8, 16} x floor {0.25, 1, 4} x the flag, on cornell and mesh.json at 8, 64 and 256 samples).
 *   The gain there is 0.2 %: on those frames the pass hardly pays, and DESIGN.md, "The firefly stage", says so.  The values the
 *   stage started from (radius 1, rank 2, threshold 4, floor 1) clip nothing on them.
 * - pt_despike_frame_host is the host instantiation of the same per-pixel source the kernel compiles (csrc/pt_despike.h) for a
 *   whole frame in host memory; it refuses what pt_ctx_despike refuses about its own arguments (everything but the ctx), in that
 *   order, with rgb, out_rgb, object_id, mask and out in the places of the device pointers. */
#define PT_DESPIKE_SAME_OBJECT 1u   /* flags: only neighbours with the centre's object id count; needs d_object_id */
typedef struct pt_despike_params {   /* every field is taken as it stands - no "0 = default" */
    uint32_t radius;                 /* 1 or 2: the window is (2*radius+1)^2, the centre excluded */
    uint32_t rank;                   /* 1..4: the reference is the rank-th LARGEST luminance among the valid neighbours */
    uint32_t flags;
    float threshold;                 /* finite, >= 1 */
    float floor;                     /* finite, >= 0, in the frame's radiance units */
} pt_despike_params;
typedef struct pt_despike_stats {
    uint64_t pixels;                 /* width * height */
    uint64_t spikes;                 /* pixels that were scaled down */
    uint64_t nonfinite;              /* pixels with a NaN or infinite channel, written as 0 */
} pt_despike_stats;

int pt_despike_defaults(pt_despike_params *out);
int pt_ctx_despike(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_despike_params *params /* NULL = the defaults */,
                   const float *d_rgb, const int32_t *d_object_id /* may be NULL */, float *d_out,
                   uint8_t *d_mask /* may be NULL */, pt_despike_stats *out /* host, may be NULL */, void *hip_stream);
int pt_despike_frame_host(uint32_t width, uint32_t height, const pt_despike_params *params, const float *rgb,
                          const int32_t *object_id, float *out_rgb, uint8_t *mask, pt_despike_stats *out); /* host only */

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_DESPIKE_H */
