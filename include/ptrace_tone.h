/* ptrace_tone.h — radiance above 1: pt_ctx_accum_hdr, pt_ctx_meter, pt_ctx_tonemap.  C ABI of libptrace_hip.so. */
#ifndef PTRACE_TONE_H
#define PTRACE_TONE_H

#include "ptrace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the tone stage: the held frame without the clamp, a luminance histogram, exposure and a curve ---------------------
 * A header of its own beside ptrace.h, which it includes, for the reason ptrace_solid.h is one: tests/test_abi.py holds ptrace.h
 * and abi.py to 22 structs, tests/test_streams_abi.py holds every hip_stream prototype of ptrace.h to a table of cases, and this
 * stage adds four structs and three such prototypes without changing either.  The symbols are libptrace_hip.so's like all
 * others (PT_ABI_VERSION stays 5: symbols are only added); path-tracer-rust_amd/tone_abi.py describes this header to Python.
 *
 * Every frame the other calls hand out is clamped to [0, 1] at resolve ("THE SUMS" of ptrace.h), so an exposure below 1 turns a
 * lamp flat grey instead of showing what was there.  The held sums of pt_ctx_accumulate are not clamped; this stage reads them
 * and maps radiance to display range by a curve:  accumulate -> accum_hdr -> [denoise] -> meter -> tonemap -> overlay -> present.
 * What denoising an unclamped frame does to the filters' defaults (their sigmas were chosen on clamped frames) is not studied.
 *
 * All three device calls: `hip_stream` obeys the paragraph of ptrace.h that begins "`hip_stream` is a hipStream_t": NULL is the
 * context's own stream; the copies, clears and kernels of the call are ordered on that stream, behind what the caller queued
 * there, and everything is complete when the call returns.  Blocking.  No scene is needed, except that pt_ctx_accum_hdr needs
 * the held frame.  A call changes no state of the context but its own scratch (a table of per-part counts; the meter's 1040 B of
 * counters), which grows on demand, is freed by pt_ctx_destroy and is shared with nothing.  Every refusal is made before any
 * device is touched and leaves every output as it was.
 *
 * 1. pt_ctx_accum_hdr: the frame pt_ctx_accumulate holds, resolved without the clamp.
 * - `cfg` names the held frame as for pt_ctx_accum_info: only its key matters (size, band, chunks, seed), not spp or backend.
 * - d_out_rgb: device memory laid out as pt_ctx_accumulate lays its output out (band and chunks included): 3 floats per pixel
 *   the call owns.
 * - Value: with S the pixel channel's u64 sum and n the samples its PART holds (parts as pt_ctx_accum_info counts them),
 *   (float)((double)S * 2^-32) / (float)n: the u64 goes to binary64 (round to nearest even), the product is exact, one rounding
 *   to binary32, one correctly rounded binary32 division.  That is pt_ctx_accumulate's resolve with the clamp left off; n = 0
 *   gives 0.  So clamping the result to [0, 1] (v < 0 ? 0 : v > 1 ? 1 : v) gives pt_ctx_accumulate's frame bit for bit.
 * - It reads the held sums and writes nothing else: not the counts, not the sums of half A.
 * - The frame pt_ctx_accumulate_adaptive holds (pt_ctx_adaptive_resolve) is out of scope: there is no unclamped resolve of it.
 * - PT_ERR_INVALID, in this order: NULL ctx, cfg or d_out_rgb; a cfg pt_ctx_accum_info refuses; a cfg that does not name the
 *   held frame, or no held frame.  PT_ERR_HIP: a HIP call failed.
 *
 * 2. pt_ctx_meter: a luminance histogram of a float frame (3 floats per pixel, framebuffer order, width * height pixels).
 * - Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b in binary32, every operation rounded, none contracted.
 * - A pixel is DARK if !(Y > 0) or Y < 2^-20: NaN, +-0, negatives, denormals.  It is counted in `dark` and in no bin.
 * - Otherwise k = bits(Y) >> 20 (exponent and three mantissa bits) and bin = min(k, 1111) - 856: 256 bins, eight per octave,
 *   from 2^-20 to 2^12; the last bin takes everything above, +inf included.  (The scheme of pt_noise_stats.histogram.)
 * - params->flags: with PT_METER_SKIP_MISSES a pixel whose d_object_id is below 0 is not looked at.
 * - params->x0, y0, x1, y1: a half-open rectangle in framebuffer coordinates (x = idx % width, y = idx / width); all four 0
 *   stand for the whole frame.  Only its pixels are looked at, and only its rows are read.
 * - pt_meter_stats: pixels = looked at; dark; histogram; max_luminance = the largest Y > 0 seen (not NaN; dark ones and +inf
 *   count), taken as the integer maximum of the bit patterns; 0 when there is none.  pixels = dark + the histogram's sum.
 *   Integer counts and an integer maximum: the result does not depend on the order in which lanes run.
 * - PT_ERR_INVALID, in this order: unknown flag bits; width or height 0; width * height above 2^28; a rectangle that is not all
 *   zero and is empty (x0 >= x1 or y0 >= y1) or leaves the frame (x1 > width or y1 > height); NULL d_rgb;
 *   PT_METER_SKIP_MISSES with a NULL d_object_id; NULL out; NULL ctx.  PT_ERR_HIP: a HIP call failed.
 * Host only, no device needed:
 * - pt_meter_bin_host(Y, &bin): the bin of one luminance, -1 for dark; compiled from the kernel's source.
 * - pt_meter_exposure(stats, params, &exposure), params NULL = the defaults.  Arithmetic in binary64.  N = the histogram's sum
 *   (an integer), lo = low_fraction * N, hi = N - high_fraction * N, each product and the difference rounded once.  For bin b in
 *   ascending order, with c the sum of the bins below it: kept_b = max(0, min(c + h_b, hi) - max(c, lo)) - the darkest
 *   low_fraction and the brightest high_fraction of the counted pixels are dropped, and a bin cut by a limit contributes the part
 *   of its count that is kept.  L = exp2(sum_b kept_b * (-20 + (b + 0.5) / 8) / sum_b kept_b), both sums in ascending order;
 *   exposure = key / L, clamped to [min_exposure, max_exposure], rounded to binary32.  N = 0: exposure = 1 (not clamped).
 *   The weights are exact (pt_meter_exposure_weights hands them out); the value goes through the host's exp2 and is stated to
 *   2 ulp of binary32, no tighter.  PT_ERR_INVALID, in this order: NULL stats or exposure; a key that is not finite and > 0; a
 *   fraction outside [0, 1) or not a number; low_fraction + high_fraction >= 1; a min_exposure that is not finite and > 0; a
 *   max_exposure that is not finite or is below min_exposure.
 * - pt_meter_exposure_defaults: key 0.18, low_fraction 0.05, high_fraction 0.02, range [2^-8, 2^8].
 * - pt_meter_adapt(current, target, dt, tau, &next): eye adaptation in log2 exposure, binary64 inside:
 *   next = current * 2^((log2 target - log2 current) * (1 - exp(-dt / tau))), rounded to binary32; tau == 0 gives the target
 *   itself.  PT_ERR_INVALID, in this order: NULL next; a current or target that is not finite and > 0; a dt or tau that is
 *   negative or not finite.
 *
 * 3. pt_ctx_tonemap: exposure and a curve, a float frame to a float frame in [0, 1] (3 floats per pixel each).
 * - d_out may be d_rgb (a pixel reads its own value before it writes and gathers nothing).  It may overlap it in no other way.
 * - The output is display-linear: pt_ctx_overlay and pt_ctx_present take it from there, present's gamma table is untouched.
 * - Every field of pt_tonemap_params is taken as it stands: there is no "0 = default".  params == NULL stands for the defaults.
 * THE ARITHMETIC.  All operations are IEEE binary32 + - * /, correctly rounded, never contracted, in the order the parentheses
 * give; the divisions are the compiler's correctly rounded ones.  clamp01(v) = v > 0 ? (v > 1 ? 1 : v) : 0, so a NaN gives 0.
 *   Per value v:  x = v * exposure;  x = x > 0 ? (x > 2^32 ? 2^32 : x) : 0.  NaN and -0 give +0, +inf gives 2^32.
 *   PT_TONE_CLAMP:    f(x) = x
 *   PT_TONE_REINHARD: f(x) = (x * (1 + x * iw2)) / (1 + x),  iw2 = 1 / (white * white) made on the host in binary32
 *   PT_TONE_ACES:     f(x) = (x * (2.51f*x + 0.03f)) / (x * (2.43f*x + 0.59f) + 0.14f)      (Narkowicz's fit)
 *   Without PT_TONE_LUMA: out_c = clamp01(f(x_c)).
 *   With PT_TONE_LUMA: Y = (0.2126f*x_r + 0.7152f*x_g) + 0.0722f*x_b;  s = Y > 0 ? f(Y) / Y : 0;  out_c = clamp01(x_c * s).
 * PT_TONE_CLAMP without the flag at exposure e IS steps 2 and 3 of pt_ctx_present's arithmetic at that exposure: presenting the
 * tonemapped frame at exposure 1 gives the bytes presenting the source at exposure e gives.
 * - PT_ERR_INVALID, in this order: a curve above PT_TONE_ACES; unknown flag bits; an exposure that is not finite and > 0; with
 *   PT_TONE_REINHARD a white that is not finite and > 0; width or height 0; width * height above 2^28; NULL d_rgb; NULL d_out;
 *   NULL ctx.  PT_ERR_HIP: a HIP call failed.
 * - pt_tonemap_defaults: PT_TONE_ACES, no flags, exposure 1, white 4.  pt_tonemap_pixel_host is the host instantiation of the
 *   arithmetic for one pixel, from the source the kernel compiles (csrc/pt_tone.h); it refuses what pt_ctx_tonemap refuses about
 *   params, and a NULL rgb or out. */
#define PT_METER_SKIP_MISSES 1u   /* flags: pixels whose object id is below 0 are not looked at */
#define PT_METER_BINS 256u
typedef struct pt_meter_params {
    uint32_t flags;
    uint32_t x0, y0, x1, y1;              /* half open, framebuffer coordinates; all zero = the whole frame */
} pt_meter_params;
typedef struct pt_meter_stats {
    uint64_t pixels;                      /* looked at */
    uint64_t dark;                        /* of them: !(Y > 0) or Y < 2^-20 */
    uint32_t histogram[PT_METER_BINS];    /* the others, eight bins per octave from 2^-20 */
    float max_luminance;                  /* the largest Y > 0 seen; 0: none */
} pt_meter_stats;
typedef struct pt_meter_exposure_params {
    float key;                            /* the luminance the kept pixels' log-average is mapped to */
    float low_fraction, high_fraction;    /* the darkest / brightest share of the counted pixels that is dropped */
    float min_exposure, max_exposure;
} pt_meter_exposure_params;

#define PT_TONE_CLAMP    0u
#define PT_TONE_REINHARD 1u
#define PT_TONE_ACES     2u
#define PT_TONE_LUMA     1u   /* flags: the curve acts on the luminance, the colour keeps its ratios */
typedef struct pt_tonemap_params {        /* every field is taken as it stands - no "0 = default" */
    uint32_t curve;                       /* PT_TONE_* */
    uint32_t flags;
    float exposure;                       /* finite, > 0 */
    float white;                          /* finite, > 0; read only by PT_TONE_REINHARD: the x that maps to 1 */
} pt_tonemap_params;

int pt_ctx_accum_hdr(pt_ctx *ctx, const pt_config *cfg, float *d_out_rgb, void *hip_stream);

int pt_ctx_meter(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_meter_params *params /* NULL = no flags, whole frame */,
                 const float *d_rgb, const int32_t *d_object_id /* may be NULL */, pt_meter_stats *out, void *hip_stream);
int pt_meter_bin_host(float Y, int32_t *bin);                                                      /* host only */
int pt_meter_exposure_defaults(pt_meter_exposure_params *out);
int pt_meter_exposure(const pt_meter_stats *stats, const pt_meter_exposure_params *params /* NULL = the defaults */,
                      float *exposure);                                                            /* host only */
int pt_meter_exposure_weights(const pt_meter_stats *stats, const pt_meter_exposure_params *params /* NULL = the defaults */,
                              double kept[PT_METER_BINS]);                                         /* host only */
int pt_meter_adapt(float current, float target, float dt, float tau, float *next);                 /* host only */

int pt_tonemap_defaults(pt_tonemap_params *out);
int pt_ctx_tonemap(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_tonemap_params *params /* NULL = the defaults */,
                   const float *d_rgb, float *d_out, void *hip_stream);
int pt_tonemap_pixel_host(const pt_tonemap_params *params /* NULL = the defaults */, const float rgb[3], float out[3]); /* host only */

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_TONE_H */
