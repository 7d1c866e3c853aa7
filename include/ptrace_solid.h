/* ptrace_solid.h — pt_ctx_solid: a lit solid view of the scene from the first-hit guides.  C ABI of libptrace_hip.so. */
#ifndef PTRACE_SOLID_H
#define PTRACE_SOLID_H

#include "ptrace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the solid view: ambient, diffuse and one highlight per pixel, from the guides alone --------------------------------
 * A header of its own beside ptrace.h, which it includes, for the reason ptrace_overlay.h is one: tests/test_abi.py holds
 * ptrace.h and abi.py to 22 structs, tests/test_streams_abi.py holds every hip_stream prototype of ptrace.h to a table of cases,
 * and this pass adds two structs and one such prototype without changing either.  The symbols are libptrace_hip.so's like all
 * others (PT_ABI_VERSION stays 5: symbols are only added); path-tracer-rust_amd/solid_abi.py describes this header to Python as
 * abi.py describes ptrace.h.
 *
 * pt_ctx_solid shades a whole frame without tracing a path: what the editing viewport shows while the user works on the scene
 * (src/views/viewport_tab.rs) - the objects lit and solid, by one light, times their colour - where pt_ctx_render shows the
 * path-traced picture.  Its inputs are the planes ONE sample of pt_ctx_render_aov writes, so a noise-free frame of what is being
 * dragged costs the guides and one image pass: set_camera / set_object -> render_aov -> solid -> overlay -> present.  The looks
 * table carries what a first-hit albedo plane does not know: an object's emission (a lamp is drawn as a lamp) and whether it is
 * a mirror.
 * - Buffers: device pointers, whole frames of width * height pixels in framebuffer order, the layouts pt_ctx_render_aov writes
 *   for a cfg without a band and without chunks: d_albedo and d_normal 3 floats per pixel, d_depth 1 float, d_object_id 1 int32
 *   (below 0: a miss), d_out 3 floats per pixel.  d_albedo may be NULL: every albedo is (1, 1, 1), a clay view.
 * - Aliasing: d_out may be d_albedo or d_normal (a pixel reads its own inputs before it writes and gathers nothing).  d_out may
 *   alias nothing else.
 * - `hip_stream` obeys the paragraph of ptrace.h that begins "`hip_stream` is a hipStream_t": NULL is the context's own stream;
 *   the table's copy, the kernel and whatever else the call does are ordered on that stream, behind what the caller queued
 *   there, and everything is complete when the call returns.  (pt_ctx_overlay, the next call of the loop, has no stream
 *   parameter: a loop on a caller's stream synchronises before it, as its header says.)
 * - Blocking; no scene is needed.  The call changes no state of the context but its own scratch for the looks table.
 * - The looks table: `looks` is a HOST array indexed by object id, copied per call on the call's stream into scratch of its own
 *   in the context - 16 B per record, grown on demand, freed by pt_ctx_destroy, shared with nothing (the mechanism of
 *   pt_ctx_reproject_moved's motion table).  With looks == NULL or n_looks == 0 nothing is copied.  An id beyond the table is
 *   never an error and never a read outside it: its record is {0, 0, 0, PT_DIFFUSE}.  pt_solid_look_of copies `emission` and
 *   `reflect_type` of a pt_object (PT_ERR_INVALID for a NULL argument).
 * - Every field of pt_solid_params is taken as it stands: there is no "0 = default".  params == NULL stands for the defaults.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: unknown flag bits; shininess_log2 above
 *   PT_SOLID_MAX_SHININESS_LOG2; an ambient, diffuse or specular that is negative or not finite; without PT_SOLID_HEADLIGHT a
 *   light component that is not finite; a background, sky_top or sky_bottom component that is negative or not finite; width or
 *   height 0; width * height above 2^28; NULL cam; a camera whose lens centre is not finite; NULL d_normal, d_depth,
 *   d_object_id or d_out; n_looks above 2^20; NULL looks with n_looks != 0; a look whose reflect_type is above PT_REFRACT, or
 *   that has a negative or non-finite emission component; NULL ctx.  PT_ERR_HIP: a HIP call failed.
 *
 * THE ARITHMETIC.  pt_ctx_overlay's and pt_ctx_denoise's rules: every operation is IEEE binary32 + - * / and sqrt, correctly
 * rounded, never contracted, in the order the parentheses give.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * pos(v) = v > 0 ? v : 0, so a NaN gives 0.  mix(a, b, t) = a + (b - a) * t.  clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v).
 * (L, su, sv) = pt_camera_basis(cam), computed on the host in binary32.  For pixel idx, with id = object_id[idx]:
 * 1. Miss.  If id < 0: out[idx][c] = background[c], and no other plane of this pixel is read.
 * 2. Point and view.  d is the direction of the pixel centre's ray, exactly as step 1 of pt_ctx_overlay makes it.
 *    P[a] = L[a] + d[a] * depth[idx].  v = -d.
 * 3. Normal.  N = N(idx), pt_ctx_denoise's normalised normal word for word: (0, 0, 0) when the length is not > 0.
 * 4. Light.  Q = L with PT_SOLID_HEADLIGHT, else `light`.  lv = Q - P.  ll = sqrt(dot(lv, lv)).
 *    ld = ll > 0 ? lv * (1 / ll) : (0, 0, 0).  ndl = dot(N, ld).  dif = pos(ndl).
 * 5. Highlight.  r[a] = N[a] * (2 * ndl) - ld[a].  s = ndl > 0 ? pos(dot(v, r)) : 0.  Then s = s * s, shininess_log2 times:
 *    the exponent is a power of two, so that no powf exists on either side.
 * 6. Shade.  k = (ambient + diffuse * dif) + specular * s.  A[c] = albedo[idx][c], or 1 when d_albedo is NULL.  b[c] = A[c] * k.
 * 7. Look.  rec = (uint32)id < n_looks ? looks[id] : {0, 0, 0, PT_DIFFUSE}.  With PT_SOLID_REFLECT_SKY and
 *    rec.reflect_type == PT_SPECULAR: dn = dot(N, d); m_y = d.y - N.y * (2 * dn); t = clamp(m_y * 0.5 + 0.5);
 *    b[c] = A[c] * mix(sky_bottom[c], sky_top[c], t) + specular * s.  PT_REFRACT is shaded as PT_DIFFUSE: a see-through glass
 *    is out of scope.
 * 8. Output.  out[idx][c] = clamp(b[c] + rec.emission[c]).
 *
 * pt_solid_defaults writes the defaults out: flags PT_SOLID_HEADLIGHT (a light at a fixed world position leaves half of an
 * orbit unlit), light (0, 0, 0), ambient 0.1, diffuse 1, specular 0.5, shininess_log2 5, background (0, 0, 0), sky_top and
 * sky_bottom as pt_overlay_defaults gives them: (0.25, 0.5, 0.75) and (0.75, 0.75, 0.75).  PT_ERR_INVALID for a NULL `out`.
 * pt_solid_pixel_host is the host instantiation of steps 1 to 8 for one pixel, from the source the kernel compiles
 * (csrc/pt_solid.h).  It refuses what pt_ctx_solid refuses about params, camera, frame size and look, an idx outside the frame,
 * and a NULL `normal` or `rgb_out`; a NULL `look` is the default record, a NULL `albedo` is (1, 1, 1).  None of the three host
 * functions needs a device. */
#define PT_SOLID_HEADLIGHT    1u   /* the light sits at the lens centre L; params->light is not read */
#define PT_SOLID_REFLECT_SKY  2u   /* PT_SPECULAR objects (by the looks table) show the sky gradient they reflect */
#define PT_SOLID_MAX_SHININESS_LOG2 10u
typedef struct pt_solid_params {          /* 17 words; every field is taken as it stands - no "0 = default" */
    uint32_t flags;
    float light[3];                       /* world position of the light */
    float ambient, diffuse, specular;     /* strengths, finite, >= 0 */
    uint32_t shininess_log2;              /* the highlight's exponent is 2^shininess_log2, 0..10 */
    float background[3];                  /* what a pixel that missed gets */
    float sky_top[3], sky_bottom[3];      /* PT_SOLID_REFLECT_SKY's gradient: pt_ctx_overlay's two colours */
} pt_solid_params;
typedef struct pt_solid_look {            /* 16 B, a HOST array indexed by object id */
    float emission[3];                    /* added after the light; finite, >= 0 */
    uint32_t reflect_type;                /* PT_DIFFUSE / PT_SPECULAR / PT_REFRACT */
} pt_solid_look;
int pt_solid_defaults(pt_solid_params *out);
int pt_solid_look_of(const pt_object *obj, pt_solid_look *out);            /* host only */
int pt_ctx_solid(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_solid_params *params /* NULL = the defaults */,
                 const pt_camera *cam, const float *d_albedo /* may be NULL: (1,1,1), a clay view */, const float *d_normal,
                 const float *d_depth, const int32_t *d_object_id, const pt_solid_look *looks /* host, may be NULL */,
                 uint32_t n_looks, float *d_out, void *hip_stream);
int pt_solid_pixel_host(const pt_camera *cam, uint32_t width, uint32_t height, const pt_solid_params *params, uint32_t idx,
                        int32_t object_id, float depth, const float albedo[3] /* may be NULL */, const float normal[3],
                        const pt_solid_look *look /* may be NULL */, float rgb_out[3]);   /* host only */

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_SOLID_H */
