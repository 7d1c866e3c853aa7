/* ptrace_overlay.h — pt_ctx_overlay: the editing cues drawn on a frame before pt_ctx_present.  C ABI of libptrace_hip.so. */
#ifndef PTRACE_OVERLAY_H
#define PTRACE_OVERLAY_H

#include "ptrace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the editing cues on a frame: selection outline, sky, ground grid ------------------------------------------------
 * A header of its own beside ptrace.h, which it includes: tests/test_abi.py holds ptrace.h and abi.py to 22 structs, and this
 * pass adds one without changing that file.  The symbols are libptrace_hip.so's like all others (PT_ABI_VERSION stays 5: symbols
 * are only added); path-tracer-rust_amd/overlay_abi.py describes this header to Python as abi.py describes ptrace.h.  Once
 * test_abi.py may count 23, the section moves into ptrace.h and the table into abi.py, word for word.
 *
 * pt_ctx_overlay draws on a whole float frame what an editing viewport shows around the picture: a backdrop gradient where no
 * object is seen, a ground grid in a plane y = grid_y that objects hide, and an outline (and an optional tint) for the selected
 * objects.  One image-space pass between the denoiser and pt_ctx_present, which still scales and quantises its result: the loop
 * is set_camera / set_object -> render -> render_aov -> reproject_var -> denoise_var -> overlay -> present.  Every input is on
 * the device already - the object-id and depth planes of pt_ctx_render_aov, and the camera - so the host downloads nothing.
 * - Buffers: device pointers, whole frames of width * height pixels in framebuffer order: d_rgb and d_out 3 floats per pixel,
 *   d_object_id 1 int32 (-1: a miss), d_depth 1 float (+inf on a miss).  d_object_id may be NULL when nothing is selected and
 *   PT_OVERLAY_SKY is not set, d_depth when PT_OVERLAY_GRID is not set, cam when no flag is set.
 * - Aliasing: d_out may be d_rgb (a pixel reads its own colour before it writes; only the id plane is gathered).  d_out may
 *   alias nothing else.
 * - NO STREAM PARAMETER: the call runs on the context's own stream and returns when its output is complete.  Every other entry
 *   point is blocking too, so a loop that passes NULL streams is ordered as before.  A caller with work pending on a stream of
 *   its own - the frame's denoiser, say - must synchronise that stream before the call.
 * - Blocking; no scene is needed; no scratch is taken: the selection and the camera travel as kernel arguments, there is no
 *   device table and no copy.  The call changes no state of the context.
 * - `radius` is in frame pixels: a host that presents at 1/k size passes k times the width it wants to see.
 * - Lines have hard edges: a pixel is on a grid line or it is not, so distant lines alias.  Antialiasing is out of scope.
 * - KNOWN LIMIT: the sky goes only where sample 0 missed (object_id < 0).  A silhouette pixel of the frame is an antialiased
 *   mix of the object with black and keeps a dark fringe against the sky: the frame has no coverage plane to do better.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: unknown flag bits; n_selected above
 *   PT_OVERLAY_MAX_SELECTED, or a listed id below 0; radius above PT_OVERLAY_MAX_RADIUS; a colour component or an alpha that
 *   is not finite, or an alpha outside [0, 1]; with PT_OVERLAY_GRID a grid_spacing, grid_half_width or grid_extent that is not
 *   finite or not > 0, or a grid_y that is not finite; width or height 0, or width * height above 2^28; NULL d_rgb or d_out;
 *   NULL d_object_id while n_selected > 0 or PT_OVERLAY_SKY is set; NULL d_depth with PT_OVERLAY_GRID; NULL cam with either
 *   flag; a camera whose lens centre is not finite; NULL ctx.  PT_ERR_HIP: a HIP call failed.  params == NULL stands for all
 *   zero: no flags and no selection - the call copies d_rgb to d_out, or does nothing when run in place.
 *
 * THE ARITHMETIC.  Every operation is IEEE binary32 + - * / and sqrt, correctly rounded, never contracted, in the order the
 * parentheses give - pt_ctx_reproject's rules, and its dot(a, b) and |v|.  mix(a, b, t) = a + (b - a) * t.  M(q) = 1 when
 * object_id[q] equals one of the n_selected listed ids, else 0; an id below 0 is never selected.  R = radius (0 stands for 2);
 * outline_alpha 0 and grid_alpha 0 stand for 1; fill_alpha 0 means no fill.  (L, su, sv) = pt_camera_basis(cam), computed on the
 * host in binary32; C is cam's position; W, H = width, height.  For pixel idx: x = idx % W, r = idx / W, y = H-1-r.
 * 1. Ray (only when a flag is set).  sx, sy, S and g = L - S exactly as step 3 of pt_ctx_reproject computes them;
 *    d = g * (1 / sqrt(dot(g, g))): the direction of the pixel centre's ray.
 * 2. Start.  v[c] = rgb[idx][c].
 * 3. Sky, when PT_OVERLAY_SKY is set and object_id[idx] < 0.  s = d.y * 0.5 + 0.5; s = s > 0 ? (s > 1 ? 1 : s) : 0;
 *    v[c] = mix(sky_bottom[c], sky_top[c], s).
 * 4. Grid, when PT_OVERLAY_GRID is set.  t = (grid_y - L.y) / d.y.  The pixel sees the plane iff t > 0 && t < depth[idx] (a NaN
 *    rejects; depth is +inf on a miss).  Qx = L.x + d.x * t; Qz = L.z + d.z * t.  It is inside iff |Qx| <= grid_extent &&
 *    |Qz| <= grid_extent.  On an axis a (x, then z): k = floor(Qa / grid_spacing + 0.5); dist = |Qa - k * grid_spacing|; the
 *    pixel is on a line iff dist <= grid_half_width.  If the pixel sees the plane, is inside, and is on a line of either axis:
 *    v[c] = mix(v[c], grid_color[c], grid_alpha).
 * 5. Fill.  If M(idx) and fill_alpha != 0: v[c] = mix(v[c], fill_color[c], fill_alpha).
 * 6. Outline, drawn outside the silhouette.  A pixel is outlined when M(idx) == 0 and some q = (x+i, r+j) inside the frame has
 *    M(q) == 1, with |i| <= R and |j| <= R.  For such a pixel v[c] = mix(v[c], outline_color[c], outline_alpha).  The object's
 *    own pixels keep their colour.
 * 7. Output.  out[idx][c] = v[c].  A pixel that no step touched has its input's bits, NaN payloads and -0 included.
 *
 * pt_overlay_defaults writes every default out: flags 0, nothing selected, radius 2, outline (0, 1, 0) at alpha 1, fill (1, 1, 1)
 * at alpha 0 (off), sky_top (0.25, 0.5, 0.75), sky_bottom (0.75, 0.75, 0.75), grid colour (0.5, 0.5, 0.5) at alpha 0.5, and the
 * grid of a camera 5 units from the origin: grid_y 0, grid_spacing 1, grid_half_width 0.01, grid_extent 5.  With a camera it sizes
 * the grid the way the editing viewport sizes its own: zoom = |position| / 5; grid_spacing = 10^floor(log10(zoom * 1.2 + 1));
 * grid_half_width = 0.01 * zoom; grid_extent = 5 * grid_spacing; grid_y = 0 - computed in binary64 and rounded to binary32 once.
 * PT_ERR_INVALID for a NULL `out` or a camera position that is not finite.
 * pt_overlay_pixel_host is the host instantiation of steps 1 to 7 for one pixel, from the source the kernel compiles
 * (csrc/pt_overlay.h): the pixel's own object_id and depth, whether it is selected (M(idx)) and whether step 6's window found a
 * selected pixel are given (the outline is drawn when `outlined` != 0 and `selected` == 0); rgb_out may be rgb_in.
 * PT_ERR_INVALID for params pt_ctx_overlay refuses, an empty frame, one above 2^28 pixels, idx outside it, a NULL colour
 * pointer, or a NULL or non-finite camera with a flag set.  Neither needs a device. */
#define PT_OVERLAY_SKY  1u
#define PT_OVERLAY_GRID 2u
#define PT_OVERLAY_MAX_SELECTED 16u
#define PT_OVERLAY_MAX_RADIUS 8u
typedef struct pt_overlay_params {
    uint32_t flags;                 /* PT_OVERLAY_SKY | PT_OVERLAY_GRID */
    uint32_t n_selected;            /* <= PT_OVERLAY_MAX_SELECTED */
    int32_t  selected[16];          /* object indices, >= 0 */
    uint32_t radius;                /* outline reach in frame pixels; 0 = 2; <= PT_OVERLAY_MAX_RADIUS */
    float outline_color[3], outline_alpha;   /* alpha 0 = 1 */
    float fill_color[3], fill_alpha;         /* alpha 0 = no fill */
    float sky_top[3], sky_bottom[3];
    float grid_color[3], grid_alpha;         /* alpha 0 = 1 */
    float grid_y, grid_spacing, grid_half_width, grid_extent;
} pt_overlay_params;
int pt_overlay_defaults(const pt_camera *cam /* may be NULL */, pt_overlay_params *out);
int pt_ctx_overlay(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_overlay_params *params, const pt_camera *cam,
                   const float *d_rgb, const int32_t *d_object_id, const float *d_depth, float *d_out);
int pt_overlay_pixel_host(const pt_camera *cam, uint32_t width, uint32_t height, const pt_overlay_params *params, uint32_t idx,
                          int32_t object_id, float depth, int selected, int outlined, const float rgb_in[3], float rgb_out[3]);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_OVERLAY_H */
