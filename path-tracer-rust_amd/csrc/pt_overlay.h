// pt_overlay.h — pt_ctx_overlay (pt_overlay.hip): the editing cues on a whole float frame - the sky where nothing is seen, the
// ground grid that objects hide, the tint and the outline of the selected objects.  The arithmetic is the contract in
// include/ptrace_overlay.h ("THE ARITHMETIC" of pt_ctx_overlay), operation for operation.  Steps 1 to 7 for one pixel are stated once,
// below, for host and device: pt_overlay_pixel_host (host/scene_io.cpp) is the host instantiation of the source the kernel
// compiles, as pt_present_quantize_host is of pt_present.h.  Step 1 is pt_reproject.h's reproject_ray, not a restatement.
// A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace_overlay.h"
#include "pt_math.h"
#include "pt_reproject.h"

namespace pt {

// the values a zero radius and a zero outline_alpha / grid_alpha stand for, and the workgroup's tile (pt_reproject.hip's kernel B)
constexpr uint32_t kOverlayRadius = 2u;
constexpr uint32_t kOverlayTileW = kReprojectVarTileW, kOverlayTileH = kReprojectVarTileH;

// The call once it has passed.  Host pointers on the host, device pointers on the device; a kernel argument as it stands.
struct OverlayFrame {
    uint32_t width, height;
    const float *rgb, *depth;  // depth NULL without PT_OVERLAY_GRID
    const int32_t *object_id;  // NULL when nothing is selected and PT_OVERLAY_SKY is not set
    float *out;                // may be rgb
    pt_overlay_params p;       // the defaults filled in: radius, outline_alpha and grid_alpha are never 0
    vec3 C, L, su, sv;         // cam's position and its pt_camera_basis, in binary32; zeros when no flag is set
};

// mix(a, b, t) = a + (b - a) * t
PT_HD float overlay_mix(float a, float b, float t) { return a + (b - a) * t; }

// M: the id is one of the listed ones; an id below 0 never is.  Sixteen compares at most, once per id loaded.
PT_HD bool overlay_selected(const pt_overlay_params &p, int32_t id) {
    bool m = false;
#pragma unroll
    for (uint32_t i = 0; i < PT_OVERLAY_MAX_SELECTED; ++i) m = m || (i < p.n_selected && p.selected[i] == id);
    return m && id >= 0;
}

// step 4's test on one axis: the pixel is on a line
PT_HD bool overlay_on_line(float q, float spacing, float half_width) {
    const float k = __builtin_floorf(q / spacing + 0.5f);
    return __builtin_fabsf(q - k * spacing) <= half_width;
}

// Steps 1 to 7 for pixel idx but for the loads, the window and the store: v holds rgb[idx] on entry and out[idx] on return.
// `id` is read with PT_OVERLAY_SKY alone and `depth` with PT_OVERLAY_GRID alone.  false: no step touched the pixel, v is as it was.
PT_HD bool overlay_pixel(const OverlayFrame &f, uint32_t idx, int32_t id, float depth, bool selected, bool outlined, float v[3]) {
    const pt_overlay_params &p = f.p;
    bool touched = false;
    if (p.flags & (PT_OVERLAY_SKY | PT_OVERLAY_GRID)) {
        const uint32_t x = idx % f.width, r = idx / f.width, y = f.height - 1u - r;
        const vec3 d = reproject_ray(f.C, f.L, f.su, f.sv, f.width, f.height, x, y);
        if ((p.flags & PT_OVERLAY_SKY) && id < 0) {
            float s = d.y * 0.5f + 0.5f;
            s = s > 0.0f ? (s > 1.0f ? 1.0f : s) : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = overlay_mix(p.sky_bottom[c], p.sky_top[c], s);
            touched = true;
        }
        if (p.flags & PT_OVERLAY_GRID) {
            const float t = (p.grid_y - f.L.y) / d.y;
            const float qx = f.L.x + d.x * t, qz = f.L.z + d.z * t;
            const bool sees = t > 0.0f && t < depth;  // a NaN rejects
            const bool inside = __builtin_fabsf(qx) <= p.grid_extent && __builtin_fabsf(qz) <= p.grid_extent;
            const bool line = overlay_on_line(qx, p.grid_spacing, p.grid_half_width) || overlay_on_line(qz, p.grid_spacing, p.grid_half_width);
            if (sees && inside && line) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = overlay_mix(v[c], p.grid_color[c], p.grid_alpha);
                touched = true;
            }
        }
    }
    if (selected && p.fill_alpha != 0.0f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = overlay_mix(v[c], p.fill_color[c], p.fill_alpha);
        touched = true;
    }
    if (outlined && !selected) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = overlay_mix(v[c], p.outline_color[c], p.outline_alpha);
        touched = true;
    }
    return touched;
}

namespace host {
// The refusals that need the params alone, in the header's order (its first five): PT_OK: P holds the params with the
// defaults filled in (params NULL: all zero).  pt_overlay_pixel_host makes them too.
int check_overlay_params(const pt_overlay_params *params, pt_overlay_params &P);
// the camera of a call with a flag set (cam not NULL): PT_ERR_INVALID for a lens centre that is not finite, else f's C, L, su, sv
int overlay_view(const pt_camera &cam, OverlayFrame &f);
// pt_ctx_overlay's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call.  No device is touched.
int check_overlay(const void *ctx, uint32_t width, uint32_t height, const pt_overlay_params *params, const pt_camera *cam,
                  const float *d_rgb, const int32_t *d_object_id, const float *d_depth, float *d_out, OverlayFrame &f);
}  // namespace host

#if defined(__HIPCC__)
// one workgroup of 256 lanes per tile of 32 x 8
void launch_overlay(hipStream_t st, const OverlayFrame &f);
#endif

}  // namespace pt
