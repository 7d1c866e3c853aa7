// pt_probe.h — pt_ctx_scatter (pt_probe.hip): one radiance() invocation after its intersect_scene call, on the device, through
// the functions the frame kernels call - shade_surface in its three instantiations, fetch_surface, fetch_surface_rank - with
// everything the step decides handed back.  A parity probe: tests/kats_scatter.py is the independent restatement it is held to.
// A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ptrace.h"

namespace pt {

// a surface of the PT_SCATTER_GIVEN form as the kernel reads it: the caller's, plus what a MatRec adds to a colour
struct ScatterSurf {
    float x[3], n[3], color[3], emission[3];
    float max_refl, inv_max_refl;  // host::material_reflectance, as flatten_scene fills a MatRec
    uint32_t reflect;
};

// The call on the device.  items / surf / out: device arrays of n.
struct ScatterCall {
    const pt_scatter_item *items;
    const ScatterSurf *surf;  // PT_SCATTER_GIVEN only
    pt_scatter_out *out;
    uint32_t n;
    uint32_t form;            // PT_SCATTER_* as checked
    uint32_t seed_lo, seed_hi;
    uint32_t head;            // PT_SCATTER_BY_RANK: leading ranks of DevScene.surf a workgroup copies to LDS (0: none)
};

static_assert(sizeof(pt_scatter_item) == 52 && sizeof(pt_scatter_surface) == 52 && sizeof(pt_scatter_out) == 104, "ptrace.h layout");

constexpr uint32_t kScatterSourceMask = 3u;
constexpr uint32_t kScatterModeMask = PT_SCATTER_DEFER_REFRACT | PT_SCATTER_REFRACT_ONLY;

namespace host {
// max_reflection (mod.rs:668) and its reciprocal (mod.rs:679) of a colour: the one routine flatten_scene and the probe use
void material_reflectance(const float color[3], float &max_refl, float &inv_max_refl);
// pt_ctx_scatter's refusals in the header's order up to the NULL context (PT_ERR_INVALID + message); PT_OK: `given` holds the
// PT_SCATTER_GIVEN form's surfaces as the kernel reads them (empty for the other sources).  No device is touched.
int check_scatter(const void *ctx, uint32_t form, const pt_scatter_item *items, const pt_scatter_surface *surfaces, uint32_t n,
                  const pt_scatter_out *out, std::vector<ScatterSurf> &given);
}  // namespace host

#if defined(__HIPCC__)
struct DevScene;
// bytes of LDS a workgroup of the probe may use for the head of the surf table, beside what the scene's BVH walk needs
size_t scatter_head_room(const DevScene &S);
// S: the context's scene as pt_ctx_intersect scans it (not read by the PT_SCATTER_GIVEN form)
void launch_scatter(hipStream_t st, const DevScene &S, const ScatterCall &call);
#endif

}  // namespace pt
