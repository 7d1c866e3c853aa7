// pt_aov.h — first-hit AOVs of a frame (pt_ctx_render_aov, pt_aov.hip): per pixel of the call the mean albedo and the mean
// ray-facing normal over samples [0, spp), and sample 0's hit distance and object index.  A translation unit of its own:
// pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.h"

namespace pt {

// F: the call's pixels (npix, band, chunks, k_begin) and its samples (spp, seed); S: the scene as the call scans it
// (n_bvh_nodes 0 = the linear scan).  Outputs in the call's pixel order; any of them may be NULL.
void launch_aov(hipStream_t st, const DevScene &S, const FrameParams &F, float *albedo, float *normal, float *depth,
                int32_t *object_id);

// The same through mirror and glass surfaces (pt_ctx_render_aov_ex with PT_AOV_THROUGH_DELTA): the guides of the surface that
// ends each sample's deterministic chain, at most max_chain (1..PT_AOV_MAX_CHAIN) delta steps; chain[k] = sample 0's steps.
void launch_aov_chain(hipStream_t st, const DevScene &S, const FrameParams &F, uint32_t max_chain, float *albedo, float *normal,
                      float *depth, int32_t *object_id, uint32_t *chain);

}  // namespace pt
