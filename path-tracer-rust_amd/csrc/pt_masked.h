// pt_masked.h — pt_ctx_select_pixels and the device side of pt_ctx_render_masked beside the trace (pt_masked.hip): the select
// pass that turns the viewport loop's planes (pt_ctx_upsample's d_out_weight, pt_ctx_reproject*'s d_out_len) into a byte mask
// and counts it, the compaction of a mask into a list of call indices, and the scatter of the compact accumulator into a frame
// through k_resolve's arithmetic - and pt_ctx_spp_plane, which turns such a mask into the plane of per-pixel sample counts
// pt_ctx_reproject_var_weighted reads.  The predicate is the contract in include/ptrace.h, stated once, below, for host and device.
// The trace itself is the tile pass (pt_tile.h) over a grid of 1x1 tiles.  A translation unit of its own: pt_kernels.s, and so
// pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace.h"
#include "pt_math.h"

namespace pt {

// The select call's whole frames.  Host pointers on the host, device pointers on the device.
struct SelectFrame {
    uint32_t npix;               // width * height
    const float *weight, *len;   // either may be NULL, not both
    uint8_t *mask;
    float weight_max, len_max;   // taken literally
    uint32_t *count;             // the number of ones is ADDED here (the entry point's scratch word; NULL on the host)
};

// the predicate on a pixel's values: !(v > max) is true for a NaN, which selects the pixel
PT_HD uint32_t select_test(bool has_weight, float weight, float weight_max, bool has_len, float len, float len_max) {
    return ((has_weight && !(weight > weight_max)) || (has_len && !(len > len_max))) ? 1u : 0u;
}

// mask[p] for pixel p (< npix)
PT_HD uint32_t select_pixel(const SelectFrame &f, uint32_t p) {
    return select_test(f.weight != nullptr, f.weight ? f.weight[p] : 0.0f, f.weight_max, f.len != nullptr, f.len ? f.len[p] : 0.0f,
                       f.len_max);
}

// pt_ctx_spp_plane: the count of a pixel whose mask byte is m (no mask: m = 0)
PT_HD uint32_t spp_plane_value(uint32_t m, uint32_t base, uint32_t masked) { return m != 0u ? masked : base; }

namespace host {
// pt_ctx_spp_plane's refusals in the header's order.  No device is touched.
int check_spp_plane(const void *ctx, uint32_t width, uint32_t height, const uint32_t *d_spp);
// pt_ctx_select_pixels' refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call, all but `count`.
// No device is touched.
int check_select_pixels(const void *ctx, uint32_t width, uint32_t height, const pt_select_params *params, const float *d_weight,
                        const float *d_len, uint8_t *d_mask, SelectFrame &f);
// pt_ctx_render_masked's refusals about the band and the flags, which are pt_ctx_render_adaptive's: whole rows, then chunk_step
// <= 1 and no PT_FLAG_PIPELINES
int check_masked_cfg(const pt_config &cfg);
}  // namespace host

#if defined(__HIPCC__)
// four pixels per lane; *f.count += the ones, one integer atomic per workgroup that found any
void launch_select(hipStream_t st, const SelectFrame &f);

// The indices k < n with mask[k] != 0, appended to `list` in no particular order through one integer atomic per workgroup on *len
// (zeroed by the caller): a slot of the list only names where a pixel's entry of the compact accumulator lies.  *len counts
// every selected pixel; only the slots below `cap` are written, so a caller whose list was too short grows it and runs again.
void launch_masked_compact(hipStream_t st, const uint8_t *mask, uint32_t n, uint32_t *list, uint32_t cap, uint32_t *len);

// rgb[3 * list[k] + c] = clamp(mean of acc[c * n + k] over spp samples), k < n (> 0): k_resolve's arithmetic; nothing else is written
void launch_masked_scatter(hipStream_t st, const uint32_t *list, uint32_t n, const unsigned long long *acc, uint32_t spp, float *rgb);

// spp[p] = spp_plane_value(mask ? mask[p] : 0, base, masked), p < n (> 0): sixteen pixels per lane
void launch_spp_plane(hipStream_t st, const uint8_t *mask, uint32_t n, uint32_t base, uint32_t masked, uint32_t *spp);
#endif

}  // namespace pt
