// pt_overlay.hip — pt_ctx_overlay's kernel: the sky, the ground grid and the selected objects' tint and outline drawn on a whole
// float frame.  The arithmetic is the contract of include/ptrace_overlay.h ("THE ARITHMETIC" of pt_ctx_overlay), operation for
// operation; the pixel is pt_overlay.h's overlay_pixel, which the host compiles too.  Built with -ffp-contract=off and correctly
// rounded / and sqrt, so a restatement in numpy binary32 (tests/overlay_ref.py) gives the same bytes.
//
// Memory-bound: 4 B of object id per pixel, 4 B of depth with the grid, 12 B of colour read and 12 B written - and in place only
// the pixels a step touches are read and written at all.  One workgroup of 256 lanes per tile of 32 x 8, pt_reproject.hip's
// kernel B shape, one lane per pixel.
// - The selection and the camera are kernel arguments (OverlayFrame): no device table, no copy before the launch.
// - The lanes load the ids of tile + halo of R once, compare each against the listed ids ONCE (sixteen compares per id loaded, not
//   per window tap) and keep the answer as a byte in LDS: bit 0 = selected, bit 1 = a miss (id < 0), which is all the sky needs
//   of the id.  48 x 24 B at most, at a pitch of 48 known at compile time; positions outside the frame hold 0.  A byte per
//   position, because the window below reads single positions: four lanes of a row read four bytes of one dword, which the LDS
//   serves as one address.
// - A workgroup-wide vote (__syncthreads_or, which is the barrier behind the staging as well) says whether tile + halo holds a
//   selected pixel at all.  If it holds none and no flag is set the tile is finished: out of place it copies its colours, in
//   place it loads and stores no colour - the whole pass then costs the id plane.
// - The window of step 6 is a dilation by a square, which is separable: the mask is ORed along rows into a second LDS array
//   (24 x 32 B), then that along columns: 2 * (2R + 1) LDS reads per pixel instead of (2R + 1)^2.
#include "pt_overlay.h"

namespace pt {
namespace {

constexpr uint32_t kOvTileW = kOverlayTileW, kOvTileH = kOverlayTileH, kOvMaxR = PT_OVERLAY_MAX_RADIUS;
constexpr uint32_t kOvStageW = kOvTileW + 2u * kOvMaxR, kOvStageH = kOvTileH + 2u * kOvMaxR;
constexpr uint32_t kOvSelected = 1u, kOvMiss = 2u;

// out may be rgb (no __restrict__ on the two): a lane reads its pixel's colour before it stores
__global__ __launch_bounds__(kOvTileW *kOvTileH) void k_overlay(const OverlayFrame f, uint32_t tiles_x) {
    __shared__ uint8_t sh_m[kOvStageW * kOvStageH];  // tile + halo: kOvSelected | kOvMiss
    __shared__ uint8_t sh_row[kOvTileW * kOvStageH];  // bit 0 of sh_m ORed over [sx, sx + 2R] of each staged row
    const int32_t W = (int32_t)f.width, H = (int32_t)f.height, R = (int32_t)f.p.radius;
    const int32_t tx = (int32_t)(threadIdx.x % kOvTileW), ty = (int32_t)(threadIdx.x / kOvTileW);
    const int32_t bx = (int32_t)((blockIdx.x % tiles_x) * kOvTileW), br = (int32_t)((blockIdx.x / tiles_x) * kOvTileH);
    const int32_t x = bx + tx, r = br + ty;
    const bool in_frame = x < W && r < H;
    const int32_t stage_w = (int32_t)kOvTileW + 2 * R, stage_h = (int32_t)kOvTileH + 2 * R;  // at most kOvStageW, kOvStageH
    constexpr int32_t pitch = (int32_t)kOvStageW;
    const bool ids = f.object_id != nullptr;  // uniform: a kernel argument
    bool any = false;
    if (ids) {
        bool mine = false;
        for (int32_t sy = ty; sy < stage_h; sy += (int32_t)kOvTileH) {
            for (int32_t sx = tx; sx < stage_w; sx += (int32_t)kOvTileW) {
                const int32_t qx = bx - R + sx, qr = br - R + sy;
                const bool in = qx >= 0 && qx < W && qr >= 0 && qr < H;
                const int32_t id = in ? f.object_id[(uint32_t)qr * f.width + (uint32_t)qx] : 0;
                const bool m = in && overlay_selected(f.p, id);
                sh_m[sy * pitch + sx] = (uint8_t)((m ? kOvSelected : 0u) | (in && id < 0 ? kOvMiss : 0u));
                mine = mine || m;
            }
        }
        any = __syncthreads_or(mine) != 0;
    }
    const uint32_t flags = f.p.flags;
    const bool in_place = f.out == f.rgb;
    const size_t i3 = ((size_t)(uint32_t)r * f.width + (uint32_t)x) * 3u;
    if (!any && !flags) {  // nothing to draw in this tile
        if (!in_place && in_frame) {
            const float v0 = f.rgb[i3], v1 = f.rgb[i3 + 1], v2 = f.rgb[i3 + 2];
            f.out[i3] = v0;
            f.out[i3 + 1] = v1;
            f.out[i3 + 2] = v2;
        }
        return;
    }
    bool selected = false, miss = false, outlined = false;
    if (ids) {
        const uint32_t own = sh_m[(ty + R) * pitch + tx + R];
        selected = (own & kOvSelected) != 0u;
        miss = (own & kOvMiss) != 0u;
    }
    if (any) {  // uniform
        for (int32_t sy = ty; sy < stage_h; sy += (int32_t)kOvTileH) {
            uint32_t o = 0u;
            for (int32_t i = 0; i <= 2 * R; ++i) o |= sh_m[sy * pitch + tx + i];
            sh_row[sy * (int32_t)kOvTileW + tx] = (uint8_t)(o & kOvSelected);
        }
        __syncthreads();
        uint32_t o = 0u;
        for (int32_t j = 0; j <= 2 * R; ++j) o |= sh_row[(ty + j) * (int32_t)kOvTileW + tx];
        outlined = o != 0u && !selected;
    }
    if (!in_frame) return;
    // in place a pixel that no step can touch is neither read nor written; with a flag set the ray decides
    if (in_place && !flags && !outlined && !(selected && f.p.fill_alpha != 0.0f)) return;
    const uint32_t idx = (uint32_t)r * f.width + (uint32_t)x;
    float v[3] = {f.rgb[i3], f.rgb[i3 + 1], f.rgb[i3 + 2]};
    const float depth = (flags & PT_OVERLAY_GRID) ? f.depth[idx] : 0.0f;
    const bool touched = overlay_pixel(f, idx, miss ? -1 : 0, depth, selected, outlined, v);
    if (touched || !in_place) {
        f.out[i3] = v[0];
        f.out[i3 + 1] = v[1];
        f.out[i3 + 2] = v[2];
    }
}

}  // namespace

void launch_overlay(hipStream_t st, const OverlayFrame &f) {
    // a grid of one dimension, as pt_reproject.hip's kernel B: at most 2^28 pixels, so at most 2^28 tiles
    const uint32_t tiles_x = (f.width + kOvTileW - 1u) / kOvTileW, tiles_y = (f.height + kOvTileH - 1u) / kOvTileH;
    hipLaunchKernelGGL(k_overlay, dim3(tiles_x * tiles_y), dim3(kOvTileW * kOvTileH), 0, st, f, tiles_x);
}

}  // namespace pt
