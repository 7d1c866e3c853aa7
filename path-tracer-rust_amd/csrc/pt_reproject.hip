// pt_reproject.hip — the kernels of pt_ctx_reproject and its _var, _moved and _weighted forms, and launch_reproject, the one
// launcher that picks among them: the history frame gathered into this frame's pixels and blended by the history
// length.  The arithmetic is the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_reproject), operation for operation;
// the pixel is pt_reproject.h's reproject_pixel, which the host compiles too.  Built with -ffp-contract=off and correctly
// rounded / and sqrt, so a restatement in numpy binary32 (tests/reproject_ref.py) gives the same bytes.
//
// Memory-bound: 84 B per pixel at most (32 read of this frame, 36 of the history, 16 written), about forty operations.  One lane
// per pixel, a plain gather.  Consecutive lanes take consecutive pixels, so a wave's loads of a plane of 3 floats per pixel touch
// the same cache lines three times and its loads of the 1-float planes are one line each.  The pixel's own planes are read once by
// one lane: non-temporal loads, which pass the L1 by.  The four taps of neighbouring pixels overlap - a history pixel is read by
// up to four lanes, mostly of the same wave or the next row's - and stay on the default policy, where L1 and L2 serve the repeats.
// The taps are clamped into the frame and all read before the first is tested (reproject_gather): one round trip, not twelve.
// No LDS: under a camera move the footprint of a workgroup's taps is not a rectangle known before the projection.
#include "pt_reproject.h"

namespace pt {
namespace {

constexpr uint32_t kReprojectBlock = 256;

// out_color may be color (no __restrict__ on the two): a lane reads its pixel's colour before it stores
__global__ __launch_bounds__(kReprojectBlock) void k_reproject(const ReprojectFrame f, uint32_t npix) {
    const uint32_t idx = blockIdx.x * kReprojectBlock + threadIdx.x;
    if (idx >= npix) return;
    float out[3], len;
    reproject_pixel(f, idx, out, &len);
    float *o = f.out_color + (size_t)idx * 3u;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    f.out_len[idx] = len;
}

// ---- pt_ctx_reproject_var.  Two launches, because which pixels are short is known only after the projection and the gather,
// and because d_out_color may be d_color: the window reads its neighbours' s values, so the s plane has to be complete before any
// colour is overwritten.
//
// Kernel A is k_reproject with the moments riding along (reproject_gather<NT, true>): 112 B per pixel at most - 32 read of this
// frame, 36 + 8 of the history, 16 + 8 + 4 + 4 written.
__global__ __launch_bounds__(kReprojectBlock) void k_reproject_var(const ReprojectVarFrame v, uint32_t npix) {
    const uint32_t idx = blockIdx.x * kReprojectBlock + threadIdx.x;
    if (idx >= npix) return;
    reproject_var_pixel(v, idx);
}

// Kernel B: the spatial estimate of the pixels kernel A marked.  One workgroup per tile of 32 x 8, one lane per pixel.  In steady
// state a few percent of the pixels are short, so a workgroup reads its tile's markers (4 B per pixel, one line per row) and
// returns when none is set.  Otherwise it stages s, object id and depth of tile + halo in LDS once - three planes of
// 38 x 14 words, 6384 B: the halo of the largest radius, whatever R is - and the marked lanes run the window from there:
// up to 49 taps of three words each from LDS instead of from L1.  Entries outside the frame are staged as zeros and never
// read: the window skips them by their coordinates.
constexpr uint32_t kRvTileW = kReprojectVarTileW, kRvTileH = kReprojectVarTileH, kRvMaxR = kReprojectVarMaxRadius;
constexpr uint32_t kRvStageW = kRvTileW + 2u * kRvMaxR, kRvStageH = kRvTileH + 2u * kRvMaxR;

struct RvTile {
    const float *s, *z;
    const int32_t *id;
    int32_t x0, r0, pitch;  // the frame position of entry (0, 0), and the entries per staged row
    __device__ void operator()(int32_t qx, int32_t qr, float &so, int32_t &ido, float &zo) const {
        const int32_t e = (qr - r0) * pitch + (qx - x0);
        so = s[e];
        ido = id[e];
        zo = z[e];
    }
};

// (pt_ctx_reproject_var_weighted's form, WEIGHTED, stages the counts as a fourth plane - 8512 B - because a tap is then taken
// only when its count is the centre's; the early return is the same.  Without WEIGHTED nothing of it is compiled.)
struct RvTileWeighted : RvTile {
    const uint32_t *c;
    __device__ uint32_t count(int32_t qx, int32_t qr) const { return c[(qr - r0) * pitch + (qx - x0)]; }
};

template <bool WEIGHTED>
__device__ __forceinline__ void rv_spatial_tile(const ReprojectVarFrame &v, uint32_t tiles_x, const uint32_t *spp) {
    __shared__ float sh_s[kRvStageW * kRvStageH], sh_z[kRvStageW * kRvStageH];
    __shared__ int32_t sh_id[kRvStageW * kRvStageH];
    uint32_t *sh_c = nullptr;
    if constexpr (WEIGHTED) {
        __shared__ uint32_t counts[kRvStageW * kRvStageH];
        sh_c = counts;
    }
    const int32_t W = (int32_t)v.f.width, H = (int32_t)v.f.height;
    const int32_t tx = (int32_t)(threadIdx.x % kRvTileW), ty = (int32_t)(threadIdx.x / kRvTileW);
    const int32_t bx = (int32_t)((blockIdx.x % tiles_x) * kRvTileW), br = (int32_t)((blockIdx.x / tiles_x) * kRvTileH);
    const int32_t x = bx + tx, r = br + ty;
    const bool in_frame = x < W && r < H;
    const uint32_t idx = in_frame ? (uint32_t)r * v.f.width + (uint32_t)x : 0u;
    const bool marked = in_frame && v.error[idx] == kReprojectVarShort;
    if (!__syncthreads_or(marked)) return;
    // (always the halo of the largest radius: a pitch known at compile time, so that e % pitch and e / pitch are multiplies)
    constexpr int32_t pitch = (int32_t)kRvStageW, rows = (int32_t)kRvStageH;
    const int32_t x0 = bx - (int32_t)kRvMaxR, r0 = br - (int32_t)kRvMaxR;
    for (int32_t e = (int32_t)threadIdx.x; e < pitch * rows; e += (int32_t)(kRvTileW * kRvTileH)) {
        const int32_t qx = x0 + e % pitch, qr = r0 + e / pitch;
        const bool in = qx >= 0 && qx < W && qr >= 0 && qr < H;
        const uint32_t q = in ? (uint32_t)qr * v.f.width + (uint32_t)qx : 0u;
        sh_s[e] = in ? v.s_plane[q] : 0.0f;
        sh_id[e] = in ? v.f.object_id[q] : 0;
        sh_z[e] = in ? v.f.depth[q] : 0.0f;
        if constexpr (WEIGHTED) sh_c[e] = in ? spp[q] : 0u;
    }
    __syncthreads();
    if (!marked) return;
    const RvTile tile = {sh_s, sh_z, sh_id, x0, r0, pitch};
    if constexpr (WEIGHTED) {
        RvTileWeighted wt;
        static_cast<RvTile &>(wt) = tile;
        wt.c = sh_c;
        v.error[idx] = reproject_var_short_pixel<RvTileWeighted, true>(v, wt, idx);
    } else {
        v.error[idx] = reproject_var_short_pixel(v, tile, idx);
    }
}

__global__ __launch_bounds__(kRvTileW *kRvTileH) void k_reproject_var_spatial(const ReprojectVarFrame v, uint32_t tiles_x) {
    rv_spatial_tile<false>(v, tiles_x, nullptr);
}

// ---- pt_ctx_reproject_moved / pt_ctx_reproject_var_moved: the same two kernels with the per-object motion table
// (reproject_pixel_t<MOM, true>).  The compulsory bytes are the plain kernels' plus the table's 16 B per object once: the record
// is one 16-byte load by object id, issued as soon as the id is known and long before the taps' addresses are; a wave's lanes
// mostly share an object, so it is one line of L1 or L2.  The table is a kernel argument of its own, so that ReprojectFrame,
// and with it every plain kernel, stays what it is.
__global__ __launch_bounds__(kReprojectBlock) void k_reproject_moved(const ReprojectFrame f, const ReprojectMotion m, uint32_t npix) {
    const uint32_t idx = blockIdx.x * kReprojectBlock + threadIdx.x;
    if (idx >= npix) return;
    float out[3], len;
    reproject_pixel_moved(f, m, idx, out, &len);
    float *o = f.out_color + (size_t)idx * 3u;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    f.out_len[idx] = len;
}

__global__ __launch_bounds__(kReprojectBlock) void k_reproject_var_moved(const ReprojectVarFrame v, const ReprojectMotion m, uint32_t npix) {
    const uint32_t idx = blockIdx.x * kReprojectBlock + threadIdx.x;
    if (idx >= npix) return;
    reproject_var_pixel<true>(v, idx, &m);
}

// ---- pt_ctx_reproject_var_weighted: the two var kernels with the plane of per-pixel counts (reproject_var_pixel<MOVED, true>).
// Kernel A reads 4 B more per pixel - the pixel's own count, one non-temporal load issued with its colour's: 116 B per pixel at
// most - and does per lane what the plain kernel does with a uniform: the count as a float is the pixel's wt, and a pixel without
// samples takes the gathered history as it is.  Its d_error is final for every pixel without samples (+inf where it is not
// long), so kernel B's markers are pixels with a count.  The plane and (float)min_frames are a kernel argument of their own.
template <bool MOVED>
__global__ __launch_bounds__(kReprojectBlock) void k_reproject_var_weighted(const ReprojectVarFrame v, const ReprojectMotion m,
                                                                            const ReprojectWeights wts, uint32_t npix) {
    const uint32_t idx = blockIdx.x * kReprojectBlock + threadIdx.x;
    if (idx >= npix) return;
    reproject_var_pixel<MOVED, true>(v, idx, &m, &wts);
}

// Kernel B with the counts: the one tile body with the fourth staged plane
__global__ __launch_bounds__(kRvTileW *kRvTileH) void k_reproject_var_spatial_weighted(const ReprojectVarFrame v, const uint32_t *spp,
                                                                                      uint32_t tiles_x) {
    rv_spatial_tile<true>(v, tiles_x, spp);
}

}  // namespace

// The one launcher.  Which kernel A: by the moments, the plane and call.moved() - without a history nothing can have moved, so
// the plain kernels run whatever the table says.  Kernel B reads neither the history nor the table.
void launch_reproject(hipStream_t st, const ReprojectCall &call, const ReprojectMotion *table) {
    const ReprojectVarFrame &v = call.v;
    const uint32_t npix = v.f.width * v.f.height;  // at most 2^28: 2^20 workgroups
    const dim3 grid((npix + kReprojectBlock - 1u) / kReprojectBlock), block(kReprojectBlock);
    const bool moved = call.moved();
    const ReprojectMotion m = moved ? *table : ReprojectMotion{nullptr, 0u};
    if (!call.var) {
        if (moved)
            hipLaunchKernelGGL(k_reproject_moved, grid, block, 0, st, v.f, m, npix);
        else
            hipLaunchKernelGGL(k_reproject, grid, block, 0, st, v.f, npix);
        return;
    }
    if (call.weighted && moved)
        hipLaunchKernelGGL((k_reproject_var_weighted<true>), grid, block, 0, st, v, m, call.wts, npix);
    else if (call.weighted)
        hipLaunchKernelGGL((k_reproject_var_weighted<false>), grid, block, 0, st, v, m, call.wts, npix);
    else if (moved)
        hipLaunchKernelGGL(k_reproject_var_moved, grid, block, 0, st, v, m, npix);
    else
        hipLaunchKernelGGL(k_reproject_var, grid, block, 0, st, v, npix);
    // a grid of one dimension: a frame of one column and 2^28 rows is 2^25 tiles down, more than a grid's y takes
    const uint32_t tiles_x = (v.f.width + kRvTileW - 1u) / kRvTileW, tiles_y = (v.f.height + kRvTileH - 1u) / kRvTileH;
    const dim3 tiles(tiles_x * tiles_y), tile(kRvTileW * kRvTileH);
    if (call.weighted)
        hipLaunchKernelGGL(k_reproject_var_spatial_weighted, tiles, tile, 0, st, v, call.wts.spp, tiles_x);
    else
        hipLaunchKernelGGL(k_reproject_var_spatial, tiles, tile, 0, st, v, tiles_x);
}

}  // namespace pt
