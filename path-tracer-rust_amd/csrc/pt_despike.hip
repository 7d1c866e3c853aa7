// pt_despike.hip — pt_ctx_despike's kernel: a pixel whose luminance is above threshold * (the rank-th largest luminance of its
// neighbours) + floor is scaled down to that limit.  The arithmetic is the contract of include/ptrace_despike.h, operation for
// operation; what happens to one value is pt_despike.h's, which the host compiles too.  Built with -ffp-contract=off and correctly
// rounded /, so a restatement in numpy binary32 (tests/despike_ref.py) gives the same bytes.
//
// A gathering pass over 24 B of colour per pixel (12 in, 12 out), 4 B more with ids, 1 B more with the mask: memory should bind
// it.  One workgroup of 256 lanes per tile of 32 x 8, pt_overlay.hip's shape, one lane per pixel, a wave two rows of the tile.
// - A lane loads ITS pixel's three channels once, as one 12-byte access (which asks for 4-byte alignment only, so there is one
//   form for every plane), and keeps them in registers to the store.  The luminance is computed once per loaded pixel, not once
//   per tap: y(q) goes to LDS, one float per pixel of tile + halo of RADIUS, kDespikeNone where q is outside the frame or
//   non-finite.  With the flag an int32 id per pixel stands beside it.  The halo's 84 (radius 1) or 176 (radius 2) pixels are
//   loaded by the first lanes of the workgroup, one each.
// - LDS: (32 + 2R) x (8 + 2R) words at a row pitch of 33 + 2R.  A tap is one ds_read_b32 per wave (or half a ds_read2_b32):
//   the LDS serves it in two groups of 32 lanes, and a group is one row of the tile - 32 consecutive words, 32 distinct banks -
//   so the taps are free of conflicts at any pitch.  The odd pitch is for the staging: a halo column's lanes write words one
//   pitch apart, which an odd pitch spreads over all 32 banks where 32 + 2R would fold them onto 16.
// - The rank largest of up to 24 values is a running top-RANK in RANK registers, a maximum and a minimum per value and register
//   (despike_push): no sort, no array indexed by a lane.  RADIUS, RANK and the flag are template parameters, the taps are
//   unrolled row by row, and a neighbour of another object enters as kDespikeNone.  m < rank is t[RANK-1] < 0: no count is kept.
// - A wave in which no lane has a finite pixel with Y > floor skips the window: one ballot.  Such a pixel is never a spike
//   (L >= floor), so the wave's pixels are copied - or zeroed where non-finite - as the window would have left them, bit for bit.
// - Counters: a ballot and a popcount per wave and counter, one LDS add per wave, then at most two global integer atomics per
//   workgroup; a workgroup with nothing to add issues none, and a call without `out` none of all this.
// - The stores of d_out are 12 bytes per lane and of d_mask one, consecutive along a row.
#include "pt_despike.h"

namespace pt {
namespace {

struct __attribute__((packed, aligned(4))) rgb3 {
    float r, g, b;
};

constexpr uint32_t kDsBlock = kDespikeTileW * kDespikeTileH;

template <int R, int RANK, bool SAME>
__global__ __launch_bounds__(kDsBlock) void k_despike(const DespikeFrame f, uint32_t tiles_x) {
    constexpr int32_t TW = (int32_t)kDespikeTileW, TH = (int32_t)kDespikeTileH;
    constexpr int32_t SW = TW + 2 * R, SH = TH + 2 * R, PITCH = TW + 1 + 2 * R;
    constexpr int32_t HALO_ROWS = 2 * R * SW, HALO = HALO_ROWS + TH * 2 * R;  // at most 176: one lane each
    __shared__ float sh_y[PITCH * SH];
    __shared__ int32_t sh_id[SAME ? PITCH * SH : 1];
    __shared__ uint32_t sh_cnt[2];
    const int32_t W = (int32_t)f.width, H = (int32_t)f.height;
    const int32_t tid = (int32_t)threadIdx.x, tx = tid % TW, ty = tid / TW;
    const int32_t bx = (int32_t)(blockIdx.x % tiles_x) * TW, br = (int32_t)(blockIdx.x / tiles_x) * TH;
    const int32_t x = bx + tx, r = br + ty;
    const bool in_frame = x < W && r < H;
    const uint32_t idx = (uint32_t)r * f.width + (uint32_t)x;  // (used in_frame only)

    // the lane's own pixel: registers, and its y into the stage
    rgb3 c = {0.0f, 0.0f, 0.0f};
    int32_t own_id = 0;
    float yc = kDespikeNone;
    if (in_frame) {
        c = *reinterpret_cast<const rgb3 *>(f.rgb + (size_t)idx * 3u);
        yc = despike_y(c.r, c.g, c.b);
        if (SAME) own_id = f.object_id[idx];
    }
    sh_y[(ty + R) * PITCH + tx + R] = yc;
    if (SAME) sh_id[(ty + R) * PITCH + tx + R] = own_id;
    // the halo: R rows above and below over the stage's width, then R columns left and right of the tile's rows
    if (tid < HALO) {
        int32_t sx, sy;
        if (tid < HALO_ROWS) {
            const int32_t row = tid / SW;
            sx = tid - row * SW;
            sy = row < R ? row : row + TH;
        } else {
            const int32_t k = tid - HALO_ROWS, row = k / (2 * R), col = k - row * (2 * R);
            sx = col < R ? col : col + TW;
            sy = R + row;
        }
        const int32_t qx = bx - R + sx, qr = br - R + sy;
        float yq = kDespikeNone;
        int32_t idq = 0;
        if (qx >= 0 && qx < W && qr >= 0 && qr < H) {
            const uint32_t q = (uint32_t)qr * f.width + (uint32_t)qx;
            const rgb3 v = *reinterpret_cast<const rgb3 *>(f.rgb + (size_t)q * 3u);
            yq = despike_y(v.r, v.g, v.b);
            if (SAME) idq = f.object_id[q];
        }
        sh_y[sy * PITCH + sx] = yq;
        if (SAME) sh_id[sy * PITCH + sx] = idq;
    }
    const bool count = f.counters != nullptr;  // uniform: a kernel argument
    if (count && tid < 2) sh_cnt[tid] = 0u;
    __syncthreads();

    const bool nonfinite = in_frame && yc < 0.0f;
    const float v[3] = {c.r, c.g, c.b};
    float o[3] = {c.r, c.g, c.b};
    uint32_t m = kDespikeCopied;
    if (nonfinite) {
        o[0] = o[1] = o[2] = 0.0f;
        m = kDespikeNonfinite;
    }
    // a finite pixel with Y <= floor is copied whatever its window holds: the wave skips the window where all are such
    const bool candidate = in_frame && !nonfinite && despike_luma(c.r, c.g, c.b) > f.floor;
    if (__builtin_amdgcn_ballot_w64(candidate) != 0ull) {
        float t[RANK];
#pragma unroll
        for (int k = 0; k < RANK; ++k) t[k] = kDespikeNone;
#pragma unroll
        for (int32_t dy = 0; dy <= 2 * R; ++dy) {
#pragma unroll
            for (int32_t dx = 0; dx <= 2 * R; ++dx) {
                if (dy == R && dx == R) continue;
                const int32_t at = (ty + dy) * PITCH + tx + dx;
                float yq = sh_y[at];
                if (SAME) yq = sh_id[at] == own_id ? yq : kDespikeNone;
                despike_push<RANK>(t, yq);
            }
        }
        if (candidate) m = despike_verdict(f.threshold, f.floor, t[RANK - 1], v, o);
    }
    if (in_frame) {
        *reinterpret_cast<rgb3 *>(f.out + (size_t)idx * 3u) = rgb3{o[0], o[1], o[2]};
        if (f.mask) f.mask[idx] = (uint8_t)m;
    }
    if (count) {
        const uint32_t ns = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(m == kDespikeSpike));
        const uint32_t nn = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(m == kDespikeNonfinite));
        if ((tid & 63) == 0) {
            if (ns) atomicAdd(&sh_cnt[0], ns);
            if (nn) atomicAdd(&sh_cnt[1], nn);
        }
        __syncthreads();
        if (tid < 2 && sh_cnt[tid]) atomicAdd(f.counters + tid, (unsigned long long)sh_cnt[tid]);
    }
}

template <int R, int RANK>
void launch_flag(hipStream_t st, const DespikeFrame &f, dim3 grid, uint32_t tiles_x) {
    if (f.object_id)
        hipLaunchKernelGGL((k_despike<R, RANK, true>), grid, dim3(kDsBlock), 0, st, f, tiles_x);
    else
        hipLaunchKernelGGL((k_despike<R, RANK, false>), grid, dim3(kDsBlock), 0, st, f, tiles_x);
}

template <int R>
void launch_rank(hipStream_t st, const DespikeFrame &f, dim3 grid, uint32_t tiles_x) {
    switch (f.rank) {  // 1..4 (host::check_despike)
        case 1u: return launch_flag<R, 1>(st, f, grid, tiles_x);
        case 2u: return launch_flag<R, 2>(st, f, grid, tiles_x);
        case 3u: return launch_flag<R, 3>(st, f, grid, tiles_x);
        default: return launch_flag<R, 4>(st, f, grid, tiles_x);
    }
}

}  // namespace

void launch_despike(hipStream_t st, const DespikeFrame &f) {
    // a grid of one dimension, as pt_overlay.hip's: at most 2^28 pixels, so at most 2^25 tiles (a frame one pixel wide)
    const uint32_t tiles_x = (f.width + kDespikeTileW - 1u) / kDespikeTileW, tiles_y = (f.height + kDespikeTileH - 1u) / kDespikeTileH;
    const dim3 grid(tiles_x * tiles_y);
    if (f.radius == 1u)
        launch_rank<1>(st, f, grid, tiles_x);
    else
        launch_rank<2>(st, f, grid, tiles_x);
}

}  // namespace pt
