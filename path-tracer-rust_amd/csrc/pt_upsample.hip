// pt_upsample.hip — pt_ctx_upsample's kernel: a low-resolution frame gathered into the full frame's pixels through the guides of
// both.  The arithmetic is the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_upsample), operation for operation; the
// pixel is pt_upsample.h's upsample_pixel, which the host compiles too.  Built with -ffp-contract=off and correctly rounded / and
// sqrt, so a restatement in numpy binary32 (tests/upsample_ref.py) gives the same bytes.
//
// Memory-bound: per frame pixel 32 B of its own guides read at most (id, depth, normal, albedo) and 12 or 16 B written; a
// low-resolution pixel is 44 B at most (colour, id, depth, normal, albedo), shared by about 4 * (W/w) * (H/h) lanes.  One lane per
// frame pixel, a plain gather.  Consecutive lanes take consecutive pixels, so a wave's loads of its own planes are whole lines - read
// once, non-temporal, past the L1 - and its taps fall on W/w times fewer low-resolution pixels than it has lanes: the repeats are
// served by L1 within the wave and by L2 between rows, on the default policy.  All taps are read before the first is tested
// (upsample_pixel): one round trip.  The position of the taps takes three integer divisions by values the whole call shares (W, 2W,
// 2H); the host turns each into a multiplier and a shift (UpsampleDiv), so a lane spends three 64-bit products on them.
// No LDS: see DESIGN.md section 4.
#include "pt_upsample.h"

namespace pt {
namespace {

constexpr uint32_t kUpsampleBlock = 256;

// one instance per set of optional planes: straight-line code, every load issued before the first use
template <bool NORMALS, bool DEMOD>
__global__ __launch_bounds__(kUpsampleBlock) void k_upsample(const UpsampleFrame f, uint32_t npix) {
    const uint32_t idx = blockIdx.x * kUpsampleBlock + threadIdx.x;
    if (idx >= npix) return;
    float out[3], weight;
    upsample_pixel_t<NORMALS, DEMOD>(f, idx, out, &weight);
    float *o = f.out_color + (size_t)idx * 3u;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    if (f.out_weight) f.out_weight[idx] = weight;
}

}  // namespace

void launch_upsample(hipStream_t st, const UpsampleFrame &f) {
    const uint32_t npix = f.width * f.height;  // at most 2^28: 2^20 workgroups
    const dim3 grid((npix + kUpsampleBlock - 1u) / kUpsampleBlock), block(kUpsampleBlock);
    if (f.normal) {
        if (f.albedo)
            hipLaunchKernelGGL((k_upsample<true, true>), grid, block, 0, st, f, npix);
        else
            hipLaunchKernelGGL((k_upsample<true, false>), grid, block, 0, st, f, npix);
    } else {
        if (f.albedo)
            hipLaunchKernelGGL((k_upsample<false, true>), grid, block, 0, st, f, npix);
        else
            hipLaunchKernelGGL((k_upsample<false, false>), grid, block, 0, st, f, npix);
    }
}

}  // namespace pt
