// pt_reproject.hip — pt_ctx_reproject's kernel: the history frame gathered into this frame's pixels and blended by the history
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

}  // namespace

void launch_reproject(hipStream_t st, const ReprojectFrame &f) {
    const uint32_t npix = f.width * f.height;  // at most 2^28: 2^20 workgroups
    hipLaunchKernelGGL(k_reproject, dim3((npix + kReprojectBlock - 1u) / kReprojectBlock), dim3(kReprojectBlock), 0, st, f, npix);
}

}  // namespace pt
