// pt_noise.h — the per-pixel noise estimate behind pt_ctx_accum_noise (pt_noise.hip): e(p) from the two halves of a
// noise-tracked frame's samples, its fixed-point sum and its 64-bin histogram in one launch.  The arithmetic is the contract in
// include/ptrace.h, operation for operation.  A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(),
// describes the pass kernels only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pt {

constexpr uint32_t kNoiseBins = 64;
// the counters of one call: the sum of floor(e(p) * 2^28) and the histogram
struct NoiseCounters {
    unsigned long long sum;
    uint32_t hist[kNoiseBins];
};

// One part of the frame: npix pixels whose held sums start at `held` and whose half-A sums start at `half_a`, [3] planes of
// `stride` u64 each.  n_a + n_b samples per pixel, both positive; w = sqrt(n_a * n_b) / (n_a + n_b) (host binary32).
// error: npix floats, or NULL.  Adds to *counters (zeroed by the caller).
void launch_noise(hipStream_t st, const unsigned long long *held, const unsigned long long *half_a, uint32_t stride, uint32_t npix,
                  uint32_t n_a, uint32_t n_b, float w, float *error, NoiseCounters *counters);
// a part without an estimate: +inf for each of its pixels
void launch_noise_none(hipStream_t st, float *error, uint32_t npix);

}  // namespace pt
