// pt_accum.h — the two copies between the sums pt_ctx_accumulate holds across calls and a frame's accumulators
// (pt_accum.hip).  A translation unit of their own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pt {

// held: the part's first pixel in the held sums, [3] colour planes of `stride` u64 in pixel order (k_resolve's n_streams = 1).
// acc: the frame's accumulators, stream-major - pixel p at slot (p % K) * m + p / K of each of 3 planes of K * m (K = 1,
// m = npix: the megakernel's pixel order).  Needs K * m >= npix.

// held -> acc: writes EVERY one of the 3 * K * m slots, zero where p >= npix, so it stands in for the memset of a fresh frame
void launch_accum_gather(hipStream_t st, const unsigned long long *held, uint32_t stride, uint32_t npix, uint32_t K, uint32_t m,
                         unsigned long long *acc);
// acc -> held, the npix pixels of the part
void launch_accum_scatter(hipStream_t st, const unsigned long long *acc, uint32_t npix, uint32_t K, uint32_t m,
                          unsigned long long *held, uint32_t stride);
// the same, for a job of a noise-tracked frame whose samples go to half A: half_a (laid out as held) += new sum - held sum
void launch_accum_scatter_half(hipStream_t st, const unsigned long long *acc, uint32_t npix, uint32_t K, uint32_t m,
                               unsigned long long *held, unsigned long long *half_a, uint32_t stride);

}  // namespace pt
