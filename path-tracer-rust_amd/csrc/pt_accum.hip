// pt_accum.hip — pixel-order held sums <-> stream-major frame accumulators (pt_ctx_accumulate).  Two memory-bound copies,
// 24 B per pixel each way; the sums are u64 32.32 fixed point, so a copy moves them exactly.
#include "pt_accum.h"

namespace pt {

namespace {

constexpr uint32_t kAccBlock = 256;
constexpr uint32_t kAccMaxGrid = 8192;  // blocks per colour plane; each thread loops over the rest

// grid.y = colour plane.  i runs over the K * m slots of plane c: slot i is pixel j = i % m of stream b = i / m, p = j * K + b.
__global__ __launch_bounds__(kAccBlock) void k_accum_gather(const unsigned long long *__restrict__ held, uint32_t stride, uint32_t npix,
                                                            uint32_t K, uint32_t m, unsigned long long *__restrict__ acc) {
    const uint32_t c = blockIdx.y, slots = K * m;
    const unsigned long long *src = held + (size_t)c * stride;
    unsigned long long *dst = acc + (size_t)c * slots;
    for (uint32_t i = blockIdx.x * kAccBlock + threadIdx.x; i < slots; i += gridDim.x * kAccBlock) {
        const uint32_t b = i / m, j = i - b * m;
        const uint64_t p = (uint64_t)j * K + b;
        dst[i] = p < npix ? src[p] : 0ull;
    }
}

// i runs over the npix pixels of plane c (p < npix <= K * m, so p / K < m)
__global__ __launch_bounds__(kAccBlock) void k_accum_scatter(const unsigned long long *__restrict__ acc, uint32_t npix, uint32_t K,
                                                             uint32_t m, unsigned long long *__restrict__ held, uint32_t stride) {
    const uint32_t c = blockIdx.y;
    const unsigned long long *src = acc + (size_t)c * K * m;
    unsigned long long *dst = held + (size_t)c * stride;
    for (uint32_t p = blockIdx.x * kAccBlock + threadIdx.x; p < npix; p += gridDim.x * kAccBlock)
        dst[p] = src[(size_t)(p % K) * m + p / K];
}

// k_accum_scatter for a job whose samples go to half A of a noise-tracked frame (pt_ctx_accum_track_noise): what the job added
// to a pixel - the new sum minus the one held before, exact in u64 - is added to A in the same pass over the pixels
__global__ __launch_bounds__(kAccBlock) void k_accum_scatter_half(const unsigned long long *__restrict__ acc, uint32_t npix, uint32_t K,
                                                                  uint32_t m, unsigned long long *__restrict__ held,
                                                                  unsigned long long *__restrict__ half_a, uint32_t stride) {
    const uint32_t c = blockIdx.y;
    const unsigned long long *src = acc + (size_t)c * K * m;
    unsigned long long *dst = held + (size_t)c * stride, *da = half_a + (size_t)c * stride;
    for (uint32_t p = blockIdx.x * kAccBlock + threadIdx.x; p < npix; p += gridDim.x * kAccBlock) {
        const unsigned long long v = src[(size_t)(p % K) * m + p / K];
        da[p] += v - dst[p];
        dst[p] = v;
    }
}

dim3 grid_for(uint32_t n) {
    const uint32_t blocks = (n + kAccBlock - 1) / kAccBlock;
    return dim3(blocks == 0u ? 1u : (blocks < kAccMaxGrid ? blocks : kAccMaxGrid), 3);
}

}  // namespace

void launch_accum_gather(hipStream_t st, const unsigned long long *held, uint32_t stride, uint32_t npix, uint32_t K, uint32_t m,
                         unsigned long long *acc) {
    hipLaunchKernelGGL(k_accum_gather, grid_for(K * m), dim3(kAccBlock), 0, st, held, stride, npix, K, m, acc);
}

void launch_accum_scatter(hipStream_t st, const unsigned long long *acc, uint32_t npix, uint32_t K, uint32_t m,
                          unsigned long long *held, uint32_t stride) {
    hipLaunchKernelGGL(k_accum_scatter, grid_for(npix), dim3(kAccBlock), 0, st, acc, npix, K, m, held, stride);
}

void launch_accum_scatter_half(hipStream_t st, const unsigned long long *acc, uint32_t npix, uint32_t K, uint32_t m,
                               unsigned long long *held, unsigned long long *half_a, uint32_t stride) {
    hipLaunchKernelGGL(k_accum_scatter_half, grid_for(npix), dim3(kAccBlock), 0, st, acc, npix, K, m, held, half_a, stride);
}

}  // namespace pt
