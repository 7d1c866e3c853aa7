// pt_noise.hip — pt_ctx_accum_noise's kernel: the dual-buffer error estimate of Dammertz, Hanika, Keller and Lensch (2010)
// over a noise-tracked frame.  Half A of every pixel's samples is held next to the whole (pt_ctx_accum_track_noise); half B is
// their difference, exact in u64.  The arithmetic is the contract of include/ptrace.h ("THE NOISE ESTIMATE"), operation for
// operation and in its order; this unit is built with -ffp-contract=off and correctly rounded / and sqrt, so a restatement in
// numpy binary32 (tests/noise_ref.py) gives the same bytes.
//
// Memory-bound: 48 B read (three planes of two buffers) and 4 B written per pixel.  A thread takes whole pixels, consecutive
// lanes consecutive pixels of a plane (8 B per lane, 512 B per wave and load), in a grid-stride loop as pt_accum.hip's copies.
// The frame statistics ride along: every workgroup keeps the histogram and the sum of floor(e * 2^28) in 264 B of LDS (integer
// LDS atomics: the order of the adds does not matter) and ends with one global integer atomic per non-empty bin and one for
// the sum.  No scratch memory beyond those 65 counters.
#include "pt_noise.h"

namespace pt {
namespace {

constexpr uint32_t kNoiseBlock = 256;
constexpr uint32_t kNoiseMaxGrid = 2048;  // 256 CUs x 8 workgroups: every CU full at 32 waves; each thread loops over the rest

__device__ __forceinline__ float ns_clamp(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
// k_resolve's conversion of a 32.32 sum over n samples, clamped as the displayed frame is
__device__ __forceinline__ float ns_mean(unsigned long long s, float n) {
    return ns_clamp((float)((double)s * (1.0 / 4294967296.0)) / n);
}

__global__ __launch_bounds__(kNoiseBlock) void k_noise(const unsigned long long *__restrict__ held,
                                                       const unsigned long long *__restrict__ half_a, uint32_t stride, uint32_t npix,
                                                       float fa, float fb, float fn, float w, float *__restrict__ error,
                                                       NoiseCounters *__restrict__ counters) {
    __shared__ uint32_t s_hist[kNoiseBins];
    __shared__ unsigned long long s_sum;
    if (threadIdx.x < kNoiseBins) s_hist[threadIdx.x] = 0u;
    if (threadIdx.x == kNoiseBins) s_sum = 0ull;
    __syncthreads();
    unsigned long long sum = 0ull;
    for (uint32_t p = blockIdx.x * kNoiseBlock + threadIdx.x; p < npix; p += gridDim.x * kNoiseBlock) {
        float d[3], m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long h = held[(size_t)c * stride + p], a = half_a[(size_t)c * stride + p];
            const float va = ns_mean(a, fa), vb = ns_mean(h - a, fb);
            d[c] = __builtin_fabsf(va - vb);
            m[c] = ns_mean(h, fn);
        }
        const float e = (((d[0] + d[1]) + d[2]) * w) / __builtin_sqrtf(0.015625f + ((m[0] + m[1]) + m[2]));
        if (error) error[p] = e;
        sum += (unsigned long long)(e * 268435456.0f);  // floor(e * 2^28): the product is exact, e <= 12
        const uint32_t k = __float_as_uint(e) >> 21;    // sign (0), exponent, two mantissa bits
        const uint32_t bin = k <= 460u ? 0u : (k >= 523u ? 63u : k - 460u);
        atomicAdd(&s_hist[bin], 1u);
    }
    if (sum) atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x < kNoiseBins) {
        const uint32_t v = s_hist[threadIdx.x];
        if (v) atomicAdd(&counters->hist[threadIdx.x], v);
    } else if (threadIdx.x == kNoiseBins) {
        if (s_sum) atomicAdd(&counters->sum, s_sum);
    }
}

__global__ __launch_bounds__(kNoiseBlock) void k_noise_none(float *__restrict__ error, uint32_t npix) {
    for (uint32_t p = blockIdx.x * kNoiseBlock + threadIdx.x; p < npix; p += gridDim.x * kNoiseBlock) error[p] = __builtin_inff();
}

dim3 noise_grid(uint32_t n) {
    const uint32_t blocks = (n + kNoiseBlock - 1) / kNoiseBlock;
    return dim3(blocks == 0u ? 1u : (blocks < kNoiseMaxGrid ? blocks : kNoiseMaxGrid));
}

}  // namespace

void launch_noise(hipStream_t st, const unsigned long long *held, const unsigned long long *half_a, uint32_t stride, uint32_t npix,
                  uint32_t n_a, uint32_t n_b, float w, float *error, NoiseCounters *counters) {
    hipLaunchKernelGGL(k_noise, noise_grid(npix), dim3(kNoiseBlock), 0, st, held, half_a, stride, npix, (float)n_a, (float)n_b,
                       (float)(n_a + n_b), w, error, counters);
}

void launch_noise_none(hipStream_t st, float *error, uint32_t npix) {
    hipLaunchKernelGGL(k_noise_none, noise_grid(npix), dim3(kNoiseBlock), 0, st, error, npix);
}

}  // namespace pt
