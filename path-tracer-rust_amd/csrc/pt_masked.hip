// pt_masked.hip — the kernels of pt_ctx_select_pixels, pt_ctx_render_masked beside the trace, and pt_ctx_spp_plane.  gfx950, wave64.  Built like
// pt_adaptive.hip (-ffp-contract=off, correctly rounded /, no -mllvm options): the scatter's mean is k_resolve's, bit for bit.
//
// k_select: memory-bound, 4 or 8 B read and 1 B written per pixel.  A lane takes four consecutive pixels - one 16-byte load per
// plane, non-temporal (each value is read once), and one 4-byte store of the mask - where the pointers allow it (planes aligned
// to 16 bytes, the mask to 4), single loads and byte stores otherwise and on the frame's last, partial group.  The grid is capped
// and strided, so a lane sums its ones over its trips; a workgroup adds its lanes' sums up with integer LDS atomics, and one
// integer atomic per workgroup goes to the count: at most 2048 of them whatever the frame.  Integer sums: exact, whatever the
// order.
//
// k_masked_compact: 1 B read per pixel, 4 B written per selected pixel.  A lane takes sixteen consecutive mask bytes - one
// 16-byte load where the mask is aligned to 16 bytes, byte loads otherwise and on the last, partial group - and turns them into
// sixteen flags.  Its place among the wave's entries is the prefix of the lanes' counts (0..16: five ballots, one mbcnt pair
// each); the waves' totals meet in LDS, and ONE returning integer atomic per workgroup of 1024 lanes (16 Ki pixels) reserves
// the workgroup's run of the list - a word takes about 88 returning atomics per microsecond chip-wide, so an atomic per wave of
// 64 lanes with 4 bytes each would cost more than the mask's bytes from 1024 x 768 up.  No workgroup waits for another.  The
// order of the list is whatever the atomics' arrival makes it; nothing depends on it.
//
// k_masked_scatter: one lane per list entry, 28 B read, 12 B written at list[k].
#include "pt_masked.h"

namespace pt {
namespace {

constexpr uint32_t kSelectBlock = 256, kSelectMaxGrid = 2048;
constexpr uint32_t kCompactBlock = 1024, kCompactBytes = 16;  // lanes of a workgroup, mask bytes of a lane
constexpr uint32_t kScatterBlock = 256;
constexpr uint32_t kSppBlock = 256, kSppPixels = 16;  // lanes of a workgroup, pixels of a lane

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// position of this lane among the lanes whose bit is set in `m` (the lanes below it)
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the sum over the wave of v (< 2^BITS), and the sum over the lanes below this one: one ballot per bit
template <uint32_t BITS>
__device__ __forceinline__ uint32_t wave_sum(uint32_t v, uint32_t *below) {
    uint32_t total = 0u, pre = 0u;
#pragma unroll
    for (uint32_t b = 0; b < BITS; ++b) {
        const unsigned long long m = __ballot((v >> b) & 1u);
        total += (uint32_t)__popcll(m) << b;
        pre += lanes_below(m) << b;
    }
    *below = pre;
    return total;
}

template <bool VEC>
__global__ __launch_bounds__(kSelectBlock) void k_select(const SelectFrame f) {
    __shared__ uint32_t s_ones;
    if (threadIdx.x == 0) s_ones = 0u;
    __syncthreads();
    const uint32_t groups = (f.npix + 3u) / 4u;
    const bool has_w = f.weight != nullptr, has_l = f.len != nullptr;
    uint32_t ones = 0u;  // at most 4 * trips < 2^28
    for (uint32_t g = blockIdx.x * kSelectBlock + threadIdx.x; g < groups; g += gridDim.x * kSelectBlock) {
        const uint32_t p0 = g * 4u;
        if (VEC && p0 + 4u <= f.npix) {
            f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f}, l = w;
            if (has_w) w = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(f.weight + p0));
            if (has_l) l = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(f.len + p0));
            uint32_t word = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t b = select_test(has_w, w[j], f.weight_max, has_l, l[j], f.len_max);
                word |= b << (8u * j);
                ones += b;
            }
            *reinterpret_cast<uint32_t *>(f.mask + p0) = word;
        } else {
            const uint32_t end = p0 + 4u < f.npix ? p0 + 4u : f.npix;
            for (uint32_t p = p0; p < end; ++p) {
                const uint32_t b = select_pixel(f, p);
                f.mask[p] = (uint8_t)b;
                ones += b;
            }
        }
    }
    if (ones) atomicAdd(&s_ones, ones);
    __syncthreads();
    if (threadIdx.x == 0 && s_ones) atomicAdd(f.count, s_ones);
}

template <bool VEC>
__global__ __launch_bounds__(kCompactBlock) void k_masked_compact(const uint8_t *__restrict__ mask, uint32_t n, uint32_t *__restrict__ list,
                                                                  uint32_t cap, uint32_t *__restrict__ len) {
    __shared__ uint32_t s_wave[kCompactBlock / 64u];
    // n < 2^31, so p0 < 2^31 + 16 Ki for every lane of the grid: 32 bits hold it
    const uint32_t p0 = (blockIdx.x * kCompactBlock + threadIdx.x) * kCompactBytes;
    uint32_t flags = 0u;  // bit j: mask[p0 + j] != 0
    if (p0 < n) {
        if (VEC && p0 + kCompactBytes <= n) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(mask + p0);
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) flags |= ((v[q] >> (8u * j)) & 0xffu) ? 1u << (4u * q + j) : 0u;
            }
        } else {
            const uint32_t end = p0 + kCompactBytes < n ? p0 + kCompactBytes : n;
            for (uint32_t p = p0; p < end; ++p) flags |= mask[p] ? 1u << (p - p0) : 0u;
        }
    }
    uint32_t below = 0u;
    const uint32_t total = wave_sum<5>((uint32_t)__popc(flags), &below);  // a lane's count is 0..16
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_wave[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {  // the waves' totals become the waves' first slots
        uint32_t sum = 0u;
        for (uint32_t w = 0; w < kCompactBlock / 64u; ++w) sum += s_wave[w];
        uint32_t at = sum ? atomicAdd(len, sum) : 0u;
        for (uint32_t w = 0; w < kCompactBlock / 64u; ++w) {
            const uint32_t t = s_wave[w];
            s_wave[w] = at;
            at += t;
        }
    }
    __syncthreads();
    uint32_t slot = s_wave[wave] + below;
    while (flags) {
        const uint32_t j = (uint32_t)__builtin_ctz(flags);
        flags &= flags - 1u;
        if (slot < cap) list[slot] = p0 + j;
        ++slot;
    }
}

__global__ __launch_bounds__(kScatterBlock) void k_masked_scatter(const uint32_t *__restrict__ list, uint32_t n,
                                                                  const unsigned long long *__restrict__ acc, float spp,
                                                                  float *__restrict__ rgb) {
    const uint32_t k = blockIdx.x * kScatterBlock + threadIdx.x;
    if (k >= n) return;
    float *out = rgb + (size_t)list[k] * 3u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double sum = (double)acc[(size_t)c * n + k] * (1.0 / 4294967296.0);
        out[c] = clamp01((float)sum / spp);  // (k_resolve's arithmetic)
    }
}

// k_spp_plane (pt_ctx_spp_plane): 1 B read and 4 B written per pixel.  A lane takes sixteen consecutive pixels: one 16-byte
// load of the mask, non-temporal (each byte is read once), and four 16-byte stores of counts - plain stores, the next pass reads
// the plane - where the pointers allow it (both aligned to 16 bytes); byte loads and single stores otherwise and on the frame's
// last, partial group.  Without a mask nothing is read.
template <bool VEC>
__global__ __launch_bounds__(kSppBlock) void k_spp_plane(const uint8_t *__restrict__ mask, uint32_t n, uint32_t base, uint32_t masked,
                                                         uint32_t *__restrict__ spp) {
    // n <= 2^28 and the grid covers it in whole workgroups: p0 < 2^28 + 4096
    const uint32_t p0 = (blockIdx.x * kSppBlock + threadIdx.x) * kSppPixels;
    if (p0 >= n) return;
    if (VEC && p0 + kSppPixels <= n) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (mask) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(mask + p0));
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            u32x4 o;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) o[j] = spp_plane_value((v[q] >> (8u * j)) & 0xffu, base, masked);
            *reinterpret_cast<u32x4 *>(spp + p0 + 4u * q) = o;
        }
    } else {
        const uint32_t end = p0 + kSppPixels < n ? p0 + kSppPixels : n;
        for (uint32_t p = p0; p < end; ++p) spp[p] = spp_plane_value(mask ? mask[p] : 0u, base, masked);
    }
}

bool aligned(const void *p, uintptr_t to) { return p == nullptr || ((uintptr_t)p & (to - 1u)) == 0u; }

}  // namespace

void launch_spp_plane(hipStream_t st, const uint8_t *mask, uint32_t n, uint32_t base, uint32_t masked, uint32_t *spp) {
    constexpr uint32_t per_block = kSppBlock * kSppPixels;
    const dim3 grid((n + per_block - 1u) / per_block), block(kSppBlock);  // n >= 1
    if (aligned(mask, 16u) && aligned(spp, 16u))
        hipLaunchKernelGGL((k_spp_plane<true>), grid, block, 0, st, mask, n, base, masked, spp);
    else
        hipLaunchKernelGGL((k_spp_plane<false>), grid, block, 0, st, mask, n, base, masked, spp);
}

void launch_select(hipStream_t st, const SelectFrame &f) {
    const uint32_t blocks = ((f.npix + 3u) / 4u + kSelectBlock - 1u) / kSelectBlock;  // npix >= 1
    const dim3 grid(blocks < kSelectMaxGrid ? blocks : kSelectMaxGrid), block(kSelectBlock);
    if (aligned(f.weight, 16u) && aligned(f.len, 16u) && aligned(f.mask, 4u))
        hipLaunchKernelGGL((k_select<true>), grid, block, 0, st, f);
    else
        hipLaunchKernelGGL((k_select<false>), grid, block, 0, st, f);
}

void launch_masked_compact(hipStream_t st, const uint8_t *mask, uint32_t n, uint32_t *list, uint32_t cap, uint32_t *len) {
    constexpr uint32_t per_block = kCompactBlock * kCompactBytes;
    const dim3 grid((uint32_t)(((uint64_t)n + per_block - 1u) / per_block)), block(kCompactBlock);  // n >= 1
    if (aligned(mask, 16u))
        hipLaunchKernelGGL((k_masked_compact<true>), grid, block, 0, st, mask, n, list, cap, len);
    else
        hipLaunchKernelGGL((k_masked_compact<false>), grid, block, 0, st, mask, n, list, cap, len);
}

void launch_masked_scatter(hipStream_t st, const uint32_t *list, uint32_t n, const unsigned long long *acc, uint32_t spp, float *rgb) {
    hipLaunchKernelGGL(k_masked_scatter, dim3((n + kScatterBlock - 1u) / kScatterBlock), dim3(kScatterBlock), 0, st, list, n, acc,
                       (float)spp, rgb);
}

}  // namespace pt
