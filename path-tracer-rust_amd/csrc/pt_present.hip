// pt_present.hip — pt_ctx_present's kernels: a linear float frame to gamma-corrected 8-bit pixels at the size asked for, in
// display order.  The arithmetic is the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_present), operation for
// operation; its per-value steps are pt_present.h's, which the host compiles too.  Built with -ffp-contract=off.  The eight bits
// come from the 1 KB threshold table in LDS (eight compares per channel, no branch, no powf on the device).
//
// Memory-bound, both forms.
// - Same size (k_present_same): a stream, 12 B read and 4 or 3 B written per pixel.  Consecutive lanes take consecutive OUTPUT
//   pixels in a grid-stride loop, as pt_noise.hip does; in display order the source runs backwards, which the coalescer does not
//   mind.  RGBA8 packs a pixel into one dword store.
// - Another size: two passes over an integer intermediate, rows first.  k_present_rows folds the source rows an output row covers
//   into one row of u64 sums per channel: a lane per source column, consecutive lanes consecutive pixels, so every source value
//   is fetched from HBM once, in full cache lines, whatever the ratio - and the number of lanes is width * out_height, not the
//   number of output pixels (4096 x 4096 -> 64 x 64: 262144 lanes, 4096 waves).  k_present_cols folds the columns an output pixel
//   covers, divides, looks the bytes up and stores them.  Its input is out_height / height of the first pass's (24 B per
//   element); when many columns fold into one, `group` lanes share an output pixel and add their partial sums with a butterfly.
//   The sums are integers: neither the split into passes nor the order of the adds changes a bit.
#include "pt_present.h"

namespace pt {
namespace {

constexpr uint32_t kPresentBlock = 256;   // = the table's length: one entry per thread into LDS
constexpr uint32_t kPresentMaxGrid = 2048;  // 256 CUs x 8 workgroups; each thread loops over the rest
constexpr uint32_t kPresentMaxGridY = 32768;

__device__ __forceinline__ void load_table(uint32_t *s_T, const uint32_t *__restrict__ table) {
    s_T[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
}

template <uint32_t BPP>
__device__ __forceinline__ void store_pixel(uint8_t *__restrict__ out, uint32_t o, uint32_t r, uint32_t g, uint32_t b) {
    if (BPP == 4u) {
        reinterpret_cast<uint32_t *>(out)[o] = r | (g << 8) | (b << 16) | 0xff000000u;
    } else {
        uint8_t *px = out + (size_t)o * 3u;
        px[0] = (uint8_t)r;
        px[1] = (uint8_t)g;
        px[2] = (uint8_t)b;
    }
}

template <uint32_t BPP>
__global__ __launch_bounds__(kPresentBlock) void k_present_same(const float *__restrict__ rgb, uint8_t *__restrict__ out, uint32_t npix,
                                                                uint32_t flip, float exposure, const uint32_t *__restrict__ table) {
    __shared__ uint32_t s_T[256];
    load_table(s_T, table);
    for (uint32_t o = blockIdx.x * kPresentBlock + threadIdx.x; o < npix; o += gridDim.x * kPresentBlock) {
        const float *v = rgb + (size_t)(flip ? npix - 1u - o : o) * 3u;
        uint32_t b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = present_byte(s_T, present_bits(present_clamp(v[c], exposure)));
        store_pixel<BPP>(out, o, b[0], b[1], b[2]);
    }
}

// mid[c][Y][x] = sum over the source rows y of output row Y of wy(Y, y) * q(D(x, y)[c]), x a display column
__global__ __launch_bounds__(kPresentBlock) void k_present_rows(const float *__restrict__ rgb, unsigned long long *__restrict__ mid,
                                                                uint32_t W, uint32_t H, uint32_t OH, uint32_t flip, float exposure) {
    const uint32_t npix = W * H;
    const size_t plane = (size_t)W * OH;
    for (uint32_t Y = blockIdx.y; Y < OH; Y += gridDim.y) {
        const PresentSpan sp = present_span(Y, H, OH);
        for (uint32_t x = blockIdx.x * kPresentBlock + threadIdx.x; x < W; x += gridDim.x * kPresentBlock) {
            unsigned long long acc[3] = {0ull, 0ull, 0ull};
            for (uint32_t y = sp.first; y < sp.last; ++y) {
                const unsigned long long wy = present_weight(Y, y, H, OH);
                const uint32_t p = y * W + x;
                const float *v = rgb + (size_t)(flip ? npix - 1u - p : p) * 3u;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += wy * present_fixed(present_clamp(v[c], exposure));
            }
            const size_t at = (size_t)Y * W + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) mid[(size_t)c * plane + at] = acc[c];
        }
    }
}

// out(X, Y) from S[c] = sum over the columns x of output column X of wx(X, x) * mid[c][Y][x].  `group` (a power of two up to 64)
// consecutive lanes share an output pixel.
template <uint32_t BPP>
__global__ __launch_bounds__(kPresentBlock) void k_present_cols(const unsigned long long *__restrict__ mid, uint8_t *__restrict__ out,
                                                                uint32_t W, uint32_t OW, uint32_t OH, uint32_t group, double divisor,
                                                                const uint32_t *__restrict__ table) {
    __shared__ uint32_t s_T[256];
    load_table(s_T, table);
    const size_t plane = (size_t)W * OH;
    const uint32_t per_block = kPresentBlock / group, sub = threadIdx.x & (group - 1u);
    for (uint32_t Y = blockIdx.y; Y < OH; Y += gridDim.y) {
        const unsigned long long *row = mid + (size_t)Y * W;
        // (the lanes of a group share X: they leave this loop together, and the butterfly stays inside the group)
        for (uint32_t X = blockIdx.x * per_block + threadIdx.x / group; X < OW; X += gridDim.x * per_block) {
            const PresentSpan sp = present_span(X, W, OW);
            unsigned long long S[3] = {0ull, 0ull, 0ull};
            for (uint32_t x = sp.first + sub; x < sp.last; x += group) {
                const unsigned long long wx = present_weight(X, x, W, OW);
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += wx * row[(size_t)c * plane + x];
            }
            for (uint32_t o = group >> 1; o; o >>= 1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += __shfl_xor(S[c], (int)o);
            }
            if (sub == 0u) {
                uint32_t b[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) b[c] = present_byte(s_T, present_bits(present_mean(S[c], divisor)));
                store_pixel<BPP>(out, Y * OW + X, b[0], b[1], b[2]);
            }
        }
    }
}

// the workgroups for n items at per_block each: at most cap, and as few as give every workgroup the same number of turns of the
// grid-stride loop (3072 workgroups' worth under a cap of 2048: 1536 take two each, not 1024 two and 1024 one)
uint32_t grid_for(uint32_t n, uint32_t per_block, uint32_t cap) {
    const uint32_t blocks = (n + per_block - 1u) / per_block;
    if (blocks <= 1u) return 1u;
    const uint32_t turns = (blocks + cap - 1u) / cap;
    return (blocks + turns - 1u) / turns;
}

}  // namespace

void launch_present(hipStream_t st, const PresentFrame &f) {
    const uint32_t flip = f.flip ? 1u : 0u;
    if (!f.mid) {
        const uint32_t npix = f.width * f.height;
        const dim3 grid(grid_for(npix, kPresentBlock, kPresentMaxGrid));
        if (f.bpp == 4u)
            hipLaunchKernelGGL(k_present_same<4u>, grid, dim3(kPresentBlock), 0, st, f.rgb, f.out, npix, flip, f.exposure, f.table);
        else
            hipLaunchKernelGGL(k_present_same<3u>, grid, dim3(kPresentBlock), 0, st, f.rgb, f.out, npix, flip, f.exposure, f.table);
        return;
    }
    const uint32_t gy = f.out_height < kPresentMaxGridY ? f.out_height : kPresentMaxGridY;
    hipLaunchKernelGGL(k_present_rows, dim3(grid_for(f.width, kPresentBlock, kPresentMaxGrid), gy), dim3(kPresentBlock), 0, st, f.rgb,
                       f.mid, f.width, f.height, f.out_height, flip, f.exposure);
    // lanes per output pixel: a quarter of the columns it folds, as a power of two, at most a wave
    uint32_t group = 1u;
    while (group < 64u && (uint64_t)group * 8u * f.out_width <= f.width) group <<= 1;
    const double divisor = (double)((uint64_t)f.width * f.height) * 4294967296.0;
    const dim3 grid(grid_for(f.out_width, kPresentBlock / group, kPresentMaxGrid), gy);
    if (f.bpp == 4u)
        hipLaunchKernelGGL(k_present_cols<4u>, grid, dim3(kPresentBlock), 0, st, f.mid, f.out, f.width, f.out_width, f.out_height, group,
                           divisor, f.table);
    else
        hipLaunchKernelGGL(k_present_cols<3u>, grid, dim3(kPresentBlock), 0, st, f.mid, f.out, f.width, f.out_width, f.out_height, group,
                           divisor, f.table);
}

}  // namespace pt
