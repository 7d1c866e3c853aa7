// pt_adaptive.hip — pt_ctx_render_adaptive's kernels beside the tile pass: what happens to the compact accumulator after a run
// of a level (k_tile_level) and the resolve with a count per tile (k_tile_resolve).  The estimate's arithmetic is the contract of
// include/ptrace.h ("THE NOISE ESTIMATE"), operation for operation as pt_noise.hip states it; this unit is built like that one
// (-ffp-contract=off, correctly rounded / and sqrt, no -mllvm options), so tests/adaptive_ref.py gives the same bytes.
//
// k_tile_level: memory-bound, 24 B read of the compact accumulator and up to 96 B read-modify-write of the sums per pixel of an
// open tile.  A workgroup of 256 takes whole tiles - 16, 4 or 1 of them at tile edge 4, 8 or 16, a quarter of a tile per trip at
// 32 - so every pixel of the frame is one thread's alone (plain read-modify-write, no atomics on the sums), a tile's E is summed
// with integer LDS atomics (the order does not matter), and the one thread that ends up holding a tile's E decides: the tile's
// count and E are stored, a tile that stays open is appended to the next list through one global integer atomic on its length,
// a tile that closes adds one to the level's counter.  The host reads those two words back and nothing else.
#include "pt_tile.h"

namespace pt {
namespace {

constexpr uint32_t kTileBlock = 256;
constexpr uint32_t kTileMaxPerBlock = 16;  // tiles of edge 4 in a workgroup

__device__ __forceinline__ float ts_clamp(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
// k_resolve's conversion of a 32.32 sum over n samples, clamped as the displayed frame is
__device__ __forceinline__ float ts_mean(unsigned long long s, float n) {
    return ts_clamp((float)((double)s * (1.0 / 4294967296.0)) / n);
}

__global__ __launch_bounds__(kTileBlock) void k_tile_level(TileGrid G, TileLevel V, unsigned long long *__restrict__ held,
                                                           unsigned long long *__restrict__ half_a, float *__restrict__ error) {
    __shared__ unsigned long long s_err[kTileMaxPerBlock];
    __shared__ uint32_t s_pix[kTileMaxPerBlock];
    const uint32_t sh2 = 2u * G.tile_shift, tile_px = 1u << sh2, edge = 1u << G.tile_shift;
    const uint32_t per_block = tile_px >= kTileBlock ? 1u : kTileBlock >> sh2;  // tiles of this workgroup
    const uint32_t trips = tile_px >= kTileBlock ? tile_px / kTileBlock : 1u;
    if (threadIdx.x < kTileMaxPerBlock) {
        s_err[threadIdx.x] = 0ull;
        s_pix[threadIdx.x] = 0u;
    }
    __syncthreads();
    const size_t plane = (size_t)G.width * G.rows, cplane = (size_t)V.n_open << sh2;
    for (uint32_t k = 0; k < trips; ++k) {
        const uint32_t i = k * kTileBlock + threadIdx.x;  // entry of this workgroup's tiles
        const uint32_t local = i >> sh2, q = i & (tile_px - 1u);
        const uint32_t slot = blockIdx.x * per_block + local;
        if (slot >= V.n_open) continue;
        const uint32_t t = V.open[slot];
        const uint32_t ty = t / G.tiles_x, tx = t - ty * G.tiles_x;
        const uint32_t col = (tx << G.tile_shift) + (q & (edge - 1u)), row = (ty << G.tile_shift) + (q >> G.tile_shift);
        if (col >= G.width || row >= G.rows) continue;
        const size_t p = (size_t)row * G.width + col, at = ((size_t)slot << sh2) + q;
        float d[3], m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long v = V.acc[(size_t)c * cplane + at];
            const unsigned long long h = held[(size_t)c * plane + p] + v;
            unsigned long long a = half_a[(size_t)c * plane + p];
            if (v) held[(size_t)c * plane + p] = h;
            if (V.to_a) {
                a += v;
                if (v) half_a[(size_t)c * plane + p] = a;
            }
            const float va = ts_mean(a, V.fa), vb = ts_mean(h - a, V.fb);
            d[c] = __builtin_fabsf(va - vb);
            m[c] = ts_mean(h, V.fn);
        }
        if (V.estimate) {
            const float e = (((d[0] + d[1]) + d[2]) * V.w) / __builtin_sqrtf(0.015625f + ((m[0] + m[1]) + m[2]));
            if (error) error[p] = e;
            atomicAdd(&s_err[local], (unsigned long long)(e * 268435456.0f));  // floor(e * 2^28): the product is exact, e <= 12
            atomicAdd(&s_pix[local], 1u);
        }
    }
    if (!V.evaluate) return;
    __syncthreads();
    if (threadIdx.x < per_block) {
        const uint32_t slot = blockIdx.x * per_block + threadIdx.x;
        if (slot < V.n_open) {
            const uint32_t t = V.open[slot];
            G.spp[t] = V.spp;
            bool closes = false;
            if (V.estimate) {
                const unsigned long long E = s_err[threadIdx.x];
                G.err[t] = E;
                closes = E <= V.q * (unsigned long long)s_pix[threadIdx.x];
            }
            if (closes)
                atomicAdd(&V.counters[1], 1u);
            else
                V.next[atomicAdd(&V.counters[0], 1u)] = t;
        }
    }
}

__global__ __launch_bounds__(kTileBlock) void k_tile_resolve(TileGrid G, const unsigned long long *__restrict__ held, float *__restrict__ out,
                                                             uint32_t *__restrict__ spp, unsigned long long *__restrict__ err_sum) {
    const uint32_t npix = G.width * G.rows;
    for (uint32_t p = blockIdx.x * kTileBlock + threadIdx.x; p < npix; p += gridDim.x * kTileBlock) {
        const uint32_t row = p / G.width, col = p - row * G.width;
        const uint32_t n = G.spp[(row >> G.tile_shift) * G.tiles_x + (col >> G.tile_shift)];
        if (spp) spp[p] = n;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double sum = (double)held[(size_t)c * npix + p] * (1.0 / 4294967296.0);
            out[(size_t)p * 3 + c] = n ? ts_clamp((float)sum / (float)n) : 0.0f;  // (k_resolve's arithmetic)
        }
    }
    if (err_sum)
        for (uint32_t t = blockIdx.x * kTileBlock + threadIdx.x; t < G.tiles; t += gridDim.x * kTileBlock) {
            const unsigned long long E = G.err[t];
            if (E != kTileNoError && E != 0ull) atomicAdd(err_sum, E);
        }
}

__global__ __launch_bounds__(kTileBlock) void k_tile_begin(float *__restrict__ error, uint32_t npix, uint32_t *__restrict__ open,
                                                           uint32_t tiles) {
    for (uint32_t p = blockIdx.x * kTileBlock + threadIdx.x; p < npix; p += gridDim.x * kTileBlock)
        if (error) error[p] = __builtin_inff();
    for (uint32_t t = blockIdx.x * kTileBlock + threadIdx.x; t < tiles; t += gridDim.x * kTileBlock) open[t] = t;
}

dim3 stride_grid(uint32_t n) {
    const uint32_t blocks = (n + kTileBlock - 1) / kTileBlock;
    return dim3(blocks == 0u ? 1u : (blocks < 2048u ? blocks : 2048u));
}

}  // namespace

void launch_tile_level(hipStream_t st, const TileGrid &G, const TileLevel &V, unsigned long long *held, unsigned long long *half_a,
                       float *error) {
    if (V.n_open == 0u) return;
    const uint32_t tile_px = 1u << (2u * G.tile_shift);
    const uint32_t per_block = tile_px >= kTileBlock ? 1u : kTileBlock / tile_px;
    hipLaunchKernelGGL(k_tile_level, dim3((V.n_open + per_block - 1u) / per_block), dim3(kTileBlock), 0, st, G, V, held, half_a, error);
}

void launch_tile_resolve(hipStream_t st, const TileGrid &G, const unsigned long long *held, float *out_rgb, uint32_t *spp,
                         unsigned long long *err_sum) {
    hipLaunchKernelGGL(k_tile_resolve, stride_grid(G.width * G.rows), dim3(kTileBlock), 0, st, G, held, out_rgb, spp, err_sum);
}

void launch_tile_begin(hipStream_t st, float *error, uint32_t npix, uint32_t *open, uint32_t tiles) {
    hipLaunchKernelGGL(k_tile_begin, stride_grid(npix > tiles ? npix : tiles), dim3(kTileBlock), 0, st, error, npix, open, tiles);
}

}  // namespace pt
