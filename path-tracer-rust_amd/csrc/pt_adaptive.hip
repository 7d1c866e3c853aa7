// pt_adaptive.hip — the adaptive calls' kernels beside the tile pass: which tiles a step takes (k_tile_select), what happens to
// the compact accumulator after a run of a step (k_tile_level) and the resolve with a count per tile (k_tile_resolve).  The
// estimate's arithmetic is the contract of include/ptrace.h ("THE NOISE ESTIMATE"), operation for operation as pt_noise.hip states
// it; this unit is built like that one (-ffp-contract=off, correctly rounded / and sqrt, no -mllvm options), so
// tests/adaptive_ref.py gives the same bytes - and so the weight w, which the resolve computes per tile, is the host's binary32.
//
// k_tile_level: memory-bound, 24 B read of the compact accumulator and up to 96 B read-modify-write of the sums per pixel of an
// open tile.  A workgroup of 256 takes whole tiles - 16, 4 or 1 of them at tile edge 4, 8 or 16, a quarter of a tile per trip at
// 32 - so every pixel of the frame is one thread's alone (plain read-modify-write, no atomics on the sums), a tile's E is summed
// with integer LDS atomics (the order does not matter), and the one thread that ends up holding a tile's E decides: the tile's
// count, nA and E are stored, and one of the step's two counters - the tiles it leaves open, the tiles it closed - goes up by
// one.  The host reads those two words back and nothing else.
//
// k_tile_select: one thread per tile over a strided grid (tiles are few: 12 288 at 1024 x 768 in tiles of 8), 16 B read per tile.
// A workgroup counts in LDS and adds its three counts to the global ones once.
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

// e(p) of THE NOISE ESTIMATE from a pixel's held sums h and half A's a
__device__ __forceinline__ float ts_estimate(const unsigned long long h[3], const unsigned long long a[3], float fa, float fb, float fn,
                                             float w) {
    float d[3], m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float va = ts_mean(a[c], fa), vb = ts_mean(h[c] - a[c], fb);
        d[c] = __builtin_fabsf(va - vb);
        m[c] = ts_mean(h[c], fn);
    }
    return (((d[0] + d[1]) + d[2]) * w) / __builtin_sqrtf(0.015625f + ((m[0] + m[1]) + m[2]));
}

__global__ __launch_bounds__(kTileBlock) void k_tile_level(TileGrid G, TileLevel V, unsigned long long *__restrict__ held,
                                                           unsigned long long *__restrict__ half_a) {
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
        unsigned long long h[3], a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long v = V.acc[(size_t)c * cplane + at];
            h[c] = held[(size_t)c * plane + p] + v;
            a[c] = half_a[(size_t)c * plane + p];
            if (v) held[(size_t)c * plane + p] = h[c];
            if (V.to_a) {
                a[c] += v;
                if (v) half_a[(size_t)c * plane + p] = a[c];
            }
        }
        if (V.estimate) {
            const float e = ts_estimate(h, a, V.fa, V.fb, V.fn, V.w);
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
            G.na[t] = V.na;
            bool closes = false;
            if (V.estimate) {
                const unsigned long long E = s_err[threadIdx.x];
                G.err[t] = E;
                closes = E <= V.q * (unsigned long long)s_pix[threadIdx.x];
            }
            atomicAdd(&V.counters[closes ? 1 : 0], 1u);
        }
    }
}

__global__ __launch_bounds__(kTileBlock) void k_tile_select(TileGrid G, TileSelect S) {
    __shared__ uint32_t s_n[3];
    if (threadIdx.x < 3u) s_n[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t edge = 1u << G.tile_shift;
    for (uint32_t t = blockIdx.x * kTileBlock + threadIdx.x; t < G.tiles; t += gridDim.x * kTileBlock) {
        const uint32_t ty = t / G.tiles_x, tx = t - ty * G.tiles_x;
        const uint32_t wpx = G.width - (tx << G.tile_shift), hpx = G.rows - (ty << G.tile_shift);
        const unsigned long long pixels = (unsigned long long)(wpx < edge ? wpx : edge) * (hpx < edge ? hpx : edge);
        const unsigned long long E = G.err[t];
        if (E != kTileNoError && E <= S.q * pixels) {
            atomicAdd(&s_n[2], 1u);
            continue;
        }
        const uint32_t n = G.spp[t];
        atomicAdd(&s_n[0], 1u);
        if (n >= S.cap) atomicAdd(&s_n[1], 1u);
        if (S.list && n < S.cap && n == S.c && G.na[t] == S.na) S.list[atomicAdd(S.list_len, 1u)] = t;  // (at most G.tiles entries)
    }
    __syncthreads();
    if (threadIdx.x < 3u && s_n[threadIdx.x]) atomicAdd(&S.out[threadIdx.x], s_n[threadIdx.x]);
}

__global__ __launch_bounds__(kTileBlock) void k_tile_resolve(TileGrid G, const unsigned long long *__restrict__ held,
                                                             const unsigned long long *__restrict__ half_a, float *__restrict__ out,
                                                             uint32_t *__restrict__ spp, float *__restrict__ error,
                                                             unsigned long long *__restrict__ err_sum) {
    const uint32_t npix = G.width * G.rows;
    for (uint32_t p = blockIdx.x * kTileBlock + threadIdx.x; p < npix; p += gridDim.x * kTileBlock) {
        const uint32_t row = p / G.width, col = p - row * G.width;
        const uint32_t t = (row >> G.tile_shift) * G.tiles_x + (col >> G.tile_shift);
        const uint32_t n = G.spp[t];
        if (spp) spp[p] = n;
        unsigned long long h[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            h[c] = held[(size_t)c * npix + p];
            const double sum = (double)h[c] * (1.0 / 4294967296.0);
            out[(size_t)p * 3 + c] = n ? ts_clamp((float)sum / (float)n) : 0.0f;  // (k_resolve's arithmetic)
        }
        if (error) {
            float e = __builtin_inff();
            if (G.err[t] != kTileNoError) {  // the tile's last evaluation was made at this count and nA: the same e(p) again
                const uint32_t na = G.na[t];
                const float fa = (float)na, fb = (float)(n - na);
                unsigned long long a[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = half_a[(size_t)c * npix + p];
                e = ts_estimate(h, a, fa, fb, (float)n, __builtin_sqrtf(fa * fb) / (fa + fb));  // (host::noise_part_weight)
            }
            error[p] = e;
        }
    }
    if (err_sum)
        for (uint32_t t = blockIdx.x * kTileBlock + threadIdx.x; t < G.tiles; t += gridDim.x * kTileBlock) {
            const unsigned long long E = G.err[t];
            if (E != kTileNoError && E != 0ull) atomicAdd(err_sum, E);
        }
}

dim3 stride_grid(uint32_t n) {
    const uint32_t blocks = (n + kTileBlock - 1) / kTileBlock;
    return dim3(blocks == 0u ? 1u : (blocks < 2048u ? blocks : 2048u));
}

}  // namespace

void launch_tile_level(hipStream_t st, const TileGrid &G, const TileLevel &V, unsigned long long *held, unsigned long long *half_a) {
    if (V.n_open == 0u) return;
    const uint32_t tile_px = 1u << (2u * G.tile_shift);
    const uint32_t per_block = tile_px >= kTileBlock ? 1u : kTileBlock / tile_px;
    hipLaunchKernelGGL(k_tile_level, dim3((V.n_open + per_block - 1u) / per_block), dim3(kTileBlock), 0, st, G, V, held, half_a);
}

void launch_tile_select(hipStream_t st, const TileGrid &G, const TileSelect &S) {
    hipLaunchKernelGGL(k_tile_select, stride_grid(G.tiles), dim3(kTileBlock), 0, st, G, S);
}

void launch_tile_resolve(hipStream_t st, const TileGrid &G, const unsigned long long *held, const unsigned long long *half_a,
                         float *out_rgb, uint32_t *spp, float *error, unsigned long long *err_sum) {
    hipLaunchKernelGGL(k_tile_resolve, stride_grid(G.width * G.rows), dim3(kTileBlock), 0, st, G, held, half_a, out_rgb, spp, error,
                       err_sum);
}

}  // namespace pt
