// pt_denoise.hip — pt_ctx_denoise's kernels: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a whole frame,
// guided by first-hit albedo, normal and depth.  The arithmetic is the contract of include/ptrace.h ("THE ARITHMETIC"),
// operation for operation and in its order; this unit is built with -ffp-contract=off and correctly rounded / and sqrt, so a
// restatement in numpy binary32 (tests/denoise_ref.py) gives the same bytes.
//
// k_dn_prepare packs two float4 per pixel - (N.xyz, depth) and (u0.rgb, -) - so that a tap is two 16-byte loads.
// k_dn_level runs once per level (step s = 2^i) in one of two forms that give the same bytes:
//   direct  a workgroup owns 32x8 neighbouring pixels and loads every tap from global memory (consecutive lanes, consecutive
//           16-byte words: every tap load of a wave is two full runs of 512 B).
//   LDS     a workgroup stages its pixels and their halo once - 18 KB at most - and reads the taps as ds_read_b128.  Its 32x8
//           pixels are a lattice of the taps: in y always rows y0 + j*s (12 rows hold all five dy), in x dense up to step 4
//           (32 + 4s columns) and columns x0 + j*s beyond (36 columns), where a dense halo would not fit any tile.
// No atomics, no scratch memory, no host round trip between the levels; the last level folds the finish in (times m, clamp).
//
// pt_ctx_denoise_var (VAR = true below) is the same filter whose colour weight follows a per-pixel variance V in place of one
// sigma_color.  V rides in the .w lane of the colour plane, so a tap is still two 16-byte loads and the LDS tile does not
// grow: prepare derives Vraw from the frame's error map into u[1].w, k_dn_prefilter smooths it 3x3 into u[0].w, and every
// level carries V on with the squares of the weights it used.  The VAR = false instantiations are pt_ctx_denoise's, unchanged.
#include "pt_denoise.h"

namespace pt {
namespace {

constexpr uint32_t kDnTx = 32, kDnTy = 8, kDnBlock = kDnTx * kDnTy;
constexpr uint32_t kDnDenseMaxStep = 4;                        // the LDS tile is dense in x up to this step
constexpr uint32_t kDnLw = kDnTx + 4 * kDnDenseMaxStep;        // widest LDS tile in entries (48)
constexpr uint32_t kDnLh = kDnTy + 4;

__device__ __forceinline__ float dn_pos(float v) { return v > 0.0f ? v : 0.0f; }
__device__ __forceinline__ float dn_fall(float v) {
    float t = dn_pos(1.0f - v * 0.125f);
    t = t * t;
    t = t * t;
    return t * t;
}
__device__ __forceinline__ float dn_clamp(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

struct DnSum {
    float r, g, b, w;
    float v;  // VAR only: the sum of V(q) * w^2
};

// one tap q of pixel p that lies inside the frame and is not the centre; rc: 1 / sc_i^2, or with VAR the pixel's own r
template <bool VAR>
__device__ __forceinline__ void dn_tap(DnSum &a, float h, const float4 gp, const float4 up, const float4 gq, const float4 uq,
                                       bool has_n, bool has_z, float rc, float sds) {
    const bool hp = gp.w < __builtin_inff(), hq = gq.w < __builtin_inff();
    if (hp != hq) return;  // a miss never blends with a hit
    float wn = 1.0f, xz = 0.0f;
    if (hp) {
        if (has_n) {
            float e = dn_pos((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
            e = e * e;
            e = e * e;
            e = e * e;
            e = e * e;
            wn = e * e;
        }
        if (has_z) {
            const float zm = gp.w > gq.w ? gp.w : gq.w;
            xz = __builtin_fabsf(gp.w - gq.w) * (1.0f / (sds * zm));
        }
    }
    const float dr = up.x - uq.x, dg = up.y - uq.y, db = up.z - uq.z;
    const float xc = ((dr * dr + dg * dg) + db * db) * rc;
    const float w = ((h * wn) * dn_fall(xz)) * dn_fall(xc);
    a.r = a.r + uq.x * w;
    a.g = a.g + uq.y * w;
    a.b = a.b + uq.z * w;
    a.w = a.w + w;
    if (VAR) a.v = a.v + uq.w * (w * w);
}

__device__ __forceinline__ float dn_b(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

template <bool VAR>
__global__ __launch_bounds__(kDnBlock) void k_dn_prepare(DenoiseFrame f, uint32_t npix) {
    const uint32_t p = blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= npix) return;
    const size_t p3 = (size_t)p * 3u;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // depth 0: without a depth buffer every pixel is a hit
    if (f.depth) g.w = f.depth[p];
    if (f.normal) {
        const float nx = f.normal[p3], ny = f.normal[p3 + 1], nz = f.normal[p3 + 2];
        const float l = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
        if (l > 0.0f) {
            g.x = nx / l;
            g.y = ny / l;
            g.z = nz / l;
        }
    }
    float m0 = 1.0f, m1 = 1.0f, m2 = 1.0f;
    if (f.albedo) {
        const float a0 = f.albedo[p3], a1 = f.albedo[p3 + 1], a2 = f.albedo[p3 + 2];
        m0 = a0 > 0.015625f ? a0 : 1.0f;
        m1 = a1 > 0.015625f ? a1 : 1.0f;
        m2 = a2 > 0.015625f ? a2 : 1.0f;
    }
    f.guide[p] = g;
    const float c0 = f.color[p3], c1 = f.color[p3 + 1], c2 = f.color[p3 + 2];
    f.u[0][p] = make_float4(c0 / m0, c1 / m1, c2 / m2, 0.0f);
    if (VAR) {
        // the error map's normalisation undone: the weighted L1 half difference in colour units, then demodulated
        const float e = f.error[p];
        const float ev = e < 12.0f ? dn_pos(e) : 12.0f;
        const float d = ev * __builtin_sqrtf(0.015625f + ((c0 + c1) + c2));
        const float t0 = d / m0, t1 = d / m1, t2 = d / m2;
        f.u[1][p].w = (t0 * t0 + t1 * t1) + t2 * t2;
    }
}

// V_0 = Vraw under a 3x3 binomial, renormalised at the frame's edge; no guide weights.  u[1].w -> u[0].w
__global__ __launch_bounds__(kDnBlock) void k_dn_prefilter(DenoiseFrame f) {
    const int W = (int)f.width, H = (int)f.height;
    const uint32_t gx = (f.width + kDnTx - 1u) / kDnTx;
    const int x = (int)((blockIdx.x % gx) * kDnTx + threadIdx.x % kDnTx);
    const int y = (int)((blockIdx.x / gx) * kDnTy + threadIdx.x / kDnTx);
    if (x >= W || y >= H) return;
    float sum = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float g = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            sum = sum + f.u[1][(size_t)qy * (size_t)W + (size_t)qx].w * g;
            wsum = wsum + g;
        }
    }
    f.u[0][(size_t)y * (size_t)W + (size_t)x].w = sum / wsum;
}

// gx: workgroups along x (gridDim.x = gx * workgroups along y: a one-dimensional grid has no 65535 limit)
// VAR: rc is kv = sigma_var^2, and the colour term's scale is the pixel's own 1 / (kv * V(p) + 2^-20)
template <bool LDS, bool LAST, bool VAR>
__global__ __launch_bounds__(kDnBlock) void k_dn_level(DenoiseFrame f, const float4 *__restrict__ uin, float4 *__restrict__ uout,
                                                       uint32_t s, uint32_t gx, float rc, float sds) {
    __shared__ float4 sg[LDS ? kDnLw * kDnLh : 1];
    __shared__ float4 su[LDS ? kDnLw * kDnLh : 1];
    const int W = (int)f.width, H = (int)f.height, S = (int)s;
    const uint32_t bx = blockIdx.x % gx, by = blockIdx.x / gx;
    const int tx = (int)(threadIdx.x % kDnTx), ty = (int)(threadIdx.x / kDnTx);
    const bool has_n = f.normal != nullptr, has_z = f.depth != nullptr;
    int x, y;         // this lane's pixel
    int lc = 0, kx = 0, lw = 0;  // LDS form: the lane's column in the tile, the tile columns per tap step, the tile's width
    if (LDS) {
        // residue classes: rx of the columns (one class when the tile is dense in x), ry of the rows
        const int sx = s <= kDnDenseMaxStep ? 1 : S;
        kx = S / sx;
        const int hx = 2 * kx;
        lw = (int)kDnTx + 2 * hx;
        const int nrx = sx < W ? sx : W, nry = S < H ? S : H;
        const int rx = (int)bx % nrx, tile_x = (int)bx / nrx, ry = (int)by % nry, tile_y = (int)by / nry;
        const int cx0 = tile_x * (int)kDnTx - hx, cy0 = tile_y * (int)kDnTy - 2;  // lattice index of the tile's first entry
        for (int e = (int)threadIdx.x; e < lw * (int)kDnLh; e += (int)kDnBlock) {
            const int l = e % lw, r = e / lw;
            const long long qx = (long long)rx + (long long)(cx0 + l) * sx, qy = (long long)ry + (long long)(cy0 + r) * S;
            if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                sg[e] = f.guide[q];
                su[e] = uin[q];
            }
        }
        __syncthreads();
        lc = hx + tx;
        const long long px = (long long)rx + (long long)(tile_x * (int)kDnTx + tx) * sx;
        const long long py = (long long)ry + (long long)(tile_y * (int)kDnTy + ty) * S;
        if (px >= W || py >= H) return;
        x = (int)px;
        y = (int)py;
    } else {
        x = (int)(bx * kDnTx) + tx;
        y = (int)(by * kDnTy) + ty;
        if (x >= W || y >= H) return;
    }
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const int lp = (2 + ty) * lw + lc;
    const float4 gp = LDS ? sg[lp] : f.guide[p];
    const float4 up = LDS ? su[lp] : uin[p];
    DnSum a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (VAR) rc = 1.0f / ((rc * up.w) + 0x1p-20f);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = dn_b(dy) * dn_b(dx);
            if (dx == 0 && dy == 0) {
                a.r = a.r + up.x * h;
                a.g = a.g + up.y * h;
                a.b = a.b + up.z * h;
                a.w = a.w + h;
                if (VAR) a.v = a.v + up.w * (h * h);
                continue;
            }
            const long long qx = (long long)x + (long long)dx * S, qy = (long long)y + (long long)dy * S;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            float4 gq, uq;
            if (LDS) {
                const int lq = lp + dy * lw + dx * kx;
                gq = sg[lq];
                uq = su[lq];
            } else {
                const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                gq = f.guide[q];
                uq = uin[q];
            }
            dn_tap<VAR>(a, h, gp, up, gq, uq, has_n, has_z, rc, sds);
        }
    }
    const float r = a.r / a.w, g = a.g / a.w, b = a.b / a.w;
    if (LAST) {
        float m0 = 1.0f, m1 = 1.0f, m2 = 1.0f;
        const size_t p3 = p * 3u;
        if (f.albedo) {
            const float a0 = f.albedo[p3], a1 = f.albedo[p3 + 1], a2 = f.albedo[p3 + 2];
            m0 = a0 > 0.015625f ? a0 : 1.0f;
            m1 = a1 > 0.015625f ? a1 : 1.0f;
            m2 = a2 > 0.015625f ? a2 : 1.0f;
        }
        f.out[p3] = dn_clamp(r * m0);
        f.out[p3 + 1] = dn_clamp(g * m1);
        f.out[p3 + 2] = dn_clamp(b * m2);
    } else {
        uout[p] = make_float4(r, g, b, VAR ? a.v / (a.w * a.w) : 0.0f);
    }
}

uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

}  // namespace

void launch_dn_prepare(hipStream_t st, const DenoiseFrame &f) {
    const uint32_t npix = f.width * f.height;
    const dim3 grid(ceil_div(npix, kDnBlock)), block(kDnBlock);
    if (f.error) {
        hipLaunchKernelGGL(k_dn_prepare<true>, grid, block, 0, st, f, npix);
        hipLaunchKernelGGL(k_dn_prefilter, dim3(ceil_div(f.width, kDnTx) * ceil_div(f.height, kDnTy)), block, 0, st, f);
    } else {
        hipLaunchKernelGGL(k_dn_prepare<false>, grid, block, 0, st, f, npix);
    }
}

namespace {

template <bool VAR>
void launch_level(hipStream_t st, const DenoiseFrame &f, uint32_t i, float rc, float sds, bool last, bool lds) {
    const uint32_t s = 1u << i;
    const float4 *uin = f.u[i & 1u];
    float4 *uout = f.u[(i + 1u) & 1u];
    uint32_t gx, gy;
    if (lds) {
        // per residue class of the lattice: the tiles that cover its ceil(extent / stride) pixels
        const uint32_t sx = s <= kDnDenseMaxStep ? 1u : s;
        const uint32_t nrx = sx < f.width ? sx : f.width, nry = s < f.height ? s : f.height;
        gx = nrx * ceil_div(ceil_div(f.width, sx), kDnTx);
        gy = nry * ceil_div(ceil_div(f.height, s), kDnTy);
    } else {
        gx = ceil_div(f.width, kDnTx);
        gy = ceil_div(f.height, kDnTy);
    }
    const dim3 grid(gx * gy), block(kDnBlock);
    if (lds) {
        if (last)
            hipLaunchKernelGGL((k_dn_level<true, true, VAR>), grid, block, 0, st, f, uin, uout, s, gx, rc, sds);
        else
            hipLaunchKernelGGL((k_dn_level<true, false, VAR>), grid, block, 0, st, f, uin, uout, s, gx, rc, sds);
    } else {
        if (last)
            hipLaunchKernelGGL((k_dn_level<false, true, VAR>), grid, block, 0, st, f, uin, uout, s, gx, rc, sds);
        else
            hipLaunchKernelGGL((k_dn_level<false, false, VAR>), grid, block, 0, st, f, uin, uout, s, gx, rc, sds);
    }
}

}  // namespace

void launch_dn_level(hipStream_t st, const DenoiseFrame &f, uint32_t i, float rc, float sds, bool last, bool lds) {
    if (f.error)
        launch_level<true>(st, f, i, rc, sds, last, lds);
    else
        launch_level<false>(st, f, i, rc, sds, last, lds);
}

}  // namespace pt
