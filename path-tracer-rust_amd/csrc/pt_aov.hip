// pt_aov.hip — first-hit AOVs (pt_ctx_render_aov): albedo, normal, depth and object id per pixel, for a denoiser's guide
// buffers and a GUI's pick map.  One primary ray per (pixel, sample) - primary_ray, the frame kernels' own - one
// intersect_scene_dev, one fetch_surface; no path is continued.  k_aov_chain (pt_ctx_render_aov_ex with PT_AOV_THROUGH_DELTA)
// is the same pass with the guides taken at the first non-delta surface of the deterministic mirror / glass chain.
//
// Work is sample-major, as in k_pass_cand: the lanes of a wave hold consecutive samples of one pixel, so their rays leave the
// lens towards the same sub-pixel area and walk the same nodes.  seg = min(spp, 64) lanes per pixel, 64 / seg pixels per
// wave; with spp > 64 each lane loops over samples i, i + 64, ...  A pixel's segment is summed with ds_bpermute shuffles (a
// segmented tree: lane i adds lane i + off while i + off is in the segment).  The sums are integers - u64 32.32 fixed point
// for the colours, as the frame accumulator, and two's-complement i64 for the signed normal components - so the result does
// not depend on how the samples fall on lanes and waves.  No global atomics, no scratch buffer: the outputs are the only
// memory written, each wave's run of them by consecutive lanes.
#include "pt_aov.h"

namespace pt {

// dynamic LDS: the BVH nodes when the scene stages them, and the per-lane traversal stacks (bvh_lds_bytes; 0 without a BVH)
extern __shared__ uint4 aov_lds[];

namespace {

constexpr uint32_t kAovBlock = 256;
constexpr uint32_t kAovWaves = kAovBlock / 64u;
constexpr uint32_t kAovMaxGrid = 2048;  // workgroups; each wave loops over the rest (the BVH is staged once per workgroup)

// sign(v) * to_fixed(|v|): a normal component in [-1, 1] as a signed 32.32 fixed-point term
__device__ __forceinline__ int64_t to_fixed_signed(float v) {
    const int64_t m = (int64_t)to_fixed(f_abs(v));
    return v < 0.0f ? -m : m;
}

// k_resolve's arithmetic, without the clamp
__device__ __forceinline__ float resolve_u(uint64_t sum, uint32_t spp) { return (float)((double)sum * (1.0 / 4294967296.0)) / (float)spp; }
__device__ __forceinline__ float resolve_s(int64_t sum, uint32_t spp) { return (float)((double)sum * (1.0 / 4294967296.0)) / (float)spp; }

template <bool BVH>
__global__ __launch_bounds__(kAovBlock) void k_aov(DevScene S, FrameParams F, uint32_t seg, uint32_t per_wave,
                                                   float *__restrict__ albedo, float *__restrict__ normal,
                                                   float *__restrict__ depth, int32_t *__restrict__ object_id) {
    if (BVH) stage_bvh(S, aov_lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = lane / seg, i = lane - q * seg;  // the lane's pixel slot in the wave and its first sample
    const uint32_t waves = (F.npix + per_wave - 1u) / per_wave;
    for (uint32_t w = blockIdx.x * kAovWaves + (threadIdx.x >> 6); w < waves; w += gridDim.x * kAovWaves) {
        const uint32_t k0 = w * per_wave;  // the wave's first call pixel (w < waves: no overflow)
        const uint32_t k = k0 + q;
        uint64_t ar = 0, ag = 0, ab = 0;
        int64_t nx = 0, ny = 0, nz = 0;
        float t0 = __builtin_inff();
        int32_t id0 = -1;
        if (q < per_wave && k < F.npix) {
            const uint32_t p = global_pixel(F, k);
            for (uint32_t s = i; s < F.spp; s += seg) {
                const PathRay r = primary_ray<false>(F, p, s);
                const HitRec h = intersect_scene_dev<BVH>(S, r.o, r.d, aov_lds);
                if (h.id >= 0) {
                    const Surface sf = fetch_surface(S, r.o, r.d, h);
                    const vec3 nl = dot(sf.n, r.d) < 0.0f ? sf.n : sf.n * -1.0f;  // normal_towards_ray, mod.rs:669-673
                    ar += to_fixed(sf.color.x);
                    ag += to_fixed(sf.color.y);
                    ab += to_fixed(sf.color.z);
                    nx += to_fixed_signed(nl.x);
                    ny += to_fixed_signed(nl.y);
                    nz += to_fixed_signed(nl.z);
                    if (s == 0u) {
                        t0 = h.t;
                        id0 = h.id < (int32_t)S.n_objs ? h.id : (int32_t)S.tri_shade[h.id - (int32_t)S.n_objs].owner;
                    }
                }
            }
        }
        // every lane of the wave is active again: the segment's sums go to its first lane (i == 0)
        for (uint32_t off = 1u; off < seg; off <<= 1) {
            const bool take = i + off < seg;
            const uint64_t xr = __shfl_down(ar, off, 64), xg = __shfl_down(ag, off, 64), xb = __shfl_down(ab, off, 64);
            const int64_t yx = __shfl_down(nx, off, 64), yy = __shfl_down(ny, off, 64), yz = __shfl_down(nz, off, 64);
            if (take) {
                ar += xr;
                ag += xg;
                ab += xb;
                nx += yx;
                ny += yy;
                nz += yz;
            }
        }
        const uint32_t n_here = (F.npix - k0) < per_wave ? (F.npix - k0) : per_wave;  // pixels of this wave
        // Stores: the wave's 3 * n_here floats of an RGB output are one run; element e (slot e / 3, component e % 3) is
        // fetched from the slot's first lane and stored by lane e % 64 - consecutive lanes, consecutive addresses.
        if (albedo || normal) {
            const float a0 = resolve_u(ar, F.spp), a1 = resolve_u(ag, F.spp), a2 = resolve_u(ab, F.spp);
            const float n0 = resolve_s(nx, F.spp), n1 = resolve_s(ny, F.spp), n2 = resolve_s(nz, F.spp);
            for (uint32_t e0 = 0; e0 < 3u * per_wave; e0 += 64u) {  // wave-uniform trip count
                const uint32_t e = e0 + lane, slot = e / 3u, c = e - slot * 3u;
                const int src = (int)((slot < per_wave ? slot : 0u) * seg);
                const float va0 = __shfl(a0, src, 64), va1 = __shfl(a1, src, 64), va2 = __shfl(a2, src, 64);
                const float vn0 = __shfl(n0, src, 64), vn1 = __shfl(n1, src, 64), vn2 = __shfl(n2, src, 64);
                if (slot < n_here) {
                    const size_t at = (size_t)k0 * 3u + e;
                    if (albedo) albedo[at] = c == 0u ? va0 : (c == 1u ? va1 : va2);
                    if (normal) normal[at] = c == 0u ? vn0 : (c == 1u ? vn1 : vn2);
                }
            }
        }
        if (depth || object_id) {
            const int src = (int)((lane < per_wave ? lane : 0u) * seg);
            const float vt = __shfl(t0, src, 64);
            const int32_t vid = __shfl(id0, src, 64);
            if (lane < n_here) {
                if (depth) depth[(size_t)k0 + lane] = vt;
                if (object_id) object_id[(size_t)k0 + lane] = vid;
            }
        }
    }
}

// The deterministic continuation of a ray past a mirror or glass hit (PT_AOV_THROUGH_DELTA): shade_surface's lines for the
// two delta materials (pt_device.h; mod.rs:722-723 and 729-749) without the draw, the roulette and the Fresnel weights - the
// mirror direction, not renormalised, and on glass tdir unless cos2t < 0 (total internal reflection: the mirror direction).
// The same operations in the same order under the same flags, so the values are the ones shade_surface hands its children.
__device__ __forceinline__ vec3 delta_child(const Surface &sf, vec3 d) {
    const vec3 n = sf.n;
    const float dn = dot(n, d);
    const vec3 refl = d - n * 2.0f * dn;
    if (sf.reflect != kRefract) return refl;
    const bool into = dn < 0.0f;
    const float nc = 1.0f, nt = 1.5f;
    const float nnt = into ? nc / nt : nt / nc;
    const float ddn = into ? dn : -dn;
    const float cos2t = 1.0f - (nnt * nnt) * (1.0f - ddn * ddn);
    if (cos2t < 0.0f) return refl;
    const vec3 tv = d * nnt - n * ((into ? 1.0f : -1.0f) * (ddn * nnt + f_sqrt(cos2t)));
    return normalize_ranged(tv);
}

// k_aov with the guides taken at the end of the deterministic chain (pt_ctx_render_aov_ex, PT_AOV_THROUGH_DELTA): a sample
// whose hit is a mirror or glass surface goes on - thr *= colour, L += distance, j += 1, the next ray from the hit point along
// delta_child - until it hits a diffuse surface, has made max_chain steps, or misses.  Work layout, sums, shuffles and stores
// are k_aov's; a lane loops while its chain is alive, so a wave loops while any of its lanes' is, and the staged BVH and the
// per-lane stacks serve every bounce.  Sample 0 also gives chain[k] = j.
// Four waves per SIMD, k_aov<true>'s occupancy: left alone the BVH instance takes 137 VGPRs and three waves; held to 128 it fits
// 127 without scratch (the instance without a BVH takes 97; held to k_aov<false>'s five waves it would spill).
template <bool BVH>
__global__ __launch_bounds__(kAovBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_aov_chain(DevScene S, FrameParams F, uint32_t seg, uint32_t per_wave,
                                                         uint32_t max_chain, float *__restrict__ albedo,
                                                         float *__restrict__ normal, float *__restrict__ depth,
                                                         int32_t *__restrict__ object_id, uint32_t *__restrict__ chain) {
    if (BVH) stage_bvh(S, aov_lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = lane / seg, i = lane - q * seg;
    const uint32_t waves = (F.npix + per_wave - 1u) / per_wave;
    for (uint32_t w = blockIdx.x * kAovWaves + (threadIdx.x >> 6); w < waves; w += gridDim.x * kAovWaves) {
        const uint32_t k0 = w * per_wave;
        const uint32_t k = k0 + q;
        uint64_t ar = 0, ag = 0, ab = 0;
        int64_t nx = 0, ny = 0, nz = 0;
        float t0 = __builtin_inff();
        int32_t id0 = -1;
        uint32_t ch0 = 0u;
        if (q < per_wave && k < F.npix) {
            const uint32_t p = global_pixel(F, k);
            for (uint32_t s = i; s < F.spp; s += seg) {
                const PathRay r = primary_ray<false>(F, p, s);
                vec3 o = r.o, d = r.d, thr = mk(1.0f, 1.0f, 1.0f);
                float len = 0.0f;
                uint32_t j = 0u;
                for (;;) {
                    const HitRec h = intersect_scene_dev<BVH>(S, o, d, aov_lds);
                    if (h.id < 0) {  // a miss at any stage: nothing to the sums; depth +inf, id -1 as initialised
                        if (s == 0u) ch0 = j;
                        break;
                    }
                    const Surface sf = fetch_surface(S, o, d, h);
                    len = len + h.t;
                    if (sf.reflect == kDiffuse || j == max_chain) {  // terminal
                        const vec3 nl = dot(sf.n, d) < 0.0f ? sf.n : sf.n * -1.0f;  // normal_towards_ray, mod.rs:669-673
                        const vec3 a = thr * sf.color;
                        ar += to_fixed(a.x);
                        ag += to_fixed(a.y);
                        ab += to_fixed(a.z);
                        nx += to_fixed_signed(nl.x);
                        ny += to_fixed_signed(nl.y);
                        nz += to_fixed_signed(nl.z);
                        if (s == 0u) {
                            t0 = len;
                            id0 = h.id < (int32_t)S.n_objs ? h.id : (int32_t)S.tri_shade[h.id - (int32_t)S.n_objs].owner;
                            ch0 = j;
                        }
                        break;
                    }
                    thr = thr * sf.color;
                    j += 1u;
                    d = delta_child(sf, d);
                    o = sf.x;
                }
            }
        }
        for (uint32_t off = 1u; off < seg; off <<= 1) {
            const bool take = i + off < seg;
            const uint64_t xr = __shfl_down(ar, off, 64), xg = __shfl_down(ag, off, 64), xb = __shfl_down(ab, off, 64);
            const int64_t yx = __shfl_down(nx, off, 64), yy = __shfl_down(ny, off, 64), yz = __shfl_down(nz, off, 64);
            if (take) {
                ar += xr;
                ag += xg;
                ab += xb;
                nx += yx;
                ny += yy;
                nz += yz;
            }
        }
        const uint32_t n_here = (F.npix - k0) < per_wave ? (F.npix - k0) : per_wave;
        if (albedo || normal) {
            const float a0 = resolve_u(ar, F.spp), a1 = resolve_u(ag, F.spp), a2 = resolve_u(ab, F.spp);
            const float n0 = resolve_s(nx, F.spp), n1 = resolve_s(ny, F.spp), n2 = resolve_s(nz, F.spp);
            for (uint32_t e0 = 0; e0 < 3u * per_wave; e0 += 64u) {
                const uint32_t e = e0 + lane, slot = e / 3u, c = e - slot * 3u;
                const int src = (int)((slot < per_wave ? slot : 0u) * seg);
                const float va0 = __shfl(a0, src, 64), va1 = __shfl(a1, src, 64), va2 = __shfl(a2, src, 64);
                const float vn0 = __shfl(n0, src, 64), vn1 = __shfl(n1, src, 64), vn2 = __shfl(n2, src, 64);
                if (slot < n_here) {
                    const size_t at = (size_t)k0 * 3u + e;
                    if (albedo) albedo[at] = c == 0u ? va0 : (c == 1u ? va1 : va2);
                    if (normal) normal[at] = c == 0u ? vn0 : (c == 1u ? vn1 : vn2);
                }
            }
        }
        if (depth || object_id || chain) {
            const int src = (int)((lane < per_wave ? lane : 0u) * seg);
            const float vt = __shfl(t0, src, 64);
            const int32_t vid = __shfl(id0, src, 64);
            const uint32_t vch = __shfl(ch0, src, 64);
            if (lane < n_here) {
                if (depth) depth[(size_t)k0 + lane] = vt;
                if (object_id) object_id[(size_t)k0 + lane] = vid;
                if (chain) chain[(size_t)k0 + lane] = vch;
            }
        }
    }
}

}  // namespace

void launch_aov(hipStream_t st, const DevScene &S, const FrameParams &F, float *albedo, float *normal, float *depth,
                int32_t *object_id) {
    const uint32_t seg = F.spp < 64u ? F.spp : 64u, per_wave = 64u / seg;
    const uint64_t waves = ((uint64_t)F.npix + per_wave - 1u) / per_wave;
    const uint64_t blocks = (waves + kAovWaves - 1u) / kAovWaves;
    const uint32_t grid = blocks == 0u ? 1u : (blocks < kAovMaxGrid ? (uint32_t)blocks : kAovMaxGrid);
    if (S.n_bvh_nodes != 0u)
        hipLaunchKernelGGL(k_aov<true>, dim3(grid), dim3(kAovBlock), bvh_lds_bytes(S, kAovBlock), st, S, F, seg, per_wave, albedo,
                           normal, depth, object_id);
    else
        hipLaunchKernelGGL(k_aov<false>, dim3(grid), dim3(kAovBlock), 0, st, S, F, seg, per_wave, albedo, normal, depth,
                           object_id);
}

void launch_aov_chain(hipStream_t st, const DevScene &S, const FrameParams &F, uint32_t max_chain, float *albedo, float *normal,
                      float *depth, int32_t *object_id, uint32_t *chain) {
    const uint32_t seg = F.spp < 64u ? F.spp : 64u, per_wave = 64u / seg;
    const uint64_t waves = ((uint64_t)F.npix + per_wave - 1u) / per_wave;
    const uint64_t blocks = (waves + kAovWaves - 1u) / kAovWaves;
    const uint32_t grid = blocks == 0u ? 1u : (blocks < kAovMaxGrid ? (uint32_t)blocks : kAovMaxGrid);
    if (S.n_bvh_nodes != 0u)
        hipLaunchKernelGGL(k_aov_chain<true>, dim3(grid), dim3(kAovBlock), bvh_lds_bytes(S, kAovBlock), st, S, F, seg, per_wave,
                           max_chain, albedo, normal, depth, object_id, chain);
    else
        hipLaunchKernelGGL(k_aov_chain<false>, dim3(grid), dim3(kAovBlock), 0, st, S, F, seg, per_wave, max_chain, albedo, normal,
                           depth, object_id, chain);
}

}  // namespace pt
