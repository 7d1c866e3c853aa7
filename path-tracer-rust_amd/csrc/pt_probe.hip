// pt_probe.hip — the kernel of pt_ctx_scatter.  gfx950, wave64.  Built with the options of pt_kernels.hip (the shading step is
// compiled here as it is there: -ffp-contract=off, correctly rounded / and sqrt, the same -mllvm set), outside pt_kernels.s.
//
// One lane per item.  The surface comes from the caller (PT_SCATTER_GIVEN), or from the closest hit of intersect_scene_dev as
// k_query calls it, through fetch_surface (by id) or fetch_surface_rank (by rank: a triangle's rank from DevScene.tri_rank, a
// sphere's by a search of DevScene.rank_id - a probe may afford that).  By rank a workgroup first copies `head` leading records of
// DevScene.surf to LDS, as k_pass_cand does when the whole table does not fit, and hands the copy to the fetcher.  Then
// shade_surface<MODE> with the item's ray, throughput and key, and the whole ShadeOut goes to out[i].  Nothing here restates a
// line of the shading step: the functions are pt_device.h's.
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_probe.h"

namespace pt {

// dynamic LDS: what the BVH walk of intersect_scene_dev needs (bvh_lds_bytes), then the head of the surf table
extern __shared__ uint4 probe_lds[];

namespace {

constexpr uint32_t kProbeMaxGrid = 1024;
constexpr size_t kProbeLdsMax = 48u * 1024u;  // of a workgroup, BVH area and head together

__host__ __device__ inline size_t head_offset(const DevScene &S) { return (bvh_lds_bytes(S, kBlock) + 15u) & ~(size_t)15u; }

__device__ __forceinline__ void put(float out[3], vec3 v) {
    out[0] = v.x;
    out[1] = v.y;
    out[2] = v.z;
}

template <uint32_t SRC, int MODE>
__global__ __launch_bounds__(kBlock) void k_scatter(DevScene S, ScatterCall c) {
    const SurfRec *surf_lds = nullptr;
    if (SRC != PT_SCATTER_GIVEN) stage_bvh(S, probe_lds);
    if (SRC == PT_SCATTER_BY_RANK && c.head != 0u) {  // wave-uniform
        const uint4 *src = reinterpret_cast<const uint4 *>(S.surf);
        uint4 *dst = probe_lds + head_offset(S) / 16u;
        const uint32_t rows = c.head * (uint32_t)(sizeof(SurfRec) / 16u);
        for (uint32_t k = threadIdx.x; k < rows; k += kBlock) dst[k] = src[k];
        __syncthreads();
        surf_lds = reinterpret_cast<const SurfRec *>(dst);
    }
    ShadeParams P{};
    P.seed_lo = c.seed_lo;
    P.seed_hi = c.seed_hi;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < c.n; i += gridDim.x * kBlock) {
        const pt_scatter_item it = c.items[i];
        PathRay in;
        in.o = mk(it.o[0], it.o[1], it.o[2]);
        in.d = mk(it.d[0], it.d[1], it.d[2]);
        in.thr = mk(it.thr[0], it.thr[1], it.thr[2]);
        in.pix = it.pixel;
        in.meta = pack_meta(it.sample, it.depth, it.branch);
        pt_scatter_out o{};
        Surface sf{};
        bool have = true;
        if (SRC == PT_SCATTER_GIVEN) {
            const ScatterSurf g = c.surf[i];
            sf.x = mk(g.x[0], g.x[1], g.x[2]);
            sf.n = mk(g.n[0], g.n[1], g.n[2]);
            sf.color = mk(g.color[0], g.color[1], g.color[2]);
            sf.emission = mk(g.emission[0], g.emission[1], g.emission[2]);
            sf.max_refl = g.max_refl;
            sf.inv_max_refl = g.inv_max_refl;
            sf.reflect = g.reflect;
            sf.emits = emission_nonzero(sf.emission);
        } else {
            const HitRec h = intersect_scene_dev<true>(S, in.o, in.d, probe_lds);
            o.hit = h.id;
            have = h.id >= 0;
            if (have && SRC == PT_SCATTER_BY_ID) sf = fetch_surface(S, in.o, in.d, h);
            if (have && SRC == PT_SCATTER_BY_RANK) {
                const uint32_t n_ranks = S.n_objs + S.n_tris;
                uint32_t rank = 0u;
                if (h.id >= (int32_t)S.n_objs) {
                    rank = S.tri_rank[h.id - (int32_t)S.n_objs];
                } else {
                    while (rank + 1u < n_ranks && S.rank_id[rank] != (uint32_t)h.id) ++rank;
                }
                sf = fetch_surface_rank(S.surf, in.o, in.d, h.t, rank, surf_lds, c.head);
            }
        }
        if (have && MODE == kShadeRefractOnly && sf.reflect != kRefract) {  // the frame kernels never do that
            o.hit = PT_SCATTER_NOT_SHADED;
            have = false;
        }
        if (have) {
            ShadeOut so;
            shade_surface<MODE>(P, in, sf, so);
            // shade_surface writes the second ray only where it makes one.  The record is filled as it was when the step kept
            // defaults for it: the incoming direction, the throughput below the hit and the first ray's bookkeeping.
            if (!so.deferred && so.n_rays != 2) {
                so.d1 = in.d;
                so.thr1 = so.thr;
                so.meta1 = so.meta0;
            }
            o.deferred = so.deferred ? 1u : 0u;
            o.n_rays = (uint32_t)so.n_rays;
            o.emits = so.emits ? 1u : 0u;
            if (!so.deferred) {
                put(o.x, so.x);
                put(o.contrib, so.contrib);
                put(o.d0, so.d0);
                put(o.thr0, so.thr0);
                put(o.d1, so.d1);
                put(o.thr1, so.thr1);
                o.depth0 = meta_depth(so.meta0);
                o.branch0 = meta_branch(so.meta0);
                o.depth1 = meta_depth(so.meta1);
                o.branch1 = meta_branch(so.meta1);
            }
        }
        c.out[i] = o;
    }
}

template <uint32_t SRC>
void launch_mode(hipStream_t st, const DevScene &S, const ScatterCall &c, uint32_t grid, size_t lds) {
    if (c.form & PT_SCATTER_DEFER_REFRACT)
        hipLaunchKernelGGL((k_scatter<SRC, kShadeDeferRefract>), dim3(grid), dim3(kBlock), lds, st, S, c);
    else if (c.form & PT_SCATTER_REFRACT_ONLY)
        hipLaunchKernelGGL((k_scatter<SRC, kShadeRefractOnly>), dim3(grid), dim3(kBlock), lds, st, S, c);
    else
        hipLaunchKernelGGL((k_scatter<SRC, kShadeAll>), dim3(grid), dim3(kBlock), lds, st, S, c);
}

}  // namespace

size_t scatter_head_room(const DevScene &S) {
    const size_t at = head_offset(S);
    return at < kProbeLdsMax ? kProbeLdsMax - at : 0u;
}

void launch_scatter(hipStream_t st, const DevScene &S, const ScatterCall &c) {
    const uint32_t blocks = (c.n + kBlock - 1u) / kBlock;
    const uint32_t grid = blocks < kProbeMaxGrid ? blocks : kProbeMaxGrid;
    const uint32_t src = c.form & kScatterSourceMask;
    if (src == PT_SCATTER_GIVEN)
        launch_mode<PT_SCATTER_GIVEN>(st, S, c, grid, 0u);
    else if (src == PT_SCATTER_BY_ID)
        launch_mode<PT_SCATTER_BY_ID>(st, S, c, grid, bvh_lds_bytes(S, kBlock));
    else
        launch_mode<PT_SCATTER_BY_RANK>(st, S, c, grid, head_offset(S) + (size_t)c.head * sizeof(SurfRec));
}

}  // namespace pt
