// pt_solid.hip — pt_ctx_solid's kernel: a lit solid view of a whole frame from the first-hit guides.  The arithmetic is the
// contract of include/ptrace_solid.h ("THE ARITHMETIC" of pt_ctx_solid), operation for operation; the pixel is pt_solid.h's
// solid_pixel, which the host compiles too.  Built with -ffp-contract=off and correctly rounded / and sqrt, so a restatement in
// numpy binary32 (tests/solid_ref.py) gives the same bytes.
//
// A streaming pass: 44 B per pixel (12 albedo, 12 normal, 4 depth, 4 id, 12 out; 32 B without albedo) against some sixty VALU
// operations, so memory should bind it and the accesses are made wide.
// - WIDE form: a lane owns FOUR consecutive pixels.  Its id and depth words are one 16-byte access each, its three-float planes
//   (albedo, normal, out) are 48 consecutive bytes, three 16-byte accesses each: a wave's instruction covers 1 KiB contiguously.
//   The ids are loaded first; a lane whose four ids are all below 0 loads nothing else and stores the background.  Every other
//   lane issues all its loads - depth, normals, albedo, then the records - before the first arithmetic.
// - The looks table: where every pixel of the wave's lanes has ONE id (one object fills the wave's 256 pixels - most waves of a
//   frame) the record is fetched once at a wave-uniform address (the scalar path); otherwise per lane and pixel, one 16-byte load
//   by id, as pt_reproject.hip fetches a motion record.  An id beyond the table - a miss's among them - loads nothing.
// - The parameters, the camera basis and the flags are kernel arguments (SolidFrame): scalar registers, no table, no copy.
// - EDGE form: one lane per pixel, four-byte accesses, the same solid_pixel.  It takes the npix % 4 pixels behind the last whole
//   group, and every pixel of a call in which a plane's pointer is not 16-byte aligned (host::solid_wide).  Both forms give the
//   same bits: they differ in the loads and the stores alone.
// - The grid is not capped: npix <= 2^28, so at most 2^18 + 1 workgroups of the wide form, 2^20 of the edge form.
// d_out may be d_albedo or d_normal (no __restrict__): a lane reads all its pixels' inputs before it stores any.
#include "pt_solid.h"

namespace pt {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// a lane's own words: read once and never again by this kernel (pt_reproject.h's reproject_own, 16 bytes wide)
template <class V, class T>
__device__ __forceinline__ V solid_own16(const T *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
}

// solid_rec for an id every lane at work holds (`u` comes from a readfirstlane): the load goes through the constant address
// space, which a uniform address turns into one scalar load of four dwords for the wave.  The table is the call's copy: nothing
// writes it while the kernel runs.  Read field by field: read as one ext_vector of four words and taken apart with .x .y .z, this
// compiler handed all three emission channels the first word (the 5x1 frame of one lamp in tests/test_gpu_solid.py sees it).
__device__ __forceinline__ pt_solid_look solid_rec_uniform(const pt_solid_look *looks, uint32_t n_looks, int32_t u) {
    pt_solid_look r = {{0.0f, 0.0f, 0.0f}, PT_DIFFUSE};
    if ((uint32_t)u < n_looks) {
        const auto *q = (const __attribute__((address_space(4))) pt_solid_look *)(looks + (uint32_t)u);
        r.emission[0] = q->emission[0], r.emission[1] = q->emission[1], r.emission[2] = q->emission[2];
        r.reflect_type = q->reflect_type;
    }
    return r;
}

__device__ __forceinline__ void solid_one(const SolidFrame &f, uint32_t idx) {
    const int32_t id = reproject_own(f.object_id + idx);
    const size_t i3 = (size_t)idx * 3u;
    float o[3] = {f.p.background[0], f.p.background[1], f.p.background[2]};  // step 1
    if (id >= 0) {
        const float depth = reproject_own(f.depth + idx);
        const float n[3] = {reproject_own(f.normal + i3), reproject_own(f.normal + i3 + 1), reproject_own(f.normal + i3 + 2)};
        float a[3] = {1.0f, 1.0f, 1.0f};
        if (f.albedo) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] = reproject_own(f.albedo + i3 + c);
        }
        const pt_solid_look rec = solid_rec(f.looks, f.n_looks, id);
        solid_pixel(f, idx, id, depth, a, n, rec, o);
    }
    f.out[i3] = o[0];
    f.out[i3 + 1] = o[1];
    f.out[i3 + 2] = o[2];
}

__device__ __forceinline__ void solid_four(const SolidFrame &f, uint32_t group) {
    const uint32_t i0 = group * kSolidLanePixels;
    const size_t i3 = (size_t)i0 * 3u;
    f32x4 *out4 = reinterpret_cast<f32x4 *>(f.out + i3);
    const i32x4 id4 = solid_own16<i32x4>(f.object_id + i0);
    const int32_t id[4] = {id4.x, id4.y, id4.z, id4.w};
    if ((id[0] & id[1] & id[2] & id[3]) < 0) {  // all four missed
        const float b0 = f.p.background[0], b1 = f.p.background[1], b2 = f.p.background[2];
        out4[0] = f32x4{b0, b1, b2, b0};
        out4[1] = f32x4{b1, b2, b0, b1};
        out4[2] = f32x4{b2, b0, b1, b2};
        return;
    }
    const bool with_albedo = f.albedo != nullptr;  // uniform: a kernel argument
    const f32x4 z4 = solid_own16<f32x4>(f.depth + i0);
    const f32x4 n0 = solid_own16<f32x4>(f.normal + i3), n1 = solid_own16<f32x4>(f.normal + i3 + 4), n2 = solid_own16<f32x4>(f.normal + i3 + 8);
    f32x4 a0 = {1.0f, 1.0f, 1.0f, 1.0f}, a1 = a0, a2 = a0;
    if (with_albedo) {
        a0 = solid_own16<f32x4>(f.albedo + i3);
        a1 = solid_own16<f32x4>(f.albedo + i3 + 4);
        a2 = solid_own16<f32x4>(f.albedo + i3 + 8);
    }
    // the records: one fetch at a uniform address where the lanes at work here hold one id, else one per pixel
    pt_solid_look rec[4];
    const int32_t u = __builtin_amdgcn_readfirstlane(id[0]);
    const bool mine = id[0] == u && id[1] == u && id[2] == u && id[3] == u;
    if (__builtin_amdgcn_ballot_w64(!mine) == 0ull) {
        rec[0] = solid_rec_uniform(f.looks, f.n_looks, u);
        rec[1] = rec[2] = rec[3] = rec[0];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) rec[j] = solid_rec(f.looks, f.n_looks, id[j]);
    }
    const float z[4] = {z4.x, z4.y, z4.z, z4.w};
    const float n[12] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w};
    const float a[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
    float o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) solid_pixel(f, i0 + (uint32_t)j, id[j], z[j], a + 3 * j, n + 3 * j, rec[j], o + 3 * j);
    out4[0] = f32x4{o[0], o[1], o[2], o[3]};
    out4[1] = f32x4{o[4], o[5], o[6], o[7]};
    out4[2] = f32x4{o[8], o[9], o[10], o[11]};
}

// WIDE: lanes [0, groups) own four pixels each, lanes [groups, groups + npix % 4) one pixel of the rest.  Else a lane per pixel.
template <bool WIDE>
__global__ __launch_bounds__(kSolidBlock) void k_solid(const SolidFrame f, uint32_t groups, uint32_t npix) {
    const uint32_t lane = blockIdx.x * kSolidBlock + threadIdx.x;
    if constexpr (WIDE) {
        if (lane < groups) {
            solid_four(f, lane);
            return;
        }
    }
    const uint32_t idx = WIDE ? groups * kSolidLanePixels + (lane - groups) : lane;
    if (idx < npix) solid_one(f, idx);
}

}  // namespace

void launch_solid(hipStream_t st, const SolidFrame &f) {
    const uint32_t npix = f.width * f.height;  // at most 2^28
    if (host::solid_wide(f)) {
        const uint32_t groups = npix / kSolidLanePixels, lanes = groups + npix % kSolidLanePixels;
        hipLaunchKernelGGL((k_solid<true>), dim3((lanes + kSolidBlock - 1u) / kSolidBlock), dim3(kSolidBlock), 0, st, f, groups, npix);
    } else {
        hipLaunchKernelGGL((k_solid<false>), dim3((npix + kSolidBlock - 1u) / kSolidBlock), dim3(kSolidBlock), 0, st, f, 0u, npix);
    }
}

}  // namespace pt
