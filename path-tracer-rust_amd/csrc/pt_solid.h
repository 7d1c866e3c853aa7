// pt_solid.h — pt_ctx_solid (pt_solid.hip): a lit solid view of a whole frame from the first-hit guides - ambient, diffuse and one
// highlight from one light, times the albedo, plus what the looks table knows of the object (its emission, whether it mirrors the
// sky).  The arithmetic is the contract in include/ptrace_solid.h ("THE ARITHMETIC" of pt_ctx_solid), operation for operation.
// Steps 1 to 8 for one pixel are stated once, below, for host and device: pt_solid_pixel_host (host/scene_io.cpp) is the host
// instantiation of the source the kernel compiles, as pt_overlay_pixel_host is of pt_overlay.h.  Step 2's ray is pt_reproject.h's
// reproject_ray and step 3's normal its reproject_normal, called and not restated.
// A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace_solid.h"
#include "pt_math.h"
#include "pt_reproject.h"

namespace pt {

// what a NULL params stands for and pt_solid_defaults writes out; the sky is pt_overlay_defaults' (host/scene_io.cpp)
constexpr pt_solid_params kSolidDefaults = {PT_SOLID_HEADLIGHT, {0.0f, 0.0f, 0.0f}, 0.1f, 1.0f, 0.5f, 5u, {0.0f, 0.0f, 0.0f},
                                            {0.25f, 0.5f, 0.75f}, {0.75f, 0.75f, 0.75f}};
constexpr uint32_t kSolidMaxLooks = 1u << 20;
// the kernel's units: a workgroup of 256 lanes, and in the wide form four consecutive pixels per lane (pt_solid.hip)
constexpr uint32_t kSolidBlock = 256u, kSolidLanePixels = 4u;

// The call once it has passed.  Host pointers on the host, device pointers on the device; a kernel argument as it stands.
// `looks` is the caller's HOST array when host::check_solid returns; pt_ctx_solid replaces it by the copy in the context's scratch
// (16-byte aligned) before the launch, or by NULL when n_looks is 0.
struct SolidFrame {
    uint32_t width, height;
    const float *albedo;  // NULL: every albedo is (1, 1, 1)
    const float *normal, *depth;
    const int32_t *object_id;
    float *out;  // may be albedo or normal
    const pt_solid_look *looks;
    uint32_t n_looks;
    pt_solid_params p;  // as it stands: the defaults when the call passed NULL
    vec3 C, L, su, sv;  // cam's position and its pt_camera_basis, in binary32
};

PT_HD float solid_pos(float v) { return v > 0.0f ? v : 0.0f; }  // a NaN gives 0
PT_HD float solid_mix(float a, float b, float t) { return a + (b - a) * t; }
PT_HD float solid_clamp(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// step 7's record: an id beyond the table (a miss's id as uint32 among them) reads nothing and stands for {0, 0, 0, PT_DIFFUSE},
// as a NULL table does.  One 16-byte load on the device.
PT_HD pt_solid_look solid_rec(const pt_solid_look *looks, uint32_t n_looks, int32_t id) {
    pt_solid_look r = {{0.0f, 0.0f, 0.0f}, PT_DIFFUSE};
    if ((uint32_t)id < n_looks) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 q = *reinterpret_cast<const uint4 *>(looks + (uint32_t)id);
        r.emission[0] = __builtin_bit_cast(float, q.x), r.emission[1] = __builtin_bit_cast(float, q.y);
        r.emission[2] = __builtin_bit_cast(float, q.z), r.reflect_type = q.w;
#else
        r = looks[(uint32_t)id];
#endif
    }
    return r;
}

// Steps 1 to 8 for pixel idx but for the loads and the store.  `A`: the pixel's albedo, (1, 1, 1) from the caller where the call
// has no albedo plane (1 * k is k); `n`: its normal as stored; `rec`: its object's record.  With id < 0 neither depth, A, n nor
// rec is looked at.
PT_HD void solid_pixel(const SolidFrame &f, uint32_t idx, int32_t id, float depth, const float A[3], const float n[3], const pt_solid_look &rec,
                       float out[3]) {
    const pt_solid_params &p = f.p;
    if (id < 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = p.background[c];
        return;
    }
    const uint32_t x = idx % f.width, r = idx / f.width, y = f.height - 1u - r;
    const vec3 d = reproject_ray(f.C, f.L, f.su, f.sv, f.width, f.height, x, y);
    const vec3 P = mk(f.L.x + d.x * depth, f.L.y + d.y * depth, f.L.z + d.z * depth);
    const vec3 v = mk(-d.x, -d.y, -d.z);
    const vec3 N = reproject_normal(n);
    const vec3 Q = (p.flags & PT_SOLID_HEADLIGHT) ? f.L : mk(p.light[0], p.light[1], p.light[2]);
    const vec3 lv = Q - P;
    const float ll = __builtin_sqrtf(dot(lv, lv));
    const vec3 ld = ll > 0.0f ? lv * (1.0f / ll) : mk(0.0f, 0.0f, 0.0f);
    const float ndl = dot(N, ld);
    const float dif = solid_pos(ndl);
    const float two_ndl = 2.0f * ndl;
    const vec3 rf = mk(N.x * two_ndl - ld.x, N.y * two_ndl - ld.y, N.z * two_ndl - ld.z);
    float s = ndl > 0.0f ? solid_pos(dot(v, rf)) : 0.0f;
    for (uint32_t i = 0; i < p.shininess_log2; ++i) s = s * s;
    const float spec = p.specular * s;
    const float k = (p.ambient + p.diffuse * dif) + spec;
    const bool mirror = (p.flags & PT_SOLID_REFLECT_SKY) && rec.reflect_type == PT_SPECULAR;
    float t = 0.0f;
    if (mirror) {
        const float dn = dot(N, d);
        const float my = d.y - N.y * (2.0f * dn);
        t = solid_clamp(my * 0.5f + 0.5f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = A[c];
        const float b = mirror ? a * solid_mix(p.sky_bottom[c], p.sky_top[c], t) + spec : a * k;
        out[c] = solid_clamp(b + rec.emission[c]);
    }
}

namespace host {
// The refusals that need the params alone, in the header's order (its first five): PT_OK: P holds the params, the defaults for
// a NULL.  pt_solid_pixel_host makes them too.
int check_solid_params(const pt_solid_params *params, pt_solid_params &P);
// a record of the looks table: PT_ERR_INVALID for a reflect_type above PT_REFRACT or an emission that is negative or not finite
int check_solid_look(const pt_solid_look &look);
// the frame's size and camera, the header's next four: PT_OK: f holds width, height, C, L, su, sv
int check_solid_view(uint32_t width, uint32_t height, const pt_camera *cam, SolidFrame &f);
// pt_ctx_solid's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call, f.looks the caller's host
// array.  No device is touched.
int check_solid(const void *ctx, uint32_t width, uint32_t height, const pt_solid_params *params, const pt_camera *cam, const float *d_albedo,
                const float *d_normal, const float *d_depth, const int32_t *d_object_id, const pt_solid_look *looks, uint32_t n_looks,
                float *d_out, SolidFrame &f);
// the wide form is valid: every plane handed over is 16-byte aligned and the frame holds a whole group of four pixels
bool solid_wide(const SolidFrame &f);
}  // namespace host

#if defined(__HIPCC__)
// one lane per four consecutive pixels, then one per pixel of the rest; one lane per pixel throughout where !solid_wide(f)
void launch_solid(hipStream_t st, const SolidFrame &f);
#endif

}  // namespace pt
