// pt_tone.hip — the tone stage's kernels: pt_ctx_tonemap, pt_ctx_accum_hdr, pt_ctx_meter.  The arithmetic is the contract of
// include/ptrace_tone.h, operation for operation; what happens to one value is pt_tone.h's, which the host compiles too.  Built
// with -ffp-contract=off and correctly rounded /, so a restatement in numpy (tests/tone_ref.py) gives the same bytes.
//
// k_tonemap and k_hdr are streaming passes: 24 B per pixel (12 in, 12 out) and 36 B (three u64, 12 out) against a dozen VALU
// operations and at most four divisions, so memory should bind them and the accesses are made wide, as k_solid's are.
// - WIDE form: a lane owns FOUR consecutive pixels: 48 consecutive bytes of a three-float plane, three 16-byte accesses; of a
//   held plane 32 bytes, two 16-byte loads per channel.  A lane issues all its loads before the first arithmetic and stores
//   after the last (d_out may be d_rgb).
// - EDGE form: one lane per pixel, four- and eight-byte accesses, the same per-value source.  It takes the npix % 4 pixels behind
//   the last whole group, and every pixel of a call in which a plane is not 16-byte aligned (host::tone_wide, host::hdr_wide).
//   Both forms give the same bits: they differ in the loads and the stores alone.
// - k_hdr picks a pixel's count by its part: from a table in the context's scratch, or the one count of a frame of one part.
// - The grid is not capped: npix <= 2^28, so at most 2^18 + 1 workgroups of the wide form, 2^20 of the edge form.
//
// k_meter reads 12 B per pixel (16 with ids) and adds to 1 KB of counters.
// - The frame is walked in ITEMS: a group of four pixels whose first index is a multiple of four, so that with aligned planes its
//   colours are three 16-byte loads and its ids one, wherever a rectangle's rows begin.  Which of the four pixels the call looks
//   at - inside the run, inside the frame, not skipped - is a mask; a group that is not whole inside the frame, and every group
//   of a call with an unaligned plane, is loaded pixel by pixel, masked pixels only.  No access leaves the frame.
// - The grid is capped at kMeterMaxBlocks workgroups; a workgroup strides over the items and keeps a histogram PER WAVE in LDS
//   (4 x kMeterWords words): the bins, the dark count and the maximum.  At the end the four rows are summed and each non-zero
//   word goes to the counters by one global integer atomic (the maximum by an atomic max): at most 258 per workgroup.
// - Before the LDS atomic, equal slots are combined.  Across the wave: where every pixel the wave's lanes look at in this step
//   has ONE slot (a flat region, a frame of one colour, a black frame - the case in which all 64 lanes would queue on one LDS
//   word), one lane adds the count, made by four ballots and popcounts on the scalar side.  Otherwise within the lane: a pixel
//   adds the number of the lane's pixels at its slot, once per distinct slot.
// - Counts are integers and the maximum an integer maximum: the result does not depend on the order of lanes or workgroups.
#include "pt_tone.h"

namespace pt {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// a lane's own words: read once and never again by the kernel
template <class T>
__device__ __forceinline__ T tone_own(const T *p) {
    return __builtin_nontemporal_load(p);
}
template <class V, class T>
__device__ __forceinline__ V tone_own16(const T *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
}

// ---- pt_ctx_tonemap
__device__ __forceinline__ void tonemap_one(const ToneFrame &f, uint32_t idx) {
    const size_t i3 = (size_t)idx * 3u;
    const float v[3] = {tone_own(f.rgb + i3), tone_own(f.rgb + i3 + 1), tone_own(f.rgb + i3 + 2)};
    float o[3];
    tone_pixel(f, v, o);
    f.out[i3] = o[0];
    f.out[i3 + 1] = o[1];
    f.out[i3 + 2] = o[2];
}

__device__ __forceinline__ void tonemap_four(const ToneFrame &f, uint32_t group) {
    const size_t i3 = (size_t)group * kToneLanePixels * 3u;
    const f32x4 a0 = tone_own16<f32x4>(f.rgb + i3), a1 = tone_own16<f32x4>(f.rgb + i3 + 4), a2 = tone_own16<f32x4>(f.rgb + i3 + 8);
    const float v[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
    float o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) tone_pixel(f, v + 3 * j, o + 3 * j);
    f32x4 *out4 = reinterpret_cast<f32x4 *>(f.out + i3);
    out4[0] = f32x4{o[0], o[1], o[2], o[3]};
    out4[1] = f32x4{o[4], o[5], o[6], o[7]};
    out4[2] = f32x4{o[8], o[9], o[10], o[11]};
}

// WIDE: lanes [0, groups) own four pixels each, lanes [groups, groups + npix % 4) one pixel of the rest.  Else a lane per pixel.
template <bool WIDE>
__global__ __launch_bounds__(kToneBlock) void k_tonemap(const ToneFrame f, uint32_t groups, uint32_t npix) {
    const uint32_t lane = blockIdx.x * kToneBlock + threadIdx.x;
    if constexpr (WIDE) {
        if (lane < groups) {
            tonemap_four(f, lane);
            return;
        }
    }
    const uint32_t idx = WIDE ? groups * kToneLanePixels + (lane - groups) : lane;
    if (idx < npix) tonemap_one(f, idx);
}

// ---- pt_ctx_accum_hdr
__device__ __forceinline__ uint32_t hdr_count(const HdrFrame &f, uint32_t part) { return f.counts ? f.counts[part] : f.count; }

__device__ __forceinline__ void hdr_one(const HdrFrame &f, uint32_t idx) {
    const uint32_t n = hdr_count(f, idx / f.part_px);
    const size_t i3 = (size_t)idx * 3u;
    unsigned long long S[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) S[c] = tone_own(f.sums + (size_t)c * f.total + idx);
#pragma unroll
    for (int c = 0; c < 3; ++c) f.out[i3 + c] = hdr_value(S[c], n);
}

__device__ __forceinline__ void hdr_four(const HdrFrame &f, uint32_t group) {
    const uint32_t i0 = group * kToneLanePixels;
    u64x2 lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long *p = f.sums + (size_t)c * f.total + i0;
        lo[c] = tone_own16<u64x2>(p);
        hi[c] = tone_own16<u64x2>(p + 2);
    }
    // the four pixels lie in one part: with a table of counts the parts hold a multiple of four pixels (host::hdr_wide)
    const uint32_t n = hdr_count(f, i0 / f.part_px);
    float o[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = hdr_value(lo[c].x, n);
        o[3 + c] = hdr_value(lo[c].y, n);
        o[6 + c] = hdr_value(hi[c].x, n);
        o[9 + c] = hdr_value(hi[c].y, n);
    }
    f32x4 *out4 = reinterpret_cast<f32x4 *>(f.out + (size_t)i0 * 3u);
    out4[0] = f32x4{o[0], o[1], o[2], o[3]};
    out4[1] = f32x4{o[4], o[5], o[6], o[7]};
    out4[2] = f32x4{o[8], o[9], o[10], o[11]};
}

template <bool WIDE>
__global__ __launch_bounds__(kToneBlock) void k_hdr(const HdrFrame f, uint32_t groups) {
    const uint32_t lane = blockIdx.x * kToneBlock + threadIdx.x;
    if constexpr (WIDE) {
        if (lane < groups) {
            hdr_four(f, lane);
            return;
        }
    }
    const uint32_t idx = WIDE ? groups * kToneLanePixels + (lane - groups) : lane;
    if (idx < f.total) hdr_one(f, idx);
}

// ---- pt_ctx_meter
constexpr uint32_t kMeterNone = 0xffffffffu;  // a pixel the call does not look at

template <bool WIDE>
__global__ __launch_bounds__(kToneBlock) void k_meter(const MeterFrame f, uint32_t items) {
    __shared__ uint32_t rows[kToneBlock / 64u][kMeterWords];
    for (uint32_t i = threadIdx.x; i < (kToneBlock / 64u) * kMeterWords; i += kToneBlock) (&rows[0][0])[i] = 0u;
    __syncthreads();
    uint32_t *row = rows[threadIdx.x >> 6];
    const uint32_t wave_lane = threadIdx.x & 63u;
    uint32_t mx = 0u;

    // (every lane of a wave makes the same number of trips: the ballots below see all 64)
    const uint32_t stride = gridDim.x * kToneBlock;
    for (uint32_t base = blockIdx.x * kToneBlock; base < items; base += stride) {
        const uint32_t t = base + threadIdx.x;
        uint32_t slot[4] = {kMeterNone, kMeterNone, kMeterNone, kMeterNone};
        if (t < items) {
            // item t: group k of run r; the run's pixels are [lo, lo + span)
            const uint32_t r = f.rows == 1u ? 0u : t / f.row_groups, k = t - r * f.row_groups;
            const uint32_t lo = f.first + r * f.pitch, hi = lo + f.span;
            const uint32_t i0 = (lo / 4u + k) * 4u;
            bool look[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) look[j] = i0 + j >= lo && i0 + j < hi;  // (hi <= npix)
            if (look[0] || look[1] || look[2] || look[3]) {
                float v[12];
                if (WIDE && i0 + 3u < f.npix) {
                    if (f.object_id) {
                        const i32x4 id = tone_own16<i32x4>(f.object_id + i0);
                        look[0] = look[0] && id.x >= 0, look[1] = look[1] && id.y >= 0;
                        look[2] = look[2] && id.z >= 0, look[3] = look[3] && id.w >= 0;
                    }
                    if (look[0] || look[1] || look[2] || look[3]) {
                        const float *p = f.rgb + (size_t)i0 * 3u;
                        const f32x4 a0 = tone_own16<f32x4>(p), a1 = tone_own16<f32x4>(p + 4), a2 = tone_own16<f32x4>(p + 8);
                        v[0] = a0.x, v[1] = a0.y, v[2] = a0.z, v[3] = a0.w, v[4] = a1.x, v[5] = a1.y, v[6] = a1.z, v[7] = a1.w;
                        v[8] = a2.x, v[9] = a2.y, v[10] = a2.z, v[11] = a2.w;
                    }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        if (look[j] && f.object_id) look[j] = tone_own(f.object_id + i0 + j) >= 0;
                        if (look[j]) {
                            const float *p = f.rgb + (size_t)(i0 + j) * 3u;
                            v[3 * j] = tone_own(p), v[3 * j + 1] = tone_own(p + 1), v[3 * j + 2] = tone_own(p + 2);
                        }
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if (look[j]) {
                        const float Y = tone_luma(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
                        slot[j] = meter_slot(Y);
                        const uint32_t b = meter_max_bits(Y);
                        mx = b > mx ? b : mx;
                    }
                }
            }
        }
        // one slot for the whole wave: one add by one lane
        const uint32_t mine = slot[0] != kMeterNone ? slot[0] : slot[1] != kMeterNone ? slot[1] : slot[2] != kMeterNone ? slot[2] : slot[3];
        const unsigned long long any = __builtin_amdgcn_ballot_w64(mine != kMeterNone);
        if (any == 0ull) continue;
        const uint32_t leader = (uint32_t)__builtin_ctzll(any);
        const uint32_t u = __builtin_amdgcn_readlane(mine, leader);
        bool other = false;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) other = other || (slot[j] != kMeterNone && slot[j] != u);
        if (__builtin_amdgcn_ballot_w64(other) == 0ull) {
            uint32_t count = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) count += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(slot[j] != kMeterNone));
            if (wave_lane == leader) atomicAdd(&row[u], count);
            continue;
        }
        // else per lane: a pixel adds for its slot unless an earlier pixel of the lane has it
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (slot[j] == kMeterNone) continue;
            bool seen = false;
            uint32_t count = 1u;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                if (i < j) seen = seen || slot[i] == slot[j];
                if (i > j) count += slot[i] == slot[j] ? 1u : 0u;
            }
            if (!seen) atomicAdd(&row[slot[j]], count);
        }
    }
    if (mx) atomicMax(&row[kMeterMax], mx);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= kMeterMax; i += kToneBlock) {
        if (i == kMeterMax) {
            uint32_t m = 0u;
#pragma unroll
            for (uint32_t w = 0; w < kToneBlock / 64u; ++w) m = rows[w][i] > m ? rows[w][i] : m;
            if (m) atomicMax(f.counters + i, m);
        } else {
            uint32_t s = 0u;
#pragma unroll
            for (uint32_t w = 0; w < kToneBlock / 64u; ++w) s += rows[w][i];
            if (s) atomicAdd(f.counters + i, s);
        }
    }
}

}  // namespace

void launch_tonemap(hipStream_t st, const ToneFrame &f) {
    const uint32_t npix = f.width * f.height;  // at most 2^28
    if (host::tone_wide(f)) {
        const uint32_t groups = npix / kToneLanePixels, lanes = groups + npix % kToneLanePixels;
        hipLaunchKernelGGL((k_tonemap<true>), dim3((lanes + kToneBlock - 1u) / kToneBlock), dim3(kToneBlock), 0, st, f, groups, npix);
    } else {
        hipLaunchKernelGGL((k_tonemap<false>), dim3((npix + kToneBlock - 1u) / kToneBlock), dim3(kToneBlock), 0, st, f, 0u, npix);
    }
}

void launch_hdr(hipStream_t st, const HdrFrame &f) {
    if (host::hdr_wide(f)) {
        const uint32_t groups = f.total / kToneLanePixels, lanes = groups + f.total % kToneLanePixels;
        hipLaunchKernelGGL((k_hdr<true>), dim3((lanes + kToneBlock - 1u) / kToneBlock), dim3(kToneBlock), 0, st, f, groups);
    } else {
        hipLaunchKernelGGL((k_hdr<false>), dim3((f.total + kToneBlock - 1u) / kToneBlock), dim3(kToneBlock), 0, st, f, 0u);
    }
}

void launch_meter(hipStream_t st, const MeterFrame &f) {
    const uint32_t items = f.rows * f.row_groups;  // at most 2^28 / 4 + 2 * 2^28 / span ... below 2^30 (host::check_meter)
    const uint32_t want = (items + kToneBlock - 1u) / kToneBlock;
    const dim3 grid(want < kMeterMaxBlocks ? want : kMeterMaxBlocks);
    if (host::meter_wide(f))
        hipLaunchKernelGGL((k_meter<true>), grid, dim3(kToneBlock), 0, st, f, items);
    else
        hipLaunchKernelGGL((k_meter<false>), grid, dim3(kToneBlock), 0, st, f, items);
}

}  // namespace pt
