// pt_present.h — pt_ctx_present (pt_present.hip): a linear float frame in device memory to gamma-corrected 8-bit pixels at the
// size asked for, in display order.  The arithmetic is the contract in include/ptrace.h ("THE ARITHMETIC" of pt_ctx_present),
// operation for operation.  The per-value steps and the footprint of an output cell are stated once, below, for host and device:
// pt_present_quantize_host (host/scene_io.cpp) is the host instantiation of the source the kernels compile, as pt_host_sincos is
// of sincos_f32.  A translation unit of its own: pt_kernels.s, and so pt_kernel_isa_hash(), describes the pass kernels only.
#pragma once

#include "../../include/ptrace.h"
#include "pt_math.h"

namespace pt {

// step 2: v' = v * exposure (one multiply), c(v') = v' > 0 ? (v' > 1 ? 1 : v') : 0.  NaN and -0 give +0, +inf gives 1.
PT_HD float present_clamp(float v, float exposure) {
    const float e = v * exposure;
    return e > 0.0f ? (e > 1.0f ? 1.0f : e) : 0.0f;
}

PT_HD uint32_t present_bits(float m) {
    uint32_t u;
    memcpy(&u, &m, 4);
    return u;
}

// step 5: the number of k in 1..255 with bits >= T[k], for T[0] = 0 and T non-decreasing: the largest k with T[k] <= bits, found
// in eight steps without a branch.  T may be in LDS or in host memory.
PT_HD uint32_t present_byte(const uint32_t *T, uint32_t bits) {
    uint32_t k = 0u;
#pragma unroll
    for (uint32_t s = 128u; s; s >>= 1) k += T[k + s] <= bits ? s : 0u;
    return k;
}

// step 4: q = floor(c * 2^32) (the product is exact; c = 1 gives 2^32, hence 64 bits)
PT_HD uint64_t present_fixed(float c) { return (uint64_t)(c * 4294967296.0f); }

// step 4: output cell X of `on` cells over an axis of n source pixels covers [X*n, (X+1)*n) where source pixel x covers
// [x*on, (x+1)*on).  The source pixels it overlaps are [first, last); present_weight is the integer length of the overlap with
// one of them (at most min(n, on); the weights of a cell sum to n).
struct PresentSpan {
    uint32_t first, last;
};
PT_HD PresentSpan present_span(uint32_t X, uint32_t n, uint32_t on) {
    const uint64_t lo = (uint64_t)X * n, hi = lo + n;
    PresentSpan s;
    s.first = (uint32_t)(lo / on);
    s.last = (uint32_t)((hi + on - 1u) / on);
    return s;
}
PT_HD uint32_t present_weight(uint32_t X, uint32_t x, uint32_t n, uint32_t on) {
    const uint64_t lo = (uint64_t)X * n, hi = lo + n, a = (uint64_t)x * on, b = a + on;
    return (uint32_t)((hi < b ? hi : b) - (lo > a ? lo : a));
}

// step 4: m = (float)((double)S / ((double)(W*H) * 2^32)): the conversion rounds to nearest even, the divisor is exact, one
// binary64 division, one rounding to binary32
PT_HD float present_mean(uint64_t S, double divisor) { return (float)((double)S / divisor); }

// The table T[0..255] of step 5 (host/scene_io.cpp): built once per process with the host's powf, thread-safe.
const uint32_t *present_table();

struct PresentFrame {
    const float *rgb;     // width * height * 3 floats, framebuffer order
    uint8_t *out;         // out_width * out_height * bpp bytes
    uint32_t width, height, out_width, out_height;
    uint32_t bpp;         // 4 (r, g, b, 255) or 3
    bool flip;            // display order: D(x, y) = frame[W*H-1-(y*W+x)]
    float exposure;
    const uint32_t *table;          // T on the device, 256 entries
    unsigned long long *mid;        // the resampling form's intermediate: [3] planes of width * out_height u64 (NULL: same size)
    bool resamples() const { return out_width != width || out_height != height; }  // the call needs `mid`
};

namespace host {
// pt_ctx_present's refusals in the header's order (PT_ERR_INVALID + message); PT_OK: `f` holds the call with the defaults filled
// in, but for f.table and f.mid, which the caller owns.  No device is touched.
int check_present(const void *ctx, uint32_t width, uint32_t height, const pt_present_params *params, const float *d_rgb, uint8_t *d_out,
                  PresentFrame &f);
}  // namespace host

#if defined(__HIPCC__)
// out_width == width and out_height == height: one streaming kernel.  Otherwise two passes, rows first.
void launch_present(hipStream_t st, const PresentFrame &f);
#endif

}  // namespace pt
