// despike_check — the firefly stage's host side under a sanitizer, as a program of its own (make despike-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the validator's refusals in the header's order,
// pt_despike_frame_host - the source the kernel compiles - on handcrafted frames at the window's edges (1x1, 1xN, Nx1, both
// radii, a rank equal to the neighbour count, every non-finite pattern), and a restatement written independently below (a sort
// of the window, not the insertion chain) over a few thousand random small frames: a failed check or a sanitizer report ends it
// with a non-zero status.
#include <algorithm>
#include <functional>

#include "check_common.h"
#include "../csrc/pt_despike.h"
#include "../../include/ptrace_despike.h"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// include/ptrace_despike.h restated: the window's valid luminances collected, sorted descending, element rank-1 taken
struct Restated {
    std::vector<float> out;
    std::vector<uint8_t> mask;
    uint64_t spikes = 0, nonfinite = 0;
};
static bool bad_pixel(const float *v) {
    for (int c = 0; c < 3; ++c)
        if (((bits_of(v[c]) >> 23) & 0xffu) == 0xffu) return true;
    return false;
}
static float lum(const float *v) {
    const volatile float a = 0.2126f * v[0], b = 0.7152f * v[1], c = 0.0722f * v[2];
    const volatile float ab = a + b;
    return ab + c;
}
static Restated restate(int w, int h, const pt_despike_params &p, const std::vector<float> &rgb, const int32_t *ids) {
    Restated r;
    r.out = rgb;
    r.mask.assign((size_t)w * h, 0);
    const int R = (int)p.radius;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            const float *v = &rgb[i * 3];
            if (bad_pixel(v)) {
                r.out[i * 3] = r.out[i * 3 + 1] = r.out[i * 3 + 2] = 0.0f;
                r.mask[i] = 2, ++r.nonfinite;
                continue;
            }
            std::vector<float> ys;
            for (int qy = std::max(0, y - R); qy <= std::min(h - 1, y + R); ++qy)
                for (int qx = std::max(0, x - R); qx <= std::min(w - 1, x + R); ++qx) {
                    const size_t q = (size_t)qy * w + qx;
                    if (q == i || bad_pixel(&rgb[q * 3])) continue;
                    if ((p.flags & PT_DESPIKE_SAME_OBJECT) && ids[q] != ids[i]) continue;
                    const float Y = lum(&rgb[q * 3]);
                    ys.push_back(Y > 0.0f ? Y : 0.0f);
                }
            if (ys.size() < p.rank) continue;
            std::sort(ys.begin(), ys.end(), std::greater<float>());
            const volatile float tr = p.threshold * ys[p.rank - 1];
            const float L = tr + p.floor, Y = lum(v);
            if (Y > L) {
                const float s = L / Y;
                for (int c = 0; c < 3; ++c) r.out[i * 3 + c] = v[c] * s;
                r.mask[i] = 1, ++r.spikes;
            }
        }
    return r;
}

// pt_despike_frame_host over the frame, guards around both outputs; true if it equals the restatement bit for bit
static bool agrees(int w, int h, const pt_despike_params &p, const std::vector<float> &rgb, const int32_t *ids, bool with_mask,
                   Restated *keep = nullptr) {
    const size_t n = (size_t)w * h, G = 4;
    std::vector<float> out(n * 3 + 2 * G, -7.5f);
    std::vector<uint8_t> mask(n + 2 * G, 0xEE);
    pt_despike_stats st = {};
    if (pt_despike_frame_host((uint32_t)w, (uint32_t)h, &p, rgb.data(), ids, out.data() + G, with_mask ? mask.data() + G : nullptr, &st) != PT_OK)
        return false;
    const Restated r = restate(w, h, p, rgb, ids);
    if (keep) *keep = r;
    for (size_t g = 0; g < G; ++g)
        if (out[g] != -7.5f || out[G + n * 3 + g] != -7.5f || mask[g] != 0xEE || mask[G + n + g] != 0xEE) return false;
    if (memcmp(out.data() + G, r.out.data(), n * 12) != 0) return false;
    if (with_mask ? memcmp(mask.data() + G, r.mask.data(), n) != 0 : mask[G] != 0xEE) return false;
    return st.pixels == n && st.spikes == r.spikes && st.nonfinite == r.nonfinite;
}

static std::vector<float> flat(int n, float v) { return std::vector<float>((size_t)n * 3, v); }

int main() {
    float buf[4], buf2[4];
    int32_t ibuf[4];
    uint8_t mbuf[4];
    const void *ctx = buf;  // never dereferenced
    // ---- the refusals, in the header's order: each call breaks one rule and every rule after it
    {
        pt::DespikeFrame f;
        pt_despike_params p = {0u, 0u, 2u, 0.5f, -1.0f};
        auto chk = [&](uint32_t w, uint32_t h, const float *rgb, const int32_t *ids, float *out, const void *c = nullptr) {
            return pt::host::check_despike(c, w, h, &p, rgb, ids, out, nullptr, f);
        };
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "radius"));
        p.radius = 3u;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "radius"));
        p.radius = 1u;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "rank"));
        p.rank = 5u;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "rank"));
        p.rank = 4u;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "flags"));
        p.flags = 0x80000001u;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "flags"));
        p.flags = PT_DESPIKE_SAME_OBJECT;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "threshold"));
        p.threshold = NAN;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "threshold"));
        p.threshold = INFINITY;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "threshold"));
        p.threshold = 1.0f;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "floor"));
        p.floor = NAN;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "floor"));
        p.floor = INFINITY;
        CHECK(refused(chk(0, 0, nullptr, nullptr, nullptr), "floor"));
        p.floor = 0.0f;
        CHECK(refused(chk(0, 3, nullptr, nullptr, nullptr), "must be positive"));
        CHECK(refused(chk(3, 0, nullptr, nullptr, nullptr), "must be positive"));
        CHECK(refused(chk(1u << 15, 1u << 15, nullptr, nullptr, nullptr), "2^28"));
        CHECK(refused(chk(2, 2, nullptr, nullptr, nullptr), "d_rgb"));
        CHECK(refused(chk(2, 2, buf, nullptr, nullptr), "d_out is NULL"));
        CHECK(refused(chk(2, 2, buf, nullptr, buf), "d_out is d_rgb"));
        CHECK(refused(chk(2, 2, buf, nullptr, buf2), "d_object_id"));
        CHECK(refused(chk(2, 2, buf, ibuf, buf2), "ctx"));
        CHECK(pt::host::check_despike(ctx, 1u << 14, 1u << 14, &p, buf, ibuf, buf2, mbuf, f) == PT_OK);  // 2^28 exactly
        CHECK(f.radius == 1u && f.rank == 4u && f.threshold == 1.0f && f.floor == 0.0f && f.rgb == buf && f.out == buf2 && f.object_id == ibuf &&
              f.mask == mbuf && f.counters == nullptr && f.width == (1u << 14));
        p.flags = 0u;  // the ids are not read without the flag
        CHECK(pt::host::check_despike(ctx, 2, 2, &p, buf, ibuf, buf2, nullptr, f) == PT_OK && f.object_id == nullptr && f.mask == nullptr);
        CHECK(pt::host::check_despike(ctx, 2, 2, nullptr, buf, nullptr, buf2, nullptr, f) == PT_OK);  // the defaults
        CHECK(f.radius == 1u && f.rank == 3u && f.threshold == 2.0f && f.floor == 0.25f);
        // the host call refuses the same, a context apart, and leaves its outputs as they were
        float out3[3] = {5.0f, 5.0f, 5.0f};
        const float one[3] = {1.0f, 1.0f, 1.0f};
        pt_despike_stats st = {77u, 77u, 77u};
        p.rank = 0u;
        CHECK(refused(pt_despike_frame_host(1, 1, &p, one, nullptr, out3, mbuf, &st), "rank"));
        p.rank = 1u;
        CHECK(refused(pt_despike_frame_host(1, 1, &p, nullptr, nullptr, out3, mbuf, &st), "d_rgb"));
        CHECK(refused(pt_despike_frame_host(1, 1, &p, one, nullptr, nullptr, mbuf, &st), "d_out"));
        CHECK(out3[0] == 5.0f && st.pixels == 77u && st.spikes == 77u);
        CHECK(pt_despike_frame_host(1, 1, &p, one, nullptr, out3, nullptr, nullptr) == PT_OK && out3[0] == 1.0f);  // mask and out may be NULL
        CHECK(pt_despike_frame_host(1, 1, nullptr, one, nullptr, out3, nullptr, nullptr) == PT_OK);  // NULL params: the defaults
    }
    // ---- by hand.  Background 1 (Y = 1 to an ulp), threshold 2, floor 0.5: the limit over a flat neighbourhood is about 2.5
    {
        pt_despike_params p = {1u, 1u, 0u, 2.0f, 0.5f};
        Restated r;
        // 1x1: no neighbour, copied, whatever it holds
        std::vector<float> v = {1e30f, -0.0f, 3.0f};
        CHECK(agrees(1, 1, p, v, nullptr, true, &r) && r.spikes == 0 && bits_of(r.out[1]) == 0x80000000u);
        v = {NAN, 1.0f, 1.0f};
        CHECK(agrees(1, 1, p, v, nullptr, true, &r) && r.nonfinite == 1 && r.mask[0] == 2 && bits_of(r.out[0]) == 0u && bits_of(r.out[1]) == 0u);
        // 1x7 and 7x1, a spike in the middle and one at each end; rank 2 = the neighbour count inside, above it at the ends
        for (int rank = 1; rank <= 4; ++rank)
            for (int radius = 1; radius <= 2; ++radius)
                for (int vertical = 0; vertical < 2; ++vertical) {
                    p.rank = (uint32_t)rank, p.radius = (uint32_t)radius;
                    v = flat(7, 1.0f);
                    for (int at : {0, 3, 6}) v[at * 3] = v[at * 3 + 1] = v[at * 3 + 2] = 64.0f;
                    CHECK(agrees(vertical ? 1 : 7, vertical ? 7 : 1, p, v, nullptr, true, &r));
                    // a pixel of a line has 2 * radius neighbours inside, `radius` at an end: fewer than rank leaves it alone
                    CHECK((r.mask[3] == 1) == (rank <= 2 * radius) && (r.mask[0] == 1) == (rank <= radius) && r.mask[0] == r.mask[6]);
                    if (r.mask[3] == 1) CHECK(fabsf(lum(&r.out[9]) - 2.5f) < 1e-5f && r.out[9] == r.out[10]);
                }
        // 3x3, rank 8 is refused above 4; rank 4 at radius 1 in a corner (3 neighbours) is copied, at the centre (8) clipped
        p = pt_despike_params{1u, 4u, 0u, 2.0f, 0.5f};
        v = flat(9, 1.0f);
        v[0] = v[1] = v[2] = 64.0f;
        v[12] = v[13] = v[14] = 64.0f;
        CHECK(agrees(3, 3, p, v, nullptr, true, &r) && r.mask[0] == 0 && r.mask[4] == 1 && r.spikes == 1);
        // a touching pair survives rank 1 and is clipped at rank 2; a line of three survives rank 2 but for its ends
        for (uint32_t rank = 1; rank <= 2; ++rank) {
            p = pt_despike_params{1u, rank, 0u, 2.0f, 0.5f};
            v = flat(7 * 5, 1.0f);
            for (int at : {2 * 7 + 2, 2 * 7 + 3}) v[at * 3] = v[at * 3 + 1] = v[at * 3 + 2] = 64.0f;
            CHECK(agrees(7, 5, p, v, nullptr, true, &r) && r.spikes == (rank == 1 ? 0u : 2u));
        }
        v = flat(7 * 5, 1.0f);
        for (int at : {2 * 7 + 1, 2 * 7 + 2, 2 * 7 + 3, 2 * 7 + 4, 2 * 7 + 5}) v[at * 3] = v[at * 3 + 1] = v[at * 3 + 2] = 64.0f;
        CHECK(agrees(7, 5, p, v, nullptr, true, &r) && r.spikes == 2 && r.mask[2 * 7 + 1] == 1 && r.mask[2 * 7 + 5] == 1 && r.mask[2 * 7 + 3] == 0);
        // every non-finite pattern in every channel: written as 0, mask 2, and no neighbour counts it
        const uint32_t pats[] = {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x7fa00000u};
        for (uint32_t pat : pats)
            for (int c = 0; c < 3; ++c) {
                p = pt_despike_params{1u, 1u, 0u, 2.0f, 0.5f};
                v = flat(9, 1.0f);
                v[4 * 3 + c] = from_bits(pat);       // the centre
                v[0] = v[1] = v[2] = 64.0f;          // a spike beside it
                CHECK(agrees(3, 3, p, v, nullptr, true, &r) && r.mask[4] == 2 && r.nonfinite == 1 && r.mask[0] == 1);
                for (int k = 0; k < 3; ++k) CHECK(bits_of(r.out[12 + k]) == 0u);
            }
        // the largest finite values are not non-finite; a luminance that overflows shields its neighbours (R = +inf)
        v = flat(9, 1.0f);
        v[12] = v[13] = v[14] = from_bits(0x7f7fffffu);
        v[0] = v[1] = v[2] = 64.0f;
        CHECK(agrees(3, 3, p, v, nullptr, true, &r) && r.nonfinite == 0 && r.mask[4] == 1);
        // -0 channels stay -0 where the pixel is copied; a negative luminance counts as 0 for its neighbours and is no spike
        v = flat(9, 1.0f);
        v[12] = -0.0f, v[13] = -0.0f, v[14] = -0.0f;
        v[3] = v[4] = v[5] = -3.0f;
        CHECK(agrees(3, 3, p, v, nullptr, true, &r) && r.spikes == 0 && bits_of(r.out[12]) == 0x80000000u && r.out[3] == -3.0f);
        // a frame of one colour is copied; Y <= floor is never a spike even over a black neighbourhood
        v = flat(9, 0.0f);
        v[12] = v[13] = v[14] = 0.49f;
        CHECK(agrees(3, 3, p, v, nullptr, true, &r) && r.spikes == 0);
        v[12] = v[13] = v[14] = 0.51f;
        CHECK(agrees(3, 3, p, v, nullptr, true, &r) && r.spikes == 1);
        // the flag: a spike whose neighbours all belong to another object has m = 0 and is copied
        p.flags = PT_DESPIKE_SAME_OBJECT;
        v = flat(9, 1.0f);
        v[12] = v[13] = v[14] = 64.0f;
        int32_t ids[9] = {0, 0, 0, 0, 1, 0, 0, 0, 0};
        CHECK(agrees(3, 3, p, v, ids, true, &r) && r.spikes == 0);
        ids[5] = 1;
        CHECK(agrees(3, 3, p, v, ids, true, &r) && r.spikes == 1);
        CHECK(agrees(3, 3, p, v, ids, false));
    }
    // ---- the restatement over random small frames
    {
        uint32_t s = 2024u;
        int frames = 0;
        for (int trial = 0; trial < 3000; ++trial) {
            const int w = 1 + (int)(lcg(s) >> 8) % 9, h = 1 + (int)(lcg(s) >> 8) % 7;
            pt_despike_params p;
            p.radius = 1u + (lcg(s) >> 8) % 2u;
            p.rank = 1u + (lcg(s) >> 8) % 4u;
            p.flags = (lcg(s) >> 8) % 2u;
            const float ts[] = {1.0f, 1.5f, 2.0f, 4.0f, 16.0f}, fs[] = {0.0f, 0.25f, 1.0f, 4.0f};
            p.threshold = ts[(lcg(s) >> 8) % 5u];
            p.floor = fs[(lcg(s) >> 8) % 4u];
            std::vector<float> v((size_t)w * h * 3);
            std::vector<int32_t> ids((size_t)w * h);
            for (float &x : v) {
                const uint32_t k = (lcg(s) >> 8) % 32u;
                x = k == 0u ? 64.0f * unit(s) : k == 1u ? 1e30f : k == 2u ? -unit(s) : k == 3u ? from_bits(lcg(s)) : k == 4u ? -0.0f : 0.5f + 0.5f * unit(s);
            }
            for (int32_t &i : ids) i = (int32_t)((lcg(s) >> 8) % 3u) - 1;
            CHECK(agrees(w, h, p, v, ids.data(), (trial & 1) != 0));
            ++frames;
        }
        CHECK(frames == 3000);
    }
    printf("despike_check: ok\n");
    return 0;
}
