// tone_check — the tone stage's host side under a sanitizer, as a program of its own (make tone-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  It drives the validators' refusals in the header's order, the
// meter's frame geometry, and the host functions - pt_meter_bin_host and pt_tonemap_pixel_host, the source the kernels compile,
// pt_meter_exposure, pt_meter_exposure_weights, pt_meter_adapt - over the edge tables, against values worked out by hand below: a
// failed check or a sanitizer report ends it with a non-zero status.
#include "check_common.h"
#include "../csrc/pt_tone.h"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f) { return pt::tone_bits(f); }

int main() {
    float buf[4];
    int32_t ibuf[4];
    const void *ctx = buf;  // never dereferenced
    // ---- pt_ctx_tonemap's refusals, in the header's order: each call breaks one rule and every rule after it
    {
        pt::ToneFrame f;
        pt_tonemap_params p = {3u, 2u, -1.0f, -1.0f};
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 0, &p, nullptr, nullptr, f), "curve"));
        p.curve = PT_TONE_REINHARD;
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 0, &p, nullptr, nullptr, f), "flags"));
        p.flags = PT_TONE_LUMA;
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 0, &p, nullptr, nullptr, f), "exposure"));
        p.exposure = NAN;
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 0, &p, nullptr, nullptr, f), "exposure"));
        p.exposure = 2.0f;
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 0, &p, nullptr, nullptr, f), "white"));
        p.white = INFINITY;
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 0, &p, nullptr, nullptr, f), "white"));
        p.curve = PT_TONE_ACES;  // white is not read
        CHECK(refused(pt::host::check_tonemap(nullptr, 0, 3, &p, nullptr, nullptr, f), "must be positive"));
        CHECK(refused(pt::host::check_tonemap(nullptr, 1u << 15, 1u << 15, &p, nullptr, nullptr, f), "2^28"));
        CHECK(refused(pt::host::check_tonemap(nullptr, 2, 2, &p, nullptr, buf, f), "d_rgb"));
        CHECK(refused(pt::host::check_tonemap(nullptr, 2, 2, &p, buf, nullptr, f), "d_out"));
        CHECK(refused(pt::host::check_tonemap(nullptr, 2, 2, &p, buf, buf, f), "ctx"));
        p.curve = PT_TONE_REINHARD, p.white = 4.0f;
        CHECK(pt::host::check_tonemap(ctx, 2, 2, &p, buf, buf, f) == PT_OK);
        CHECK(f.curve == PT_TONE_REINHARD && f.luma && f.exposure == 2.0f && f.iw2 == 0.0625f && f.rgb == buf && f.out == buf);
        CHECK(pt::host::check_tonemap(ctx, 1u << 14, 1u << 14, nullptr, buf, buf, f) == PT_OK);  // 2^28 exactly, the defaults
        CHECK(f.curve == PT_TONE_ACES && !f.luma && f.exposure == 1.0f);
    }
    // ---- pt_ctx_meter's refusals, and the runs it makes of a rectangle
    {
        pt::MeterFrame f;
        pt_meter_stats st;
        pt_meter_params p = {2u, 5u, 5u, 5u, 5u};
        CHECK(refused(pt::host::check_meter(nullptr, 0, 0, &p, nullptr, nullptr, nullptr, f), "flags"));
        p.flags = PT_METER_SKIP_MISSES;
        CHECK(refused(pt::host::check_meter(nullptr, 0, 0, &p, nullptr, nullptr, nullptr, f), "must be positive"));
        CHECK(refused(pt::host::check_meter(nullptr, 1u << 15, 1u << 15, &p, nullptr, nullptr, nullptr, f), "2^28"));
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, nullptr, nullptr, nullptr, f), "empty"));
        p.x1 = 9u, p.y1 = 6u;
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, nullptr, nullptr, nullptr, f), "leaves the frame"));
        p.x1 = 8u, p.y1 = 9u;
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, nullptr, nullptr, nullptr, f), "leaves the frame"));
        p.y1 = 8u;
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, nullptr, nullptr, nullptr, f), "d_rgb"));
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, buf, nullptr, nullptr, f), "d_object_id"));
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, buf, ibuf, nullptr, f), "out is NULL"));
        CHECK(refused(pt::host::check_meter(nullptr, 8, 8, &p, buf, ibuf, &st, f), "ctx"));
        CHECK(pt::host::check_meter(ctx, 8, 8, &p, buf, ibuf, &st, f) == PT_OK);  // columns 5..7 of rows 5..7
        CHECK(f.first == 45u && f.span == 3u && f.pitch == 8u && f.rows == 3u && f.row_groups == 2u && f.npix == 64u && f.object_id == ibuf);
        p = pt_meter_params{0u, 0u, 2u, 8u, 5u};  // whole rows: one run
        CHECK(pt::host::check_meter(ctx, 8, 8, &p, buf, ibuf, &st, f) == PT_OK);
        CHECK(f.first == 16u && f.span == 24u && f.rows == 1u && f.row_groups == 7u && f.object_id == nullptr);
        CHECK(pt::host::check_meter(ctx, 7, 3, nullptr, buf, nullptr, &st, f) == PT_OK);  // the whole frame
        CHECK(f.first == 0u && f.span == 21u && f.rows == 1u && f.npix == 21u);
        // every group a run can touch is among its row_groups
        for (uint32_t first = 0; first < 9u; ++first)
            for (uint32_t span = 1; span < 14u; ++span) CHECK((first + span - 1u) / 4u - first / 4u < (span + 3u) / 4u + 1u);
        uint32_t counters[pt::kMeterWords] = {};
        counters[0] = 3u, counters[255] = 4u, counters[pt::kMeterDark] = 5u, counters[pt::kMeterMax] = bits_of(2.5f);
        pt::host::meter_stats_of(counters, &st);
        CHECK(st.pixels == 12u && st.dark == 5u && st.histogram[0] == 3u && st.histogram[255] == 4u && st.max_luminance == 2.5f);
    }
    // ---- the bin: every edge and its predecessor, and the specials
    {
        int32_t b = 99;
        CHECK(pt_meter_bin_host(1.0f, nullptr) == PT_ERR_INVALID);
        for (uint32_t k = 0; k < 256u; ++k) {
            const uint32_t edge = (pt::kMeterKLo + k) << 20;
            CHECK(pt_meter_bin_host(from_bits(edge), &b) == PT_OK && b == (int32_t)k);
            CHECK(pt_meter_bin_host(from_bits(edge - 1u), &b) == PT_OK && b == (int32_t)k - 1);  // below the first edge: dark
        }
        CHECK(from_bits(pt::kMeterKLo << 20) == 9.5367431640625e-07f && from_bits((pt::kMeterKHi + 1u) << 20) == 4096.0f);
        const struct {
            uint32_t bits;
            int32_t bin;
        } special[] = {{0x7fc00000u, -1}, {0xffc00001u, -1}, {0u, -1}, {0x80000000u, -1}, {0xbf800000u, -1}, {0x007fffffu, -1},
                       {0x45800000u, 255}, {0x45800001u, 255}, {0x7f7fffffu, 255}, {0x7f800000u, 255}, {0xff800000u, -1}, {0x3f800000u, 160}};
        for (const auto &s : special) CHECK(pt_meter_bin_host(from_bits(s.bits), &b) == PT_OK && b == s.bin);
        CHECK(pt::meter_max_bits(NAN) == 0u && pt::meter_max_bits(-1.0f) == 0u && pt::meter_max_bits(-0.0f) == 0u);
        CHECK(pt::meter_max_bits(from_bits(1u)) == 1u && pt::meter_max_bits(INFINITY) == 0x7f800000u);
        CHECK(pt::tone_luma(1.0f, 1.0f, 1.0f) == (0.2126f + 0.7152f) + 0.0722f);
    }
    // ---- the pixel
    {
        float o[3];
        const float v[3] = {0.5f, 2.0f, -1.0f}, odd[3] = {NAN, INFINITY, -0.0f};
        pt_tonemap_params p = {PT_TONE_CLAMP, 0u, 1.0f, 4.0f};
        CHECK(pt_tonemap_pixel_host(&p, nullptr, o) == PT_ERR_INVALID && pt_tonemap_pixel_host(&p, v, nullptr) == PT_ERR_INVALID);
        CHECK(pt_tonemap_pixel_host(&p, v, o) == PT_OK && o[0] == 0.5f && o[1] == 1.0f && o[2] == 0.0f);
        CHECK(pt_tonemap_pixel_host(&p, odd, o) == PT_OK && o[0] == 0.0f && o[1] == 1.0f && bits_of(o[2]) == 0u);
        p.exposure = 0.25f;
        CHECK(pt_tonemap_pixel_host(&p, v, o) == PT_OK && o[0] == 0.125f && o[1] == 0.5f && o[2] == 0.0f);
        // Reinhard: f(white) = (w * (1 + w / w^2)) / (1 + w) = 1, f(1) at white 1 = (1 * 2) / 2 = 1, f(1) at white 4 = 1.0625 / 2
        p = pt_tonemap_params{PT_TONE_REINHARD, 0u, 1.0f, 4.0f};
        const float w[3] = {4.0f, 1.0f, 0.0f};
        CHECK(pt_tonemap_pixel_host(&p, w, o) == PT_OK && o[0] == 1.0f && o[1] == 0.53125f && o[2] == 0.0f);
        CHECK(pt_tonemap_pixel_host(&p, odd, o) == PT_OK && o[0] == 0.0f && o[1] == 1.0f && o[2] == 0.0f);  // 2^32 is far above white
        // ACES at 0: (0 * 0.03) / 0.14 = 0; far out it exceeds 1 (2.51 / 2.43) and is clamped
        p = pt_tonemap_params{PT_TONE_ACES, 0u, 1.0f, 4.0f};
        CHECK(pt_tonemap_pixel_host(&p, odd, o) == PT_OK && o[0] == 0.0f && o[1] == 1.0f && o[2] == 0.0f);
        const float one = (1.0f * (2.51f * 1.0f + 0.03f)) / (1.0f * (2.43f * 1.0f + 0.59f) + 0.14f);
        const float ones[3] = {1.0f, 1.0f, 1.0f};
        CHECK(pt_tonemap_pixel_host(nullptr, ones, o) == PT_OK && o[0] == one && o[1] == one && o[2] == one);  // NULL: the defaults
        // luma: a grey pixel keeps being grey; a black one divides nothing
        p = pt_tonemap_params{PT_TONE_REINHARD, PT_TONE_LUMA, 1.0f, 4.0f};
        const float zero[3] = {0.0f, -3.0f, NAN};
        CHECK(pt_tonemap_pixel_host(&p, zero, o) == PT_OK && bits_of(o[0]) == 0u && bits_of(o[1]) == 0u && bits_of(o[2]) == 0u);
        CHECK(pt_tonemap_pixel_host(&p, ones, o) == PT_OK && o[0] == o[1] && o[1] == o[2] && o[0] > 0.5f && o[0] < 0.54f);
        // over the edge table, every curve: in [0, 1], never NaN
        for (uint32_t curve = PT_TONE_CLAMP; curve <= PT_TONE_ACES; ++curve)
            for (uint32_t flags = 0; flags <= PT_TONE_LUMA; ++flags)
                for (uint32_t k = pt::kMeterKLo - 1u; k <= pt::kMeterKHi + 300u; ++k) {
                    const float t[3] = {from_bits(k << 20), from_bits((k << 20) - 1u), from_bits(0x80000000u | (k << 20))};
                    p = pt_tonemap_params{curve, flags, k % 3u ? 1.0f : 1e-3f, 1e-30f};
                    CHECK(pt_tonemap_pixel_host(&p, t, o) == PT_OK);
                    for (float c : o) CHECK(c >= 0.0f && c <= 1.0f);
                }
        p.curve = 3u;
        CHECK(refused(pt_tonemap_pixel_host(&p, v, o), "curve"));
    }
    // ---- the exposure
    {
        pt_meter_stats s = {};
        pt_meter_exposure_params p = pt::kMeterExposureDefaults, bad;
        double kept[PT_METER_BINS];
        float e = 7.0f;
        CHECK(pt_meter_exposure(nullptr, &p, &e) == PT_ERR_INVALID && pt_meter_exposure(&s, &p, nullptr) == PT_ERR_INVALID);
        CHECK(pt_meter_exposure_weights(&s, &p, nullptr) == PT_ERR_INVALID);
        bad = p, bad.key = 0.0f, bad.low_fraction = 1.0f, bad.min_exposure = 0.0f, bad.max_exposure = -1.0f;
        CHECK(refused(pt_meter_exposure(&s, &bad, &e), "key"));
        bad.key = 0.18f;
        CHECK(refused(pt_meter_exposure(&s, &bad, &e), "outside"));
        bad.low_fraction = 0.5f, bad.high_fraction = 0.5f;
        CHECK(refused(pt_meter_exposure(&s, &bad, &e), "leave nothing"));
        bad.high_fraction = 0.25f;
        CHECK(refused(pt_meter_exposure(&s, &bad, &e), "min_exposure"));
        bad.min_exposure = 1.0f;
        CHECK(refused(pt_meter_exposure(&s, &bad, &e), "max_exposure"));
        CHECK(e == 7.0f);
        CHECK(pt_meter_exposure(&s, nullptr, &e) == PT_OK && e == 1.0f);  // nothing counted
        s.dark = 100u, s.pixels = 100u;
        CHECK(pt_meter_exposure(&s, &p, &e) == PT_OK && e == 1.0f);  // all dark
        // two bins of 50: the darkest quarter of 100 cuts bin 100 in the middle, the brightest quarter bin 200
        s.histogram[100] = 50u, s.histogram[200] = 50u;
        p = pt_meter_exposure_params{0.18f, 0.25f, 0.25f, 0.00390625f, 256.0f};
        CHECK(pt_meter_exposure_weights(&s, &p, kept) == PT_OK && kept[100] == 25.0 && kept[200] == 25.0 && kept[0] == 0.0 && kept[255] == 0.0);
        // their log-average: -20 + (150 + 0.5) / 8 = -1.1875
        CHECK(pt_meter_exposure(&s, &p, &e) == PT_OK && fabs((double)e - 0.18 / exp2(-1.1875)) < 1e-6);
        p.max_exposure = 0.25f;
        CHECK(pt_meter_exposure(&s, &p, &e) == PT_OK && e == 0.25f);
        p.min_exposure = 1.0f, p.max_exposure = 2.0f;
        CHECK(pt_meter_exposure(&s, &p, &e) == PT_OK && e == 1.0f);
        // a full histogram at the largest counts
        for (uint32_t b = 0; b < PT_METER_BINS; ++b) s.histogram[b] = 0xffffffffu;
        CHECK(pt_meter_exposure_weights(&s, nullptr, kept) == PT_OK && kept[128] == 4294967295.0);
        CHECK(pt_meter_exposure(&s, nullptr, &e) == PT_OK && e > 0.00390625f && e < 256.0f);
    }
    // ---- the adaptation
    {
        float n = 7.0f;
        CHECK(pt_meter_adapt(1.0f, 2.0f, 1.0f, 1.0f, nullptr) == PT_ERR_INVALID);
        CHECK(refused(pt_meter_adapt(0.0f, 2.0f, 1.0f, 1.0f, &n), "current and target"));
        CHECK(refused(pt_meter_adapt(1.0f, NAN, 1.0f, 1.0f, &n), "current and target"));
        CHECK(refused(pt_meter_adapt(1.0f, 2.0f, -1.0f, 1.0f, &n), "dt and tau"));
        CHECK(refused(pt_meter_adapt(1.0f, 2.0f, 1.0f, INFINITY, &n), "dt and tau"));
        CHECK(n == 7.0f);
        CHECK(pt_meter_adapt(1.0f, 8.0f, 1.0f, 0.0f, &n) == PT_OK && n == 8.0f);
        CHECK(pt_meter_adapt(1.0f, 8.0f, 0.0f, 1.0f, &n) == PT_OK && n == 1.0f);
        float last = 1.0f;
        for (float dt = 0.001f; dt < 100.0f; dt *= 2.0f) {
            CHECK(pt_meter_adapt(1.0f, 8.0f, dt, 0.5f, &n) == PT_OK && n >= last && n <= 8.0f);
            last = n;
        }
        CHECK(last == 8.0f);
        // one time constant: 1 - 1/e of the way in log2: 2^(3 * 0.63212) = 3.7228
        CHECK(pt_meter_adapt(1.0f, 8.0f, 0.5f, 0.5f, &n) == PT_OK && fabsf(n - 3.7228f) < 1e-3f);
    }
    printf("tone_check: ok\n");
    return 0;
}
