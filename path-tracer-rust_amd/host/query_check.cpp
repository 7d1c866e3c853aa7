// query_check — the host side of the host-array queries under a sanitizer, as a program of its own (make query-check builds it
// with -fsanitize=address,undefined and runs it; no device, no Python).  It drives the refusals of host::check_radiance,
// check_primary_rays and check_bounds_query in each call's order over arrays allocated to their exact size, and holds
// host::pack_ray_streams to the ray queue's layout as csrc/pt_kernels.h states it (RayQueue), written out here a second time, at
// the stream boundaries; unpack_stream_hits must hand back every bit.  A failed check or a sanitizer report ends it with a
// non-zero status.
#include "check_common.h"
#include "../csrc/pt_host.h"

using namespace pt::host;

// The layout from the RayQueue comment, independently: K slices of cap * 40 bytes, each [od0: cap x float4 (origin, direction x)]
// [tp: cap x float4][od1: cap x float2 (direction yz)]; ray i is slot i % cap of slice i / cap; what no ray fills is zero.
static std::vector<char> expected_queue(const std::vector<float> &o, const std::vector<float> &d, uint32_t n, uint32_t cap) {
    const uint32_t K = n / cap + (n % cap ? 1u : 0u);
    std::vector<char> q((size_t)K * cap * 40u, 0);
    for (uint32_t b = 0; b < K; ++b) {
        float *od0 = (float *)(q.data() + (size_t)b * cap * 40u), *od1 = od0 + (size_t)cap * 8u;
        for (uint32_t j = 0; j < cap && b * cap + j < n; ++j) {
            const float *ro = &o[3u * (b * cap + j)], *rd = &d[3u * (b * cap + j)];
            od0[4u * j] = ro[0], od0[4u * j + 1u] = ro[1], od0[4u * j + 2u] = ro[2], od0[4u * j + 3u] = rd[0];
            od1[2u * j] = rd[1], od1[2u * j + 1u] = rd[2];
        }
    }
    return q;
}

static bool packs_right(uint32_t n, uint32_t cap) {
    std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n);  // exactly n rays: a read past them is a sanitizer report
    uint32_t s = n * 2654435761u + cap;
    for (float &v : o) v = unit(s) * 4.0f - 2.0f;
    for (float &v : d) v = unit(s) * 2.0f - 1.0f;
    std::vector<char> bytes(7, 'x');
    std::vector<uint32_t> counts(3, 99u);
    pack_ray_streams(o.data(), d.data(), n, cap, bytes, counts);
    const uint32_t K = (n + cap - 1u) / cap;
    if (counts.size() != K || bytes != expected_queue(o, d, n, cap)) return false;
    uint64_t total = 0;
    for (uint32_t b = 0; b < K; ++b) {
        if (counts[b] != (b + 1u < K ? cap : n - b * cap)) return false;
        total += counts[b];
        const char *tp = bytes.data() + (size_t)b * cap * 40u + (size_t)cap * 16u;  // no throughput is packed: zero, every slot
        for (size_t k = 0; k < (size_t)cap * 16u; ++k)
            if (tp[k]) return false;
    }
    return total == n;
}

int main() {
    const float o[3] = {0, 0, 0}, d[3] = {0, 0, -1};
    float rgb[3];
    const void *ctx = rgb;  // never dereferenced
    const uint32_t wave = PT_BACKEND_WAVEFRONT, pipes2 = 2u << 8;  // (PT_FLAG_PIPELINES(2))
    // ---- the refusals, in each call's order: each call breaks one rule and every rule after it
    CHECK(refused(check_radiance(nullptr, false, o, d, 12, 0, 2, pipes2, rgb), "NULL argument"));
    CHECK(refused(check_radiance(ctx, false, nullptr, d, 12, 0, 2, pipes2, rgb), "NULL argument"));
    CHECK(refused(check_radiance(ctx, false, o, nullptr, 12, 0, 2, pipes2, rgb), "NULL argument"));
    CHECK(refused(check_radiance(ctx, false, o, d, 12, 0, 2, pipes2, nullptr), "NULL argument"));
    CHECK(refused(check_radiance(ctx, false, o, d, 12, 0, 2, pipes2, rgb), "no scene set"));
    CHECK(refused(check_radiance(ctx, true, o, d, 0, 0, wave, 0, rgb), "n_samples outside"));
    CHECK(refused(check_radiance(ctx, true, o, d, 0, (1u << 24) + 1u, wave, 0, rgb), "n_samples outside"));
    CHECK(refused(check_radiance(ctx, true, o, d, 12, 1, wave, 0, rgb), "depth >= MAX_DEPTH"));
    CHECK(refused(check_radiance(ctx, true, o, d, 11, 1, 2, 0, rgb), "unknown backend"));
    CHECK(refused(check_radiance(ctx, true, o, d, 11, 1, wave, pipes2, rgb), "PT_FLAG_PIPELINES"));
    CHECK(check_radiance(ctx, true, o, d, 11, 1u << 24, PT_BACKEND_MEGAKERNEL, (1u << 8) | PT_FLAG_NO_BVH, rgb) == PT_OK);

    CHECK(refused(check_bounds_query(nullptr, false, 0, 3, 3, o, d), "NULL argument"));
    CHECK(refused(check_bounds_query(ctx, false, 0, 3, 3, nullptr, d), "NULL argument"));
    CHECK(refused(check_bounds_query(ctx, false, 0, 3, 3, o, nullptr), "NULL argument"));
    CHECK(refused(check_bounds_query(ctx, false, 0, 3, 3, o, d), "no scene set"));
    CHECK(refused(check_bounds_query(ctx, true, 0, 3, 3, o, d), "object index out of range"));
    CHECK(refused(check_bounds_query(ctx, true, 0, 0, 0, o, d), "object index out of range"));
    CHECK(check_bounds_query(ctx, true, 0, 2, 3, o, d) == PT_OK);
    CHECK(check_bounds_query(ctx, true, 1, 3, 3, o, d) == PT_OK);  // pt_ctx_orbit_point names no object
    {
        const uint32_t w = 6, h = 4;
        const std::vector<uint32_t> pix = {0, w * h - 1u, 5}, smp = {0, (1u << 24) - 1u, 7}, past = {0, 1, w * h}, late = {0, 1, 1u << 24};
        std::vector<float> ro(9), rd(9);
        pt_config cfg;
        uint32_t ib = 77, ie = 77;
        auto check = [&](const void *c, bool scene, uint32_t cw, const uint32_t *p, const uint32_t *s, uint32_t n, uint32_t form, float *po,
                         float *pd) { return check_primary_rays(c, scene, cw, h, 9, p, s, n, form, po, pd, cfg, &ib, &ie); };
        const char *first = "NULL argument, n == 0";
        CHECK(refused(check(nullptr, false, 0, past.data(), late.data(), 3, 0, ro.data(), rd.data()), first));
        CHECK(refused(check(ctx, false, 0, nullptr, late.data(), 3, 0, ro.data(), rd.data()), first));
        CHECK(refused(check(ctx, false, 0, past.data(), nullptr, 3, 0, ro.data(), rd.data()), first));
        CHECK(refused(check(ctx, false, 0, past.data(), late.data(), 3, 0, nullptr, rd.data()), first));
        CHECK(refused(check(ctx, false, 0, past.data(), late.data(), 3, 0, ro.data(), nullptr), first));
        CHECK(refused(check(ctx, false, 0, past.data(), late.data(), 0, 0, ro.data(), rd.data()), first));
        CHECK(refused(check(ctx, false, 0, past.data(), late.data(), 3, 2, ro.data(), rd.data()), first));
        CHECK(refused(check(ctx, false, 0, past.data(), late.data(), 3, 1, ro.data(), rd.data()), "no scene"));
        CHECK(refused(check(ctx, true, 0, past.data(), late.data(), 3, 1, ro.data(), rd.data()), "width, height and spp"));
        CHECK(refused(check(ctx, true, w, past.data(), smp.data(), 3, 1, ro.data(), rd.data()), "pixel index outside the frame"));
        CHECK(refused(check(ctx, true, w, pix.data(), late.data(), 3, 0, ro.data(), rd.data()), "sample >= 2^24"));
        CHECK(check(ctx, true, w, pix.data(), smp.data(), 3, 1, ro.data(), rd.data()) == PT_OK);
        CHECK(cfg.width == w && cfg.height == h && cfg.spp == 1u && cfg.seed == 9u && cfg.flags == 0u && ib == 0u && ie == w * h);
    }
    // ---- the packing at the stream boundaries
    for (uint32_t n : {1u, 4095u, 4096u, 4097u}) CHECK(packs_right(n, 4096u));
    CHECK(packs_right(9u, 4u));
    {
        // a result's second word is an id's bits: any pattern, a NaN's payload included, comes back as it is
        const uint32_t words[6] = {0x3f800000u, 0x7fc12345u, 0x7f800000u, 0xffffffffu, 0x00000001u, 0xffc00001u};
        float t[3];
        int32_t id[3];
        unpack_stream_hits(words, 3, t, id);
        for (uint32_t i = 0; i < 3; ++i) CHECK(!memcmp(&t[i], &words[2u * i], 4) && !memcmp(&id[i], &words[2u * i + 1u], 4));
    }
    printf("query_check: ok\n");
    return 0;
}
