// pt_layout.h — how the kernels that copy scene records into LDS lay out a workgroup's LDS, and the one host function that
// decides it per launch (lds_layout).  The launchers (pt_kernels.hip) launch exactly the template instance and the number of
// bytes lds_layout returns; the kernels compute the same offsets in-kernel from the same functions below.  Every decision sits
// on a size cliff - a record more or a pixel more per stream selects another instance or moves an offset - so the header needs
// no HIP headers: the tests compile it with the host compiler and get the layouts from this code (tests/lds_layouts.py).
#pragma once

#include <cstdio>
#include <string>

#include "pt_device.h"

namespace pt {

// waves per SIMD (= workgroups per compute unit) k_pass_cand is compiled for, without walks (pt_kernels_flat.hip) and with: its
// __launch_bounds__, lds_layout's LDS budget per workgroup and plan_pass's rounds of resident workgroups follow them
#ifndef PT_CAND_WAVES
#define PT_CAND_WAVES 6
#endif
#ifndef PT_ISECT_WAVES
#define PT_ISECT_WAVES 4  // k_intersect_cand (the flat unit's too)
#endif
#ifndef PT_CAND_BVH_WAVES
#define PT_CAND_BVH_WAVES 4
#endif

constexpr uint32_t kDeferCap = 128;  // k_pass: deferred glass hits per wave (63 left over + 64 new at most)
// k_pass LDS: [u64 acc: 3*m][kPassTailWords x u32: counters, camera][u32 pixel index, column, row: 3*m][pad to 16][float4 deferred hits: waves x 3 x kDeferCap]
// the words between the accumulators and the pixel tables: [0..3] counters (k_pass_cand: [0..1] the ray count, [2..3] the frame's
// width and height), [4..15] the camera for k_pass_cand's primary rays.  (Twenty words until k_pass_cand went to six waves per
// SIMD: the sixteen bytes are what keeps cornell.json's records staged up to 64 pixels per stream - lds_layout's budget.)
constexpr uint32_t kPassTailWords = 16;
// u64 slots of the accumulator area: 3*m rounded up to even, so that the words behind it start on a 16-byte boundary whatever m
// is (k_pass_cand reads the camera from there as three float4: with an odd m - small frames have m = 1 - those were
// 8-byte-aligned ds_read_b128, which only the hardware's unaligned-DS mode forgives)
PT_HDC uint32_t pass_acc_slots(uint32_t m) { return (3u * m + 1u) & ~1u; }
PT_HDC size_t pass_lds_defer_offset(uint32_t m) {
    return ((size_t)pass_acc_slots(m) * sizeof(unsigned long long) + kPassTailWords * 4u + (size_t)3 * m * sizeof(uint32_t) + 15) & ~(size_t)15;
}
static_assert(pass_acc_slots(1) == 4u && pass_acc_slots(2) == 6u && (pass_acc_slots(7) * 8u) % 16u == 0u, "tails are 16-byte aligned");

// k_pass_cand LDS: [accumulators, tails, pixel indices as k_pass][per wave: float4 ray_a [128] | u64 key [128] |
// float2 ray_b [128] | u16 ring [kCandQueueCap]][without walks: the waiting rays' rows (below)][BVH: walk queues, keys, nodes
// (below)][staged candidate records][staged surf]
PT_HDC size_t pass_lds_cand_offset(uint32_t m, bool /*defer*/) { return pass_lds_defer_offset(m); }
constexpr size_t kCandWaveBytes = 128u * 16u + 128u * 8u + 128u * 8u + kCandQueueCap * 2u;  // 4480
PT_HDC size_t pass_lds_cand_bytes() { return (size_t)(kBlock / 64u) * kCandWaveBytes; }
static_assert(kCandWaveBytes % 16u == 0u, "per-wave areas stay 16-byte aligned");

// k_pass_cand WITHOUT walks only, behind the per-wave areas: THE WAITING RAYS' ROWS, one float4 (throughput xyz, bookkeeping word)
// per lane of the workgroup - what a ray started in one trip needs again when it is finished in the next, kept out of the
// registers in between.  One row per lane, no parity: a trip reads the row of the ray it finishes and only then writes the row
// of the ray it has started (k_pass_cand: "THE WAITING RAY'S ROW").  A term of its own, not part of kCandWaveBytes, which
// k_intersect_cand and k_mega_cand share; the instances with walks keep the four values in registers and have no such area.
PT_HDC size_t pass_lds_wait_bytes(bool bvh) { return bvh ? 0u : (size_t)kBlock * 16u; }
PT_HDC size_t pass_lds_wait_offset(uint32_t m) { return pass_lds_cand_offset(m, false) + pass_lds_cand_bytes(); }
static_assert((pass_lds_wait_offset(1) % 16u) == 0u && (pass_lds_wait_offset(7) % 16u) == 0u, "rows are read and written as b128");

// k_intersect_cand LDS: [per wave as k_pass_cand][staged candidate records (STAGED)]
PT_HDC size_t intersect_cand_lds_bytes() { return (size_t)(kBlock / 64u) * kCandWaveBytes; }

// k_pass_cand with walks (BVH = true), between the per-wave candidate areas and the staged records:
//   [per wave: walk queue (pass_cand_queue_bytes)][per wave: u64 key x 64][BVH nodes (NLDS: a small tree's nodes, staged)]
// per wave: the walk queue (header + 8-byte entries: box tests from one end, leaves from the other), which is also where
// the depth-first stacks (DevScene.bvh_stack entries x 64 lanes x u16, or u32 when a tree has 32 768 nodes or leaves) and
// the leaf list of the rare second walk live
// (448 entries.  With sample-major primary rays the walkers of a session are alike and their items crowd the queue together: at
// 320 entries one wave-walk in fifty dropped pushes - those rays walk again depth-first - at 448 mesh.json gains 1.4 %; 512: the same)
#ifndef PT_WALK_QUEUE_BYTES
#define PT_WALK_QUEUE_BYTES 3584
#endif
constexpr uint32_t kWalkQueueBytes = PT_WALK_QUEUE_BYTES;
constexpr uint32_t kWalkQueueBytesStaged = 2048;  // 256 entries: beside the workgroup's copy of the nodes (bvh_in_lds bit 2)
PT_HDI size_t pass_cand_queue_bytes(const DevScene &S) {
    const size_t again = (size_t)S.bvh_stack * 64u * ((S.bvh_in_lds & 2u) ? 2u : 4u) + kLeafListCap * 4u;
    const size_t q = (S.bvh_in_lds & 4u) ? kWalkQueueBytesStaged : kWalkQueueBytes;
    return kWalkQueueHeader + (((again > q ? again : q) + 15) & ~(size_t)15);
}
PT_HDI size_t pass_cand_queues_bytes(const DevScene &S) { return (size_t)(kBlock / 64u) * pass_cand_queue_bytes(S); }
constexpr size_t kCandWalkKeyBytes = 64u * 8u;                         // per wave: the walkers' keys
// [the waves' walk queues][the waves' walk keys][the workgroup's copy of the BVH nodes, when they fit (bvh_in_lds bit 2)]
PT_HDI size_t pass_cand_nodes_offset(const DevScene &S) {
    return pass_cand_queues_bytes(S) + (size_t)(kBlock / 64u) * kCandWalkKeyBytes;
}
PT_HDI size_t pass_cand_bvh_bytes(const DevScene &S) {
    return pass_cand_nodes_offset(S) + ((S.bvh_in_lds & 4u) ? (size_t)walk_node_count(S) * sizeof(WalkNode) : 0u);
}
static_assert(kCandWalkKeyBytes % 16u == 0u && sizeof(WalkNode) % 16u == 0u, "per-wave areas stay 16-byte aligned");

// k_mega_cand LDS: [per wave as k_pass_cand][candidate records, rounded up to 16 B][BVH: walk queues, keys][spare rays: depth x
// kBlock x float4][owner table][surf by rank, when it fits (surf_off != 0)]
PT_HDC size_t mega_spare_bytes(uint32_t depth) { return (size_t)depth * kBlock * 16u; }
constexpr size_t kMegaOwnerBytes = kBlock * sizeof(uint32_t);  // the rounds' owner tables
constexpr size_t kMegaLdsBudget = 40u * 1024u;  // k_mega_cand: four workgroups per CU

// The wavefront's pass kernel of a launch_pass call.
enum PassKernel : uint32_t {
    kPassPlain = 0,    // k_pass<false, ..>: PT_CAND_SCAN=0 and the like, streams too long for the deferral buffers
    kPassDefer = 1,    // k_pass<true, ..>: the same with the glass deferral buffers in LDS
    kPassCand = 2,     // k_pass_cand<STAGED, DEFER, false, ..> (pt_kernels_flat.hip)
    kPassCandBvh = 3,  // k_pass_cand<STAGED, false, true, .., NLDS>
};

// What each kernel that stages records asks for, for one scene (its DevScene as the launch sees it) and stream length m.
struct LdsLayout {
    // launch_pass
    uint32_t pass;          // PassKernel
    uint32_t m;             // pixels per stream
    bool staged;            // k_pass_cand: the candidate records are copied to LDS (STAGED)
    bool defer;             // k_pass_cand: glass deferral (DEFER); k_pass: the deferral buffers
    bool nodes_lds;         // k_pass_cand<BVH>: the BVH nodes are staged too (NLDS; DevScene.bvh_in_lds bit 2)
    uint32_t bvh_in_lds;    // DevScene.bvh_in_lds of the k_pass_cand launch
    uint32_t surf_staged;   // DevScene.surf_staged of the k_pass_cand launch: the whole surf table follows the records
    uint32_t surf_head;     // DevScene.surf_head: else this many leading ranks of it (k_pass_cand<BVH> only)
    size_t pass_lds;        // bytes of the layout
    size_t pass_pad;        // + these (PT_LDS_PAD, k_pass_cand only): what launch_pass asks for is pass_lds + pass_pad
    // launch_intersect_cand (the separate intersect step of scenes without BVH meshes)
    bool isect_staged;      // k_intersect_cand<true>
    size_t isect_lds;
    // launch_mega
    bool mega_cand;         // k_mega_cand (else the k_mega fallback)
    uint32_t mega_depth;    // k_mega_cand: spare primary rays per lane (4 or 2)
    uint32_t mega_spare_off;
    uint32_t mega_surf_off; // 0: surf is read from global memory
    size_t mega_lds;
};

// k_pass_cand's LDS budget per workgroup: what still lets a CU's 160 KiB hold as many workgroups as the kernel is built to run
// waves per SIMD.  Measured with PT_LDS_PAD (a frame loses a twentieth to a tenth when one workgroup fewer fits): with walks
// four workgroups of 40 928 B share a CU; without, at five waves, five of 32 144 B did and five of 32 400 B did not; at six,
// six of 26 880 B do (58.1 - 58.7 G bounces/s on cornell.json) and six of 26 944 B do not (55.5 - 55.8) - 21 units of 1 280 B, 426 B short
// of a sixth of the 160 KiB.  At any other PT_CAND_WAVES (an A/B build): the five-wave rule.
PT_HDC size_t pass_cand_lds_budget(bool bvh) {
    return bvh ? 160u * 1024u / PT_CAND_BVH_WAVES : (PT_CAND_WAVES == 6 ? 26880u : 160u * 1024u / PT_CAND_WAVES - 512u);
}

inline LdsLayout lds_layout(const DevScene &S, uint32_t m, size_t lds_pad) {
    LdsLayout L{};
    L.m = m;
    const bool bvh = S.n_bvh_nodes != 0u;
    const size_t rec_cand = (size_t)S.n_cand_pairs * sizeof(CandPairRec);
    const size_t rec_surf = (size_t)(S.n_objs + S.n_tris) * sizeof(SurfRec);
    L.bvh_in_lds = S.bvh_in_lds;
    if (S.cand_scan) {
        // candidate scan: ray slots, keys and ring per wave + the workgroup's copy of the candidate and shading records while
        // as many workgroups still fit a CU's 160 KiB as the kernel is built to run waves per SIMD (with walks four: 40 KiB each)
        const size_t budget = pass_cand_lds_budget(bvh);
        DevScene S2 = S;
        S2.bvh_in_lds &= ~1u;  // (nodes from global memory: PT_BVH_LDS asks for the staged k_intersect, not for this kernel)
        // glass deferral: not with walks (their queues take its place in LDS; a walked ray is shaded in place anyway)
        // (Without levels the deferral no longer pays: a chunk mixes rays of every depth and nearly every trip shades some glass
        // anyway - shading it in place, 46.5 against 46.05 G bounces/s on cornell, builds alternated; PT_GLASS_DEFER=1 brings
        // the buffers back for that comparison.)
        L.defer = !bvh && S.glass_defer_ok;  // (the scene has glass and the context holds parking areas: pt_api.hip)
        // walks: the nodes of a small tree are staged in LDS beside (smaller) walk queues when they fit with the candidate
        // records (mesh.json: 171 nodes, 10.9 KB: up to 24 pixels per stream).  Measured: no gain and no loss against the
        // gathers from L2 (26.74 / 26.72 G bounces/s) - a box-test batch waits for its turn at the SIMD, not for its node -
        // so streams are not shortened to make room for it
        if (bvh && S.nodes_in_lds_ok) {
            DevScene S3 = S2;
            S3.bvh_in_lds |= 4u;
            L.nodes_lds = pass_lds_cand_offset(m, false) + pass_lds_cand_bytes() + pass_cand_bvh_bytes(S3) + rec_cand <= budget;
            if (L.nodes_lds) S2 = S3;
        }
        const size_t walk = bvh ? pass_cand_bvh_bytes(S2) : 0u;
        const size_t before = pass_lds_cand_offset(m, L.defer) + pass_lds_cand_bytes() + pass_lds_wait_bytes(bvh) + walk;
        L.surf_staged = before + rec_cand + rec_surf <= budget ? 1u : 0u;
        // (without walks the records are staged whole or not at all; with walks the candidate records alone may be)
        L.staged = bvh ? (L.surf_staged || before + rec_cand <= budget + 8u * 1024u) : L.surf_staged != 0u;
        // (walks, table too large: as many leading ranks as still fit - the objects visited first, the room of mesh.json)
        if (bvh && L.staged && !L.surf_staged && before + rec_cand < budget) {
            const size_t fit = (budget - before - rec_cand) / sizeof(SurfRec);
            const size_t n_ranks = (size_t)S.n_objs + S.n_tris;
            L.surf_head = (uint32_t)(fit < n_ranks ? fit : n_ranks);
        }
        L.pass = bvh ? kPassCandBvh : kPassCand;
        L.bvh_in_lds = S2.bvh_in_lds;
        L.pass_lds = before + (L.staged ? rec_cand + (L.surf_staged ? rec_surf : (size_t)L.surf_head * sizeof(SurfRec)) : 0u);
        L.pass_pad = lds_pad;
    } else {
        // The deferral buffers are 24 KB per workgroup: worth it while 5-6 workgroups still fit a CU's 160 KB of LDS (the
        // accumulators of a stream take 28 B per pixel); frames so large that a stream owns hundreds of pixels (4096^2:
        // 1024) shade every material in place instead.
        const size_t lds_plain = pass_lds_defer_offset(m);
        const size_t lds_defer = lds_plain + (size_t)(kBlock / 64u) * 3u * kDeferCap * 16u;
        L.defer = lds_defer <= 32u * 1024u;
        L.pass = L.defer ? kPassDefer : kPassPlain;
        L.pass_lds = L.defer ? lds_defer : lds_plain;
    }
    // k_intersect_cand: the records staged while they fit the workgroups per CU it is built for
    L.isect_staged = intersect_cand_lds_bytes() + rec_cand <= 160u * 1024u / PT_ISECT_WAVES;
    L.isect_lds = intersect_cand_lds_bytes() + (L.isect_staged ? rec_cand : 0u);
    // the megakernel: the candidate scan, two paths per lane (k_mega_cand), while the records and two spare rays per lane fit
    const size_t rec = (rec_cand + 15) & ~(size_t)15;
    DevScene S4 = S;
    S4.bvh_in_lds &= ~5u;  // (the candidate forms read the nodes from global memory, with full-size walk queues)
    const size_t mwalk = bvh ? pass_cand_queues_bytes(S4) + (size_t)(kBlock / 64u) * kCandWalkKeyBytes : 0u;
    const size_t base = intersect_cand_lds_bytes() + rec + mwalk;
    L.mega_cand = S.cand_scan && base + mega_spare_bytes(2) + kMegaOwnerBytes <= kMegaLdsBudget;
    if (L.mega_cand) {
        L.mega_depth = base + mega_spare_bytes(4) + kMegaOwnerBytes <= kMegaLdsBudget ? 4u : 2u;
        L.mega_spare_off = (uint32_t)base;
        const size_t after = base + mega_spare_bytes(L.mega_depth) + kMegaOwnerBytes;
        L.mega_surf_off = after + rec_surf <= kMegaLdsBudget ? (uint32_t)after : 0u;
        L.mega_lds = after + (L.mega_surf_off ? rec_surf : 0u);
    } else {
        L.mega_lds = bvh_lds_bytes(S, kBlock);
    }
    return L;
}

// The kernels that stage records, as lds_layout decides them: one line each, as the library writes them to stderr when PT_LDS_PAD
// is set (pt_api.hip) and as the tests compare them.  which: 0 = launch_pass, 1 = launch_intersect_cand, 2 = launch_mega.
inline std::string lds_layout_line(const LdsLayout &L, int which) {
    char buf[256];
    if (which == 0 && L.pass == kPassCand)
        snprintf(buf, sizeof buf, "k_pass_cand: %zu bytes of LDS per workgroup (+ %zu of padding), m = %u, staged %d, defer %d",
                 L.pass_lds, L.pass_pad, L.m, (int)L.staged, (int)L.defer);
    else if (which == 0 && L.pass == kPassCandBvh)
        snprintf(buf, sizeof buf,
                 "k_pass_cand<BVH>: %zu bytes of LDS per workgroup (+ %zu of padding), m = %u, staged %d, nodes_lds %d, surf_staged %u, surf_head %u",
                 L.pass_lds, L.pass_pad, L.m, (int)L.staged, (int)L.nodes_lds, L.surf_staged, L.surf_head);
    else if (which == 0)
        snprintf(buf, sizeof buf, "k_pass: %zu bytes of LDS per workgroup (+ 0 of padding), m = %u, defer %d", L.pass_lds, L.m, (int)L.defer);
    else if (which == 1)
        snprintf(buf, sizeof buf, "k_intersect_cand: %zu bytes of LDS per workgroup (+ 0 of padding), staged %d", L.isect_lds,
                 (int)L.isect_staged);
    else if (L.mega_cand)
        snprintf(buf, sizeof buf, "k_mega_cand: %zu bytes of LDS per workgroup (+ 0 of padding), depth %u, spare_off %u, surf_off %u",
                 L.mega_lds, L.mega_depth, L.mega_spare_off, L.mega_surf_off);
    else
        snprintf(buf, sizeof buf, "k_mega: %zu bytes of LDS per workgroup (+ 0 of padding)", L.mega_lds);
    return buf;
}

}  // namespace pt
