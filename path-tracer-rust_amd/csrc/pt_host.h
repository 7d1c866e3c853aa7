// pt_host.h — host-side setup arithmetic of the path (camera basis, Mesh::new bounds, scene flattening).
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ptrace.h"
#include "pt_device.h"
#include "pt_refit.h"

namespace pt {

void set_error(const std::string &m);
// a refusal of the caller's arguments: the message is set, the code is the one to return
inline int refuse(const char *why) {
    set_error(why);
    return PT_ERR_INVALID;
}

namespace host {

struct FlatScene {
    std::vector<ObjRec> objs;
    std::vector<ObjPairRec> obj_pairs;
    std::vector<TriPairRec> tri_pairs;
    std::vector<MatRec> mats;
    std::vector<TriShade> tri_shade;
    std::vector<BvhNode> bvh_nodes;
    std::vector<BvhNode4> bvh_nodes4;  // the same trees four children wide (two levels folded into one)
    std::vector<SphPairRec> sph_pairs;
    std::vector<FlatPairRec> flat_pairs;
    std::vector<CandPairRec> cand_pairs;  // [0, n_other_pairs): records without a filter
    std::vector<uint32_t> rank_id;
    std::vector<SurfRec> surf;  // by rank
    std::vector<uint32_t> tri_rank;  // rank of triangle k (the inverse of rank_id over the triangles)
    std::vector<BvhMeshRec> bvh_meshes;  // the meshes that have a BVH, in visiting order (last object first)
    std::vector<uint32_t> wide_src;  // host only: per child slot of bvh_nodes4, the binary 2 * node + half its box was copied from
                                     // (kRefitNone: an absent child) - what a refit's gather reads (build_refit_plan)
    uint32_t n_other_pairs = 0;
    uint32_t n_flat_exact = 0;  // flat_pairs [0, n_flat_exact) have sign_exact set (they come first)
    uint32_t n_flat_exact_axis[3] = {0, 0, 0};  // ... of which so many lie on the x, y, z axis, in that order in the table (the
                                                // kernels run one loop per axis over them)
    bool cand_ok = false;  // the scene can use the candidate scan (the records of its meshes without a BVH are numbered in
                           // 9 bits; meshes with a BVH are walked: k_pass_cand<.., BVH>)
    uint32_t bvh_stack = 0;      // traversal-stack entries the deepest tree needs (<= kBvhStack)
    uint32_t bvh_pair_base = 0;  // first TriPairRec that is a BVH leaf
    uint32_t bvh_pair_span = 0;  // leaves lie in [bvh_pair_base, bvh_pair_base + bvh_pair_span)
};

// THE SCENE'S DEVICE TABLES, written down once: X(PT_TABLE_* suffix, record type, name).  The name is the FlatScene member's, the
// DevScene pointer's and the device table's in pt_ctx (pt_api.hip: SceneTables).  What uploads, binds, hashes or compares every
// table expands this list: pt_api.hip, host/object_check.cpp.
#define PT_SCENE_TABLES(X)                 \
    X(OBJS, ObjRec, objs)                  \
    X(OBJ_PAIRS, ObjPairRec, obj_pairs)    \
    X(TRI_PAIRS, TriPairRec, tri_pairs)    \
    X(MATS, MatRec, mats)                  \
    X(TRI_SHADE, TriShade, tri_shade)      \
    X(BVH_NODES, BvhNode, bvh_nodes)       \
    X(BVH_NODES4, BvhNode4, bvh_nodes4)    \
    X(SPH_PAIRS, SphPairRec, sph_pairs)    \
    X(FLAT_PAIRS, FlatPairRec, flat_pairs) \
    X(CAND_PAIRS, CandPairRec, cand_pairs) \
    X(RANK_ID, uint32_t, rank_id)          \
    X(SURF, SurfRec, surf)                 \
    X(TRI_RANK, uint32_t, tri_rank)        \
    X(BVH_MESHES, BvhMeshRec, bvh_meshes)
#define PT_X(ID, T, name) PT_TABLE_##ID,
constexpr int kSceneTableIds[] = {PT_SCENE_TABLES(PT_X)};
#undef PT_X
constexpr bool scene_tables_in_enum_order() {
    for (int i = 0; i < PT_TABLE_COUNT; ++i)
        if (kSceneTableIds[i] != i) return false;
    return true;
}
static_assert(sizeof kSceneTableIds / sizeof kSceneTableIds[0] == PT_TABLE_COUNT && scene_tables_in_enum_order(),
              "PT_SCENE_TABLES lists the tables of ptrace.h's PT_TABLE_* enum, every one, in its order");

// CameraData::{lens_center, orthogonals} — src/render/mod.rs:211-232
void camera_basis(const pt_camera &cam, float lens_center[3], float su[3], float sv[3]);
// Mesh::new bounding sphere — src/render/mod.rs:450-499
void mesh_bounding_sphere(const pt_triangle *tris, uint32_t n, float center[3], float *radius);
// Mesh::new's bounding_box: bounding_box_to_triangles over the AABB of the (object-local) triangles — src/render/mod.rs:452-476,501-536
void mesh_bounding_box(const pt_triangle *tris, uint32_t n, pt_triangle out[12]);
// the 12 triangles of one object's bounding box as 6 pair records in list order (world space: Triangle::transformed,
// mod.rs:546-552, then the edge subtractions of mod.rs:560-561), ids 0..11 — what SceneObjectData::intersect_bounds scans
void box_pair_records(const pt_triangle box[12], const float position[3], TriPairRec out[6]);
// validate + flatten (see pt_device.h for the record layouts); false + message on malformed input
// `cam` only widens the distance bound that sizes the BVH box padding (ray origins include the lens centre)
bool bvh_refs_fit(uint64_t n_nodes, uint64_t n_pair_records);

// How a wavefront frame is cut into passes and streams (one attempt of plan_frame, below): pure arithmetic, tested on the CPU.
struct PassPlanIn {
    uint64_t npix = 0;          // pixels of the call (or of its part)
    uint32_t spp = 0;           // samples per pixel of the frame
    uint64_t want = 0;          // primary rays per pass that are asked for
    bool want_is_default = true;  // `want` is the library's choice (it may be halved to fit index ranges)
    bool stack_form = false;    // k_pass_cand: a stack of waiting rays per wave, passes sized by time
    bool stack_park = false;    // ... with walks: a parking area per wave in the second container
    bool cand_scan = false, has_bvh = false;
    uint64_t streams = 0;       // PT_STREAMS (0: derived)
    uint32_t per_stream = 0;    // PT_PER_STREAM (0: default)
    uint32_t wave_stack = 0;    // PT_WAVE_STACK (0: kWaveStackMax)
    uint32_t n_cus = 0;         // compute units of the device (0: unknown - no whole-rounds nudge)
    uint32_t groups_per_cu = 4; // workgroups of the pass kernel a compute unit holds at a time (its waves per SIMD)
    size_t stack_budget = 0;    // stack_form, default pass: bytes the streams' stacks may take (0: unbounded)
};
struct PassPlan {
    uint32_t spp_pass = 0;  // samples of a pixel per pass
    uint32_t m = 0;         // pixels per stream
    uint32_t K = 0;         // streams (workgroups per launch)
    uint32_t cap = 0;       // slots of a stream's slice of a queue container (k_pass_cand: 4 x the waves' stack)
    size_t bytes0 = 0, bytes1 = 0;  // the two containers
};
enum { kPlanOk = 0, kPlanRetry = 1, kPlanTooLarge = 2 };
// kPlanRetry: the plan does not fit (the stacks' budget, or 32-bit slot indices) - try again with in.want = *want_next
int plan_pass(const PassPlanIn &in, PassPlan &out, uint64_t *want_next);
// THE TAPER of a k_pass_cand launch: its last n_cut streams run as `pieces` workgroups each - (stream, a contiguous share of the
// pass's samples) instead of (stream, whole pass) - dispatched behind the whole-pass workgroups of the streams before them, so
// that what a launch ends on are short workgroups while the bulk of it runs long streams (a workgroup's fill and drain are paid
// once whatever it traces).  Workgroup n_whole + j is piece j % pieces of stream n_whole + j / pieces; the pieces of a stream may
// run at the same time, so every WORKGROUP has stack (and parking) slices of its own: extra0 / extra1 bytes behind
// plan.bytes0 / bytes1.  plan_pass is not asked again: the taper never changes a plan, it is dropped where it does not fit.
struct TaperIn {
    uint32_t n_cut = 0;         // streams to cut (PT_TAPER_CUT or the default; more than K: all of them)
    uint32_t pieces = 0;        // pieces per cut stream (PT_TAPER_PIECES or the default; rounded down to a power of two, <= 64)
    uint32_t pass_samples = 0;  // samples of a pixel in the shortest pass the plan will be launched with
    uint64_t resident = 0;      // workgroups the chip holds at a time (0: unknown - no rule about rounds)
    size_t budget = 0;          // bytes the containers may take, extra slices included (0: unbounded)
    bool stack_park = false;    // the second container holds the waves' parking areas (PassPlanIn.stack_park)
    bool probe = false;         // a PROBE instance (pt_ctx_scatter's frames): never tapered
    bool forced = false;        // the knobs were set by hand: neither the rule about rounds nor the one about samples applies
                                // (tests: tiny frames, pieces without a sample - such a workgroup returns at once)
};
struct Taper {
    uint32_t n_cut = 0, pieces = 1, lg_pieces = 0;  // off: 0, 1, 0
    size_t extra0 = 0, extra1 = 0;
    bool on() const { return n_cut != 0u; }
    uint32_t grid(uint32_t K) const { return K - n_cut + n_cut * pieces; }
};
constexpr uint32_t kTaperMinRounds = 4;  // launches of fewer rounds of resident workgroups are the small-frame rule's (plan_pass)
// Off (n_cut = 0) when: in.n_cut or in.pieces < 2 is 0; in.probe; the launch has fewer than kTaperMinRounds rounds of resident
// workgroups, or the pass has fewer samples than pieces (neither when in.forced); plan.bytes0 + bytes1 + the extra slices exceed
// in.budget; or the slices no longer fit 32-bit slot indices.
Taper plan_taper(const PassPlan &plan, const TaperIn &in);
// the samples [*s0, *s0 + *n) of piece `piece` of a pass of s_here samples (what k_pass_cand derives in its prologue)
inline void taper_piece(uint32_t s_here, uint32_t lg_pieces, uint32_t piece, uint32_t *s0, uint32_t *n) {
    const uint32_t share = s_here >> lg_pieces, longer = s_here & ((1u << lg_pieces) - 1u);
    *s0 = piece * share + (piece < longer ? piece : longer);
    *n = share + (piece < longer ? 1u : 0u);
}
// The taper's defaults (measured: DESIGN.md section 4, profiles/r04_taper_sweep.txt): streams cut in HALF rounds of resident
// workgroups (0: no taper), pieces per cut stream, and the primaries per stream and pass asked for with it (0: plan_pass's) -
// without walks and with.  cornell 1024x768 @4096, one session, 448.0 ms without: one round in 4 pieces 438.1 ms at 24 Ki primaries
// per stream, 439.0 at 32 Ki, 439.8 at 20 Ki; half a round in 8 pieces 436.8 - but in another session (449.9 without) half a round
// 440.4 and a third of a round 446.9: too close to where the cut stops paying, so a whole round it is.  mesh.json @1024, 194.6 ms
// without: half a round in 4 pieces at its own stream length 191.6, a whole round 192.4, 8 pieces 194.6; longer streams (32 Ki) gain
// nothing there (192.0) and lose 3 % with a cut of half a round.
constexpr uint32_t kTaperCutHalfRounds = 2, kTaperPieces = 4, kTaperPerStream = 24576;
constexpr uint32_t kTaperCutHalfRoundsBvh = 1, kTaperPiecesBvh = 4, kTaperPerStreamBvh = 0;

// THE PLAN OF A WAVEFRONT FRAME: what render_wavefront (pt_api.hip) decides before it allocates, nothing of HIP.  first_request,
// then plan_frame; when the allocation fails shrink_request and plan_frame again.  tests/golden/frame_plans_parent.json records
// what they give (tests/test_frame_plan.py).
struct FramePlanIn {
    // the caller's: npix, spp (the samples still to trace), the form, cand_scan, has_bvh, streams, per_stream, wave_stack, n_cus;
    // the planner's: want, want_is_default, groups_per_cu, stack_budget
    PassPlanIn pass;
    uint64_t rays_per_pass = 0, rays_per_pass_tuned = 0;  // pt_config's (0: the library chooses); PT_RAYS_PER_PASS, its default
    size_t mem_budget = 0;      // pt_ctx_set_memory_budget (0: none)
    size_t mem_avail = 0;       // bytes free on the device + what the context's queues hold already (0: unknown)
    uint32_t mem_share = 1;     // contexts that share the device in this call
    bool probe = false;         // a PROBE instance
    int64_t taper_cut = -1;     // PT_TAPER_CUT (< 0: the default)
    uint32_t taper_pieces = 0;  // PT_TAPER_PIECES (0: the default)
    DevScene scene{};           // the frame's scene record, for lds_layout (which reads its counts and flags, no table)
    size_t lds_pad = 0;         // PT_LDS_PAD
};
struct FrameRequest {  // what one attempt asks for: the ladder's state
    uint64_t want = 0;        // primary rays per pass
    size_t stack_budget = 0;  // k_pass_cand: bytes the streams' stacks and the taper's slices may take (0: unbounded)
    bool try_taper = false;
};
struct FramePlan {
    PassPlan pass;
    Taper taper;
    int retries = 0;  // kPlanRetry answers of plan_pass that were followed
};
// workgroups of the pass kernel a compute unit holds at a time: k_pass_cand's waves per SIMD (pt_layout.h), else four
uint32_t pass_groups_per_cu(bool stack_form, bool has_bvh);
// The first request: the default pass, cut to what the device can give (85 % of mem_avail / mem_share, or mem_budget) and to a
// mem_share-th of itself; an explicit size as given, but an explicit budget beats it; one sample per pixel at least.
FrameRequest first_request(const FramePlanIn &in);
// One attempt: plan_pass with its retries followed and, where req.try_taper, plan_taper - with the default taper on longer
// streams (kTaperPerStream*) if the pass's samples and the records' staging (lds_layout) stay as they are.  kPlanOk or kPlanTooLarge.
int plan_frame(const FramePlanIn &in, const FrameRequest &req, FramePlan &out);
// After the allocation of `plan` failed: the same without its taper, else passes of half the samples; false: nothing smaller
bool shrink_request(const FramePlanIn &in, const FramePlan &plan, FrameRequest &req);

// Samples of a pixel in the next pass (wavefront) / round (megakernel) of a frame whose passes follow the scene (pt_api.hip:
// render_wavefront, render_mega).  `rate`: primary samples per millisecond the last timed pass went through (0: nothing
// measured yet - the pass is `probe` samples in all); `s_prev`: samples per pixel of the pass before (0: none); `left`: samples
// per pixel still to be issued (> 0); `max_pass`: what one pass may hold.  As many samples as `rate` fits into `target_ms`, at
// most sixteen times the pass before, the rest of the frame in equal passes - each up to a fifth longer than the target
// rather than one pass more.
uint32_t next_pass_samples(double rate, double target_ms, uint64_t npix, uint64_t probe, uint32_t s_prev, uint32_t left,
                           uint32_t max_pass);
// How the megakernel and the tile pass cut the samples of `entries` items (a part's pixels; the compact accumulator's entries) into
// ROUNDS (run_rounds, pt_api.hip).  A round is every item x round_spp consecutive samples in one launch: rays_per_pass primary
// samples (0: 256 Mi), at least one per item, at most spp_left.  Few items get n_split lanes each - doubled until there are
// item_mult items per lane of the 2048 a compute unit holds, at most round_spp - so that a launch still fills the chip.
struct RoundPlan {
    uint32_t round_spp, n_split;
};
RoundPlan plan_rounds(uint64_t entries, uint32_t spp_left, uint64_t rays_per_pass, uint32_t item_mult, uint32_t n_cus);
// A launch of s_here (> 0) samples: `split` lanes of lane_spp samples per item, on at most 8 workgroups per compute unit
struct RoundLaunch {
    uint32_t split, lane_spp, grid;
};
RoundLaunch round_launch(uint64_t entries, uint32_t n_split, uint32_t s_here, uint32_t n_cus);
// The box that bounds every ray origin of a scene: the lens centre and the objects (spheres by their extent, meshes by their
// translated vertices).  scene_R, the box paddings, admit, rr_in and the filters' pads are conservative bounds derived from it
// and from nothing else of the camera: they hold for every camera whose lens centre lies inside (pt_ctx_set_camera).
struct Reach {
    float lo[3], hi[3];
    bool holds(const float p[3]) const {  // false for a NaN
        return lo[0] <= p[0] && p[0] <= hi[0] && lo[1] <= p[1] && p[1] <= hi[1] && lo[2] <= p[2] && p[2] <= hi[2];
    }
    bool holds(const Reach &b) const { return holds(b.lo) && holds(b.hi); }
};
// the box flatten_scene derives a scene's bounds for when it is given none
void scene_reach(const pt_camera &cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris, Reach &out);
// pt_ctx_set_camera's growth rule, in binary32: a bound the lens centre violates moves beyond it by the overshoot once more
// (lo = lens - (lo - lens), hi = lens + (lens - hi)), the others stay.  True when B changed (the lens centre was outside).
bool grow_reach(Reach &B, const float lens[3]);
// The material at the door (pt_ctx_set_scene, pt_render, pt_ctx_set_object): "color" or "emission" when a component of it is
// negative or not finite (a NaN among them; -0.0f passes), nullptr when both are fine.  The kernels' to_fixed (pt_device.h) is
// only defined for finite v >= 0, and throughput and contributions are products of these components.
const char *bad_material(const pt_object &o);
// `origin_box` (optional): the bounds are derived for scene_reach's box united with it - what the call computes without one
// when the box lies inside scene_reach's
bool flatten_scene(const pt_camera &cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris,
                   uint32_t n_tris, FlatScene &out, std::string &err, const Reach *origin_box = nullptr, Reach *used = nullptr);

// ---- pt_ctx_set_object (ptrace.h): the host side of an edit in place.  Pure, tested on the CPU (host/object_check.cpp).
// the call's refusals in the header's order: PT_ERR_INVALID + message.  objs, n_objs: the context's copy (read only past `no scene`)
int check_object_edit(bool has_ctx, const pt_object *obj, bool has_scene, const pt_object *objs, uint32_t n_objs, uint32_t index);
// do two objects agree, bit for bit, in position, radius, bs_center and bs_radius (a MATERIAL edit when they do)
bool same_geometry(const pt_object &a, const pt_object &b);
// min / max in binary32 over the object-local vertices of a mesh (+inf / -inf for none): cached per object at pt_ctx_set_scene
void local_vertex_box(const pt_triangle *tris, uint32_t n, Reach &out);
// An object's bounds as scene_reach takes them: a sphere's centre -/+ |radius|; a mesh's local vertex box + position, which is
// what min / max over its translated vertices gives, since x -> x + p is monotone in binary32
void object_bounds(const pt_object &o, const Reach &local, Reach &out);
// grow_reach's rule applied to the bounds of B that an object's box violates; true when B changed
bool grow_reach_box(Reach &B, const Reach &box);
// the visiting rank of object `index` (a sphere's own; a mesh's first triangle's)
uint32_t object_rank(const pt_object *objs, uint32_t n_objs, uint32_t index);
// What an in-reach edit of object `index` changed in fs besides objs[index] and mats[index], for the uploader
struct ObjectEdit {
    bool on_device = false;  // a mesh with a BVH: its pair records, shading records, surface records and boxes are the refit's
    uint32_t rank = 0;       // the object's first rank
    uint32_t obj_pair = 0;   // its record of obj_pairs
    uint32_t bvh_mesh = kRefitNone;  // its record of bvh_meshes
    float scene_R = 0.0f;    // the diagonal of B, as flatten_scene takes it (the refit's pads)
    std::vector<SurfRec> surf;  // the surface records at [rank, rank + size) (none for a mesh with a BVH)
    uint32_t tail_at = 0;       // object 0 only: the unused slots of surf past the last rank, [tail_at, tail_at + size), which
    std::vector<SurfRec> tail;  // flatten_scene fills from object 0 (so that an edited table equals a built one to the bit)
};
// fs - flatten_scene's tables under the origin box B for these objects but for objs[index], which the caller changed (kind and
// triangle range as before; its bounds inside B) - brought to what the scene now is, without building a tree: objs[index] and
// mats[index]; `moved`: also a listed mesh's pair and shading records, and obj_pairs, sph_pairs, flat_pairs, cand_pairs and their
// counts whole, by the code flatten_scene runs (derive_small).  NOT touched: tri_pairs, tri_shade, bvh_nodes, bvh_nodes4 of a
// mesh with a BVH (their floats go stale in fs: the refit rewrites the device's; fs keeps the topology), rank_id, surf, tri_rank.
void edit_object(FlatScene &fs, const Reach &B, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t index,
                 bool moved, ObjectEdit &e);
// The refit plan of mesh `index` (pt_refit.h), from the tree in fs: the leaves; the inner nodes but the root, grouped by height
// above the leaves, ascending (level_begin[h] .. level_begin[h + 1]: height h + 1); the child slots of its four-wide nodes.
// false: the object has no BVH.
struct RefitPlan {
    std::vector<RefitLeaf> leaves;
    std::vector<RefitNode> nodes;
    std::vector<uint32_t> level_begin;
    std::vector<RefitWide> wide;
};
bool build_refit_plan(const FlatScene &fs, uint32_t index, RefitPlan &p);
// the plan's steps in order on host tables, through the functions the kernels call (host/object_check.cpp)
void run_refit_plan(const RefitPlan &p, const RefitTables &T);

// ---- the arithmetic of a frame call and of the frame pt_ctx_accumulate holds (pt_api.hip): pure, tested on the CPU -----------
// a valid cfg's band in [*idx_begin, *idx_end); PT_ERR_INVALID + message otherwise
int check_cfg(const pt_config *cfg, uint32_t *idx_begin, uint32_t *idx_end);
// pixels of the band [b, e) that fall into chunks first, first+step, ... (all of them when step <= 1)
uint32_t owned_pixels(const pt_config *cfg, uint32_t b, uint32_t e);
// A call of more than 1.5 Mi pixels is rendered in parts of 2^20 pixels (pt_ctx_render says why); pixels per part
uint32_t part_pixels(uint32_t total, bool wavefront);
// part i of `total` pixels cut into parts of part_px: pixels [k0, k0 + n)
struct Part {
    uint32_t k0, n;
};
inline uint32_t part_count(uint32_t total, uint32_t part_px) { return (total + part_px - 1u) / part_px; }
inline Part part_extent(uint32_t total, uint32_t part_px, uint32_t i) {
    const uint32_t k0 = i * part_px;
    return {k0, (total - k0) < part_px ? (total - k0) : part_px};
}

// The frame a pt_ctx_accumulate call renders: what decides the image besides the samples (the scene is the context's).
// chunk_* as check_cfg reads them: all zero for a whole band.
struct AccumKey {
    uint32_t width, height, idx_begin, idx_end, chunk_pixels, chunk_first, chunk_step;
    uint64_t seed;
    bool operator==(const AccumKey &o) const {
        return width == o.width && height == o.height && idx_begin == o.idx_begin && idx_end == o.idx_end &&
               chunk_pixels == o.chunk_pixels && chunk_first == o.chunk_first && chunk_step == o.chunk_step && seed == o.seed;
    }
};
// pt_ctx_accumulate's frame key of a checked config (b, e: check_cfg's band)
AccumKey accum_key(const pt_config *cfg, uint32_t b, uint32_t e);

// The host's side of the frame pt_ctx_accumulate holds between calls (pt_api.hip: HeldFrame adds the device planes) and of a
// checkpoint of it: `total` pixels of the frame `key` in the call's pixel order, and the samples per pixel each part holds (parts
// of part_px pixels, cut as pt_ctx_render cuts a call).  na: how many of them went to half A of a noise-tracked frame
// (pt_ctx_accum_track_noise; half B: cnt - na).  Whether a frame is held, and whether it is tracked, IS whether cnt / na have
// entries - there are no flags that could disagree with them.
struct FrameCounts {
    AccumKey key{};
    uint32_t total = 0, part_px = 0;
    std::vector<uint32_t> cnt, na;
    bool held() const { return !cnt.empty(); }
    bool tracked() const { return !na.empty(); }
    bool holds(const AccumKey &k) const { return held() && key == k; }
    uint32_t n_parts() const { return (uint32_t)cnt.size(); }
    Part part(uint32_t i) const { return part_extent(total, part_px, i); }
    uint32_t cnt_min() const { return held() ? *std::min_element(cnt.begin(), cnt.end()) : 0u; }
    uint32_t cnt_max() const { return held() ? *std::max_element(cnt.begin(), cnt.end()) : 0u; }
};

// One piece of a frame call: pixels [k0, k0 + n) of the call, samples [s_first, s_end) of each (s_end 0: cfg->spp).  Progress
// inside it is reported as base + scale * f of the call, and its start is a progress point at `base`.  [part_lo, part_hi): the
// parts of pt_ctx_accumulate's counts it brings to its last sample.  `boundary`: the fraction reported at its start when that is
// not `base` (the second job of a part).
struct Job {
    uint32_t k0, n, s_first;
    float base, scale;
    uint32_t part_lo, part_hi;
    uint32_t s_end = 0;
    float boundary = -1.0f;
};
// What a pt_ctx_accumulate to `spp` samples renders on the held frame f: each part from its own count; the megakernel, which renders a call at once, takes the whole
// call in one go when every part holds the same counts.  Progress by pixels.  A noise-tracked frame cuts the samples [cnt, spp)
// of a part into two jobs at m = cnt + 4 * ceil((spp - cnt) / 8) - the first rounded up to whole groups of the four sub-pixels -
// so that both halves of the estimate get samples from every call (deal_to_a deals them).
std::vector<Job> accum_jobs(const FrameCounts &f, uint32_t spp, bool megakernel);
// A noise-tracked frame deals the samples of a job to the half that holds fewer of them in its part (a tie: to A); cnt, na: the
// part's counts before the job
inline bool deal_to_a(uint32_t cnt, uint32_t na) { return na <= cnt - na; }

// ---- checkpoint file (pt_ctx_accum_save / _load, ptrace.h): little-endian, the byte order of every target of this library.
// What a file says besides its planes: the frame (tracked: version 2, which brings half A; plain: version 1), the fingerprint
// of its scene, and where its planes of 24 * total bytes lie - the held sums at sums_at, half A's at a_at.  SealedFile: what
// this format and the held adaptive frame's (below) say alike.
struct SealedFile {
    uint64_t scene_fp = 0;
    size_t sums_at = 0, a_at = 0;
    size_t need = 0;  // kCkptMore: the leading bytes of the file the decoder asks for
};
struct Checkpoint : FrameCounts, SealedFile {};
// the file up to its planes (header, counts, half A's counts) appended to b; the planes follow (the held sums, then half A's),
// then ckpt_seal's hash of everything before it
void ckpt_encode_head(const Checkpoint &ck, std::vector<uint8_t> &b);
void ckpt_seal(std::vector<uint8_t> &b);
enum { kCkptOk = 0, kCkptBad = 1, kCkptMore = 2 };
// A file of file_size bytes whose first n are at b.  kCkptMore: nothing wrong so far, call again with the first out.need bytes
// (the header first; the whole file only once its size is the one the header implies); kCkptBad: `why` says what is wrong.
int ckpt_decode(uint64_t file_size, const uint8_t *b, size_t n, Checkpoint &out, std::string &why);

// ---- the noise estimate's host arithmetic (pt_ctx_accum_noise, pt_ctx_accumulate_until)
// a part's weight sqrt(nA * nB) / (nA + nB), in binary32 as the header states it
float noise_part_weight(uint32_t na, uint32_t nb);
// the upper edge of histogram bin `b` of pt_noise_stats (ptrace.h): the float whose bits are (461 + b) << 21; +inf for the last
float noise_bin_upper(uint32_t b);
// the first bin at which the cumulative count reaches ceil(quantile * pixels) (the bin count when none does)
uint32_t noise_quantile_bin(const pt_noise_stats &s, float quantile);
// is an estimate within the target: its criteria in use (non-zero mean_error, non-zero quantile), all of them
bool noise_target_met(const pt_noise_stats &s, const pt_noise_target &t);
// what the entry points ask of a tolerance or a sigma (false for a NaN)
inline bool finite_nonneg(float v) { return v >= 0.0f && v < __builtin_inff(); }
// pt_ctx_accumulate_until's refusals about its target, in the header's order: PT_ERR_INVALID + message
int check_noise_target(const pt_noise_target &t);

// ---- the sample schedules of the calls that render to a noise target (ptrace.h states them)
// samples [c, T) of a tracked part or an open tile: half A's up to m = min(T, c + 4 * ceil((T - c) / 8)), half B's from there
inline uint32_t tracked_split(uint32_t c, uint32_t T) {
    const uint64_t m = (uint64_t)c + 4ull * (((uint64_t)(T - c) + 7ull) / 8ull);
    return m < T ? (uint32_t)m : T;
}
// the count after t: twice as many, never beyond the cap
inline uint32_t next_target(uint32_t t, uint32_t cap) { return t > cap / 2u ? cap : t * 2u; }
// The first count, min_spp 0 = 16.  pt_ctx_accumulate_until: that or what is held, whichever is more.  pt_ctx_render_adaptive:
// rounded up to a multiple of 8, so that the first level fills both halves evenly.
inline uint32_t until_first_target(uint32_t held, uint32_t min_spp, uint32_t cap) {
    return std::min(cap, std::max(held, min_spp ? min_spp : 16u));
}
inline uint32_t adaptive_first_level(uint32_t min_spp, uint32_t cap) {
    const uint32_t n = min_spp ? min_spp : 16u;
    return n > 0xfffffff8u ? cap : std::min(cap, (n + 7u) / 8u * 8u);
}

// ---- pt_ctx_render_adaptive: its refusals in the header's order (PT_ERR_INVALID + message), its tiles, its totals
// tile_error, then the tile edge (0 = 8), whose log2 goes to *tile_shift
int check_adaptive_params(const pt_adaptive_params &p, uint32_t *tile_shift);
// the band of whole image rows, then chunk_step and PT_FLAG_PIPELINES
int check_adaptive_cfg(const pt_config &cfg);
// TileGrid's geometry (pt_tile.h) for a band of `rows` rows; refused: tiles that hold 2^32 entries or more (32-bit indices)
struct TileGeometry {
    uint32_t tile_shift, tiles_x, tiles;
};
int tile_geometry(uint32_t width, uint32_t rows, uint32_t tile_shift, TileGeometry &out);
// From the tiles' counts, their last E (kTileNoError: none) and the device's sum of the E: the samples traced, the pixels that
// have an estimate - a partial tile counts the pixels it has inside the band - and the mean error, +inf unless every pixel has one
struct TileTotals {
    uint64_t samples, est_pixels;
    double mean_error;
};
TileTotals tile_totals(uint32_t width, uint32_t rows, const TileGeometry &g, const uint32_t *tile_spp, const unsigned long long *tile_err,
                       unsigned long long err_sum);

// ---- the adaptive frame a context holds between calls (pt_ctx_accumulate_adaptive, ptrace.h): pure, tested on the CPU
// n_0 of the key: min_spp (0 = 16) rounded up to a multiple of 8, BEFORE any cap (never above 0xfffffff8: every count is below)
inline uint32_t adaptive_n0(uint32_t min_spp) {
    const uint64_t n = min_spp ? min_spp : 16u;
    return (uint32_t)std::min<uint64_t>((n + 7u) / 8u * 8u, 0xfffffff8ull);
}
// the count after c on the ladder n_0, 2 n_0, 4 n_0, ..: min(cap, the smallest ladder value > c)
inline uint32_t adaptive_next_count(uint32_t c, uint32_t n0, uint32_t cap) {
    uint64_t t = n0;
    while (t <= c) t *= 2u;
    return (uint32_t)std::min<uint64_t>(t, cap);
}
// The key of the held adaptive frame: pt_ctx_accumulate's, the tile edge and n_0
struct AdaptiveKey {
    AccumKey frame{};
    uint32_t tile = 0, n0 = 0;
    bool operator==(const AdaptiveKey &o) const { return frame == o.frame && tile == o.tile && n0 == o.n0; }
};
// The host's side of the held adaptive frame (pt_api.hip: HeldAdaptive adds the device planes and the tiles' device table) and
// of a checkpoint of it: `total` pixels of the frame `key` in `tiles` tiles.  A frame is held iff tiles != 0.
struct AdaptiveFrame {
    AdaptiveKey key{};
    uint32_t total = 0, tiles = 0;
    bool held() const { return tiles != 0u; }
    bool holds(const AdaptiveKey &k) const { return held() && key == k; }
};
// The per-tile state: the count, the samples of it in half A, the last E (kTileNoError: none)
struct TileTable {
    std::vector<uint32_t> cnt, na;
    std::vector<unsigned long long> err;
};
// is a tile with this E closed under q (its `pixels` inside the frame)?  A tile without an E is open.
inline bool tile_closed(unsigned long long E, unsigned long long q, uint64_t pixels) { return E != kTileNoError && E <= q * pixels; }
// pixels of tile i inside a band of `rows` rows
inline uint64_t tile_pixels(uint32_t width, uint32_t rows, const TileGeometry &g, uint32_t i) {
    const uint32_t tile = 1u << g.tile_shift, x0 = i % g.tiles_x * tile, y0 = i / g.tiles_x * tile;
    return (uint64_t)std::min(width - x0, tile) * std::min(rows - y0, tile);
}

// One step of a pt_ctx_accumulate_adaptive call: the class - the n open tiles that hold c samples, na of them in half A - goes
// to T samples in the runs [c, m) and [m, T) (the second one empty when m == T); to_a[r]: run r goes to half A (the half that
// holds fewer samples of the tile, a tie to A); na_end: half A's samples afterwards.
struct AdaptiveStep {
    uint32_t c, na, n, T, m, na_end;
    bool to_a[2];
    uint32_t runs() const { return m < T ? 2u : 1u; }
};
// WHICH CLASS IS NEXT.  Built from the tiles' table once, re-decided under q and the cap: how many tiles every class (c, nA)
// holds open - never which ones (the device finds them: k_tile_select).  next(): the open tiles with the smallest c below the
// cap, among those the smallest nA; false when no open tile is below the cap.  done(): the step's two words - the tiles it left
// open and the tiles it closed - move the class to (T, na_end).
class AdaptiveSchedule {
   public:
    AdaptiveSchedule(const TileTable &t, uint32_t width, uint32_t rows, const TileGeometry &g, unsigned long long q, uint32_t cap, uint32_t n0);
    bool next(AdaptiveStep &s) const;
    void done(const AdaptiveStep &s, uint32_t still_open, uint32_t closed);
    uint32_t tiles_open() const { return open_; }
    uint32_t tiles_at_cap() const;  // open tiles that take no samples: c >= cap

   private:
    std::vector<std::pair<uint64_t, uint32_t>> classes_;  // (c << 32 | nA, open tiles), ascending, none empty
    uint32_t cap_, n0_, open_ = 0;
};

// ---- checkpoint of the held adaptive frame (pt_ctx_adaptive_save / _load, ptrace.h): as the held accumulate frame's
struct AdaptiveCheckpoint : AdaptiveFrame, SealedFile {
    TileTable table;
};
// the file up to its planes appended to b; the planes follow (the held sums, then half A's), then ckpt_seal's hash
void adckpt_encode_head(const AdaptiveCheckpoint &ck, std::vector<uint8_t> &b);
// as ckpt_decode; kCkptBad also for nA > count, a count above 2^24, an E where a half is empty, sizes that do not fit the tiles
int adckpt_decode(uint64_t file_size, const uint8_t *b, size_t n, AdaptiveCheckpoint &out, std::string &why);

// ---- host-array queries (pt_ctx_radiance .. pt_ctx_scatter, ptrace.h; pt_api.hip: HostCall): pure, tested on the CPU
// (host/query_check.cpp).  The refusals of the calls that test more than "NULL / no scene", in each call's order: PT_ERR_INVALID +
// message.  ctx is never dereferenced; the arrays are only read past the refusals that do not need them.
int check_radiance(const void *ctx, bool has_scene, const float *o, const float *d, uint32_t depth, uint32_t n_samples, uint32_t backend,
                   uint32_t flags, const float *out_rgb);
// PT_OK: cfg is the width x height frame of one sample the rays belong to, [*idx_begin, *idx_end) its band (check_cfg's)
int check_primary_rays(const void *ctx, bool has_scene, uint32_t width, uint32_t height, uint64_t seed, const uint32_t *pixel,
                       const uint32_t *sample, uint32_t n, uint32_t form, const float *o, const float *d, pt_config &cfg,
                       uint32_t *idx_begin, uint32_t *idx_end);
// pt_ctx_intersect_bounds (mode 0: `object` of n_objs) and pt_ctx_orbit_point (mode 1)
int check_bounds_query(const void *ctx, bool has_scene, uint32_t mode, uint32_t object, uint32_t n_objs, const float *o, const float *d);
// n rays (o, d: 3 floats each) as K = ceil(n / cap) slices of a ray queue (pt_kernels.h: RayQueue), cap * kRayBytes bytes each.
// Slot j of slice b is ray b * cap + j: od0 = (ox, oy, oz, dx), tp = 0, od1 = (dy, dz).  counts[b]: the rays of slice b,
// min(cap, n - b * cap); the slots behind them are zero.
void pack_ray_streams(const float *o, const float *d, uint32_t n, uint32_t cap, std::vector<char> &bytes, std::vector<uint32_t> &counts);
// the inverse for the intersect step's results - per slot, one slice after the other, a float2 (hit distance, hit id as bits); this
// header is also compiled without HIP's vector types, hence the bytes - of the first n rays
void unpack_stream_hits(const void *hits, uint32_t n, float *t, int32_t *id);

}  // namespace host
}  // namespace pt
