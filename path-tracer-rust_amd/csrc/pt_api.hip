// pt_api.hip — C ABI of the compute path (include/ptrace.h): contexts, scene flattening, the pass loop
// of the wavefront pipeline, the megakernel launch, single-ray queries.  No CPU fallback exists here:
// without a HIP device every entry point returns PT_ERR_NO_DEVICE.
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ptrace.h"
#include "pt_accum.h"
#include "pt_aov.h"
#include "pt_denoise.h"
#include "pt_despike.h"
#include "pt_host.h"
#include "pt_kernels.h"
#include "pt_masked.h"
#include "pt_noise.h"
#include "pt_overlay.h"
#include "pt_present.h"
#include "pt_probe.h"
#include "pt_refit.h"
#include "pt_reproject.h"
#include "pt_solid.h"
#include "pt_tone.h"
#include "pt_upsample.h"
#include "pt_tile.h"

namespace pt {

thread_local std::string g_last_error;

void set_error(const std::string &m) { g_last_error = m; }

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                              \
            return PT_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

// DevBuf::ensure's "out of device memory" (never leaves the library: render_wavefront retries with smaller passes and
// reports PT_ERR_HIP when even the smallest does not fit)
constexpr int PT_ERR_NOMEM_INTERNAL = -1000;

// A device allocation and its owner: freed with it (on the device that is current then - pt_ctx_destroy makes it the context's)
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    ~DevBuf() { release(); }
    size_t bytes() const { return p ? n * sizeof(T) : 0; }
    int ensure(size_t count, bool tell_oom = false) {
        if (count <= n && p) return PT_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc((void **)&p, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();  // (the error is reported through the return value; do not leave it sticky)
            set_error(std::string("hipMalloc of ") + std::to_string((count ? count : 1) * sizeof(T)) + " bytes: " + hipGetErrorString(e));
            return (tell_oom && e == hipErrorOutOfMemory) ? PT_ERR_NOMEM_INTERNAL : PT_ERR_HIP;
        }
        n = count;
        return PT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // `count` records from the host to [at, at + count) of the buffer (none: no copy); `what` names it in a failure's message
    int copy_in(size_t at, const T *src, size_t count, const char *what) {
        const hipError_t e = count ? hipMemcpy(p + at, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
        if (e != hipSuccess) set_error(std::string("hipMemcpy to ") + what + ": " + hipGetErrorString(e));
        return e == hipSuccess ? PT_OK : PT_ERR_HIP;
    }
    // the buffer made large enough for the records and filled with them
    int upload(const T *src, size_t count, const char *what) {
        const int rc = ensure(count);
        return rc ? rc : copy_in(0, src, count, what);
    }
    int upload(const std::vector<T> &v, const char *what) { return upload(v.data(), v.size(), what); }
};

// A table of the scene on the device (host::PT_SCENE_TABLES): the buffer, and the records it holds now - what
// pt_ctx_table_hashes hashes and DevScene's n_* report.  buf.n is the CAPACITY, which never shrinks; a table that an edit made
// shorter keeps its allocation.  The count outlives the host's copy (keep_flat drops three tables there).
template <class T>
struct DevTable {
    DevBuf<T> buf;
    size_t count = 0;
    int upload(const std::vector<T> &v, const char *name) {  // the table whole
        const int rc = buf.upload(v, name);
        count = rc ? 0 : v.size();
        return rc;
    }
    int upload_range(size_t at, const T *src, size_t n, const char *name) {  // its records [at, at + n)
        if (at <= count && n <= count - at) return buf.copy_in(at, src, n, name);
        set_error(std::string("internal: a range past the end of the device table ") + name);
        return PT_ERR_INVALID;
    }
};

// The device buffers of one state, made large enough and filled one after the other: each from host bytes (a checkpoint's: on the
// device when done() returns) or, from NULL, with a byte value on `st`.  The first failure stops the rest; done() returns it - a
// HIP failure's message begins "uploading the checkpoint: " or, when nothing was uploaded, with `clearing`.
struct DevFill {
    hipStream_t st;
    const char *clearing;
    int rc = PT_OK;
    bool uploaded = false;
    template <class T>
    void operator()(DevBuf<T> &d, size_t count, const void *from, int byte = 0) {
        if (rc || (rc = d.ensure(count))) return;
        uploaded = uploaded || from;
        hip(from ? hipMemcpy(d.p, from, count * sizeof(T), hipMemcpyHostToDevice) : hipMemsetAsync(d.p, byte, count * sizeof(T), st));
    }
    void hip(hipError_t e) {
        if (e != hipSuccess) rc = PT_ERR_HIP, set_error(std::string(uploaded ? "uploading the checkpoint: " : clearing) + hipGetErrorString(e));
    }
    int done() {
        if (!rc && uploaded) hip(hipStreamSynchronize(st));
        return rc;
    }
};

// The device planes of a held frame and their one owner: the sums, [3] planes of `total` u64, and the sums of half A of the
// samples in `a`, laid out as `sums` (half B: sums - a) - only when asked for: an untracked frame allocates no half A.
struct HeldPlanes {
    DevBuf<unsigned long long> sums, a;
    void release() { sums.release(), a.release(); }
    void fill(DevFill &fill, uint32_t total, bool with_a, const uint8_t *from_sums, const uint8_t *from_a) {
        fill(sums, 3 * (size_t)total, from_sums);
        if (with_a) fill(a, 3 * (size_t)total, from_a);
    }
};

// The frame pt_ctx_accumulate keeps between calls, and its one owner: host::FrameCounts plus the planes, half A's for a noise-
// tracked frame.  start() is the only place that gives the counts any entries, after the planes are allocated and filled: a frame
// is held whole or not at all.
struct HeldFrame : host::FrameCounts, HeldPlanes {
    void drop() {
        static_cast<host::FrameCounts &>(*this) = {};
        release();
    }
    // Hold the frame f in place of whatever was held.  The planes come from the host bytes from_sums / from_a (a checkpoint's)
    // or start at zero on `st` (NULL).  On any failure nothing is held, and the memory is given back.
    int start(host::FrameCounts f, const uint8_t *from_sums, const uint8_t *from_a, hipStream_t st) {
        drop();
        DevFill fill{st, "clearing the held sums: "};
        HeldPlanes::fill(fill, f.total, f.tracked(), from_sums, from_a);
        if (fill.done()) drop();
        else static_cast<host::FrameCounts &>(*this) = std::move(f);
        return fill.rc;
    }
};

// The adaptive frame a context keeps between calls (pt_ctx_accumulate_adaptive), and its one owner: host::AdaptiveFrame plus the
// device side - the planes, both of them, and the tiles' table (per tile the count, nA and the last E).  start() is the only place
// that makes a frame held, after everything is allocated and filled: a frame is held whole or not at all.  forget() stops holding
// it and keeps the memory for the next frame (pt_ctx_render_adaptive renders frame after frame); drop() gives the memory back.
struct HeldAdaptive : host::AdaptiveFrame, HeldPlanes {
    DevBuf<unsigned long long> err;
    DevBuf<uint32_t> cnt, na;
    host::TileGeometry geo{};

    void forget() { static_cast<host::AdaptiveFrame &>(*this) = {}; }
    void drop() {
        forget();
        release(), err.release(), cnt.release(), na.release();
    }
    // Hold the frame f (tiles as g cuts it) in place of whatever was held.  The state comes from a checkpoint - the table and the
    // host bytes from_sums / from_a - or starts at zero on `st` (table NULL).  On any failure nothing is held, and the memory is
    // given back.
    int start(const host::AdaptiveFrame &f, const host::TileGeometry &g, const host::TileTable *table, const uint8_t *from_sums,
              const uint8_t *from_a, hipStream_t st) {
        forget();
        geo = g;
        DevFill fill{st, "clearing the held adaptive frame: "};
        HeldPlanes::fill(fill, f.total, true, from_sums, from_a);
        fill(err, f.tiles, table ? table->err.data() : nullptr, 0xff);  // kTileNoError
        fill(cnt, f.tiles, table ? table->cnt.data() : nullptr);
        fill(na, f.tiles, table ? table->na.data() : nullptr);
        if (fill.done()) drop();
        else static_cast<host::AdaptiveFrame &>(*this) = f;
        return fill.rc;
    }
    // the tiles' table as the device holds it (the host waits for `st`)
    int download(host::TileTable &t, hipStream_t st) const {
        t.cnt.resize(tiles);
        t.na.resize(tiles);
        t.err.resize(tiles);
        HIP_TRY(hipMemcpyAsync(t.cnt.data(), cnt.p, (size_t)tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t.na.data(), na.p, (size_t)tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t.err.data(), err.p, (size_t)tiles * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return PT_OK;
    }
};

}  // namespace pt

using namespace pt;
using host::check_cfg;
using host::owned_pixels;

// Tuning switches (A/B runs, profiling).  Read from the environment ONCE, when a context is created, and kept with the
// context: a frame never sees two different answers.  PT_DEBUG (ablation switches that change the image) exists only in
// builds made with -DPT_ALLOW_DEBUG; the shipped library ignores it.
struct Tuning {
    bool pass_kernel = true;   // PT_PASS_KERNEL=0: generate / intersect / shade as separate kernels
    bool pass_bvh = true;      // PT_PASS_BVH=0: BVH scenes through the separate kernels
    bool bvh_lds = false;      // PT_BVH_LDS=1: stage BVH nodes in LDS (separate kernels only)
    bool cand_scan = true;     // PT_CAND_SCAN=0: k_pass scans every triangle per ray (the round-1 form) instead of candidates
    uint32_t walk_queue_cap = 0;  // PT_WALK_QUEUE_CAP=n: the walk queue of k_pass_cand holds n entries (>= 128) instead of what its
                                  // LDS area allows - small values exercise the depth-first second walk (tests)
    bool cand_bvh = true;      // PT_CAND_BVH=0: scenes with BVH meshes run k_pass_bvh (scan + parked walks) instead of
                               // the candidate scan with parked walks (k_pass_cand<.., BVH>)
    uint32_t leaf_quorum = 12; // PT_LEAF_QUORUM: lanes on a leaf that send a walking wave to the triangle code
    uint64_t streams = 0;      // PT_STREAMS: ray streams per pass (0 = derived from the frame)
    uint32_t per_stream = 0;   // PT_PER_STREAM: primary rays per stream and pass that k_pass_cand's stream count aims at (0 = default)
    int64_t taper_cut = -1;    // PT_TAPER_CUT=n: k_pass_cand's launches run their last n streams in pieces (host::plan_taper; 0 = off,
                               // unset = the default, host::kTaper*)
    uint32_t taper_pieces = 0; // PT_TAPER_PIECES=c: ... c pieces each, a power of two (unset = the default)
    uint64_t rays_per_pass = 0;  // PT_RAYS_PER_PASS: the default of pt_config.rays_per_pass (probes; 0 = the library's)
    bool glass_defer = false;    // PT_GLASS_DEFER=1: k_pass_cand collects glass hits per wave and shades them 64 at a time (A/B: it
                                 // paid with levels, it does not without)
    bool nodes_lds = true;       // PT_NODES_LDS=0: k_pass_cand with walks reads the BVH nodes from global memory even when they
                                 // would fit its LDS (A/B)
    uint32_t wave_stack = 0;     // PT_WAVE_STACK=n: k_pass_cand's stacks hold n slots (a power of two, 512 <= n < kWaveStackMax)
                                 // instead of kWaveStackMax - the waves then have to hold their primaries back (tests)
    uint32_t mega_items = 0;     // PT_MEGA_ITEMS=n: the megakernel cuts a round into n items per lane the chip holds (0 = default)
    bool lds_say = false;        // PT_LDS_PAD set: the kernels that stage records in LDS say their layout on stderr (say_layout)
    size_t lds_pad = 0;          // PT_LDS_PAD=n: k_pass_cand asks for n bytes of LDS it does not use (diagnosis: where does the
                                 // fifth workgroup of a CU stop fitting?)
    uint32_t dn_lds_maxstep = 0;  // PT_DN_LDS_MAXSTEP=n: pt_ctx_denoise's levels with step <= n stage their taps in LDS, the others
                                  // load them through the caches (same bytes; 0 = every level direct, 128 = every level LDS)
    uint32_t debug = 0;
};
constexpr uint32_t kDnLdsMaxStepDefault = 4;  // measured: LDS wins at steps 1, 2, 4 and loses from 8 on
static Tuning read_tuning() {
    Tuning t;
    auto num = [](const char *name, long long dflt) {
        const char *e = getenv(name);
        return e ? atoll(e) : dflt;
    };
    t.pass_kernel = num("PT_PASS_KERNEL", 1) != 0;
    t.pass_bvh = num("PT_PASS_BVH", 1) != 0;
    t.bvh_lds = num("PT_BVH_LDS", 0) != 0;
    t.cand_scan = num("PT_CAND_SCAN", 1) != 0;
    t.cand_bvh = num("PT_CAND_BVH", 1) != 0;
    t.walk_queue_cap = (uint32_t)num("PT_WALK_QUEUE_CAP", 0);
    t.leaf_quorum = (uint32_t)num("PT_LEAF_QUORUM", 12);
    const long long st = num("PT_STREAMS", 0);
    t.streams = st > 0 ? (uint64_t)st : 0;
    t.per_stream = (uint32_t)num("PT_PER_STREAM", 0);
    {
        const long long tc = num("PT_TAPER_CUT", -1), tp = num("PT_TAPER_PIECES", 0);
        t.taper_cut = tc < 0 ? -1 : (tc > 0xffffffffll ? 0xffffffffll : tc);
        t.taper_pieces = tp > 0 ? (uint32_t)(tp > 64 ? 64 : tp) : 0u;
    }
    t.rays_per_pass = (uint64_t)num("PT_RAYS_PER_PASS", 0);
    t.nodes_lds = num("PT_NODES_LDS", 1) != 0;
    t.glass_defer = num("PT_GLASS_DEFER", 0) != 0;
    t.lds_say = getenv("PT_LDS_PAD") != nullptr;
    {
        const long long pad = num("PT_LDS_PAD", 0);
        t.lds_pad = pad > 0 ? (size_t)pad : 0u;
    }
    {
        const long long mi = num("PT_MEGA_ITEMS", 0);
        t.mega_items = mi > 0 && mi <= 4096 ? (uint32_t)mi : 0u;
    }
    {
        const long long ws = num("PT_WAVE_STACK", 0);
        if (ws >= 512 && ws < (long long)kWaveStackMax && (ws & (ws - 1)) == 0) t.wave_stack = (uint32_t)ws;
    }
    {
        const long long ms = num("PT_DN_LDS_MAXSTEP", kDnLdsMaxStepDefault);
        t.dn_lds_maxstep = ms < 0 ? 0u : (ms > 128 ? 128u : (uint32_t)ms);
    }
#ifdef PT_ALLOW_DEBUG
    t.debug = (uint32_t)num("PT_DEBUG", 0);
#endif
    return t;
}

// The frame call in progress (pt_ctx_render / pt_ctx_accumulate), for pt_ctx_snapshot from the progress callback; the call
// clears it whenever it returns.  A large call is rendered in parts: pixels [0, k0) of it are final in `out`, [k0, k0 + npix)
// are the part in progress (spp_issued samples per pixel issued, accumulators of `streams` x `m` slots), the rest has not
// been started (`total` pixels in all).
struct LiveFrame {
    uint32_t npix = 0, spp_issued = 0, streams = 1, m = 0;
    uint32_t k0 = 0, total = 0;
    float *out = nullptr;
    hipStream_t stream = nullptr;
    bool accum = false;        // a pt_ctx_accumulate: pt_ctx_snapshot shows the other parts at their counts
    double cb_last_ms = 0.0;   // time of the last progress callback (throttle: pt_config.progress_ms; one clock per call)
};

struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool has_scene = false;
    bool profiling = false;
    Tuning tune;
    std::string lds_said[3];  // the layout line say_layout last wrote for each launcher of this context
    pt_camera cam{};
    DevScene scene{};
    struct SceneTables {  // one DevTable per table of the list, under the list's name
#define PT_X(ID, T, name) DevTable<T> name;
        PT_SCENE_TABLES(PT_X)
#undef PT_X
    } tab;
    bool cand_ok = false;
    uint32_t n_bvh_nodes = 0;
    uint32_t n_cus = 0;  // compute units of the device (pt_ctx_create: never 0 afterwards)
    // Mesh.bounding_box of every object (12 object-local triangles each; Mesh::new's unless pt_ctx_set_mesh_bounds gave
    // the stored ones) and their device form (6 pair records per object), for intersect_bounds / orbit-point queries
    std::vector<pt_triangle> h_boxes;
    std::vector<pt_object> h_objs;
    // the triangles as pt_ctx_set_scene got them (36 B each) and the box its bounds were derived for: what pt_ctx_set_camera
    // rebuilds the tables from when the lens centre leaves the box, and what the lazy fingerprint hashes
    std::vector<pt_triangle> h_tris;
    host::Reach reach{};
    // pt_ctx_set_object.  fs: the tables as flatten_scene made them for `reach`, kept on the host without the three that hold
    // nothing an edit reads (rank_id, surf, tri_rank) - an in-reach edit rewrites one object's records in it and uploads those.
    // Of a mesh with a BVH it keeps the TOPOLOGY (ids, child references, wide_src): the floats of its pair records, shading
    // records and boxes go stale with the first refit, which rewrites the device's.  h_local: every mesh's object-local vertex
    // box.  refit: the device plans of the meshes moved since the last full build (upload_flat drops them).
    host::FlatScene fs;
    std::vector<host::Reach> h_local;
    struct DevRefit {
        DevBuf<pt_triangle> local;
        DevBuf<RefitLeaf> leaves;
        DevBuf<RefitNode> nodes;
        DevBuf<RefitWide> wide;
        std::vector<uint32_t> level_begin;
        uint32_t n_leaves = 0, n_wide = 0;
    };
    std::map<uint32_t, DevRefit> refit;
    DevBuf<TriPairRec> d_boxes;
    bool boxes_dirty = true;
    // scratch of the single-ray query entry points (kept across calls: a picking caller sends one ray per click)
    DevBuf<float> q_o, q_d, q_t, q_x, q_n;
    DevBuf<int32_t> q_oid, q_tid;
    // wavefront queues
    DevBuf<char> q_buf[2];  // the two ray-queue containers: K slices of cap * 40 bytes each (RayQueue, pt_kernels.h)
    DevBuf<float2> hit;
    DevBuf<uint32_t> cnt, flags;
    DevBuf<unsigned long long> blk_rays, acc, total_rays;
    std::vector<hipEvent_t> ev_pool;
    LiveFrame live;
    // concurrent pipelines (PT_FLAG_PIPELINES): child contexts that borrow this context's scene tables
    std::vector<pt_ctx *> pipes;
    std::vector<DevBuf<float>> pipe_out;
    bool borrowed_scene = false;
    // memory-aware pass sizing: contexts that will hold ray queues on this device at the same time (pipelines of one call,
    // ranks of pt_render_multi that share a device) and an explicit cap on the queue memory of this context (0 = 85 % of
    // what hipMemGetInfo reports free, divided by `mem_share`)
    uint32_t mem_share = 1;
    size_t mem_budget = 0;
    // Passes sized by TIME (k_pass_cand, megakernel rounds): primary samples per millisecond the last timed pass / round of this
    // scene went through, per backend (0: not measured yet - the next frame starts with a short timed pass).  pt_ctx_set_scene
    // forgets them.
    double pass_rate = 0.0, round_rate = 0.0;
    const char *pass_rate_kernel = nullptr;  // the kernel pass_rate was measured on (flags choose other kernels)
    // pt_ctx_accumulate: the frame kept between calls.  scene_fp: the checkpoint fingerprint of the scene pt_ctx_set_scene got,
    // which drops the held frame.  acc_track (pt_ctx_accum_track_noise): the frames this context starts are noise-tracked.
    // noise_cnt: pt_ctx_accum_noise's counters.
    // fp_stale: the camera changed since scene_fp was computed (pt_ctx_set_camera) - read it through scene_fp_of().
    HeldFrame held;
    uint64_t scene_fp = 0;
    bool fp_stale = false;
    bool acc_track = false;
    DevBuf<NoiseCounters> noise_cnt;
    // pt_ctx_denoise's scratch, kept between calls: the two colour planes and the packed guides, one float4 per pixel each
    DevBuf<float4> dn_u[2], dn_guide;
    // pt_ctx_present's scratch, its own (outside the ray-queue budget): the threshold table, uploaded by the first call, and the
    // resampling form's intermediate, [3] planes of width * out_height u64, grown on demand
    DevBuf<uint32_t> pr_table;
    DevBuf<unsigned long long> pr_mid;
    // pt_ctx_reproject_var's scratch, its own too: the frame's s values, one float per pixel, grown on demand
    DevBuf<float> rv_s;
    // pt_ctx_reproject*_moved's scratch, its own too: the call's motion table, 16 B per record, grown on demand
    DevBuf<pt_object_motion> rm_table;
    // pt_ctx_solid's scratch, its own too: the call's looks table, 16 B per record, grown on demand
    DevBuf<pt_solid_look> solid_looks;
    // the tone stage's scratch, its own too: pt_ctx_meter's counters (kMeterWords), pt_ctx_accum_hdr's count per part
    DevBuf<uint32_t> meter_cnt;
    DevBuf<uint32_t> hdr_counts;
    // pt_ctx_despike's scratch, its own too: the call's two counters, 16 B
    DevBuf<unsigned long long> despike_cnt;
    // The adaptive calls: the frame kept between calls (pt_ctx_set_scene drops it), and their scratch, kept too and grown on
    // demand: the compact accumulator of a step's tiles, the step's open-tile list, the counters (u64 [0]: the sum of E at the
    // end; u32 [2], [3]: the tiles a step left open / closed; u32 [4]: the list's length; u32 [5..7]: k_tile_select's counts),
    // the tile pass's ray counters, and the rate its own rounds measured (pt_ctx_set_scene forgets it)
    HeldAdaptive adaptive;
    DevBuf<unsigned long long> ad_acc, ad_cnt, ad_rays;
    DevBuf<uint32_t> ad_open;
    DevBuf<char> ad_stack;
    double ad_rate = 0.0;
    // pt_ctx_select_pixels and pt_ctx_render_masked.  Their own: two counter words ([0]: the select pass's count, [1]: the list's
    // length), the list of a call's selected pixels (4 B each, grown on demand: NOT ad_open, whose slots must name tiles of the
    // held adaptive frame whatever a launch reads of them) and the rate the call's rounds measured (pt_ctx_set_scene forgets
    // it).  The compact accumulator, the ray counters and the split stacks are the adaptive calls' per-step scratch - ad_acc,
    // ad_rays, ad_stack - which hold nothing between calls.
    DevBuf<uint32_t> mk_cnt, mk_list;
    double mk_rate = 0.0;
};

namespace {

int device_count_quiet() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

FrameParams make_frame(const pt_ctx *ctx, const pt_config *cfg, uint32_t idx_begin, uint32_t idx_end) {
    FrameParams F{};
    float lens[3], su[3], sv[3];
    host::camera_basis(ctx->cam, lens, su, sv);
    F.width = cfg->width;
    F.height = cfg->height;
    F.spp = cfg->spp;
    F.idx_begin = idx_begin;
    F.npix = owned_pixels(cfg, idx_begin, idx_end);
    F.chunk_pixels = cfg->chunk_pixels;
    F.chunk_first = cfg->chunk_first;
    F.chunk_step = cfg->chunk_step;
    F.n_streams = 1;  // set by the wavefront renderer
    F.seed_lo = (uint32_t)cfg->seed;
    F.seed_hi = (uint32_t)(cfg->seed >> 32);
    F.cam_px = ctx->cam.position[0];
    F.cam_py = ctx->cam.position[1];
    F.cam_pz = ctx->cam.position[2];
    F.lens_x = lens[0];
    F.lens_y = lens[1];
    F.lens_z = lens[2];
    F.su_x = su[0];
    F.su_y = su[1];
    F.su_z = su[2];
    F.sv_x = sv[0];
    F.sv_y = sv[1];
    F.sv_z = sv[2];
    F.debug = ctx->tune.debug;
    F.k_begin = 0;
    return F;
}

RayQueue queue_of(pt_ctx *c, int which) {
    RayQueue q;
    q.buf = c->q_buf[which].p;
    return q;
}

hipEvent_t get_event(pt_ctx *c, size_t i) {
    while (c->ev_pool.size() <= i) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->ev_pool.push_back(e);
    }
    return c->ev_pool[i];
}

// does a frame with these flags run the candidate scan (k_pass_cand)?  Scenes with BVH meshes: with parked walks, unless
// their nodes are staged in LDS (PT_BVH_LDS=1) or PT_CAND_BVH=0 asks for k_pass_bvh.
static uint32_t cand_scan_for(const pt_ctx *c, uint32_t flags) {
    if (!c->tune.cand_scan || !c->cand_ok || (flags & PT_FLAG_NO_BVH)) return 0u;
    if (c->n_bvh_nodes != 0u && (!c->tune.cand_bvh || (c->scene.bvh_in_lds & 1u))) return 0u;
    return 1u;
}

// How a call with these flags runs, decided once per call.  The context's scene record is never changed for a call: the
// call works on `scene`, a copy with the flags' BVH mode and candidate scan.
struct FrameForm {
    DevScene scene;
    bool one_kernel;     // a wavefront pass is one launch (k_pass*), not generate / intersect / shade
    bool stack_form;     // ... and that launch is k_pass_cand, whose waves keep their rays on stacks (passes sized by time)
    bool stack_park;     // ... with container 1 for the waves' parked rays (scenes with walks) or deferred glass hits
    const char *kernel;  // what pt_ctx_pass_kernel reports (and what pass_rate is keyed on)
};

FrameForm form_for(const pt_ctx *c, uint32_t flags) {
    FrameForm f;
    DevScene &S = f.scene;
    S = c->scene;
    // PT_FLAG_NO_BVH: scan meshes triangle by triangle as the reference does (same result, for A/B checks)
    S.n_bvh_nodes = (flags & PT_FLAG_NO_BVH) ? 0u : c->n_bvh_nodes;
    S.planar = (flags & PT_FLAG_NO_BVH) ? 0u : 1u;
    S.cand_scan = cand_scan_for(c, flags);
    // scenes without BVH meshes run a pass as one launch (k_pass), BVH scenes as k_pass_bvh unless their nodes are staged
    // in LDS; PT_FLAG_SEPARATE_KERNELS / PT_PASS_KERNEL=0 / PT_PASS_BVH=0 keep the three-kernel form (A/B, profiling)
    const bool bvh = S.n_bvh_nodes != 0u;
    const bool bvh_ok = !bvh || (!(S.bvh_in_lds & 1u) && c->tune.pass_bvh);
    f.one_kernel = bvh_ok && c->tune.pass_kernel && !(flags & PT_FLAG_SEPARATE_KERNELS);
    f.stack_form = f.one_kernel && S.cand_scan != 0u;
    f.stack_park = f.stack_form && (bvh || S.glass_defer_ok != 0u);
    if (!f.one_kernel)
        f.kernel = (!bvh && S.cand_scan) ? "k_intersect_cand" : "k_intersect";
    else if (S.cand_scan)
        f.kernel = bvh ? "k_pass_cand_bvh" : "k_pass_cand";  // (k_pass_cand<.., BVH = true>)
    else
        f.kernel = bvh ? "k_pass_bvh" : "k_pass";
    return f;
}

// pt_config.progress_ms as milliseconds between two progress callbacks (0 = 500 ms, PT_PROGRESS_EVERY_PASS = every pass
// boundary)
double progress_interval_ms(const pt_config *cfg) {
    return cfg->progress_ms == PT_PROGRESS_EVERY_PASS ? 0.0 : (cfg->progress_ms ? (double)cfg->progress_ms : 500.0);
}

// PT_LDS_PAD set: the layout a kernel that stages records runs with (lds_layout_line, pt_layout.h), on stderr whenever it
// differs from the last one this context said for that launcher (which: 0 launch_pass, 1 launch_intersect_cand, 2 launch_mega)
static void say_layout(pt_ctx *c, const LdsLayout &L, int which) {
    if (!c->tune.lds_say) return;
    const std::string line = lds_layout_line(L, which);
    if (line == c->lds_said[which]) return;
    c->lds_said[which] = line;
    fprintf(stderr, "%s\n", line.c_str());
}

// pt_ctx_accumulate's sums of a part's pixels: [3] planes of `stride` u64 in pixel order, the part's first pixel at p.  A
// renderer given them starts its accumulators from them (launch_accum_gather) instead of from zero.
struct HeldSums {
    const unsigned long long *p;
    uint32_t stride;
};

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// The progress callback, throttled to pt_config.progress_ms on the call's clock (LiveFrame::cb_last_ms); true when it was made
bool progress(pt_ctx *c, const pt_config *cfg, pt_progress_fn cb, void *user, float f) {
    const double t_now = now_ms();
    if (t_now - c->live.cb_last_ms < progress_interval_ms(cfg)) return false;
    c->live.cb_last_ms = t_now;
    cb(user, f);
    return true;
}

// The frame call in progress owns pt_ctx.live: its clock starts here, and however the call returns, pt_ctx_snapshot finds no frame
// in progress afterwards
struct LiveScope {
    pt_ctx *c;
    explicit LiveScope(pt_ctx *c_) : c(c_) { c->live.cb_last_ms = now_ms(); }
    LiveScope(const LiveScope &) = delete;
    ~LiveScope() { c->live = LiveFrame{}; }
};

// A progress relay: the fractions below 1 of an inner call, passed on as base + scale * f of the outer one.  The inner call's
// "1.0" is not passed on: the outer call says when IT is complete (the next job, every pipeline or rank finished and the frame
// assembled).
struct Relay {
    pt_progress_fn cb;
    void *user;
    float base = 0.0f, scale = 1.0f;
    static void fn(void *self, float f) {
        Relay *r = (Relay *)self;
        if (f < 1.0f) r->cb(r->user, r->base + r->scale * f);
    }
};

// The cadence of a renderer's launches (the wavefront's passes, the megakernel's rounds) on events 0..5 of the context's pool.
// The cancel byte is read at EVERY launch boundary (the reference polls it every 100 ms, mod.rs:947-958) and again after a
// progress callback; the callback (RenderUpdate, mod.rs:965-982) is throttled to pt_config.progress_ms.  With ONE launch in
// flight (`one`: asked for, or wherever launches are sized by time) the launch before is waited for before the next is
// issued - a few microseconds against a launch of 0.1 s - and progress counts the samples issued; otherwise two launches are
// in flight and progress counts the launches known done.
//
// LAUNCHES THAT FOLLOW THE SCENE (`adaptive`).  A launch must not take much longer than 0.1 s WHATEVER a ray of the scene
// costs - 512 Mi primary rays are 0.1 s on cornell.json, 0.15 s on mesh.json, and a scene of 392 unfiltered candidate records
// inside an emitting sphere (tests) is fifty times dearer per primary ray.  So the first launch of a scene is TINY (kProbeRays
// primary rays) and every launch is timed: the next one gets as many samples as the measured rate fits into kTargetMs
// (host::next_pass_samples: up to a fifth more where that saves a launch, at most sixteen times the launch before - a short
// launch measures overheads too - never more than `max_spp`, the rest of the frame in equal launches).  The rate is kept with
// the context (pt_ctx.pass_rate / round_rate), so the following frames of the scene start at full length: the bench frame is
// six passes of 683 samples, and the first frame of a scene pays three short passes.  Frames of at most kAdaptiveMinRays
// primary rays are one launch; an explicit rays_per_pass is taken as given.  Launches only batch the samples: the image does
// not depend on them.
struct PassPacer {
    static constexpr uint64_t kProbeRays = 1ull << 20, kAdaptiveMinRays = 4ull << 20;
    static constexpr double kTargetMs = 100.0;
    static constexpr int kLaunch = 1;  // next(): issue the launch it sized
    pt_ctx *c;
    const pt_config *cfg;
    hipStream_t st;
    const volatile uint8_t *cancel;
    pt_progress_fn cb;
    void *user;
    uint64_t npix;
    uint32_t max_spp, n_pass;  // samples per pixel of a launch at most; launches of max_spp that the frame takes
    bool adaptive, one;
    double rate;               // primary samples per millisecond the last timed launch went through (0: not measured)
    hipEvent_t ev[6] = {};     // frame begun, frame done, launch done [2], launch begun [2]
    uint32_t p = 0;            // launches issued
    uint32_t s0 = 0, s_here = 0, s_next, s_prev = 0;  // the launch next() sized: samples [s0, s0 + s_here); issued; in the last
    bool cancelled = false;

    // samples [s_first, cfg->spp) of npix pixels; `may_adapt`: this renderer's launches may be sized by time, starting
    // from `known_rate` (0: with a probe)
    PassPacer(pt_ctx *c_, const pt_config *cfg_, hipStream_t st_, const volatile uint8_t *cancel_, pt_progress_fn cb_, void *user_,
              uint64_t npix_, uint32_t s_first, uint32_t max_spp_, bool one_in_flight, bool may_adapt, double known_rate)
        : c(c_), cfg(cfg_), st(st_), cancel(cancel_), cb(cb_), user(user_), npix(npix_), max_spp(max_spp_),
          n_pass((cfg_->spp - s_first + max_spp_ - 1) / max_spp_),
          adaptive(may_adapt && !cfg_->rays_per_pass && npix_ * (cfg_->spp - s_first) > kAdaptiveMinRays),
          one(one_in_flight || adaptive), rate(adaptive ? known_rate : 0.0), s_next(s_first) {}

    hipEvent_t done(uint32_t i) const { return ev[2 + (i & 1u)]; }
    hipEvent_t begun(uint32_t i) const { return ev[4 + (i & 1u)]; }

    int start() {
        for (size_t i = 0; i < 6; ++i) ev[i] = get_event(c, i);
        for (hipEvent_t e : ev)
            if (!e) {
                set_error("hipEventCreate failed");
                return PT_ERR_HIP;
            }
        HIP_TRY(hipEventRecord(ev[0], st));
        return PT_OK;
    }

    // Before launch p: wait for what must have ended, look at the cancel byte, make the progress callback and size the launch
    // (s0, s_here).  kLaunch: issue it, then launched(); PT_OK: the frame is complete, or cancelled (`cancelled`).
    int next() {
        if (s_next >= cfg->spp) return PT_OK;
        if (one && p >= 1u) {
            HIP_TRY(hipEventSynchronize(done(p - 1u)));
            if (adaptive) {
                float ms = 0.0f;
                HIP_TRY(hipEventElapsedTime(&ms, begun(p - 1u), done(p - 1u)));
                if (ms > 0.0f) rate = (double)npix * s_prev / ms;
            }
        }
        if (p >= 2u) HIP_TRY(hipEventSynchronize(done(p)));
        cancelled = cancel && *cancel;
        // (the samples known to be done)
        if (!cancelled && cb && p >= (one ? 1u : 2u) &&
            progress(c, cfg, cb, user, one ? (float)s_next / (float)cfg->spp : (float)(p - 1u) / (float)n_pass))
            cancelled = cancel && *cancel;  // raised from inside the callback
        if (cancelled) return PT_OK;
        s0 = s_next;
        s_here = (cfg->spp - s0) < max_spp ? (cfg->spp - s0) : max_spp;
        if (adaptive) s_here = host::next_pass_samples(rate, kTargetMs, npix, kProbeRays, s_prev, cfg->spp - s0, max_spp);
        s_next = s0 + s_here;
        s_prev = s_here;
        c->live.spp_issued = s_next;
        if (adaptive) HIP_TRY(hipEventRecord(begun(p), st));
        return kLaunch;
    }

    int launched() {
        HIP_TRY(hipEventRecord(done(p), st));
        ++p;
        return PT_OK;
    }

    // After the last launch: wait for the frame.  The last launch's rate counts too (a frame of one probe and one long launch
    // would otherwise only know the probe) when it was long enough to measure.
    int finish() {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
        if (measured()) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, begun(p - 1u), done(p - 1u)));
            if (ms > 0.0f && (double)npix * s_prev >= 16.0 * (double)kProbeRays) rate = (double)npix * s_prev / ms;
        }
        return PT_OK;
    }

    // `rate` is one to keep with the context
    bool measured() const { return adaptive && p != 0u; }

    int frame_ms(double &out) const {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        out = ms;
        return PT_OK;
    }
};

// The device buffers of a wavefront frame planned as `plan`.  PT_ERR_NOMEM_INTERNAL: out of device memory.
static int ensure_pass_buffers(pt_ctx *c, const FrameForm &form, const host::FramePlan &plan) {
    const host::PassPlan &p = plan.pass;
    int rc = c->q_buf[0].ensure(p.bytes0 + plan.taper.extra0, true);
    if (!rc && p.bytes1) rc = c->q_buf[1].ensure(p.bytes1 + plan.taper.extra1, true);
    // only the three-kernel form needs the hit records: k_pass keeps hits in registers
    if (!rc && !form.one_kernel) rc = c->hit.ensure((size_t)p.K * p.cap, true);
    if (!rc) rc = c->cnt.ensure((size_t)kLevels * p.K, true);
    if (!rc) rc = c->flags.ensure(1, true);
    if (!rc) rc = c->blk_rays.ensure(p.K, true);
    if (!rc) rc = c->acc.ensure(3 * (size_t)p.K * p.m, true);
    return rc;
}

// Samples [s_first, cfg->spp) of every pixel of the part; the accumulators start from `held` (NULL: from zero).
int render_wavefront(pt_ctx *c, const FrameForm &form, const pt_config *cfg, const FrameParams &frame, hipStream_t st,
                     const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats &stats, uint32_t s_first,
                     const HeldSums *held) {
    const DevScene &S = form.scene;
    FrameParams F = frame;
    const uint64_t npix = F.npix;
    // THE FRAME'S PLAN - passes, streams, slices, k_pass_cand's taper - is host arithmetic (pt_host.h: first_request, plan_frame,
    // shrink_request).  A default pass is cut to what the DEVICE can give: the free memory plus what this context's queues hold
    // already, shared among the contexts of this call (PT_FLAG_PIPELINES, ranks of pt_render_multi on one GPU).
    host::FramePlanIn pin;
    pin.pass.npix = npix;
    pin.pass.spp = cfg->spp - s_first;  // samples per pixel this call traces
    pin.pass.stack_form = form.stack_form;
    pin.pass.stack_park = form.stack_park;
    pin.pass.cand_scan = S.cand_scan != 0u;
    pin.pass.has_bvh = S.n_bvh_nodes != 0u;
    pin.pass.streams = c->tune.streams;
    pin.pass.per_stream = c->tune.per_stream;
    pin.pass.wave_stack = c->tune.wave_stack;
    pin.pass.n_cus = c->n_cus;
    pin.rays_per_pass = cfg->rays_per_pass;
    pin.rays_per_pass_tuned = c->tune.rays_per_pass;
    pin.mem_budget = c->mem_budget;
    pin.mem_share = c->mem_share;
    pin.probe = F.probe != 0u;
    pin.taper_cut = c->tune.taper_cut;
    pin.taper_pieces = c->tune.taper_pieces;
    pin.scene = S;
    pin.lds_pad = c->tune.lds_pad;
    if (!pin.rays_per_pass && !pin.rays_per_pass_tuned && !pin.mem_budget) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess)
            pin.mem_avail = mem_free + c->hit.bytes() + c->q_buf[0].bytes() + c->q_buf[1].bytes();
    }
    host::FrameRequest req = host::first_request(pin);
    host::FramePlan plan;
    for (;;) {
        if (host::plan_frame(pin, req, plan) != host::kPlanOk) return refuse("rays per pass too large");
        const int rc = ensure_pass_buffers(c, form, plan);
        if (!rc) break;
        if (rc != PT_ERR_NOMEM_INTERNAL) return rc;
        // out of device memory: give back what this attempt took and ask for less
        for (int w = 0; w < 2; ++w) c->q_buf[w].release();
        c->hit.release();
        if (!host::shrink_request(pin, plan, req)) return PT_ERR_HIP;  // (the message names the allocation that failed)
    }
    const bool stack_form = form.stack_form, taper_forced = c->tune.taper_cut >= 0;
    const uint32_t spp_pass = plan.pass.spp_pass, m = plan.pass.m, K = plan.pass.K, cap = plan.pass.cap;
    const host::Taper &taper = plan.taper;
    F.n_streams = K;  // stream b owns pixels b, b+K, ...; accumulators are stream-major (K*m slots per channel)
    c->live.streams = K;
    c->live.m = m;
    const LdsLayout lay = lds_layout(S, m, c->tune.lds_pad);
    if (form.one_kernel && (S.n_bvh_nodes == 0u || S.cand_scan)) say_layout(c, lay, 0);
    if (!form.one_kernel && S.n_bvh_nodes == 0u && S.cand_scan) say_layout(c, lay, 1);
    if (held)
        launch_accum_gather(st, held->p, held->stride, (uint32_t)npix, K, m, c->acc.p);
    else
        HIP_TRY(hipMemsetAsync(c->acc.p, 0, 3 * (size_t)K * m * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(c->blk_rays.p, 0, K * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(c->flags.p, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(c->cnt.p, 0, (size_t)kLevels * K * sizeof(uint32_t), st));

    const int n_depth = kMaxDepth;  // rays of depth 0..11 exist
    // k_pass_cand's long passes: one in flight, and sized by time at the library's own pass size
    PassPacer pace(c, cfg, st, cancel, cb, user, npix, s_first, spp_pass, stack_form, stack_form && !c->tune.rays_per_pass,
                   c->pass_rate_kernel == form.kernel ? c->pass_rate : 0.0);
    int rc = pace.start();
    if (rc) return rc;
    const size_t ev_prof0 = 6;  // profiling events follow the pacer's
    size_t n_prof = 0;
    while ((rc = pace.next()) == PassPacer::kLaunch) {
        const uint32_t s0 = pace.s0, s_here = pace.s_here;
        // (a launch of fewer samples than pieces - the pacer's first, short ones - runs whole streams: the slices are there either way)
        const bool taper_now = taper.on() && (taper_forced || s_here >= taper.pieces);
        if (form.one_kernel) {  // the whole pass in one launch (k_pass)
            hipEvent_t a = nullptr, b = nullptr;
            if (c->profiling) {
                a = get_event(c, ev_prof0 + 2 * n_prof), b = get_event(c, ev_prof0 + 2 * n_prof + 1);
                if (!a || !b) {
                    set_error("hipEventCreate failed");
                    return PT_ERR_HIP;
                }
                HIP_TRY(hipEventRecord(a, st));
            }
            if (S.n_bvh_nodes != 0u && !S.cand_scan)
                launch_pass_bvh(st, K, S, F, queue_of(c, 0), queue_of(c, 1), cap, s0, s_here, m, c->acc.p, c->blk_rays.p, c->flags.p);
            else if (launch_pass(st, K, S, lay, F, queue_of(c, 0), queue_of(c, 1), cap, s0, s_here, m, c->acc.p, c->blk_rays.p,
                                 c->flags.p, taper_now ? taper.n_cut : 0u, taper_now ? taper.lg_pieces : 0u) != hipSuccess)
                return PT_ERR_HIP;  // (the message says how much LDS the scene's kernel asked for)
            if (c->profiling) {
                HIP_TRY(hipEventRecord(b, st));
                ++n_prof;
            }
        } else {
            launch_generate(st, K, F, queue_of(c, 0), c->cnt.p, cap, s0, s_here, m);
            for (int d = 0; d < n_depth; ++d) {
                const RayQueue qin = queue_of(c, d & 1), qout = queue_of(c, (d + 1) & 1);
                if (c->profiling) {
                    hipEvent_t a = get_event(c, ev_prof0 + 2 * n_prof), b = get_event(c, ev_prof0 + 2 * n_prof + 1);
                    if (!a || !b) {
                        set_error("hipEventCreate failed");
                        return PT_ERR_HIP;
                    }
                    HIP_TRY(hipEventRecord(a, st));
                    launch_intersect(st, K, S, lay, qin, c->hit.p, c->cnt.p + (size_t)d * K, cap, c->blk_rays.p);
                    HIP_TRY(hipEventRecord(b, st));
                    ++n_prof;
                } else {
                    launch_intersect(st, K, S, lay, qin, c->hit.p, c->cnt.p + (size_t)d * K, cap, c->blk_rays.p);
                }
                launch_shade(st, K, S, F, qin, qout, c->hit.p, c->cnt.p + (size_t)d * K, c->cnt.p + (size_t)(d + 1) * K, cap,
                             c->acc.p, c->flags.p, m, s0);
            }
        }
        if ((rc = pace.launched())) return rc;
    }
    if (rc || (rc = pace.finish())) return rc;
    if (pace.measured()) {
        c->pass_rate = pace.rate;
        c->pass_rate_kernel = form.kernel;
    }
    std::vector<unsigned long long> rays(K);
    HIP_TRY(hipMemcpy(rays.data(), c->blk_rays.p, K * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint32_t flags = 0;
    HIP_TRY(hipMemcpy(&flags, c->flags.p, sizeof flags, hipMemcpyDeviceToHost));
    unsigned long long total = 0;
    for (auto v : rays) total += v;
    stats.ray_bounces = total;
    stats.intersect_rays = total;
    stats.intersect_launches = form.one_kernel ? pace.p : pace.p * (uint32_t)n_depth;
    stats.passes = pace.p;
    stats.samples = npix * (uint64_t)(pace.s_next - s_first);  // (every pass that was issued has run: the stream is synchronised)
    if ((rc = pace.frame_ms(stats.ms_device))) return rc;
    double mi = 0.0;
    for (size_t i = 0; i < n_prof; ++i) {
        float e = 0.0f;
        HIP_TRY(hipEventElapsedTime(&e, c->ev_pool[ev_prof0 + 2 * i], c->ev_pool[ev_prof0 + 2 * i + 1]));
        mi += e;
    }
    stats.ms_intersect = mi;
    if (flags & 3u) {
        set_error((flags & 2u) ? "ray stream slices too small for k_pass_cand's wave stacks" : "ray stream overflow");
        return PT_ERR_OVERFLOW;
    }
    if (pace.cancelled) {
        set_error("cancelled");
        return PT_CANCELLED;
    }
    return PT_OK;
}

// Samples [s_first, cfg->spp) of `entries` items in ROUNDS (host::plan_rounds), for the kernels that hand (item, sample range)
// pieces out from a counter: the megakernel (an item is a pixel of the part) and the tile pass (an entry of the compact
// accumulator).  A round is one launch, sized to about a tenth of a second - it follows the scene as k_pass_cand's passes do
// (PassPacer, from `rate`, which is brought up to date) unless cfg->rays_per_pass sizes it - so cancel and cb (either may be NULL)
// are served between launches (the reference polls cancel every 100 ms, mod.rs:947-958) and every item holds the same number of
// samples at every boundary: what pt_ctx_snapshot and a cancelled frame resolve.  Before each launch counters[7], the kernels'
// item counter, is zeroed and the split stacks (mega_cand) cover the grid; launch(grid, s0, s_end, lane_spp, split) issues it.
struct Rounds {
    uint32_t launches = 0, s_issued = 0;  // launches issued; samples [s_first, s_issued) of every item have run
    bool cancelled = false;
    double ms_device = 0.0;  // first to last launch
};
template <class Launch>
int run_rounds(pt_ctx *c, const pt_config *cfg, hipStream_t st, const volatile uint8_t *cancel, pt_progress_fn cb, void *user,
               uint64_t entries, uint32_t s_first, bool mega_cand, uint32_t item_mult, unsigned long long *counters, DevBuf<char> &stacks,
               double &rate, Launch launch, Rounds &out) {
    const host::RoundPlan plan = host::plan_rounds(entries, cfg->spp - s_first, cfg->rays_per_pass, item_mult, c->n_cus);
    PassPacer pace(c, cfg, st, cancel, cb, user, entries, s_first, plan.round_spp, false, true, rate);
    int rc = pace.start();
    if (rc) return rc;
    while ((rc = pace.next()) == PassPacer::kLaunch) {
        const host::RoundLaunch l = host::round_launch(entries, plan.n_split, pace.s_here, c->n_cus);
        if (mega_cand && (rc = stacks.ensure(mega_stack_mem_bytes(l.grid)))) return rc;
        HIP_TRY(hipMemsetAsync(counters + 7, 0, sizeof(unsigned long long), st));
        launch(l.grid, pace.s0, pace.s0 + pace.s_here, l.lane_spp, l.split);
        if ((rc = pace.launched())) return rc;
    }
    if (rc || (rc = pace.finish())) return rc;
    if (pace.measured()) rate = pace.rate;
    out.launches = pace.p;
    out.s_issued = pace.s_next;
    out.cancelled = pace.cancelled;
    return pace.frame_ms(out.ms_device);
}

// Samples [s_first, cfg->spp) of every pixel of the part; the accumulators start from `held` (NULL: from zero).
int render_mega(pt_ctx *c, const FrameForm &form, const pt_config *cfg, const FrameParams &F, hipStream_t st,
                const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats &stats, uint32_t s_first,
                const HeldSums *held) {
    const DevScene &S = form.scene;
    const uint64_t npix = F.npix;
    int rc;
    if ((rc = c->acc.ensure(3 * npix)) || (rc = c->total_rays.ensure(16))) return rc;
    c->live.streams = 1;  // accumulators in pixel order
    c->live.m = (uint32_t)npix;
    if (held)
        launch_accum_gather(st, held->p, held->stride, (uint32_t)npix, 1u, (uint32_t)npix, c->acc.p);
    else
        HIP_TRY(hipMemsetAsync(c->acc.p, 0, 3 * npix * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(c->total_rays.p, 0, 16 * sizeof(unsigned long long), st));
    const LdsLayout lay = lds_layout(S, 1u, c->tune.lds_pad);
    say_layout(c, lay, 2);
    // (PT_MEGA_ITEMS for A/B runs and tests)
    const uint32_t item_mult = c->tune.mega_items ? c->tune.mega_items : (lay.mega_cand ? 8u : 4u);
    Rounds r;
    rc = run_rounds(
        c, cfg, st, cancel, cb, user, npix, s_first, lay.mega_cand, item_mult, c->total_rays.p, c->q_buf[0], c->round_rate,
        [&](uint32_t grid, uint32_t s0, uint32_t s_end, uint32_t lane_spp, uint32_t split) {
            launch_mega(st, grid, S, lay, F, c->acc.p, s0, s_end, lane_spp, split, c->total_rays.p, c->q_buf[0].p);
        },
        r);
    if (rc) return rc;
    unsigned long long total2[16] = {0};
    HIP_TRY(hipMemcpy(total2, c->total_rays.p, sizeof total2, hipMemcpyDeviceToHost));
#ifdef PT_MEGA_STATS
    fprintf(stderr, "mega stats: trips %llu, started per trip %.2f, finished per trip %.2f, maker iterations %llu (per trip %.3f) at %.1f lanes\n",
            total2[2], (double)total2[3] / (double)(total2[2] ? total2[2] : 1), (double)total2[4] / (double)(total2[2] ? total2[2] : 1), total2[5],
            (double)total2[5] / (double)(total2[2] ? total2[2] : 1), (double)total2[6] / (double)(total2[5] ? total2[5] : 1));
    fprintf(stderr, "mega stats: lanes with an item %.2f, of them dry (no ray to start, samples used up) %.2f, lanes told no more %.2f per trip\n",
            (double)total2[8] / (double)(total2[2] ? total2[2] : 1), (double)total2[9] / (double)(total2[2] ? total2[2] : 1),
            (double)total2[10] / (double)(total2[2] ? total2[2] : 1));
#endif
    if (total2[1]) {
        set_error("megakernel: a lane's split stack overflowed");
        return PT_ERR_OVERFLOW;
    }
    stats.ray_bounces = total2[0];
    stats.intersect_rays = 0;
    stats.intersect_launches = 0;
    stats.passes = r.launches;
    stats.samples = npix * (uint64_t)(r.s_issued - s_first);
    stats.ms_device = r.ms_device;
    stats.ms_intersect = 0.0;
    if (r.cancelled) {
        set_error("cancelled");
        return PT_CANCELLED;
    }
    return PT_OK;
}

// The checkpoint's scene fingerprint: SipHash-1-3 (zero key) over n_objs, n_tris (u32 each), then the camera, the objects and
// the triangles as pt_ctx_set_scene got them
uint64_t scene_fingerprint(const pt_camera *cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris) {
    std::vector<uint8_t> b(8 + sizeof(pt_camera) + (size_t)n_objs * sizeof(pt_object) + (size_t)n_tris * sizeof(pt_triangle));
    uint8_t *w = b.data();
    memcpy(w, &n_objs, 4);
    memcpy(w + 4, &n_tris, 4);
    w += 8;
    memcpy(w, cam, sizeof(pt_camera));
    w += sizeof(pt_camera);
    if (n_objs) memcpy(w, objs, (size_t)n_objs * sizeof(pt_object));
    w += (size_t)n_objs * sizeof(pt_object);
    if (n_tris) memcpy(w, tris, (size_t)n_tris * sizeof(pt_triangle));
    return pt_siphash(1, 3, 0, 0, b.data(), b.size());
}

// The fingerprint pt_ctx_set_scene would give for the context's camera and scene: pt_ctx_set_camera only marks it stale, the first
// checkpoint call afterwards hashes the kept host copies
uint64_t scene_fp_of(pt_ctx *c) {
    if (c->fp_stale) {
        c->scene_fp = scene_fingerprint(&c->cam, c->h_objs.data(), (uint32_t)c->h_objs.size(), c->h_tris.data(), (uint32_t)c->h_tris.size());
        c->fp_stale = false;
    }
    return c->scene_fp;
}

// resolve part `i` of the held sums into the call's output: over its own count, black at 0
int accum_resolve_part(const HeldFrame &h, uint32_t i, float *out, hipStream_t st) {
    const host::Part p = h.part(i);
    if (h.cnt[i] != 0u)
        launch_resolve(st, h.sums.p + p.k0, out + (size_t)p.k0 * 3, p.n, h.cnt[i], 1u, h.total);
    else
        HIP_TRY(hipMemsetAsync(out + (size_t)p.k0 * 3, 0, (size_t)p.n * 3 * sizeof(float), st));
    return PT_OK;
}

using host::Job;  // one piece of a frame call (pt_host.h); pt_ctx_accumulate's start from the held sums of their pixels

void add_stats(pt_stats *stats, const pt_stats &s) {
    stats->ray_bounces += s.ray_bounces;
    stats->samples += s.samples;
    stats->intersect_rays += s.intersect_rays;
    stats->intersect_launches += s.intersect_launches;
    stats->passes += s.passes;
    stats->ms_device += s.ms_device;
    stats->ms_intersect += s.ms_intersect;
}

// the stats of pipelines or ranks that ran side by side: summed, but the device time of the call is the longest of theirs
void add_stats_concurrent(pt_stats *stats, const std::vector<pt_stats> &each) {
    double longest = stats->ms_device;
    for (const pt_stats &s : each) {
        add_stats(stats, s);
        longest = s.ms_device > longest ? s.ms_device : longest;
    }
    stats->ms_device = longest;
}

// pt_ctx_render after a job: its part resolved into the call's output over the samples per pixel it accumulated.  A
// cancelled part is resolved over the samples that were issued (live.spp_issued, also reported through stats->samples):
// every pixel at full brightness over fewer samples - the same picture pt_ctx_snapshot gives.  (The reference's partial
// image has finished pixels at full spp and the rest black; a GPU pass covers every pixel, so "fewer samples everywhere" is
// its counterpart.)  Nothing accumulated yet: all zero, as the reference's untouched `pixels` vector; so are the parts that
// were never started.
int resolve_job(pt_ctx *c, const pt_config *cfg, const Job &j, int rc, hipStream_t st) {
    float *out_p = c->live.out + (size_t)j.k0 * 3;
    const uint32_t spp_done = rc == PT_OK ? cfg->spp : c->live.spp_issued;
    if (spp_done != 0u)
        launch_resolve(st, c->acc.p, out_p, j.n, spp_done, c->live.streams, c->live.m);
    else
        HIP_TRY(hipMemsetAsync(out_p, 0, (size_t)j.n * 3 * sizeof(float), st));
    if (rc == PT_CANCELLED && j.k0 + j.n < c->live.total)  // the parts that were never started
        HIP_TRY(hipMemsetAsync(out_p + (size_t)j.n * 3, 0, (size_t)(c->live.total - j.k0 - j.n) * 3 * sizeof(float), st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// pt_ctx_accumulate after a job: what it traced joins the held sums (every pass that was issued has run: the renderers
// synchronise the stream), and its parts' counts follow
int keep_job(pt_ctx *c, const pt_config *cfg, const Job &j, int rc, hipStream_t st) {
    const uint32_t done = rc == PT_OK ? cfg->spp : c->live.spp_issued;
    if (done <= j.s_first) return rc;
    const uint64_t slots = (uint64_t)c->live.streams * c->live.m;
    if (slots < j.n || slots > 0xffffffffull) {
        set_error("accumulator layout does not cover the part");
        return PT_ERR_HIP;
    }
    // A noise-tracked frame deals the samples of a job to the half that holds fewer of them in its part (a tie: to A); the
    // parts of one job hold the same counts.  Half B is never stored: a job that goes to it only moves the counts.
    HeldFrame &h = c->held;
    const bool to_a = h.tracked() && host::deal_to_a(h.cnt[j.part_lo], h.na[j.part_lo]);
    if (to_a)
        launch_accum_scatter_half(st, c->acc.p, j.n, c->live.streams, c->live.m, h.sums.p + j.k0, h.a.p + j.k0, h.total);
    else
        launch_accum_scatter(st, c->acc.p, j.n, c->live.streams, c->live.m, h.sums.p + j.k0, h.total);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error(std::string("storing the held sums: ") + hipGetErrorString(e));
        h.drop();  // (their state is unknown)
        return PT_ERR_HIP;
    }
    for (uint32_t i = j.part_lo; i < j.part_hi; ++i) {
        if (to_a) h.na[i] += done - j.s_first;
        h.cnt[i] = done;
    }
    return rc;
}

// pt_ctx_accumulate's output at the end of the call: every part over its own count
int resolve_held(pt_ctx *c, float *out, hipStream_t st, int rc) {
    for (uint32_t i = 0; i < c->held.n_parts(); ++i) {
        const int r2 = accum_resolve_part(c->held, i, out, st);
        if (r2) {
            rc = r2;
            break;
        }
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess && (rc == PT_OK || rc == PT_CANCELLED)) {
        set_error(std::string("resolving the held sums: ") + hipGetErrorString(e));
        rc = PT_ERR_HIP;
    }
    if (rc == PT_CANCELLED) set_error("cancelled");
    return rc;
}

// The driver of pt_ctx_render and pt_ctx_accumulate: the call's jobs in order on one form of cfg->flags, into `out` (`total`
// pixels; F: the call's frame).  After each job its part is resolved into the output (pt_ctx_render) or its sums are kept
// (pt_ctx_accumulate, which resolves every part at the end).
int run_frame_call(pt_ctx *c, const pt_config *cfg, const FrameParams &F, const std::vector<Job> &jobs, bool accumulate,
                   float *out, uint32_t total, hipStream_t st, const volatile uint8_t *cancel, pt_progress_fn cb, void *user,
                   pt_stats *stats) {
    const double t0 = now_ms();
    const FrameForm form = form_for(c, cfg->flags);
    Relay relay{cb, user};  // a job's fractions as fractions of the call; its completion is reported by the next job / the end
    LiveScope live(c);
    c->live.out = out;
    c->live.total = total;
    c->live.stream = st;
    c->live.accum = accumulate;
    int rc = PT_OK;
    bool started = false;
    for (const Job &j : jobs) {
        pt_config jcfg = *cfg;  // the job's own last sample (a noise-tracked call cuts a part's samples into two jobs)
        if (j.s_end) jcfg.spp = j.s_end;
        if (j.s_first >= jcfg.spp) continue;  // nothing left to trace here
        // a job boundary is a progress point of its own (a part of one or two passes makes no callback from inside); a cancel
        // raised there is seen by the job's first pass, which leaves it and the parts behind it black
        if (cb && started) progress(c, cfg, cb, user, j.boundary >= 0.0f ? j.boundary : j.base);
        started = true;
        FrameParams Fj = F;
        Fj.k_begin = j.k0;
        Fj.npix = j.n;
        c->live.k0 = j.k0;
        c->live.npix = j.n;
        c->live.spp_issued = j.s_first;
        relay.base = j.base;
        relay.scale = j.scale;
        pt_stats js{};
        HeldSums held{nullptr, 0u};  // pt_ctx_accumulate: the job starts from the held sums of its pixels
        if (accumulate) held = {c->held.sums.p + j.k0, c->held.total};
        rc = (cfg->backend == PT_BACKEND_WAVEFRONT ? render_wavefront : render_mega)(
            c, form, &jcfg, Fj, st, cancel, cb ? &Relay::fn : nullptr, &relay, js, j.s_first, accumulate ? &held : nullptr);
        if (rc == PT_OK || rc == PT_CANCELLED) rc = accumulate ? keep_job(c, &jcfg, j, rc, st) : resolve_job(c, &jcfg, j, rc, st);
        if (stats) add_stats(stats, js);
        if (rc != PT_OK) break;
    }
    if (accumulate && (rc == PT_OK || rc == PT_CANCELLED)) rc = resolve_held(c, out, st, rc);
    if (cb && rc == PT_OK) cb(user, 1.0f);
    if (stats) stats->ms_total = now_ms() - t0;
    return rc;
}

// The prologue of a frame call: a scene, a valid cfg (its band in *ib, *ie), the context's device current
int frame_prologue(pt_ctx *c, const pt_config *cfg, uint32_t *ib, uint32_t *ie) {
    if (!c->has_scene) return refuse("no scene set");
    const int rc = check_cfg(cfg, ib, ie);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return PT_OK;
}

// One run of a step of pt_ctx_accumulate_adaptive: samples [s_first, s_end) of every open tile into the compact accumulator (zeroed
// here), in the megakernel's rounds at a rate of their own.  The cancel byte is the step loop's business, not the rounds'.
int tile_run(pt_ctx *c, const DevScene &S, const LdsLayout &lay, const pt_config *cfg, TileParams F, uint32_t n_open, uint32_t s_first,
             uint32_t s_end, hipStream_t st, pt_stats &stats) {
    const uint64_t entries = (uint64_t)n_open << (2u * F.tile_shift);
    F.npix = (uint32_t)entries;
    int rc = c->ad_acc.ensure(3 * entries);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->ad_acc.p, 0, 3 * entries * sizeof(unsigned long long), st));
    pt_config run = *cfg;
    run.spp = s_end;
    Rounds r;
    rc = run_rounds(
        c, &run, st, nullptr, nullptr, nullptr, entries, s_first, lay.mega_cand, lay.mega_cand ? 8u : 4u, c->ad_rays.p, c->ad_stack, c->ad_rate,
        [&](uint32_t grid, uint32_t s0, uint32_t s1, uint32_t lane_spp, uint32_t split) {
            launch_tile_pass(st, grid, S, lay, F, c->ad_acc.p, s0, s1, lane_spp, split, c->ad_rays.p, c->ad_stack.p);
        },
        r);
    stats.passes += r.launches;
    return rc;
}

// the key of the held adaptive frame a checked call names (b, e: check_cfg's band)
host::AdaptiveKey adaptive_key(const pt_config *cfg, uint32_t b, uint32_t e, uint32_t tile_shift, uint32_t min_spp) {
    return {host::accum_key(cfg, b, e), 1u << tile_shift, host::adaptive_n0(min_spp)};
}

TileGrid tile_grid(const HeldAdaptive &h) {
    TileGrid G{};
    G.width = h.key.frame.width;
    G.rows = h.total / G.width;
    G.tile_shift = h.geo.tile_shift;
    G.tiles_x = h.geo.tiles_x;
    G.tiles = h.geo.tiles;
    G.spp = h.cnt.p;
    G.na = h.na.p;
    G.err = h.err.p;
    return G;
}

unsigned long long tile_threshold(float tile_error) { return (unsigned long long)__builtin_floor((double)tile_error * 268435456.0); }

// pt_ctx_accumulate_adaptive after its refusals about the arguments: the band [ib, ie) of a checked cfg in tiles of 1 <<
// tile_shift.  The held frame of this key (or a new one, from zero) is re-decided under this call's target and cap and taken on
// step by step - host::AdaptiveSchedule says which class is next, k_tile_select finds its tiles, a step's two runs are
// host::tracked_split's - then the outputs are written from what is held.
int accumulate_adaptive(pt_ctx *c, const pt_config *cfg, uint32_t ib, uint32_t ie, uint32_t tile_shift, const pt_adaptive_params *params,
                        float *d_out_rgb, uint32_t *d_spp, float *d_error, hipStream_t st, const volatile uint8_t *cancel,
                        pt_progress_fn cb, void *user, pt_stats *stats, pt_adaptive_stats *astats) {
    const double t0 = now_ms();
    if (stats) memset(stats, 0, sizeof *stats);
    memset(astats, 0, sizeof *astats);
    pt_stats ps{};
    const FrameForm form = form_for(c, cfg->flags);
    const DevScene &S = form.scene;
    const LdsLayout lay = lds_layout(S, 1u, c->tune.lds_pad);
    const uint32_t npix = ie - ib;
    host::TileGeometry geo;
    int rc = host::tile_geometry(cfg->width, npix / cfg->width, tile_shift, geo);
    if (rc) return rc;
    HeldAdaptive &h = c->adaptive;
    const host::AdaptiveKey key = adaptive_key(cfg, ib, ie, tile_shift, params->min_spp);
    host::TileTable tab;  // the tiles' state at the start of the call: all the scheduler ever learns about single tiles
    if (h.holds(key)) {
        if ((rc = h.download(tab, st))) return rc;
    } else {  // another frame (or none): from zero
        host::AdaptiveFrame f;
        f.key = key;
        f.total = npix;
        f.tiles = geo.tiles;
        if ((rc = h.start(f, geo, nullptr, nullptr, nullptr, st))) return rc;
        tab.cnt.assign(geo.tiles, 0u);
        tab.na.assign(geo.tiles, 0u);
        tab.err.assign(geo.tiles, kTileNoError);
    }
    const TileGrid G = tile_grid(h);
    TileParams F{};
    static_cast<FrameParams &>(F) = make_frame(c, cfg, ib, ie);
    F.chunk_step = 0u;
    F.tile_shift = G.tile_shift;
    F.tiles_x = G.tiles_x;
    F.rows = G.rows;
    if (c->ad_open.n < G.tiles) {  // (a slot of the list names a tile whatever a launch reads of it)
        if ((rc = c->ad_open.ensure(G.tiles))) return rc;
        HIP_TRY(hipMemsetAsync(c->ad_open.p, 0, (size_t)G.tiles * sizeof(uint32_t), st));
    }
    if ((rc = c->ad_cnt.ensure(4)) || (rc = c->ad_rays.ensure(16))) return rc;
    F.open = c->ad_open.p;
    uint32_t *const words = reinterpret_cast<uint32_t *>(c->ad_cnt.p);
    hipEvent_t ev0 = get_event(c, 6), ev1 = get_event(c, 7);  // (0..5 are the rounds' pacer's)
    if (!ev0 || !ev1) {
        set_error("hipEventCreate failed");
        return PT_ERR_HIP;
    }
    HIP_TRY(hipEventRecord(ev0, st));
    HIP_TRY(hipMemsetAsync(c->ad_rays.p, 0, 16 * sizeof(unsigned long long), st));
    LiveScope live(c);  // (the rounds' pacer notes its samples in the live frame)
    const uint32_t cap = cfg->spp;
    const unsigned long long q = tile_threshold(params->tile_error);
    host::AdaptiveSchedule sched(tab, G.width, G.rows, geo, q, cap, key.n0);
    uint64_t held_before = 0;
    for (uint32_t i = 0; i < geo.tiles; ++i) held_before += host::tile_pixels(G.width, G.rows, geo, i) * tab.cnt[i];
    uint64_t samples = std::min<uint64_t>(held_before, (uint64_t)npix * cap);
    bool cancelled = false;
    astats->tiles = G.tiles;
    host::AdaptiveStep s;
    // an error inside a step leaves sums without their counts: the frame is not held any more
    auto broken = [&](int code) {
        h.forget();
        return code;
    };
    for (uint32_t j = 0; sched.next(s); ++j) {
        cancelled = cancel && *cancel;
        if (!cancelled && cb && j != 0u && progress(c, cfg, cb, user, (float)((double)samples / ((double)npix * cap))))
            cancelled = cancel && *cancel;  // raised from inside the callback
        if (cancelled) break;
        HIP_TRY(hipMemsetAsync(c->ad_cnt.p + 1, 0, 3 * sizeof(unsigned long long), st));
        TileSelect sel{};
        sel.q = q;
        sel.cap = cap;
        sel.c = s.c;
        sel.na = s.na;
        sel.list = c->ad_open.p;
        sel.list_len = words + 4;
        sel.out = words + 5;
        launch_tile_select(st, G, sel);
        const uint32_t n_b = s.T - s.na_end;
        TileLevel V{};
        V.open = F.open;
        V.n_open = s.n;
        V.spp = s.T;
        V.na = s.na_end;
        V.q = q;
        V.counters = words + 2;
        V.fa = (float)s.na_end;
        V.fb = (float)n_b;
        V.fn = (float)s.T;
        V.w = n_b != 0u ? host::noise_part_weight(s.na_end, n_b) : 0.0f;
        for (uint32_t run = 0; run < s.runs(); ++run) {
            const uint32_t r0 = run ? s.m : s.c, r1 = run ? s.T : s.m;
            if ((rc = tile_run(c, S, lay, cfg, F, s.n, r0, r1, st, ps))) return broken(rc);
            V.acc = c->ad_acc.p;
            V.to_a = s.to_a[run] ? 1u : 0u;
            V.evaluate = r1 == s.T ? 1u : 0u;
            V.estimate = V.evaluate && n_b != 0u ? 1u : 0u;
            launch_tile_level(st, G, V, h.sums.p, h.a.p);
        }
        uint32_t back[2] = {0u, 0u};  // the tiles the step left open, the tiles it closed: all that comes back per step
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(back, words + 2, sizeof back, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            set_error(std::string("a step of the adaptive frame: ") + hipGetErrorString(e));
            return broken(PT_ERR_HIP);
        }
        if (back[0] + back[1] != s.n) {
            set_error("the adaptive frame's tiles and the host's count of them disagree");
            return broken(PT_ERR_HIP);
        }
        // (partial tiles counted whole: this only feeds the progress fraction; the exact total comes from the counts at the end)
        samples += ((uint64_t)s.n << (2u * G.tile_shift)) * (s.T - s.c);
        if (samples > (uint64_t)npix * cap) samples = (uint64_t)npix * cap;
        if (j < 32u) {
            astats->level_spp[j] = s.T;
            astats->tiles_closed[j] = back[1];
            astats->levels = j + 1u;
        }
        sched.done(s, back[0], back[1]);
    }
    astats->tiles_open = sched.tiles_open();
    // the outputs: every pixel over its tile's count, the counts, the error map, the sum of E over the tiles
    HIP_TRY(hipMemsetAsync(c->ad_cnt.p, 0, sizeof(unsigned long long), st));
    launch_tile_resolve(st, G, h.sums.p, h.a.p, d_out_rgb, d_spp, d_error, c->ad_cnt.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, st));
    unsigned long long err_sum = 0, rays[16] = {0};
    HIP_TRY(hipMemcpyAsync(&err_sum, c->ad_cnt.p, sizeof err_sum, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rays, c->ad_rays.p, sizeof rays, hipMemcpyDeviceToHost, st));
    if ((rc = h.download(tab, st))) return rc;
    if (rays[1]) {
        set_error("tile pass: a lane's split stack overflowed");
        return broken(PT_ERR_OVERFLOW);
    }
    const host::TileTotals tot = host::tile_totals(G.width, G.rows, geo, tab.cnt.data(), tab.err.data(), err_sum);
    astats->samples = tot.samples;
    astats->mean_error = tot.mean_error;
    ps.samples = tot.samples - held_before;
    ps.ray_bounces = rays[0];
    float ms_dev = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms_dev, ev0, ev1));
    ps.ms_device = ms_dev;
    ps.ms_total = now_ms() - t0;
    if (stats) *stats = ps;
    if (cancelled) {
        set_error("cancelled");
        return PT_CANCELLED;
    }
    if (cb) cb(user, 1.0f);
    return PT_OK;
}

// the refusals of the adaptive calls that name a frame by cfg and params, in the header's order, up to the band: no device is touched
int adaptive_prologue(pt_ctx *c, const pt_config *cfg, const pt_adaptive_params *params, uint32_t *tile_shift, uint32_t *ib, uint32_t *ie) {
    int rc = host::check_adaptive_params(*params, tile_shift);
    if (rc) return rc;
    if (!c) return refuse("ctx is NULL");
    if (!c->has_scene) return refuse("no scene set");
    if ((rc = host::check_adaptive_cfg(*cfg)) || (rc = check_cfg(cfg, ib, ie))) return rc;
    return PT_OK;
}

// a file written next to its target and renamed over it: a process that dies while saving leaves the last checkpoint whole
int write_renamed(const std::vector<uint8_t> &b, const char *path) {
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) {
        set_error(std::string("cannot open ") + tmp + " for writing: " + strerror(errno));
        return PT_ERR_IO;
    }
    const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
    if (fclose(f) != 0 || !ok) {
        set_error(std::string("cannot write ") + tmp);
        remove(tmp.c_str());
        return PT_ERR_IO;
    }
    if (rename(tmp.c_str(), path) != 0) {
        set_error(std::string("cannot rename ") + tmp + " to " + path + ": " + strerror(errno));
        remove(tmp.c_str());
        return PT_ERR_IO;
    }
    return PT_OK;
}

// A checkpoint file read as its decoder asks for it - the header first, the rest only once the file's size is the one the header
// implies - into b and ck.  decode: host::ckpt_decode or host::adckpt_decode.
template <class Ckpt, class Decode>
int read_checkpoint(const char *path, Decode decode, Ckpt &ck, std::vector<uint8_t> &b) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        set_error(std::string("cannot open ") + path + ": " + strerror(errno));
        return PT_ERR_IO;
    }
    struct Closer {
        FILE *f;
        ~Closer() { fclose(f); }
    } closer{f};
    if (fseeko(f, 0, SEEK_END) != 0) {
        set_error(std::string("cannot read ") + path);
        return PT_ERR_IO;
    }
    const off_t fsize = ftello(f);
    if (fsize < 0 || fseeko(f, 0, SEEK_SET) != 0) {
        set_error(std::string("cannot read ") + path);
        return PT_ERR_IO;
    }
    std::string why;
    int d;
    while ((d = decode((uint64_t)fsize, b.data(), b.size(), ck, why)) == host::kCkptMore) {
        const size_t at = b.size();
        b.resize(ck.need);
        if (fread(b.data() + at, 1, ck.need - at, f) != ck.need - at) {
            set_error(std::string("cannot read ") + path);
            return PT_ERR_IO;
        }
    }
    if (d != host::kCkptOk) {
        set_error(std::string(path) + " is not a checkpoint of this library: " + why);
        return PT_ERR_PARSE;
    }
    return PT_OK;
}

// pt_ctx_accum_save's and pt_ctx_adaptive_save's steps behind the file's head in b (the context's device is current): the planes
// (half A's when with_a), the seal, the file written beside `path` and renamed
int save_checkpoint(std::vector<uint8_t> &b, const HeldPlanes &h, uint32_t total, bool with_a, const char *path) {
    const size_t at = b.size(), plane = 3 * (size_t)total * sizeof(unsigned long long);
    b.resize(at + (with_a ? 2u : 1u) * plane);
    HIP_TRY(hipMemcpy(b.data() + at, h.sums.p, plane, hipMemcpyDeviceToHost));
    if (with_a) HIP_TRY(hipMemcpy(b.data() + at + plane, h.a.p, plane, hipMemcpyDeviceToHost));
    host::ckpt_seal(b);
    return write_renamed(b, path);
}

// pt_ctx_accum_load's and pt_ctx_adaptive_load's steps up to "the file is decoded into ck and b, it belongs to this context's
// scene, and the device is current": nothing the context holds is touched
template <class Ckpt, class Decode>
int load_checkpoint(pt_ctx *c, const char *path, Decode decode, Ckpt &ck, std::vector<uint8_t> &b) {
    if (!c || !path) return refuse("NULL argument");
    if (!c->has_scene) return refuse("no scene set: a checkpoint is loaded under the scene it was rendered from");
    const int rc = read_checkpoint(path, decode, ck, b);
    if (rc) return rc;
    if (ck.scene_fp != scene_fp_of(c)) {
        set_error(std::string(path) + " was rendered from another scene than the one set on this context");
        return PT_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    return PT_OK;
}

// An image pass once its arguments are checked (host::check_*: everything that can be refused is refused there, before the device is
// touched): the context's device is made current, the pass runs on the caller's stream or the context's - launch(st) grows what
// scratch it needs and issues the kernels; its error is the call's - and the call waits for it.
template <class Launch>
int run_image_pass(pt_ctx *c, void *hip_stream, Launch launch) {
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int rc = launch(st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

// A host-array query once its arguments are checked: host arrays staged on the device, one launch, the results copied back.  The
// context's device is made current, and every copy, clear and the launch go to the context's stream in the order they are asked for.
// The FIRST failure - a buffer's (DevBuf::ensure's code and message) or HIP's ("<call>: <what HIP says>", PT_ERR_HIP) - is the
// call's, and every step after it does nothing.  finish() waits for the stream whenever anything was issued on it, failure or not:
// the copies read and write the CALLER's arrays, which are the caller's again the moment the call returns.
class HostCall {
   public:
    HostCall(pt_ctx *c, const char *name) : name_(name), st_(c->stream) { hip(hipSetDevice(c->device)); }
    HostCall(const HostCall &) = delete;
    bool ok() const { return rc_ == PT_OK; }
    // a buffer of at least `count` records, cleared if asked
    template <class T>
    void room(DevBuf<T> &b, size_t count, bool zero = false) {
        if (ok()) rc_ = b.ensure(count);
        if (ok() && zero) issued(hipMemsetAsync(b.p, 0, count * sizeof(T), st_));
    }
    // ... filled with the host's
    template <class T>
    void in(DevBuf<T> &b, const T *src, size_t count) {
        room(b, count);
        if (ok()) issued(hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, st_));
    }
    // launch(stream): the call's kernel; what the launch itself reports is picked up here, before any result is copied
    template <class Launch>
    void run(Launch launch) {
        if (!ok()) return;
        launch(st_);
        issued(hipGetLastError());
    }
    // the buffer's first `count` records to the host (NULL: an output the caller did not ask for)
    template <class T>
    void out(T *dst, const DevBuf<T> &b, size_t count) {
        if (dst && ok()) issued(hipMemcpyAsync(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost, st_));
    }
    int finish() {
        if (issued_) {
            const hipError_t e = hipStreamSynchronize(st_);
            if (ok()) hip(e);
        }
        return rc_;
    }

   private:
    void hip(hipError_t e) {
        if (e == hipSuccess) return;
        set_error(std::string(name_) + ": " + hipGetErrorString(e));
        rc_ = PT_ERR_HIP;
    }
    void issued(hipError_t e) {
        issued_ = true;
        hip(e);
    }
    const char *name_;
    hipStream_t st_;
    int rc_ = PT_OK;
    bool issued_ = false;
};

// pt_*_defaults: the values a zero field of a pass's parameters stands for
template <class Params>
int give_defaults(Params *out, const Params &defaults) {
    if (!out) return refuse("out is NULL");
    *out = defaults;
    return PT_OK;
}

}  // namespace

extern "C" {

const char *pt_version(void) { return "ptrace-hip 0.3 (gfx950)"; }
#ifndef PT_BUILD_FLAGS
#define PT_BUILD_FLAGS ""
#endif
const char *pt_build_flags(void) { return PT_BUILD_FLAGS; }
const char *pt_last_error(void) { return g_last_error.c_str(); }
int pt_abi_version(void) { return PT_ABI_VERSION; }
int pt_device_count(void) { return device_count_quiet(); }

uint32_t pt_config_pixels(const pt_config *cfg) {
    uint32_t b = 0, e = 0;
    if (check_cfg(cfg, &b, &e) != PT_OK) return 0;
    return owned_pixels(cfg, b, e);
}

int pt_camera_basis(const pt_camera *cam, float lens_center[3], float su[3], float sv[3]) {
    if (!cam || !lens_center || !su || !sv) return refuse("NULL argument");
    host::camera_basis(*cam, lens_center, su, sv);
    return PT_OK;
}

int pt_mesh_bounding_sphere(const pt_triangle *tris, uint32_t n_tris, float center[3], float *radius) {
    if (!tris || !center || !radius || n_tris == 0) return refuse("NULL argument or empty mesh");
    host::mesh_bounding_sphere(tris, n_tris, center, radius);
    return PT_OK;
}

int pt_ctx_create(int device, pt_ctx **out) {
    if (!out) return refuse("out is NULL");
    *out = nullptr;
    const int n = device_count_quiet();
    if (n <= 0) {
        set_error("no HIP device: libptrace_hip has no CPU fallback");
        return PT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return refuse("device index out of range");
    HIP_TRY(hipSetDevice(device));
    int cus = 0;  // (every launch of the megakernel and the tile pass is sized by it: never 0)
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus <= 0) {
        set_error("the device reports no compute units");
        return PT_ERR_HIP;
    }
    pt_ctx *c = new pt_ctx();
    c->device = device;
    c->tune = read_tuning();
    c->n_cus = (uint32_t)cus;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
        delete c;
        return PT_ERR_HIP;
    }
    *out = c;
    return PT_OK;
}

void pt_ctx_destroy(pt_ctx *c) {
    if (!c) return;
    for (pt_ctx *p : c->pipes) pt_ctx_destroy(p);  // children own their queues, not the scene tables
    c->pipes.clear();
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);  // before anything is freed
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    // every DevBuf of the context frees itself here.  A child (borrowed_scene) holds copies of the parent's device pointers in
    // `scene`, never the parent's DevBufs: nothing is freed twice.
    const hipStream_t st = c->stream;
    delete c;
    (void)hipStreamDestroy(st);
}

// glass deferral only where there is glass to defer
static void set_glass_defer(pt_ctx *c, const pt_object *objs, uint32_t n_objs) {
    bool has_glass = false;
    for (uint32_t i = 0; i < n_objs; ++i) has_glass = has_glass || objs[i].reflect_type == PT_REFRACT;
    c->scene.glass_defer_ok = (c->tune.glass_defer && has_glass) ? 1u : 0u;
}

// the host keeps the tables it uploaded, for pt_ctx_set_object (pt_ctx.fs says what of them)
static void keep_flat(pt_ctx *c, host::FlatScene &fs) {
    std::vector<uint32_t>().swap(fs.rank_id);
    std::vector<SurfRec>().swap(fs.surf);
    std::vector<uint32_t>().swap(fs.tri_rank);
    c->fs = std::move(fs);
}

// c->scene pointed at the device tables: every pointer, and every n_* that is a table's length
static void bind_tables(pt_ctx *c) {
#define PT_X(ID, T, name) c->scene.name = c->tab.name.buf.p;
    PT_SCENE_TABLES(PT_X)
#undef PT_X
    c->scene.n_bvh_nodes = c->n_bvh_nodes = (uint32_t)c->tab.bvh_nodes.count;
    c->scene.n_bvh_nodes4 = (uint32_t)c->tab.bvh_nodes4.count;
    c->scene.n_bvh_meshes = (uint32_t)c->tab.bvh_meshes.count;
    c->scene.n_sph_pairs = (uint32_t)c->tab.sph_pairs.count;
    c->scene.n_flat_pairs = (uint32_t)c->tab.flat_pairs.count;
    c->scene.n_cand_pairs = (uint32_t)c->tab.cand_pairs.count;
}

// the candidate scan's counts, and whether the scene uses it: cand_scan_for reads c->n_bvh_nodes (bind_tables) and
// scene.bvh_in_lds (upload_flat), which are set by now
static void bind_cand_counts(pt_ctx *c, const host::FlatScene &fs) {
    c->scene.n_other_pairs = fs.n_other_pairs;
    c->scene.n_flat_exact = fs.n_flat_exact;
    for (int k = 0; k < 3; ++k) c->scene.n_flat_exact_axis[k] = fs.n_flat_exact_axis[k];
    c->cand_ok = fs.cand_ok;
    c->scene.cand_scan = cand_scan_for(c, 0u);
}

// instrumented builds only (PT_WALK_STATS, PT_PHASE_STATS, PT_TAIL_STATS): a zeroed table of n counters, made with the
// context's first scene and never freed
static int ensure_stats(unsigned long long **p, size_t n) {
    if (*p) return PT_OK;
    HIP_TRY(hipMalloc((void **)p, n * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(*p, 0, n * sizeof(unsigned long long)));
    return PT_OK;
}

// The device form of a flattened scene: the tables uploaded and c->scene pointed at them (pt_ctx_set_scene; the rebuilds of
// pt_ctx_set_camera and pt_ctx_reserve_camera_reach).  Nothing of the context's host state changes here.  Every allocation
// comes before the stream is waited for, every copy after.
static int upload_flat(pt_ctx *c, const host::FlatScene &fs, const pt_object *objs, uint32_t n_objs, uint32_t n_tris) {
    int rc;
#define PT_X(ID, T, name) if ((rc = c->tab.name.buf.ensure(fs.name.size()))) return rc;
    PT_SCENE_TABLES(PT_X)
#undef PT_X
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->refit.clear();  // (the plans name records of the tables before)
#define PT_X(ID, T, name) if ((rc = c->tab.name.upload(fs.name, #name))) return rc;
    PT_SCENE_TABLES(PT_X)
#undef PT_X
    bind_tables(c);
    c->scene.n_objs = n_objs;
    c->scene.n_tris = n_tris;
    // what the tuning and the trees' shape decide
    c->scene.leaf_quorum = c->tune.leaf_quorum;  // mesh.json: 65 (all) 11.7, 32 12.5, 16 12.8, 8 12.8, 1 11.0 G bounces/s
    c->scene.walk_queue_cap = c->tune.walk_queue_cap;
    c->scene.nodes_in_lds_ok = c->tune.nodes_lds ? 1u : 0u;
    c->scene.planar = 1u;
    {
        // bit 1: node and leaf references fit 16 bits (u16 traversal stacks); bit 0: nodes staged in LDS by every
        // workgroup.  With the walks done in dense waves (k_intersect<true>) occupancy is worth more than LDS-resident
        // nodes - mesh.json: 7.7 G bounces/s staged, 8.6 G from L1/L2 - so staging is opt-in (PT_BVH_LDS=1).
        const bool ref16 = c->n_bvh_nodes < 0x8000u && ((uint64_t)fs.bvh_pair_span << kBvhLeafBits) < 0x8000u;
        const bool stage = ref16 && c->n_bvh_nodes <= kBvhMaxLdsNodes && c->tune.bvh_lds;
        c->scene.bvh_in_lds = (ref16 ? 2u : 0u) | (stage ? 1u : 0u);
    }
    c->scene.bvh_pair_base = fs.bvh_pair_base;
    c->scene.bvh_stack = fs.bvh_stack;
    c->scene.cand_staged = 0u;
    c->scene.surf_staged = 0u;
    c->scene.surf_head = 0u;
    set_glass_defer(c, objs, n_objs);
    bind_cand_counts(c, fs);
#ifdef PT_WALK_STATS
    if ((rc = ensure_stats(&c->scene.stats, 16))) return rc;
#endif
#ifdef PT_PHASE_STATS
    if ((rc = ensure_stats(&c->scene.phase_stats, kPhCount * 3 + 2))) return rc;
#endif
#ifdef PT_TAIL_STATS
    if ((rc = ensure_stats(&c->scene.tail_stats, 2 * (size_t)kTailStatsCap))) return rc;
#endif
    return PT_OK;
}

int pt_ctx_set_scene(pt_ctx *c, const pt_camera *cam, const pt_object *objs, uint32_t n_objs,
                     const pt_triangle *tris, uint32_t n_tris) {
    if (!c || !cam || (!objs && n_objs) || (!tris && n_tris)) return refuse("NULL argument");
    host::FlatScene fs;
    host::Reach reach;
    std::string err;
    if (!host::flatten_scene(*cam, objs, n_objs, tris, n_tris, fs, err, nullptr, &reach)) {
        set_error(err);
        return PT_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->held.drop();  // (the held sums are of the scene before)
    c->adaptive.drop();
    c->scene_fp = 0;
    c->fp_stale = false;
    int rc = upload_flat(c, fs, objs, n_objs, n_tris);
    if (rc) return rc;
    keep_flat(c, fs);
    c->cam = *cam;
    c->reach = reach;
    c->h_objs.assign(objs, objs + n_objs);
    c->h_tris.assign(tris, tris + n_tris);
    c->h_boxes.assign((size_t)12 * n_objs, pt_triangle{});
    c->h_local.assign(n_objs, host::Reach{});
    for (uint32_t i = 0; i < n_objs; ++i)
        if (objs[i].kind == PT_MESH && objs[i].tri_count != 0u) {
            host::mesh_bounding_box(tris + objs[i].tri_offset, objs[i].tri_count, &c->h_boxes[(size_t)12 * i]);
            host::local_vertex_box(tris + objs[i].tri_offset, objs[i].tri_count, c->h_local[i]);
        }
    c->boxes_dirty = true;
    c->has_scene = true;
    c->pass_rate = c->round_rate = c->ad_rate = c->mk_rate = 0.0;  // (another scene: the passes' length is measured again)
    c->pass_rate_kernel = nullptr;
    c->scene_fp = scene_fingerprint(cam, objs, n_objs, tris, n_tris);
    return PT_OK;
}

// the tables rebuilt for the origin box B from the kept host copies (the camera is the context's unless `cam` brings another);
// on a failure of flatten_scene the context is as it was
static int rebuild_for_reach(pt_ctx *c, const pt_camera &cam, const host::Reach &B) {
    host::FlatScene fs;
    host::Reach used;
    std::string err;
    const uint32_t n_objs = (uint32_t)c->h_objs.size(), n_tris = (uint32_t)c->h_tris.size();
    if (!host::flatten_scene(cam, c->h_objs.data(), n_objs, c->h_tris.data(), n_tris, fs, err, &B, &used)) {
        set_error(err);
        return PT_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int rc = upload_flat(c, fs, c->h_objs.data(), n_objs, n_tris);
    if (rc) return rc;
    keep_flat(c, fs);
    c->reach = used;
    return PT_OK;
}

int pt_ctx_set_camera(pt_ctx *c, const pt_camera *cam, int *rebuilt) {
    if (!c) return refuse("ctx is NULL");
    if (!cam) return refuse("cam is NULL");
    if (!c->has_scene) return refuse("no scene set: pt_ctx_set_camera moves the camera of the scene pt_ctx_set_scene gave");
    float lens[3], su[3], sv[3];
    host::camera_basis(*cam, lens, su, sv);
    if (!std::isfinite(lens[0]) || !std::isfinite(lens[1]) || !std::isfinite(lens[2])) return refuse("the camera's lens centre is not finite");
    if (rebuilt) *rebuilt = 0;
    if (memcmp(cam, &c->cam, sizeof(pt_camera)) == 0) return PT_OK;  // nine floats, no padding
    if (!c->reach.holds(lens)) {
        host::Reach B = c->reach;
        host::grow_reach(B, lens);
        const int rc = rebuild_for_reach(c, *cam, B);
        if (rc) return rc;
        if (rebuilt) *rebuilt = 1;
    }
    c->cam = *cam;
    // the held frames' key includes the camera (an empty one frees nothing: no HIP call then)
    c->held.drop();
    c->adaptive.drop();
    c->fp_stale = true;
    return PT_OK;
}

// ---- pt_ctx_set_object ---------------------------------------------------------------------------------------------------
// the refit plan of mesh `index` on the device: built from the tree in c->fs and uploaded, with the mesh's object-local
// triangles, by the first MOVE edit of the mesh; kept until the next full build
static int refit_plan_for(pt_ctx *c, uint32_t index, pt_ctx::DevRefit **out) {
    auto it = c->refit.find(index);
    if (it != c->refit.end()) {
        *out = &it->second;
        return PT_OK;
    }
    host::RefitPlan plan;
    if (!host::build_refit_plan(c->fs, index, plan)) return refuse("internal: refit plan asked for an object without a BVH");
    pt_ctx::DevRefit &d = c->refit[index];
    const pt_object &o = c->h_objs[index];
    int rc;
    if ((rc = d.local.upload(c->h_tris.data() + o.tri_offset, o.tri_count, "a refit plan's triangles")) ||
        (rc = d.leaves.upload(plan.leaves, "a refit plan's leaves")) || (rc = d.nodes.upload(plan.nodes, "a refit plan's nodes")) ||
        (rc = d.wide.upload(plan.wide, "a refit plan's wide slots"))) {
        c->refit.erase(index);
        return rc;
    }
    d.level_begin = plan.level_begin;
    d.n_leaves = (uint32_t)plan.leaves.size();
    d.n_wide = (uint32_t)plan.wide.size();
    *out = &d;
    return PT_OK;
}

// an in-reach edit: the records edit_object rewrote in c->fs go to their offsets in the device tables; a mesh with a BVH is
// refit by the kernels.  c->h_objs[index] is the edited object already.
static int upload_object_edit(pt_ctx *c, uint32_t index, bool moved, bool material, const host::ObjectEdit &e) {
    const host::FlatScene &fs = c->fs;
    const pt_object &o = c->h_objs[index];
    const uint32_t n_objs = (uint32_t)c->h_objs.size();
    pt_ctx::SceneTables &t = c->tab;
    int rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = t.objs.upload_range(index, &fs.objs[index], 1, "objs")) || (rc = t.mats.upload_range(index, &fs.mats[index], 1, "mats")))
        return rc;
    if (moved) {
        if ((rc = t.obj_pairs.upload_range(e.obj_pair, &fs.obj_pairs[e.obj_pair], 1, "obj_pairs"))) return rc;
        if (e.on_device) {
            if ((rc = t.bvh_meshes.upload_range(e.bvh_mesh, &fs.bvh_meshes[e.bvh_mesh], 1, "bvh_meshes"))) return rc;
        } else {
            // the candidate scan's tables whole (a few records per sphere and listed mesh): a translation can, through rounding,
            // change which records are flat, their order and their count
            if ((rc = t.sph_pairs.upload(fs.sph_pairs, "sph_pairs")) || (rc = t.flat_pairs.upload(fs.flat_pairs, "flat_pairs")) ||
                (rc = t.cand_pairs.upload(fs.cand_pairs, "cand_pairs")))
                return rc;
            bind_tables(c);
            bind_cand_counts(c, fs);
            if (o.kind == PT_MESH && o.tri_count != 0u) {
                const ObjRec &r = fs.objs[index];
                if ((rc = t.tri_pairs.upload_range(r.pair_begin, fs.tri_pairs.data() + r.pair_begin, r.pair_count, "tri_pairs")) ||
                    (rc = t.tri_shade.upload_range(o.tri_offset, fs.tri_shade.data() + o.tri_offset, o.tri_count, "tri_shade")))
                    return rc;
            }
        }
    }
    if ((rc = t.surf.upload_range(e.rank, e.surf.data(), e.surf.size(), "surf")) ||
        (rc = t.surf.upload_range(e.tail_at, e.tail.data(), e.tail.size(), "surf")))
        return rc;
    if (e.on_device) {
        if (moved) {
            pt_ctx::DevRefit *d = nullptr;
            if ((rc = refit_plan_for(c, index, &d))) return rc;
            RefitTables T{};
            T.tri_pairs = t.tri_pairs.buf.p, T.tri_shade = t.tri_shade.buf.p, T.surf = t.surf.buf.p;
            T.nodes = t.bvh_nodes.buf.p, T.nodes4 = t.bvh_nodes4.buf.p, T.tri_rank = t.tri_rank.buf.p;
            T.local = d->local.p, T.tri_offset = o.tri_offset;
            T.px = o.position[0], T.py = o.position[1], T.pz = o.position[2];
            T.scene_R = e.scene_R;
            launch_refit_leaves(c->stream, T, d->leaves.p, d->n_leaves);
            for (size_t h = 0; h + 1 < d->level_begin.size(); ++h)
                launch_refit_nodes(c->stream, T.nodes, d->nodes.p + d->level_begin[h], d->level_begin[h + 1] - d->level_begin[h]);
            launch_refit_wide(c->stream, T.nodes4, T.nodes, d->wide.p, d->n_wide);
        }
        if (material) launch_refit_materials(c->stream, t.surf.buf.p + e.rank, o.tri_count, fs.mats[index]);
        HIP_TRY(hipGetLastError());
    }
    set_glass_defer(c, c->h_objs.data(), n_objs);
    // a frame may render on a stream of the caller's: the tables are final when the call returns
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_ctx_set_object(pt_ctx *c, uint32_t index, const pt_object *obj, int *rebuilt) {
    {
        const int rc = host::check_object_edit(c != nullptr, obj, c && c->has_scene, c ? c->h_objs.data() : nullptr,
                                               c ? (uint32_t)c->h_objs.size() : 0u, index);
        if (rc) return rc;
    }
    if (rebuilt) *rebuilt = 0;
    const pt_object before = c->h_objs[index];
    if (memcmp(obj, &before, sizeof(pt_object)) == 0) return PT_OK;  // nineteen words, no padding
    const bool moved = !host::same_geometry(*obj, before);
    const bool material = memcmp(obj->color, before.color, sizeof before.color) != 0 ||
                          memcmp(obj->emission, before.emission, sizeof before.emission) != 0 || obj->reflect_type != before.reflect_type;
    const uint32_t n_objs = (uint32_t)c->h_objs.size();
    HIP_TRY(hipSetDevice(c->device));
    host::Reach box;
    host::object_bounds(*obj, c->h_local[index], box);
    const bool has_bounds = obj->kind == PT_SPHERE || obj->tri_count != 0u;
    if (moved && has_bounds && !c->reach.holds(box)) {
        host::Reach B = c->reach;
        host::grow_reach_box(B, box);
        c->h_objs[index] = *obj;
        const int rc = rebuild_for_reach(c, c->cam, B);
        if (rc) {
            c->h_objs[index] = before;
            return rc;
        }
        if (rebuilt) *rebuilt = 1;
    } else {
        c->h_objs[index] = *obj;
        host::ObjectEdit e;
        host::edit_object(c->fs, c->reach, c->h_objs.data(), n_objs, c->h_tris.data(), index, moved, e);
        const int rc = upload_object_edit(c, index, moved, material, e);
        if (rc) return rc;  // (a HIP failure: the tables are in no known state, as after a failed pt_ctx_set_scene)
    }
    c->held.drop();
    c->adaptive.drop();
    c->fp_stale = true;
    c->boxes_dirty = true;  // (the boxes of pt_ctx_set_mesh_bounds take the object's position)
    return PT_OK;
}

int pt_ctx_table_hashes(pt_ctx *c, uint64_t out[PT_TABLE_COUNT]) {
    if (!c || !out) return refuse("NULL argument");
    if (!c->has_scene) return refuse("no scene set");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<uint8_t> h;
#define PT_X(ID, T, name)                                                                                 \
    h.resize(c->tab.name.count * sizeof(T));                                                              \
    if (!h.empty()) HIP_TRY(hipMemcpy(h.data(), c->tab.name.buf.p, h.size(), hipMemcpyDeviceToHost));     \
    out[PT_TABLE_##ID] = pt_siphash(1, 3, 0, 0, h.data(), h.size());
    PT_SCENE_TABLES(PT_X)
#undef PT_X
    return PT_OK;
}

int pt_ctx_camera_reach(const pt_ctx *c, float lo[3], float hi[3]) {
    if (!c || !lo || !hi) return refuse("NULL argument");
    if (!c->has_scene) return refuse("no scene set");
    memcpy(lo, c->reach.lo, sizeof c->reach.lo);
    memcpy(hi, c->reach.hi, sizeof c->reach.hi);
    return PT_OK;
}

int pt_ctx_reserve_camera_reach(pt_ctx *c, const float lo[3], const float hi[3], int *rebuilt) {
    if (!c || !lo || !hi) return refuse("NULL argument");
    if (!c->has_scene) return refuse("no scene set");
    host::Reach want;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return refuse("a bound of the box is not finite");
        if (lo[a] > hi[a]) return refuse("lo > hi on an axis of the box");
        want.lo[a] = lo[a];
        want.hi[a] = hi[a];
    }
    if (rebuilt) *rebuilt = 0;
    if (c->reach.holds(want)) return PT_OK;
    host::Reach B = c->reach;
    for (int a = 0; a < 3; ++a) {
        B.lo[a] = std::fmin(B.lo[a], want.lo[a]);
        B.hi[a] = std::fmax(B.hi[a], want.hi[a]);
    }
    const int rc = rebuild_for_reach(c, c->cam, B);
    if (rc) return rc;
    if (rebuilt) *rebuilt = 1;
    return PT_OK;
}

int pt_scene_reach(const pt_camera *cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris, float lo[3],
                   float hi[3]) {
    if (!cam || (!objs && n_objs) || (!tris && n_tris) || !lo || !hi) return refuse("NULL argument");
    host::Reach r;
    host::scene_reach(*cam, objs, n_objs, tris, n_tris, r);
    memcpy(lo, r.lo, sizeof r.lo);
    memcpy(hi, r.hi, sizeof r.hi);
    return PT_OK;
}

int pt_device_malloc(int device, size_t bytes, void **out) {
    if (!out) return refuse("out is NULL");
    *out = nullptr;
    if (device_count_quiet() <= 0) {
        set_error("no HIP device");
        return PT_ERR_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // reported here: a refused allocation must not show up again as the next frame's error
        *out = nullptr;
        set_error(std::string("hipMalloc of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
        return PT_ERR_HIP;
    }
    return PT_OK;
}

int pt_device_free(int device, void *p) {
    if (!p) return PT_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(p));
    return PT_OK;
}

int pt_device_download(int device, void *dst_host, const void *src_device, size_t bytes) {
    if (!dst_host || !src_device) return refuse("NULL argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

const char *pt_ctx_pass_kernel(const pt_ctx *c, uint32_t flags) {
    if (!c || !c->has_scene) return nullptr;
    return form_for(c, flags).kernel;
}

int pt_bvh_refs_fit(uint64_t n_bvh_nodes, uint64_t n_pair_records) { return host::bvh_refs_fit(n_bvh_nodes, n_pair_records) ? 1 : 0; }

int pt_ctx_set_memory_budget(pt_ctx *c, size_t bytes) {
    if (!c) return refuse("ctx is NULL");
    c->mem_budget = bytes;
    return PT_OK;
}

int pt_ctx_set_profiling(pt_ctx *c, int enabled) {
    if (!c) return refuse("ctx is NULL");
    c->profiling = enabled != 0;
    return PT_OK;
}

// n concurrent wavefront pipelines over the pixels of one call (PT_FLAG_PIPELINES)
static int render_pipelined(pt_ctx *c, const pt_config *cfg, uint32_t n, uint32_t ib, uint32_t ie, float *d_out, hipStream_t st,
                            const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats) {
    // the caller's partition of [ib, ie): chunks first, first+step, ... of C pixels (whole band: rows of the image)
    const uint32_t C = cfg->chunk_step > 1u ? cfg->chunk_pixels : cfg->width;
    const uint32_t first = cfg->chunk_step > 1u ? cfg->chunk_first : 0u;
    const uint32_t step = cfg->chunk_step > 1u ? cfg->chunk_step : 1u;
    while (c->pipes.size() < n) {
        pt_ctx *p = nullptr;
        int rc = pt_ctx_create(c->device, &p);
        if (rc) return rc;
        p->borrowed_scene = true;
        c->pipes.push_back(p);
        c->pipe_out.emplace_back();
    }
    std::vector<pt_config> cfgs(n, *cfg);
    std::vector<pt_stats> sts(n);
    std::vector<int> rcs(n, PT_OK);
    std::vector<std::string> errs(n);
    std::vector<uint32_t> own(n, 0);
    for (uint32_t j = 0; j < n; ++j) {
        pt_ctx *p = c->pipes[j];
        p->scene = c->scene;  // device pointers of the parent's scene tables (read-only)
        p->cam = c->cam;
        p->n_bvh_nodes = c->n_bvh_nodes;
        p->cand_ok = c->cand_ok;
        p->has_scene = true;
        p->profiling = c->profiling;
        p->mem_share = n;  // n sets of ray queues on this device at once
        p->mem_budget = c->mem_budget / n;
        cfgs[j].flags &= ~PT_FLAG_PIPELINES(15);
        cfgs[j].idx_begin = ib;
        cfgs[j].idx_end = ie;
        cfgs[j].chunk_pixels = C;
        cfgs[j].chunk_first = first + step * j;
        cfgs[j].chunk_step = step * n;
        own[j] = owned_pixels(&cfgs[j], ib, ie);
        int rc = c->pipe_out[j].ensure((size_t)own[j] * 3);
        if (rc) return rc;
    }
    std::vector<std::thread> th;
    Relay relay{cb, user};  // pipeline 0 / rank 0 reports for the call
    for (uint32_t j = 0; j < n; ++j) {
        if (own[j] == 0u) continue;
        th.emplace_back([&, j]() {
            rcs[j] = pt_ctx_render(c->pipes[j], &cfgs[j], c->pipe_out[j].p, nullptr, cancel, (j == 0 && cb) ? &Relay::fn : nullptr,
                                   &relay, &sts[j]);
            if (rcs[j] != PT_OK) errs[j] = g_last_error;
        });
    }
    for (auto &t : th) t.join();
    HIP_TRY(hipSetDevice(c->device));
    int worst = PT_OK;
    for (uint32_t j = 0; j < n; ++j) {
        if (own[j] == 0u) continue;
        if (rcs[j] != PT_OK && rcs[j] != PT_CANCELLED) {
            set_error("pipeline " + std::to_string(j) + ": " + errs[j]);
            return rcs[j];
        }
        if (rcs[j] == PT_CANCELLED) worst = PT_CANCELLED;
        // pipeline j's k-th chunk is the call's (k*n + j)-th chunk; the pipelines wrote library memory and have finished, the
        // caller's buffer is only written here, on the call's stream
        launch_scatter_chunks(st, c->pipe_out[j].p, d_out, own[j], C, n, j);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) add_stats_concurrent(stats, sts);
    if (worst == PT_CANCELLED) set_error("cancelled");
    return worst;
}

int pt_ctx_render(pt_ctx *c, const pt_config *cfg, void *d_out_rgb, void *hip_stream, const volatile uint8_t *cancel,
                  pt_progress_fn cb, void *user, pt_stats *stats) {
    if (!c || !d_out_rgb) return refuse("NULL argument");
    uint32_t ib = 0, ie = 0;
    int rc = frame_prologue(c, cfg, &ib, &ie);
    if (rc) return rc;
    const uint32_t n_pipes = (cfg->flags >> 8) & 15u;
    if (n_pipes > 1u && cfg->backend == PT_BACKEND_WAVEFRONT) {
        if (n_pipes > 8u) return refuse("at most 8 concurrent pipelines");
        if (stats) memset(stats, 0, sizeof *stats);
        const double t0p = now_ms();
        rc = render_pipelined(c, cfg, n_pipes, ib, ie, (float *)d_out_rgb, hip_stream ? (hipStream_t)hip_stream : c->stream, cancel, cb,
                              user, stats);
        if (cb && rc == PT_OK) cb(user, 1.0f);  // every pipeline has finished and the chunks are in place
        if (stats) stats->ms_total = now_ms() - t0p;
        return rc;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const FrameParams F = make_frame(c, cfg, ib, ie);
    if (stats) memset(stats, 0, sizeof *stats);
    if (F.npix == 0u) return PT_OK;  // this rank owns no chunk of the band
    // Parts.  The wavefront kernels are tuned for streams of a few dozen pixels with a couple of thousand rays per pass
    // (accumulators, ray slots and deferral buffers share 40 KB of LDS per workgroup); a call of many millions of pixels
    // (4096^2: BASELINE config 5) would need streams of 1024 pixels or passes of hundreds of GB.  Such a call is
    // rendered as consecutive parts of about a million call-local pixels, each exactly like a frame of that size - the
    // RNG is keyed on the global pixel index, so the image is the same bits.  Progress counts finished parts; a
    // cancelled call leaves the parts it did not start black (the reference's unrendered pixels are black too,
    // mod.rs:1003-1016) and the part in progress averaged over its accumulated samples.
    const uint32_t total = F.npix;
    const uint32_t part_px = host::part_pixels(total, cfg->backend == PT_BACKEND_WAVEFRONT);
    const uint32_t n_parts = host::part_count(total, part_px);
    std::vector<Job> jobs;
    for (uint32_t part = 0; part < n_parts; ++part) {
        const host::Part p = host::part_extent(total, part_px, part);
        jobs.push_back({p.k0, p.n, 0u, (float)part / (float)n_parts, 1.0f / (float)n_parts, 0u, 0u});
    }
    return run_frame_call(c, cfg, F, jobs, false, (float *)d_out_rgb, total, st, cancel, cb, user, stats);
}

int pt_ctx_accumulate(pt_ctx *c, const pt_config *cfg, void *d_out_rgb, void *hip_stream, const volatile uint8_t *cancel,
                      pt_progress_fn cb, void *user, pt_stats *stats) {
    if (!c || !d_out_rgb || !cfg) return refuse("NULL argument");
    uint32_t ib = 0, ie = 0;
    int rc = frame_prologue(c, cfg, &ib, &ie);
    if (rc) return rc;
    if (((cfg->flags >> 8) & 15u) > 1u)
        return refuse("pt_ctx_accumulate does not take PT_FLAG_PIPELINES: its accumulators live in child contexts");
    const host::AccumKey key = host::accum_key(cfg, ib, ie);
    const uint32_t total = owned_pixels(cfg, ib, ie);
    HeldFrame &h = c->held;
    if (h.holds(key) && cfg->spp < h.cnt_max()) {
        set_error("cfg->spp (" + std::to_string(cfg->spp) + ") is below the " + std::to_string(h.cnt_max()) +
                  " samples per pixel held for this frame: samples cannot be removed (pt_ctx_accum_reset starts over)");
        return PT_ERR_INVALID;
    }
    if (stats) memset(stats, 0, sizeof *stats);
    if (total == 0u) return PT_OK;  // this rank owns no chunk of the band
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!h.holds(key)) {  // another frame (or none): start from zero, half A of a tracked frame too
        host::FrameCounts f{key, total, host::part_pixels(total, true)};  // counts are kept per part as the wavefront cuts a call, whatever the backend
        f.cnt.assign(host::part_count(total, f.part_px), 0u);
        if (c->acc_track) f.na = f.cnt;
        if ((rc = h.start(std::move(f), nullptr, nullptr, st))) return rc;
    }
    const std::vector<Job> jobs = host::accum_jobs(h, cfg->spp, cfg->backend == PT_BACKEND_MEGAKERNEL);
    return run_frame_call(c, cfg, make_frame(c, cfg, ib, ie), jobs, true, (float *)d_out_rgb, total, st, cancel, cb, user, stats);
}

int pt_ctx_accum_info(const pt_ctx *c, const pt_config *cfg, uint32_t *spp_min, uint32_t *spp_max) {
    if (!c || !cfg || !spp_min || !spp_max) return refuse("NULL argument");
    uint32_t ib = 0, ie = 0;
    const int rc = check_cfg(cfg, &ib, &ie);
    if (rc) return rc;
    *spp_min = *spp_max = 0u;
    if (!c->held.holds(host::accum_key(cfg, ib, ie))) return PT_OK;
    *spp_min = c->held.cnt_min();
    *spp_max = c->held.cnt_max();
    return PT_OK;
}

int pt_ctx_accum_reset(pt_ctx *c) {
    if (!c) return refuse("ctx is NULL");
    if (c->held.sums.p) HIP_TRY(hipSetDevice(c->device));
    c->held.drop();
    return PT_OK;
}

int pt_ctx_accum_save(pt_ctx *c, const char *path) {
    if (!c || !path) return refuse("NULL argument");
    const HeldFrame &h = c->held;
    if (!h.held()) return refuse("nothing accumulated on this context");
    HIP_TRY(hipSetDevice(c->device));
    host::Checkpoint ck;
    static_cast<host::FrameCounts &>(ck) = h;
    ck.scene_fp = scene_fp_of(c);
    std::vector<uint8_t> b;
    host::ckpt_encode_head(ck, b);
    return save_checkpoint(b, h, h.total, h.tracked(), path);
}

int pt_ctx_accum_load(pt_ctx *c, const char *path) {
    host::Checkpoint ck;
    std::vector<uint8_t> b;
    const int rc = load_checkpoint(c, path, host::ckpt_decode, ck, b);
    if (rc) return rc;
    // a file of a noise-tracked frame brings half A; a plain one loaded into a tracking context starts it empty (all held
    // samples then count as half B)
    const uint8_t *half_a = ck.tracked() ? b.data() + ck.a_at : nullptr;
    if (!ck.tracked() && c->acc_track) ck.na.assign(ck.n_parts(), 0u);
    return c->held.start(std::move(ck), b.data() + ck.sums_at, half_a, c->stream);
}

int pt_ctx_accum_track_noise(pt_ctx *c, int enabled) {
    if (!c) return refuse("ctx is NULL");
    if (c->held.held())
        return refuse("an accumulator is held: tracking applies to frames started after the call - call pt_ctx_accum_reset first");
    c->acc_track = enabled != 0;
    return PT_OK;
}

// pt_ctx_accum_noise without the argument checks.  kNoiseNone: the frame is held and tracked but no part has samples in both
// halves yet (*out then holds the counts, pixels 0 and mean_error +inf).
constexpr int kNoiseNone = 1;
static int accum_noise(pt_ctx *c, float *d_error, pt_noise_stats *out, hipStream_t st) {
    memset(out, 0, sizeof *out);
    const HeldFrame &fr = c->held;
    const uint32_t n_parts = fr.n_parts();
    out->spp_min = out->spp_a_min = out->spp_b_min = 0xffffffffu;
    bool any = false;
    for (uint32_t i = 0; i < n_parts; ++i) {
        const uint32_t cnt = fr.cnt[i], na = fr.na[i], nb = cnt - na;
        out->spp_min = cnt < out->spp_min ? cnt : out->spp_min;
        out->spp_max = cnt > out->spp_max ? cnt : out->spp_max;
        out->spp_a_min = na < out->spp_a_min ? na : out->spp_a_min;
        out->spp_b_min = nb < out->spp_b_min ? nb : out->spp_b_min;
        any = any || (na != 0u && nb != 0u);
    }
    if (n_parts == 0u) out->spp_min = out->spp_a_min = out->spp_b_min = 0u;
    if (!any) {
        out->mean_error = (double)__builtin_inff();
        return kNoiseNone;
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->noise_cnt.ensure(1);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->noise_cnt.p, 0, sizeof(NoiseCounters), st));
    for (uint32_t i = 0; i < n_parts; ++i) {
        const host::Part p = fr.part(i);
        const uint32_t na = fr.na[i], nb = fr.cnt[i] - na;
        if (na != 0u && nb != 0u) {
            launch_noise(st, fr.sums.p + p.k0, fr.a.p + p.k0, fr.total, p.n, na, nb, host::noise_part_weight(na, nb),
                         d_error ? d_error + p.k0 : nullptr, c->noise_cnt.p);
            out->pixels += p.n;
        } else if (d_error) {
            launch_noise_none(st, d_error + p.k0, p.n);
        }
    }
    HIP_TRY(hipGetLastError());
    NoiseCounters h;
    HIP_TRY(hipMemcpyAsync(&h, c->noise_cnt.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(out->histogram, h.hist, sizeof h.hist);
    out->mean_error = (double)h.sum * (1.0 / 268435456.0) / (double)out->pixels;
    return PT_OK;
}

// is cfg's frame the held one (PT_OK), and is it noise-tracked?
static int held_tracked_frame(const pt_ctx *c, const pt_config *cfg) {
    uint32_t ib = 0, ie = 0;
    const int rc = check_cfg(cfg, &ib, &ie);
    if (rc) return rc;
    if (!c->held.holds(host::accum_key(cfg, ib, ie))) return refuse("cfg does not name the frame this context holds");
    if (!c->held.tracked())
        return refuse("the held frame is not noise-tracked (pt_ctx_accum_track_noise before the frame is started)");
    return PT_OK;
}

int pt_ctx_accum_noise(pt_ctx *c, const pt_config *cfg, float *d_error, pt_noise_stats *out, void *hip_stream) {
    if (!c || !cfg || !out) return refuse("NULL argument");
    int rc = held_tracked_frame(c, cfg);
    if (rc) return rc;
    rc = accum_noise(c, d_error, out, hip_stream ? (hipStream_t)hip_stream : c->stream);
    if (rc == kNoiseNone) return refuse("no part of the frame has samples in both halves yet: accumulate more");
    return rc;
}

int pt_ctx_accumulate_until(pt_ctx *c, const pt_config *cfg, const pt_noise_target *tgt, void *d_out_rgb, void *hip_stream,
                            const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats, pt_noise_stats *noise) {
    if (!cfg || !tgt || !d_out_rgb || !noise) return refuse("NULL argument");
    int rc = host::check_noise_target(*tgt);
    if (rc) return rc;
    if (!c) return refuse("ctx is NULL");
    uint32_t ib = 0, ie = 0;
    if ((rc = check_cfg(cfg, &ib, &ie))) return rc;
    const bool held = c->held.holds(host::accum_key(cfg, ib, ie));
    if (!(held ? c->held.tracked() : c->acc_track))
        return refuse("pt_ctx_accumulate_until needs noise tracking (pt_ctx_accum_track_noise before the frame is started)");
    const double t0 = now_ms();
    if (stats) memset(stats, 0, sizeof *stats);
    memset(noise, 0, sizeof *noise);
    const uint32_t have = held ? c->held.cnt_max() : 0u, cap = cfg->spp;
    if (cap < have) return refuse("cfg->spp, the cap, is below the samples per pixel held for this frame");
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    Relay relay{cb, user};  // a step's fractions as fractions of the cap's samples; the end of the call reports 1
    for (uint32_t t = host::until_first_target(have, tgt->min_spp, cap);; t = host::next_target(t, cap)) {
        pt_config step = *cfg;
        step.spp = t;
        relay.scale = (float)t / (float)cap;  // (base 0: pt_ctx_accumulate's fractions count the samples held as done)
        pt_stats ss{};
        rc = pt_ctx_accumulate(c, &step, d_out_rgb, hip_stream, cancel, cb ? &Relay::fn : nullptr, &relay, &ss);
        if (stats) add_stats(stats, ss);
        if (rc != PT_OK && rc != PT_CANCELLED) break;
        const int rc_frame = rc;
        const int rn = accum_noise(c, nullptr, noise, st);
        if (rn != PT_OK && rn != kNoiseNone) {
            rc = rn;
            break;
        }
        if (rc_frame == PT_CANCELLED) {
            set_error("cancelled");
            break;
        }
        if ((rn == PT_OK && host::noise_target_met(*noise, *tgt)) || t >= cap) break;
    }
    if (cb && rc == PT_OK) cb(user, 1.0f);
    if (stats) stats->ms_total = now_ms() - t0;
    return rc;
}

int pt_ctx_accumulate_adaptive(pt_ctx *c, const pt_config *cfg, const pt_adaptive_params *params, void *d_out_rgb, uint32_t *d_spp,
                               float *d_error, void *hip_stream, const volatile uint8_t *cancel, pt_progress_fn cb, void *user,
                               pt_stats *stats, pt_adaptive_stats *astats) {
    if (!cfg || !params || !d_out_rgb || !astats) return refuse("NULL argument");
    uint32_t tile_shift = 0, ib = 0, ie = 0;
    const int rc = adaptive_prologue(c, cfg, params, &tile_shift, &ib, &ie);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return accumulate_adaptive(c, cfg, ib, ie, tile_shift, params, (float *)d_out_rgb, d_spp, d_error,
                               hip_stream ? (hipStream_t)hip_stream : c->stream, cancel, cb, user, stats, astats);
}

int pt_ctx_render_adaptive(pt_ctx *c, const pt_config *cfg, const pt_adaptive_params *params, void *d_out_rgb, uint32_t *d_spp,
                           float *d_error, void *hip_stream, const volatile uint8_t *cancel, pt_progress_fn cb, void *user,
                           pt_stats *stats, pt_adaptive_stats *astats) {
    if (c) c->adaptive.forget();  // pt_ctx_adaptive_reset, its memory kept for this frame: the call starts from zero
    return pt_ctx_accumulate_adaptive(c, cfg, params, d_out_rgb, d_spp, d_error, hip_stream, cancel, cb, user, stats, astats);
}

int pt_ctx_adaptive_info(pt_ctx *c, const pt_config *cfg, const pt_adaptive_params *params, pt_adaptive_info *out) {
    if (!cfg || !params || !out) return refuse("NULL argument");
    uint32_t tile_shift = 0, ib = 0, ie = 0;
    int rc = adaptive_prologue(c, cfg, params, &tile_shift, &ib, &ie);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    const HeldAdaptive &h = c->adaptive;
    if (!h.holds(adaptive_key(cfg, ib, ie, tile_shift, params->min_spp))) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the re-decision is the device's scan, the one a call's steps start with; the counts and the E come down with it
    if ((rc = c->ad_cnt.ensure(4))) return rc;
    uint32_t *const words = reinterpret_cast<uint32_t *>(c->ad_cnt.p);
    HIP_TRY(hipMemsetAsync(c->ad_cnt.p + 2, 0, 2 * sizeof(unsigned long long), c->stream));
    const TileGrid G = tile_grid(h);
    TileSelect sel{};
    sel.q = tile_threshold(params->tile_error);
    sel.cap = cfg->spp;
    sel.out = words + 5;
    launch_tile_select(c->stream, G, sel);
    HIP_TRY(hipGetLastError());
    uint32_t counts[3] = {0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(counts, words + 5, sizeof counts, hipMemcpyDeviceToHost, c->stream));
    host::TileTable tab;
    if ((rc = h.download(tab, c->stream))) return rc;
    out->tiles = h.tiles;
    out->tiles_open = counts[0];
    out->tiles_at_cap = counts[1];
    out->spp_min = *std::min_element(tab.cnt.begin(), tab.cnt.end());
    out->spp_max = *std::max_element(tab.cnt.begin(), tab.cnt.end());
    unsigned long long err_sum = 0;
    for (unsigned long long E : tab.err)
        if (E != kTileNoError) err_sum += E;
    const host::TileTotals tot = host::tile_totals(G.width, G.rows, h.geo, tab.cnt.data(), tab.err.data(), err_sum);
    out->samples = tot.samples;
    out->mean_error = tot.mean_error;
    return PT_OK;
}

int pt_ctx_adaptive_resolve(pt_ctx *c, const pt_config *cfg, void *d_out_rgb, uint32_t *d_spp, float *d_error, void *hip_stream) {
    if (!c || !cfg || !d_out_rgb) return refuse("NULL argument");
    uint32_t ib = 0, ie = 0;
    int rc;
    if ((rc = host::check_adaptive_cfg(*cfg)) || (rc = check_cfg(cfg, &ib, &ie))) return rc;
    const HeldAdaptive &h = c->adaptive;
    if (!h.held() || !(h.key.frame == host::accum_key(cfg, ib, ie))) return refuse("cfg does not name the adaptive frame this context holds");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    launch_tile_resolve(st, tile_grid(h), h.sums.p, h.a.p, (float *)d_out_rgb, d_spp, d_error, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

int pt_ctx_adaptive_reset(pt_ctx *c) {
    if (!c) return refuse("ctx is NULL");
    if (c->adaptive.sums.p) HIP_TRY(hipSetDevice(c->device));
    c->adaptive.drop();
    return PT_OK;
}

int pt_ctx_adaptive_save(pt_ctx *c, const char *path) {
    if (!c || !path) return refuse("NULL argument");
    const HeldAdaptive &h = c->adaptive;
    if (!h.held()) return refuse("no adaptive frame is held on this context");
    HIP_TRY(hipSetDevice(c->device));
    host::AdaptiveCheckpoint ck;
    static_cast<host::AdaptiveFrame &>(ck) = h;
    ck.scene_fp = scene_fp_of(c);
    int rc = h.download(ck.table, c->stream);
    if (rc) return rc;
    std::vector<uint8_t> b;
    host::adckpt_encode_head(ck, b);
    return save_checkpoint(b, h, h.total, true, path);
}

int pt_ctx_adaptive_load(pt_ctx *c, const char *path) {
    host::AdaptiveCheckpoint ck;
    std::vector<uint8_t> b;
    int rc = load_checkpoint(c, path, host::adckpt_decode, ck, b);
    if (rc) return rc;
    host::TileGeometry geo;
    uint32_t tile_shift = 0;
    while ((1u << tile_shift) < ck.key.tile) ++tile_shift;
    if ((rc = host::tile_geometry(ck.key.frame.width, ck.total / ck.key.frame.width, tile_shift, geo))) return rc;
    return c->adaptive.start(ck, geo, &ck.table, b.data() + ck.sums_at, b.data() + ck.a_at, c->stream);
}

int pt_ctx_radiance(pt_ctx *c, const float o[3], const float d[3], uint32_t depth, uint32_t n_samples, uint64_t seed,
                    uint32_t pixel, uint32_t backend, uint32_t flags, float out_rgb[3], pt_stats *stats) {
    int rc = host::check_radiance(c, c && c->has_scene, o, d, depth, n_samples, backend, flags, out_rgb);
    if (rc) return rc;
    HostCall q(c, "pt_ctx_radiance");
    if (!q.ok()) return q.finish();
    // a frame of ONE pixel whose samples all start with the given ray: the pixel index is only the RNG counter
    pt_config cfg{};
    cfg.width = 1;
    cfg.height = 1;
    cfg.spp = n_samples;
    cfg.backend = backend;
    cfg.seed = seed;
    cfg.flags = flags;
    FrameParams F = make_frame(c, &cfg, 0u, 1u);
    F.idx_begin = pixel;
    F.npix = 1;
    F.probe = 1u;
    F.depth0 = depth;
    F.probe_ox = o[0];
    F.probe_oy = o[1];
    F.probe_oz = o[2];
    F.probe_dx = d[0];
    F.probe_dy = d[1];
    F.probe_dz = d[2];
    if (stats) memset(stats, 0, sizeof *stats);
    const double t0 = now_ms();
    pt_stats ps{};
    rc = (backend == PT_BACKEND_WAVEFRONT ? render_wavefront : render_mega)(c, form_for(c, flags), &cfg, F, c->stream, nullptr, nullptr,
                                                                          nullptr, ps, 0u, nullptr);
    if (rc != PT_OK) return rc;
    DevBuf<float> d_out;
    q.room(d_out, 3);
    q.run([&](hipStream_t st) {
        launch_resolve(st, c->acc.p, d_out.p, 1u, n_samples, c->live.streams, c->live.m, false);  // the mean, not clamped
    });
    q.out(out_rgb, d_out, 3);
    if ((rc = q.finish())) return rc;
    if (stats) {
        *stats = ps;
        stats->ms_total = now_ms() - t0;
    }
    return PT_OK;
}

int pt_ctx_intersect_streams(pt_ctx *c, const float *o, const float *d, uint32_t n, uint32_t flags, float *t, int32_t *id) {
    if (!c || !o || !d || !t || !id) return refuse("NULL argument");
    if (!c->has_scene) return refuse("no scene set");
    if (n == 0) return PT_OK;
    // the rays as ray streams of 4096 slots (the queue layout of the wavefront pipeline), one workgroup per stream
    const uint32_t cap = 4096u;
    std::vector<char> hq;
    std::vector<uint32_t> hc;
    host::pack_ray_streams(o, d, n, cap, hq, hc);
    const uint32_t K = (uint32_t)hc.size();
    HostCall q(c, "pt_ctx_intersect_streams");
    DevBuf<char> d0;
    DevBuf<float2> dh;
    DevBuf<uint32_t> dc;
    DevBuf<unsigned long long> dr;
    q.in(d0, hq.data(), hq.size());
    q.in(dc, hc.data(), K);
    q.room(dr, K, true);
    q.room(dh, (size_t)K * cap);
    q.run([&](hipStream_t st) {
        const DevScene S = form_for(c, flags).scene;
        launch_intersect(st, K, S, lds_layout(S, 1u, c->tune.lds_pad), RayQueue{d0.p}, dh.p, dc.p, cap, dr.p);
    });
    std::vector<float2> hh((size_t)K * cap);
    q.out(hh.data(), dh, hh.size());
    const int rc = q.finish();
    if (rc == PT_OK) host::unpack_stream_hits(hh.data(), n, t, id);
    return rc;
}

// the rays of an interactive query (pt_ctx_intersect, bounds_query: once per click) into the context's scratch, which persists
// from call to call, and room there for every output of n rays
static void stage_rays(HostCall &q, pt_ctx *c, const float *o, const float *d, uint32_t n) {
    q.in(c->q_o, o, 3 * (size_t)n);
    q.in(c->q_d, d, 3 * (size_t)n);
    q.room(c->q_t, n);
    q.room(c->q_x, 3 * (size_t)n);
    q.room(c->q_n, 3 * (size_t)n);
    q.room(c->q_oid, n);
    q.room(c->q_tid, n);
}

int pt_ctx_intersect(pt_ctx *c, const float *o, const float *d, uint32_t n, float *t, int32_t *object_id,
                     int32_t *tri_id, float *x, float *normal) {
    if (!c || !o || !d) return refuse("NULL argument");
    if (!c->has_scene) return refuse("no scene set");
    if (n == 0) return PT_OK;
    HostCall q(c, "pt_ctx_intersect");
    stage_rays(q, c, o, d, n);
    q.run([&](hipStream_t st) {
        launch_query(st, c->scene, c->q_o.p, c->q_d.p, n, c->q_t.p, c->q_oid.p, c->q_tid.p, c->q_x.p, c->q_n.p);
    });
    q.out(t, c->q_t, n);
    q.out(object_id, c->q_oid, n);
    q.out(tri_id, c->q_tid, n);
    q.out(x, c->q_x, 3 * (size_t)n);
    q.out(normal, c->q_n, 3 * (size_t)n);
    return q.finish();
}

// device form of the bounding boxes (rebuilt after pt_ctx_set_scene / pt_ctx_set_mesh_bounds)
static int upload_boxes(pt_ctx *c) {
    if (!c->boxes_dirty) return PT_OK;
    const size_t n_objs = c->h_objs.size();
    std::vector<TriPairRec> recs(6 * (n_objs ? n_objs : 1), TriPairRec{});
    for (size_t i = 0; i < n_objs; ++i)
        if (c->h_objs[i].kind == PT_MESH) host::box_pair_records(&c->h_boxes[12 * i], c->h_objs[i].position, &recs[6 * i]);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int rc = c->d_boxes.upload(recs, "the bounding boxes");
    if (rc) return rc;
    c->boxes_dirty = false;
    return PT_OK;
}

static int bounds_query(pt_ctx *c, uint32_t mode, uint32_t object, const float *o, const float *d, uint32_t n, int32_t *hit,
                        float *t, float *x, float *normal, int32_t *object_id) {
    int rc = host::check_bounds_query(c, c && c->has_scene, mode, object, c ? (uint32_t)c->h_objs.size() : 0u, o, d);
    if (rc || n == 0) return rc;
    HostCall q(c, mode ? "pt_ctx_orbit_point" : "pt_ctx_intersect_bounds");
    if (q.ok() && (rc = upload_boxes(c))) return rc;
    stage_rays(q, c, o, d, n);
    q.run([&](hipStream_t st) {
        launch_bounds(st, c->scene, c->d_boxes.p, mode, object, c->q_o.p, c->q_d.p, n, c->q_tid.p, c->q_t.p, c->q_x.p, c->q_n.p,
                      c->q_oid.p);
    });
    q.out(hit, c->q_tid, n);
    q.out(t, c->q_t, n);
    q.out(x, c->q_x, 3 * (size_t)n);
    q.out(normal, c->q_n, 3 * (size_t)n);
    q.out(object_id, c->q_oid, n);
    return q.finish();
}

int pt_ctx_intersect_bounds(pt_ctx *c, uint32_t object, const float *o, const float *d, uint32_t n, int32_t *hit, float *t,
                            float *x, float *normal) {
    return bounds_query(c, 0u, object, o, d, n, hit, t, x, normal, nullptr);
}

int pt_ctx_orbit_point(pt_ctx *c, const float *o, const float *d, uint32_t n, int32_t *found, float *point,
                       int32_t *object_id, float *t) {
    return bounds_query(c, 1u, 0u, o, d, n, found, t, point, nullptr, object_id);
}

int pt_ctx_set_mesh_bounds(pt_ctx *c, uint32_t object, const pt_triangle box[12]) {
    if (!c || !box) return refuse("NULL argument");
    if (!c->has_scene || object >= c->h_objs.size() || c->h_objs[object].kind != PT_MESH)
        return refuse("no scene set, or object is not a mesh of it");
    memcpy(&c->h_boxes[(size_t)12 * object], box, 12 * sizeof(pt_triangle));
    c->boxes_dirty = true;
    return PT_OK;
}

int pt_mesh_bounding_box(const pt_triangle *tris, uint32_t n_tris, pt_triangle out[12]) {
    if (!tris || !out || n_tris == 0) return refuse("NULL argument or empty mesh");
    host::mesh_bounding_box(tris, n_tris, out);
    return PT_OK;
}

void pt_host_sincos(float y, float *s, float *c) { sincos_f32(y, s, c); }

int pt_ctx_snapshot(pt_ctx *c, void *d_out_rgb, uint32_t *spp_done) {
    if (!c || !d_out_rgb) return refuse("NULL argument");
    if (c->live.npix == 0 || c->live.spp_issued == 0)
        return refuse("no frame in progress on this context (call from the progress callback of pt_ctx_render; under "
                      "PT_FLAG_PIPELINES the accumulators live in child contexts and no snapshot is offered)");
    HIP_TRY(hipSetDevice(c->device));
    // stream order: the resolve runs after every pass issued so far, i.e. over live.spp_issued samples per pixel.  A call
    // rendered in parts: the finished parts are copied from the call's own output, the part in progress is resolved,
    // the parts not started are black.
    float *snap = (float *)d_out_rgb;
    const LiveFrame &L = c->live;
    hipStream_t st = L.stream;
    if (L.accum) {  // pt_ctx_accumulate: every part outside the one in progress at its own count, from the held sums
        for (uint32_t i = 0; i < c->held.n_parts(); ++i) {
            const uint32_t k0 = c->held.part(i).k0;
            if (k0 >= L.k0 && k0 < L.k0 + L.npix) continue;
            int rc = accum_resolve_part(c->held, i, snap, st);
            if (rc) return rc;
        }
    } else if (L.k0 != 0u && L.out && L.out != snap) {
        HIP_TRY(hipMemcpyAsync(snap, L.out, (size_t)L.k0 * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    launch_resolve(st, c->acc.p, snap + (size_t)L.k0 * 3, L.npix, L.spp_issued, L.streams, L.m);
    const uint32_t done = L.k0 + L.npix;
    if (!L.accum && done < L.total)
        HIP_TRY(hipMemsetAsync(snap + (size_t)done * 3, 0, (size_t)(L.total - done) * 3 * sizeof(float), st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (spp_done) *spp_done = L.spp_issued;
    return PT_OK;
}

int pt_ctx_numerics_probe(pt_ctx *c, const float *in, uint32_t n, float *out_sin, float *out_cos, float *out_sqrt,
                          float *out_rcp, uint32_t *out_philox) {
    if (!c || !in || !out_sin || !out_cos || !out_sqrt || !out_rcp || !out_philox || n == 0) return refuse("NULL argument");
    HostCall q(c, "pt_ctx_numerics_probe");
    DevBuf<float> d_in, d_s, d_c, d_q, d_r;
    DevBuf<uint32_t> d_p;
    q.in(d_in, in, n);
    q.room(d_s, n);
    q.room(d_c, n);
    q.room(d_q, n);
    q.room(d_r, n);
    q.room(d_p, 4 * (size_t)n);
    q.run([&](hipStream_t st) { launch_numerics(st, d_in.p, n, d_s.p, d_c.p, d_q.p, d_r.p, d_p.p); });
    q.out(out_sin, d_s, n);
    q.out(out_cos, d_c, n);
    q.out(out_sqrt, d_q, n);
    q.out(out_rcp, d_r, n);
    q.out(out_philox, d_p, 4 * (size_t)n);
    return q.finish();
}

static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the sweeps' counters are copied into the caller's uint64_t as they are");

int pt_ctx_numerics_sweep(pt_ctx *c, uint64_t out[4]) {
    if (!c || !out) return refuse("NULL argument");
    HostCall q(c, "pt_ctx_numerics_sweep");
    DevBuf<unsigned long long> d;
    q.room(d, 4, true);
    q.run([&](hipStream_t st) { launch_numerics_sweep(st, d.p); });
    q.out(reinterpret_cast<unsigned long long *>(out), d, 4);
    return q.finish();
}

int pt_ctx_sincos_sweep(pt_ctx *c, uint64_t out[2]) {
    if (!c || !out) return refuse("NULL argument");
    // the host instantiation of the shared numerics header on the 2^24 arguments shade_surface can form (mod.rs:691,703)
    const uint32_t n = 1u << 24;
    std::vector<uint32_t> hs(n), hc(n);
    for (uint32_t k = 0; k < n; ++k) {
        const float r1 = (2.0f * 3.141592653589793f) * unit_f32(k << 8);
        float s, co;
        sincos_f32(r1, &s, &co);
        memcpy(&hs[k], &s, 4);
        memcpy(&hc[k], &co, 4);
    }
    HostCall q(c, "pt_ctx_sincos_sweep");
    DevBuf<uint32_t> ds, dc;
    DevBuf<unsigned long long> d;
    q.in(ds, hs.data(), n);
    q.in(dc, hc.data(), n);
    q.room(d, 2, true);
    q.run([&](hipStream_t st) { launch_sincos_sweep(st, ds.p, dc.p, d.p); });
    q.out(reinterpret_cast<unsigned long long *>(out), d, 2);
    return q.finish();
}

int pt_ctx_primary_rays(pt_ctx *c, uint32_t width, uint32_t height, uint64_t seed, const uint32_t *pixel, const uint32_t *sample,
                        uint32_t n, uint32_t form, float *o, float *d) {
    pt_config cfg{};
    uint32_t ib = 0, ie = 0;
    const int rc = host::check_primary_rays(c, c && c->has_scene, width, height, seed, pixel, sample, n, form, o, d, cfg, &ib, &ie);
    if (rc) return rc;
    HostCall q(c, "pt_ctx_primary_rays");
    const FrameParams F = make_frame(c, &cfg, ib, ie);
    DevBuf<uint32_t> dp, dsm;
    DevBuf<float> d_o, d_d;
    q.in(dp, pixel, n);
    q.in(dsm, sample, n);
    q.room(d_o, 3 * (size_t)n);
    q.room(d_d, 3 * (size_t)n);
    q.run([&](hipStream_t st) { launch_primary_rays(st, F, dp.p, dsm.p, n, form, d_o.p, d_d.p); });
    q.out(o, d_o, 3 * (size_t)n);
    q.out(d, d_d, 3 * (size_t)n);
    return q.finish();
}

int pt_ctx_scatter(pt_ctx *c, uint64_t seed, uint32_t form, const pt_scatter_item *items, const pt_scatter_surface *surfaces,
                   uint32_t n, pt_scatter_out *out) {
    std::vector<ScatterSurf> given;
    const int rc = host::check_scatter(c, form, items, surfaces, n, out, given);
    if (rc) return rc;
    if (device_count_quiet() <= 0) {
        set_error("no HIP device: libptrace_hip has no CPU fallback");
        return PT_ERR_NO_DEVICE;
    }
    const uint32_t src = form & kScatterSourceMask;
    if (src != PT_SCATTER_GIVEN && !c->has_scene) return refuse("no scene set");
    if (src == PT_SCATTER_BY_RANK && !c->cand_ok) return refuse("PT_SCATTER_BY_RANK: the scene has no candidate tables");
    ScatterCall call{};
    call.n = n;
    call.form = form;
    call.seed_lo = (uint32_t)seed;
    call.seed_hi = (uint32_t)(seed >> 32);
    if (src == PT_SCATTER_BY_RANK) {
        // the head k_pass_cand would stage for this scene (pt_layout.h; one-pixel streams), while it fits the probe's workgroup
        const DevScene F = form_for(c, 0u).scene;
        const size_t room = scatter_head_room(c->scene) / sizeof(SurfRec);
        call.head = (uint32_t)std::min<size_t>(lds_layout(F, 1u, c->tune.lds_pad).surf_head, room);
    }
    HostCall q(c, "pt_ctx_scatter");
    DevBuf<pt_scatter_item> d_items;
    DevBuf<ScatterSurf> d_surf;
    DevBuf<pt_scatter_out> d_out;
    q.in(d_items, items, n);
    if (!given.empty()) q.in(d_surf, given.data(), n);
    q.room(d_out, n);
    q.run([&](hipStream_t st) {
        call.items = d_items.p;
        call.surf = d_surf.p;
        call.out = d_out.p;
        launch_scatter(st, c->scene, call);
    });
    q.out(out, d_out, n);
    return q.finish();
}

int pt_ctx_render_aov(pt_ctx *c, const pt_config *cfg, float *d_albedo, float *d_normal, float *d_depth, int32_t *d_object_id,
                      void *hip_stream) {
    if (!c || !cfg) return refuse("NULL argument");
    if (!d_albedo && !d_normal && !d_depth && !d_object_id) return refuse("every output is NULL");
    // the frame's pixels and samples as pt_ctx_render reads them; backend, pass sizes and pipelines do not apply
    pt_config fc = *cfg;
    fc.backend = PT_BACKEND_WAVEFRONT;
    uint32_t ib = 0, ie = 0;
    const int rc = frame_prologue(c, &fc, &ib, &ie);
    if (rc) return rc;
    const FrameParams F = make_frame(c, &fc, ib, ie);
    if (F.npix == 0u) return PT_OK;  // this rank owns no chunk of the band
    const DevScene S = form_for(c, cfg->flags).scene;  // (k_aov reads neither the candidate scan nor an LDS layout)
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        launch_aov(st, S, F, d_albedo, d_normal, d_depth, d_object_id);
        return PT_OK;
    });
}

// pt_aov_params with every default written out: a through-delta call of kAovDefaultChain steps (a plain call has no parameters
// to default; {0, 8} would be a set the call itself refuses)
static constexpr uint32_t kAovDefaultChain = 8u;
int pt_aov_defaults(pt_aov_params *out) { return give_defaults(out, pt_aov_params{PT_AOV_THROUGH_DELTA, kAovDefaultChain}); }

int pt_ctx_render_aov_ex(pt_ctx *c, const pt_config *cfg, const pt_aov_params *params, float *d_albedo, float *d_normal,
                         float *d_depth, int32_t *d_object_id, uint32_t *d_chain, void *hip_stream) {
    const pt_aov_params P = params ? *params : pt_aov_params{0u, 0u};
    if (P.flags & ~PT_AOV_THROUGH_DELTA) return refuse("pt_aov_params.flags: unknown bits");
    if (P.max_chain > PT_AOV_MAX_CHAIN) return refuse("pt_aov_params.max_chain exceeds PT_AOV_MAX_CHAIN");
    if (P.max_chain != 0u && !(P.flags & PT_AOV_THROUGH_DELTA))
        return refuse("pt_aov_params.max_chain without PT_AOV_THROUGH_DELTA");
    if (!d_albedo && !d_normal && !d_depth && !d_object_id && !d_chain) return refuse("every output is NULL");
    if (!cfg || !c) return refuse("NULL argument");
    // from here on pt_ctx_render_aov's own steps
    pt_config fc = *cfg;
    fc.backend = PT_BACKEND_WAVEFRONT;
    uint32_t ib = 0, ie = 0;
    const int rc = frame_prologue(c, &fc, &ib, &ie);
    if (rc) return rc;
    const FrameParams F = make_frame(c, &fc, ib, ie);
    if (F.npix == 0u) return PT_OK;
    const DevScene S = form_for(c, cfg->flags).scene;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        if (P.flags & PT_AOV_THROUGH_DELTA) {
            launch_aov_chain(st, S, F, P.max_chain ? P.max_chain : kAovDefaultChain, d_albedo, d_normal, d_depth, d_object_id,
                             d_chain);
            return PT_OK;
        }
        // the plain call's kernel; no chain was followed
        if (d_albedo || d_normal || d_depth || d_object_id) launch_aov(st, S, F, d_albedo, d_normal, d_depth, d_object_id);
        if (d_chain) HIP_TRY(hipMemsetAsync(d_chain, 0, (size_t)F.npix * sizeof(uint32_t), st));
        return PT_OK;
    });
}

// pt_ctx_denoise and pt_ctx_denoise_var once host::check_denoise* has passed: the scratch, prepare, the levels of the schedule
static int run_denoise(pt_ctx *c, DenoiseCall &call, void *hip_stream) {
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        DenoiseFrame &f = call.f;
        const size_t npix = (size_t)f.width * f.height;
        int rc;
        if ((rc = c->dn_u[0].ensure(npix)) || (rc = c->dn_u[1].ensure(npix)) || (rc = c->dn_guide.ensure(npix))) return rc;
        f.guide = c->dn_guide.p;
        f.u[0] = c->dn_u[0].p;
        f.u[1] = c->dn_u[1].p;
        launch_dn_prepare(st, f);
        for (uint32_t i = 0; i < call.levels; ++i)
            launch_dn_level(st, f, i, call.rc[i], call.sds[i], i + 1u == call.levels, (1u << i) <= c->tune.dn_lds_maxstep);
        return PT_OK;
    });
}

int pt_denoise_defaults(pt_denoise_params *out) { return give_defaults(out, kDenoiseDefaults); }

int pt_ctx_denoise(pt_ctx *c, uint32_t width, uint32_t height, const pt_denoise_params *params, const float *d_color,
                   const float *d_albedo, const float *d_normal, const float *d_depth, float *d_out, void *hip_stream) {
    DenoiseCall call;
    const int rc = host::check_denoise(c, width, height, params, d_color, d_albedo, d_normal, d_depth, d_out, call);
    return rc ? rc : run_denoise(c, call, hip_stream);
}

int pt_denoise_var_defaults(pt_denoise_var_params *out) { return give_defaults(out, kDenoiseVarDefaults); }

int pt_ctx_denoise_var(pt_ctx *c, uint32_t width, uint32_t height, const pt_denoise_var_params *params, const float *d_color,
                       const float *d_error, const float *d_albedo, const float *d_normal, const float *d_depth, float *d_out,
                       void *hip_stream) {
    DenoiseCall call;
    const int rc = host::check_denoise_var(c, width, height, params, d_color, d_error, d_albedo, d_normal, d_depth, d_out, call);
    return rc ? rc : run_denoise(c, call, hip_stream);
}

int pt_ctx_present(pt_ctx *c, uint32_t width, uint32_t height, const pt_present_params *params, const float *d_rgb, uint8_t *d_out,
                   void *hip_stream) {
    PresentFrame f;
    const int rc = host::check_present(c, width, height, params, d_rgb, d_out, f);
    if (rc) return rc;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        if (!c->pr_table.p) {
            const int rt = c->pr_table.ensure(256);
            if (rt) return rt;
            // (the table lives as long as the process: the copy may read it whenever it runs)
            const hipError_t e = hipMemcpyAsync(c->pr_table.p, present_table(), 256 * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) {
                c->pr_table.release();
                set_error(std::string("uploading the present table: ") + hipGetErrorString(e));
                return PT_ERR_HIP;
            }
        }
        f.table = c->pr_table.p;
        if (f.resamples()) {
            const int rm = c->pr_mid.ensure(3 * (size_t)f.width * f.out_height);
            if (rm) return rm;
            f.mid = c->pr_mid.p;
        }
        launch_present(st, f);
        return PT_OK;
    });
}

// (no stream parameter: the context's own stream)
int pt_ctx_overlay(pt_ctx *c, uint32_t width, uint32_t height, const pt_overlay_params *params, const pt_camera *cam, const float *d_rgb,
                   const int32_t *d_object_id, const float *d_depth, float *d_out) {
    OverlayFrame f;
    const int rc = host::check_overlay(c, width, height, params, cam, d_rgb, d_object_id, d_depth, d_out, f);
    if (rc) return rc;
    return run_image_pass(c, nullptr, [&](hipStream_t st) {
        launch_overlay(st, f);
        return PT_OK;
    });
}

// The looks table goes the way upload_motion's table goes: copied into the context's scratch on the call's stream, which the call
// waits for before it returns, so the caller's array outlives the copy.
int pt_ctx_solid(pt_ctx *c, uint32_t width, uint32_t height, const pt_solid_params *params, const pt_camera *cam, const float *d_albedo,
                 const float *d_normal, const float *d_depth, const int32_t *d_object_id, const pt_solid_look *looks, uint32_t n_looks,
                 float *d_out, void *hip_stream) {
    SolidFrame f;
    const int rc = host::check_solid(c, width, height, params, cam, d_albedo, d_normal, d_depth, d_object_id, looks, n_looks, d_out, f);
    if (rc) return rc;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        if (f.n_looks) {
            const int rt = c->solid_looks.ensure(f.n_looks);
            if (rt) return rt;
            const hipError_t e = hipMemcpyAsync(c->solid_looks.p, f.looks, (size_t)f.n_looks * sizeof(pt_solid_look), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) {
                set_error(std::string("uploading the looks table: ") + hipGetErrorString(e));
                return PT_ERR_HIP;
            }
            f.looks = c->solid_looks.p;
        }
        launch_solid(st, f);
        return PT_OK;
    });
}

// ---- the tone stage (ptrace_tone.h)
int pt_ctx_accum_hdr(pt_ctx *c, const pt_config *cfg, float *d_out_rgb, void *hip_stream) {
    if (!c || !cfg || !d_out_rgb) return refuse("NULL argument");
    uint32_t ib = 0, ie = 0;
    const int rc = check_cfg(cfg, &ib, &ie);
    if (rc) return rc;
    if (!c->held.holds(host::accum_key(cfg, ib, ie))) return refuse("cfg does not name the frame this context holds");
    const HeldFrame &h = c->held;
    HdrFrame f{h.sums.p, d_out_rgb, h.total, h.part_px, h.cnt[0], nullptr};
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        if (h.n_parts() > 1u) {
            // (the counts are the context's own: they outlive the copy, which the call waits for)
            const int rt = c->hdr_counts.ensure(h.n_parts());
            if (rt) return rt;
            const hipError_t e = hipMemcpyAsync(c->hdr_counts.p, h.cnt.data(), (size_t)h.n_parts() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) {
                set_error(std::string("uploading the parts' counts: ") + hipGetErrorString(e));
                return PT_ERR_HIP;
            }
            f.counts = c->hdr_counts.p;
        }
        launch_hdr(st, f);
        return PT_OK;
    });
}

int pt_ctx_meter(pt_ctx *c, uint32_t width, uint32_t height, const pt_meter_params *params, const float *d_rgb, const int32_t *d_object_id,
                 pt_meter_stats *out, void *hip_stream) {
    MeterFrame f;
    const int rc = host::check_meter(c, width, height, params, d_rgb, d_object_id, out, f);
    if (rc) return rc;
    uint32_t counters[kMeterWords];
    const int rr = run_image_pass(c, hip_stream, [&](hipStream_t st) {
        const int rt = c->meter_cnt.ensure(kMeterWords);
        if (rt) return rt;
        f.counters = c->meter_cnt.p;
        HIP_TRY(hipMemsetAsync(f.counters, 0, sizeof counters, st));
        launch_meter(st, f);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counters, f.counters, sizeof counters, hipMemcpyDeviceToHost, st));
        return PT_OK;
    });
    if (rr) return rr;
    host::meter_stats_of(counters, out);
    return PT_OK;
}

int pt_meter_exposure_defaults(pt_meter_exposure_params *out) { return give_defaults(out, kMeterExposureDefaults); }
int pt_tonemap_defaults(pt_tonemap_params *out) { return give_defaults(out, kTonemapDefaults); }

int pt_ctx_tonemap(pt_ctx *c, uint32_t width, uint32_t height, const pt_tonemap_params *params, const float *d_rgb, float *d_out,
                   void *hip_stream) {
    ToneFrame f;
    const int rc = host::check_tonemap(c, width, height, params, d_rgb, d_out, f);
    if (rc) return rc;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        launch_tonemap(st, f);
        return PT_OK;
    });
}

// ---- the firefly stage (ptrace_despike.h)
int pt_despike_defaults(pt_despike_params *out) { return give_defaults(out, kDespikeDefaults); }

int pt_ctx_despike(pt_ctx *c, uint32_t width, uint32_t height, const pt_despike_params *params, const float *d_rgb,
                   const int32_t *d_object_id, float *d_out, uint8_t *d_mask, pt_despike_stats *out, void *hip_stream) {
    DespikeFrame f;
    const int rc = host::check_despike(c, width, height, params, d_rgb, d_object_id, d_out, d_mask, f);
    if (rc) return rc;
    unsigned long long counters[2] = {0ull, 0ull};
    const int rr = run_image_pass(c, hip_stream, [&](hipStream_t st) {
        if (out) {  // without it nothing is cleared, counted or downloaded
            const int rt = c->despike_cnt.ensure(2);
            if (rt) return rt;
            f.counters = c->despike_cnt.p;
            HIP_TRY(hipMemsetAsync(f.counters, 0, sizeof counters, st));
        }
        launch_despike(st, f);
        HIP_TRY(hipGetLastError());
        if (out) HIP_TRY(hipMemcpyAsync(counters, f.counters, sizeof counters, hipMemcpyDeviceToHost, st));
        return PT_OK;
    });
    if (rr) return rr;
    if (out) *out = pt_despike_stats{(uint64_t)width * height, counters[0], counters[1]};
    return PT_OK;
}

int pt_reproject_defaults(pt_reproject_params *out) {
    return give_defaults(out, pt_reproject_params{1u, kReprojectMaxHistory, kReprojectDepthTol, kReprojectNormalMin, 0u});
}

int pt_reproject_var_defaults(pt_reproject_var_params *out) {
    return give_defaults(out, pt_reproject_var_params{1u, kReprojectMaxHistory, kReprojectDepthTol, kReprojectNormalMin,
                                                      kReprojectVarMinFrames, kReprojectVarRadius, 0u});
}

// the moved calls' table, copied into the context's scratch on the call's stream (the call waits for the stream before it returns,
// so the caller's array outlives the copy)
static int upload_motion(pt_ctx *c, hipStream_t st, const pt_object_motion *motion, uint32_t n_motion, ReprojectMotion &m) {
    const int rt = c->rm_table.ensure(n_motion);
    if (rt) return rt;
    const hipError_t e = hipMemcpyAsync(c->rm_table.p, motion, (size_t)n_motion * sizeof(pt_object_motion), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        set_error(std::string("uploading the motion table: ") + hipGetErrorString(e));
        return PT_ERR_HIP;
    }
    m = ReprojectMotion{c->rm_table.p, n_motion};
    return PT_OK;
}

// The five reproject entry points once their arguments have names (pt_reproject.h, ReprojectArgs): the check, then on the call's
// stream the scratch of the s plane where the call has moments, the table where something moved, and the launch
static int run_reproject(pt_ctx *c, const ReprojectArgs &a, void *hip_stream) {
    ReprojectCall call;
    const int rc = host::check_reproject(a, call);
    if (rc) return rc;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        if (call.var) {
            const int rs = c->rv_s.ensure((size_t)a.width * a.height);
            if (rs) return rs;
            call.v.s_plane = c->rv_s.p;
        }
        ReprojectMotion m{nullptr, 0u};
        if (call.moved()) {
            const int ru = upload_motion(c, st, a.motion, a.n_motion, m);
            if (ru) return ru;
        }
        launch_reproject(st, call, &m);
        return PT_OK;
    });
}

int pt_ctx_reproject(pt_ctx *c, uint32_t width, uint32_t height, const pt_reproject_params *params, const pt_camera *cam,
                     const float *d_color, const float *d_depth, const int32_t *d_object_id, const float *d_normal,
                     const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len, const float *d_hist_depth,
                     const int32_t *d_hist_object_id, const float *d_hist_normal, float *d_out_color, float *d_out_len,
                     void *hip_stream) {
    ReprojectArgs a{};
    a.ctx = c, a.width = width, a.height = height, a.params = params, a.cam = cam, a.hist_cam = hist_cam;
    a.color = d_color, a.depth = d_depth, a.object_id = d_object_id, a.normal = d_normal;
    a.hist_color = d_hist_color, a.hist_len = d_hist_len, a.hist_depth = d_hist_depth, a.hist_object_id = d_hist_object_id;
    a.hist_normal = d_hist_normal, a.out_color = d_out_color, a.out_len = d_out_len;
    return run_reproject(c, a, hip_stream);
}

int pt_ctx_reproject_var(pt_ctx *c, uint32_t width, uint32_t height, const pt_reproject_var_params *params, const pt_camera *cam,
                         const float *d_color, const float *d_depth, const int32_t *d_object_id, const float *d_normal,
                         const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len, const float *d_hist_moments,
                         const float *d_hist_depth, const int32_t *d_hist_object_id, const float *d_hist_normal, float *d_out_color,
                         float *d_out_len, float *d_out_moments, float *d_error, void *hip_stream) {
    ReprojectArgs a{};
    a.ctx = c, a.var = true, a.width = width, a.height = height, a.var_params = params, a.cam = cam, a.hist_cam = hist_cam;
    a.color = d_color, a.depth = d_depth, a.object_id = d_object_id, a.normal = d_normal;
    a.hist_color = d_hist_color, a.hist_len = d_hist_len, a.hist_moments = d_hist_moments, a.hist_depth = d_hist_depth;
    a.hist_object_id = d_hist_object_id, a.hist_normal = d_hist_normal;
    a.out_color = d_out_color, a.out_len = d_out_len, a.out_moments = d_out_moments, a.error = d_error;
    return run_reproject(c, a, hip_stream);
}

int pt_ctx_reproject_moved(pt_ctx *c, uint32_t width, uint32_t height, const pt_reproject_params *params, const pt_camera *cam,
                           const float *d_color, const float *d_depth, const int32_t *d_object_id, const float *d_normal,
                           const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len, const float *d_hist_depth,
                           const int32_t *d_hist_object_id, const float *d_hist_normal, float *d_out_color, float *d_out_len,
                           const pt_object_motion *motion, uint32_t n_motion, void *hip_stream) {
    ReprojectArgs a{};
    a.ctx = c, a.width = width, a.height = height, a.params = params, a.cam = cam, a.hist_cam = hist_cam;
    a.color = d_color, a.depth = d_depth, a.object_id = d_object_id, a.normal = d_normal;
    a.hist_color = d_hist_color, a.hist_len = d_hist_len, a.hist_depth = d_hist_depth, a.hist_object_id = d_hist_object_id;
    a.hist_normal = d_hist_normal, a.out_color = d_out_color, a.out_len = d_out_len, a.motion = motion, a.n_motion = n_motion;
    return run_reproject(c, a, hip_stream);
}

int pt_ctx_reproject_var_moved(pt_ctx *c, uint32_t width, uint32_t height, const pt_reproject_var_params *params, const pt_camera *cam,
                               const float *d_color, const float *d_depth, const int32_t *d_object_id, const float *d_normal,
                               const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len, const float *d_hist_moments,
                               const float *d_hist_depth, const int32_t *d_hist_object_id, const float *d_hist_normal, float *d_out_color,
                               float *d_out_len, float *d_out_moments, float *d_error, const pt_object_motion *motion, uint32_t n_motion,
                               void *hip_stream) {
    ReprojectArgs a{};
    a.ctx = c, a.var = true, a.width = width, a.height = height, a.var_params = params, a.cam = cam, a.hist_cam = hist_cam;
    a.color = d_color, a.depth = d_depth, a.object_id = d_object_id, a.normal = d_normal;
    a.hist_color = d_hist_color, a.hist_len = d_hist_len, a.hist_moments = d_hist_moments, a.hist_depth = d_hist_depth;
    a.hist_object_id = d_hist_object_id, a.hist_normal = d_hist_normal;
    a.out_color = d_out_color, a.out_len = d_out_len, a.out_moments = d_out_moments, a.error = d_error;
    a.motion = motion, a.n_motion = n_motion;
    return run_reproject(c, a, hip_stream);
}

int pt_ctx_reproject_var_weighted(pt_ctx *c, uint32_t width, uint32_t height, const pt_reproject_var_params *params,
                                  const pt_camera *cam, const float *d_color, const float *d_depth, const int32_t *d_object_id,
                                  const float *d_normal, const uint32_t *d_spp, const pt_camera *hist_cam, const float *d_hist_color,
                                  const float *d_hist_len, const float *d_hist_moments, const float *d_hist_depth,
                                  const int32_t *d_hist_object_id, const float *d_hist_normal, float *d_out_color, float *d_out_len,
                                  float *d_out_moments, float *d_error, const pt_object_motion *motion, uint32_t n_motion,
                                  void *hip_stream) {
    ReprojectArgs a{};
    a.ctx = c, a.var = true, a.width = width, a.height = height, a.var_params = params, a.cam = cam, a.hist_cam = hist_cam;
    a.color = d_color, a.depth = d_depth, a.object_id = d_object_id, a.normal = d_normal, a.spp = d_spp;
    a.hist_color = d_hist_color, a.hist_len = d_hist_len, a.hist_moments = d_hist_moments, a.hist_depth = d_hist_depth;
    a.hist_object_id = d_hist_object_id, a.hist_normal = d_hist_normal;
    a.out_color = d_out_color, a.out_len = d_out_len, a.out_moments = d_out_moments, a.error = d_error;
    a.motion = motion, a.n_motion = n_motion;
    return run_reproject(c, a, hip_stream);
}

int pt_ctx_spp_plane(pt_ctx *c, uint32_t width, uint32_t height, uint32_t base, const uint8_t *d_mask, uint32_t masked, uint32_t *d_spp,
                     void *hip_stream) {
    const int rc = host::check_spp_plane(c, width, height, d_spp);
    if (rc) return rc;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        launch_spp_plane(st, d_mask, width * height, base, masked, d_spp);
        return PT_OK;
    });
}

int pt_upsample_defaults(pt_upsample_params *out) {
    return give_defaults(out, pt_upsample_params{kUpsampleDepthTol, kUpsampleNormalMin, 0u});
}

int pt_ctx_upsample(pt_ctx *c, uint32_t width, uint32_t height, uint32_t lo_width, uint32_t lo_height, const pt_upsample_params *params,
                    const float *d_lo_color, const float *d_lo_depth, const int32_t *d_lo_object_id, const float *d_lo_normal,
                    const float *d_lo_albedo, const float *d_depth, const int32_t *d_object_id, const float *d_normal,
                    const float *d_albedo, float *d_out_color, float *d_out_weight, void *hip_stream) {
    UpsampleFrame f;
    const int rc = host::check_upsample(c, width, height, lo_width, lo_height, params, d_lo_color, d_lo_depth, d_lo_object_id, d_lo_normal,
                                        d_lo_albedo, d_depth, d_object_id, d_normal, d_albedo, d_out_color, d_out_weight, f);
    if (rc) return rc;
    return run_image_pass(c, hip_stream, [&](hipStream_t st) {
        launch_upsample(st, f);
        return PT_OK;
    });
}

int pt_ctx_select_pixels(pt_ctx *c, uint32_t width, uint32_t height, const pt_select_params *params, const float *d_weight,
                         const float *d_len, uint8_t *d_mask, uint32_t *n_selected, void *hip_stream) {
    SelectFrame f;
    int rc = host::check_select_pixels(c, width, height, params, d_weight, d_len, d_mask, f);
    if (rc) return rc;
    uint32_t ones = 0u;
    rc = run_image_pass(c, hip_stream, [&](hipStream_t st) {
        const int r2 = c->mk_cnt.ensure(2);
        if (r2) return r2;
        f.count = c->mk_cnt.p;
        HIP_TRY(hipMemsetAsync(f.count, 0, sizeof(uint32_t), st));
        launch_select(st, f);
        if (n_selected) HIP_TRY(hipMemcpyAsync(&ones, f.count, sizeof ones, hipMemcpyDeviceToHost, st));
        return PT_OK;
    });
    if (rc == PT_OK && n_selected) *n_selected = ones;
    return rc;
}

// The mask of a checked call compacted into c->mk_list on `st`; *n: the selected pixels.  The list's length is known only after
// the pass, so a list that turns out too short (the kernel counts every selected pixel and writes the slots it has) is grown to
// the length and the pass runs again: one synchronisation per call once the list has its size.
static int masked_list(pt_ctx *c, const uint8_t *d_mask, uint32_t npix, hipStream_t st, uint32_t *n) {
    int rc;
    if ((rc = c->mk_cnt.ensure(2))) return rc;
    if (!c->mk_list.p && (rc = c->mk_list.ensure(std::min<uint32_t>(npix, 1024u)))) return rc;
    for (;;) {
        uint32_t *const len = c->mk_cnt.p + 1;
        const uint32_t cap = (uint32_t)std::min<size_t>(c->mk_list.n, 0xffffffffu);
        HIP_TRY(hipMemsetAsync(len, 0, sizeof(uint32_t), st));
        launch_masked_compact(st, d_mask, npix, c->mk_list.p, cap, len);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(n, len, sizeof *n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (*n <= cap) return PT_OK;
        if ((rc = c->mk_list.ensure(std::min<uint64_t>(npix, (uint64_t)*n + *n / 4u)))) return rc;
    }
}

int pt_ctx_render_masked(pt_ctx *c, const pt_config *cfg, const uint8_t *d_mask, void *d_rgb, void *hip_stream,
                         const volatile uint8_t *cancel, pt_stats *stats, uint32_t *n_pixels) {
    if (!cfg || !d_mask || !d_rgb) return refuse("NULL argument");
    if (!c) return refuse("ctx is NULL");
    if (!c->has_scene) return refuse("no scene set");
    uint32_t ib = 0, ie = 0;
    int rc;
    if ((rc = host::check_masked_cfg(*cfg)) || (rc = check_cfg(cfg, &ib, &ie))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const double t0 = now_ms();
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_pixels) *n_pixels = 0u;
    uint32_t n = 0u;
    if ((rc = masked_list(c, d_mask, ie - ib, st, &n))) return rc;
    if (n_pixels) *n_pixels = n;
    if (n == 0u) {  // (nothing to trace, and a grid of zero is an error)
        if (stats) stats->ms_total = now_ms() - t0;
        return PT_OK;
    }
    if (cancel && *cancel) {  // (before anything is traced; between the rounds their pacer reads it)
        if (stats) stats->ms_total = now_ms() - t0;
        set_error("cancelled");
        return PT_CANCELLED;
    }
    // the trace: the tile pass over a grid of 1 x 1 tiles, entry k of the compact accumulator being pixel ib + list[k]
    const FrameForm form = form_for(c, cfg->flags);
    const DevScene &S = form.scene;
    const LdsLayout lay = lds_layout(S, 1u, c->tune.lds_pad);
    TileParams F{};
    static_cast<FrameParams &>(F) = make_frame(c, cfg, ib, ie);
    F.chunk_step = 0u;
    F.npix = n;
    F.open = c->mk_list.p;
    F.tile_shift = 0u;
    F.tiles_x = cfg->width;
    F.rows = (ie - ib) / cfg->width;
    if ((rc = c->ad_acc.ensure(3 * (size_t)n)) || (rc = c->ad_rays.ensure(16))) return rc;
    HIP_TRY(hipMemsetAsync(c->ad_acc.p, 0, 3 * (size_t)n * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(c->ad_rays.p, 0, 16 * sizeof(unsigned long long), st));
    LiveScope live(c);  // (the rounds' pacer notes its samples in the live frame)
    Rounds r;
    rc = run_rounds(
        c, cfg, st, cancel, nullptr, nullptr, n, 0u, lay.mega_cand, lay.mega_cand ? 8u : 4u, c->ad_rays.p, c->ad_stack, c->mk_rate,
        [&](uint32_t grid, uint32_t s0, uint32_t s1, uint32_t lane_spp, uint32_t split) {
            launch_tile_pass(st, grid, S, lay, F, c->ad_acc.p, s0, s1, lane_spp, split, c->ad_rays.p, c->ad_stack.p);
        },
        r);
    if (rc) return rc;
    // (the rounds have ended: run_rounds waits for the stream)
    unsigned long long rays[16] = {0};
    HIP_TRY(hipMemcpy(rays, c->ad_rays.p, sizeof rays, hipMemcpyDeviceToHost));
    if (rays[1]) {
        set_error("masked trace: a lane's split stack overflowed");
        return PT_ERR_OVERFLOW;
    }
    if (stats) {
        stats->ray_bounces = rays[0];
        stats->samples = (uint64_t)n * r.s_issued;
        stats->passes = r.launches;
        stats->ms_device = r.ms_device;
    }
    if (r.cancelled) {  // the frame is kept whole: nothing was written
        if (stats) stats->ms_total = now_ms() - t0;
        set_error("cancelled");
        return PT_CANCELLED;
    }
    launch_masked_scatter(st, c->mk_list.p, n, c->ad_acc.p, cfg->spp, (float *)d_rgb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) stats->ms_total = now_ms() - t0;
    return PT_OK;
}

// one band on one device into the host framebuffer
static int render_band_to_host(int dev, const pt_config *cfg, const pt_camera *cam, const pt_object *objs,
                               uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris, float *out_rgb,
                               const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats,
                               std::string *err, uint32_t mem_share = 1) {
    uint32_t ib = 0, ie = 0;
    int rc = check_cfg(cfg, &ib, &ie);
    if (stats) memset(stats, 0, sizeof *stats);
    const uint32_t own = rc ? 0u : owned_pixels(cfg, ib, ie);
    if (!rc && own == 0u) return PT_OK;  // this rank owns no chunk of the band: nothing was created yet
    pt_ctx *c = nullptr;
    if (!rc) rc = pt_ctx_create(dev, &c);
    if (!rc) c->mem_share = mem_share;
    if (!rc) rc = pt_ctx_set_scene(c, cam, objs, n_objs, tris, n_tris);
    float *d_out = nullptr;
    const size_t nfl = (size_t)own * 3;
    if (!rc) {
        hipError_t e = hipMalloc((void **)&d_out, nfl * sizeof(float));
        if (e != hipSuccess) {
            set_error(std::string("hipMalloc(out): ") + hipGetErrorString(e));
            rc = PT_ERR_HIP;
        }
    }
    if (!rc) {
        rc = pt_ctx_render(c, cfg, d_out, nullptr, cancel, cb, user, stats);
        if (rc == PT_OK || rc == PT_CANCELLED) {
            hipError_t e = hipSuccess;
            if (cfg->chunk_step <= 1u) {
                e = hipMemcpy(out_rgb + (size_t)ib * 3, d_out, nfl * sizeof(float), hipMemcpyDeviceToHost);
            } else {  // chunks go back to their places in the frame
                std::vector<float> tmp(nfl);
                e = hipMemcpy(tmp.data(), d_out, nfl * sizeof(float), hipMemcpyDeviceToHost);
                const uint64_t span = ie - ib, C = cfg->chunk_pixels;
                size_t at = 0;
                for (uint64_t ck = cfg->chunk_first; e == hipSuccess && ck * C < span; ck += cfg->chunk_step) {
                    const uint64_t lo = ck * C, hi = (lo + C < span) ? lo + C : span;
                    memcpy(out_rgb + ((size_t)ib + lo) * 3, tmp.data() + at, (size_t)(hi - lo) * 3 * sizeof(float));
                    at += (size_t)(hi - lo) * 3;
                }
            }
            if (e != hipSuccess) {
                set_error(std::string("hipMemcpy(out): ") + hipGetErrorString(e));
                rc = PT_ERR_HIP;
            }
        }
    }
    if (rc && err) *err = g_last_error;  // the message lives in this thread's slot
    if (d_out) (void)hipFree(d_out);
    if (c) pt_ctx_destroy(c);
    return rc;
}

int pt_render(const pt_config *cfg, const pt_camera *cam, const pt_object *objs, uint32_t n_objs,
              const pt_triangle *tris, uint32_t n_tris, float *out_rgb, const volatile uint8_t *cancel,
              pt_progress_fn cb, void *user, pt_stats *stats) {
    if (!out_rgb) return refuse("out_rgb is NULL");
    int dev = 0;
    if (const char *e = getenv("PT_DEVICE")) dev = atoi(e);
    return render_band_to_host(dev, cfg, cam, objs, n_objs, tris, n_tris, out_rgb, cancel, cb, user, stats, nullptr);
}

int pt_render_multi(const pt_config *cfg, uint32_t n_ranks, const pt_camera *cam, const pt_object *objs,
                    uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris, float *out_rgb,
                    const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats) {
    if (!out_rgb || n_ranks == 0 || n_ranks > 64) return refuse("out_rgb is NULL or n_ranks outside 1..64");
    uint32_t ib = 0, ie = 0;
    int rc = check_cfg(cfg, &ib, &ie);
    if (rc) return rc;
    const int n_dev = device_count_quiet();
    if (n_dev <= 0) {
        set_error("no HIP device: libptrace_hip has no CPU fallback");
        return PT_ERR_NO_DEVICE;
    }
    // rank r renders the chunks r, r+n_ranks, ... of [ib, ie) (one chunk = one image row) on device r mod n_dev:
    // interleaving evens out the cost per rank; pixels are independent and the RNG is keyed on the global pixel
    // index, so the image does not depend on n_ranks (mod.rs:1021-1023)
    std::vector<pt_config> cfgs(n_ranks, *cfg);
    std::vector<pt_stats> sts(n_ranks);
    std::vector<int> rcs(n_ranks, PT_OK);
    std::vector<std::string> errs(n_ranks);
    std::vector<std::thread> th;
    const double t0 = now_ms();
    Relay relay{cb, user};  // pipeline 0 / rank 0 reports for the call
    for (uint32_t r = 0; r < n_ranks; ++r) {
        cfgs[r].idx_begin = ib;
        cfgs[r].idx_end = ie;
        if (n_ranks > 1) {
            cfgs[r].chunk_pixels = cfg->width;
            cfgs[r].chunk_first = r;
            cfgs[r].chunk_step = n_ranks;
        }
        if (owned_pixels(&cfgs[r], ib, ie) == 0u) continue;  // more ranks than chunks
        // ranks r, r + n_dev, ... share device r % n_dev: each takes its share of that device's memory for its ray queues
        const uint32_t dev = r % (uint32_t)n_dev;
        const uint32_t on_dev = (n_ranks - dev + (uint32_t)n_dev - 1u) / (uint32_t)n_dev;
        th.emplace_back([&, r, dev, on_dev]() {
            rcs[r] = render_band_to_host((int)dev, &cfgs[r], cam, objs, n_objs, tris, n_tris, out_rgb, cancel,
                                         (r == 0 && cb) ? &Relay::fn : nullptr, &relay, &sts[r], &errs[r], on_dev);
        });
    }
    for (auto &t : th) t.join();
    if (stats) {
        memset(stats, 0, sizeof *stats);
        add_stats_concurrent(stats, sts);
        stats->ms_total = now_ms() - t0;
    }
    for (uint32_t r = 0; r < n_ranks; ++r)
        if (rcs[r] != PT_OK) {
            set_error("rank " + std::to_string(r) + ": " + errs[r]);
            return rcs[r];
        }
    if (cb) cb(user, 1.0f);  // every rank has finished and its rows are in out_rgb
    return PT_OK;
}

#ifdef PT_WALK_STATS
// instrumented builds only (tools/walk_stats.py): read and clear the walk counters
int pt_debug_walk_stats(pt_ctx *c, unsigned long long *out16) {
    if (!c || !c->scene.stats) return PT_ERR_INVALID;
    hipDeviceSynchronize();
    hipMemcpy(out16, c->scene.stats, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    hipMemset(c->scene.stats, 0, 16 * sizeof(unsigned long long));
    return PT_OK;
}
#endif

#ifdef PT_PHASE_STATS
// instrumented builds only (tools/phase_budget.py): read and clear the phase counters; returns the number of phases
int pt_debug_phase_stats(pt_ctx *c, unsigned long long *out, uint32_t cap) {
    if (!c || !c->scene.phase_stats || cap < kPhCount * 3 + 2) return PT_ERR_INVALID;
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(out, c->scene.phase_stats, (kPhCount * 3 + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipMemset(c->scene.phase_stats, 0, (kPhCount * 3 + 2) * sizeof(unsigned long long));
    return (int)kPhCount;
}
#endif

#ifdef PT_TAIL_STATS
// instrumented builds only (tools/tail_probe.py): read and clear the begin / end stamps of the first n workgroups of the launches
// since the last call (a later launch writes over an earlier one: the probe renders one pass); returns the table's capacity
int pt_debug_tail_stats(pt_ctx *c, unsigned long long *out, uint32_t n) {
    if (!c || !c->scene.tail_stats || n > kTailStatsCap) return PT_ERR_INVALID;
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(out, c->scene.tail_stats, 2 * (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipMemset(c->scene.tail_stats, 0, 2 * (size_t)kTailStatsCap * sizeof(unsigned long long));
    return (int)kTailStatsCap;
}
#endif

}  // extern "C"
