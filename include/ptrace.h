/*
 * ptrace.h — C ABI of libptrace_hip.so, the MI355X (gfx950) implementation of the
 * per-pixel radiance() path-tracing loop of filippo-orru/path-tracer-rust.
 *
 * The reference has no FFI/plugin interface (it is safe Rust only).  The narrowest seam is
 * the parallel section of render() — src/render/mod.rs:1017-1024 — which fills
 * `pixels: Vec<Vec3>` (index (H-1-y)*W+x, mod.rs:805-806) for a RenderConfig
 * (mod.rs:859-864) under a cancel flag (mod.rs:943,1003) and a progress counter
 * (mod.rs:960,850).  pt_render() replaces exactly that loop; everything in this header is
 * what a Rust `extern "C"` block for that seam would bind (INTEGRATION.md shows the shim).
 *
 * Conventions: plain pointers and sizes, caller owns every buffer, no unwinding, every
 * entry point returns an int status (PT_OK or a negative PT_ERR_*), message through
 * pt_last_error().  There is no CPU fallback: without a HIP device every compute entry
 * point fails with PT_ERR_NO_DEVICE.
 */
#ifndef PTRACE_H
#define PTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 5

/* status codes (reference behaviour: unwrap() panics, mod.rs:96,309,1032,1042,1093) */
#define PT_OK 0
#define PT_ERR_INVALID (-1)    /* bad argument / malformed scene */
#define PT_ERR_NO_DEVICE (-2)  /* no HIP device (the product never falls back to the CPU) */
#define PT_ERR_HIP (-3)        /* a HIP runtime call failed; text in pt_last_error() */
#define PT_CANCELLED (-4)      /* *cancel became non-zero; framebuffer = the samples accumulated so far / their count */
#define PT_ERR_OVERFLOW (-5)   /* a ray queue overflowed (cannot happen with the sizes pt_render picks) */
#define PT_ERR_IO (-6)         /* file could not be read / written */
#define PT_ERR_PARSE (-7)      /* scene JSON / OFF syntax or shape error */
#define PT_ERR_COMM (-8)       /* an RCCL call failed (pt_comm_*); text in pt_last_error() */

/* ReflectType — enum order of src/render/mod.rs:71-76 */
#define PT_DIFFUSE 0u
#define PT_SPECULAR 1u
#define PT_REFRACT 2u

/* SceneObject kind — src/render/mod.rs:326-335 */
#define PT_SPHERE 0u
#define PT_MESH 1u

/* backends of the hot path (both run on the GPU) */
#define PT_BACKEND_WAVEFRONT 0u /* SoA ray queues in HBM, generate/intersect/shade kernels per bounce */
#define PT_BACKEND_MEGAKERNEL 1u /* persistent threads: whole render_pixel loop per lane (two interleaved paths), no ray queues */

/* pt_config.flags */
#define PT_FLAG_NO_BVH 1u /* meshes are scanned triangle by triangle as the reference does (mod.rs:558) */
/* Wavefront backend: generate / intersect / shade as separate kernels per depth even where a whole pass could run as
 * one launch (scenes without BVH meshes).  Same image, bit for bit; for A/B checks and per-step profiling. */
#define PT_FLAG_SEPARATE_KERNELS 2u
/* Concurrent pipelines (wavefront backend): bits 8..11 of flags = n (2..8).  The call's pixels are dealt chunk by
 * chunk to n independent wavefront pipelines on n HIP streams of the same GPU, so the VALU-bound intersect kernels
 * of one pipeline overlap the HBM-bound shade kernels of another (cornell: +15 % with 2; 3 or more only help when
 * the runtime exposes enough hardware queues, GPU_MAX_HW_QUEUES=8).  Same
 * image, bit for bit.  Per-kernel timings (pt_stats.ms_intersect, rocprof) then describe kernels that share the
 * machine, which is why it is opt-in: the default single pipeline keeps per-kernel roofline numbers meaningful. */
#define PT_FLAG_PIPELINES(n) (((uint32_t)(n) & 15u) << 8)

/* CameraData — src/render/mod.rs:162-176.  `direction` is used as stored (not renormalised). */
typedef struct pt_camera {
    float position[3];
    float direction[3];
    float focal_length;
    float sensor_width;
    float aspect_ratio;
} pt_camera;

/* Triangle — src/render/mod.rs:538-543, object-local vertices. */
typedef struct pt_triangle {
    float a[3];
    float b[3];
    float c[3];
} pt_triangle;

/* SceneObjectData + Material flattened — src/render/mod.rs:253-258, 78-83, 326-335, 440-448.
 * For PT_MESH, triangles [tri_offset, tri_offset+tri_count) of the triangle array belong to the
 * object and (bs_center, bs_radius) is Mesh.bounding_sphere exactly as stored/computed
 * (object-local centre; mod.rs:268 adds `position`). */
typedef struct pt_object {
    uint32_t kind;
    float position[3];
    float radius; /* PT_SPHERE only */
    float color[3];    /* every component finite and >= 0 (-0.0f counts as 0): see pt_ctx_set_scene */
    float emission[3]; /* the same; the reference spells it `emmission` */
    uint32_t reflect_type;
    uint32_t tri_offset;
    uint32_t tri_count;
    float bs_center[3];
    float bs_radius;
} pt_object;

/* RenderConfig + Resolution (src/render/mod.rs:859-870) plus what the GPU path needs. */
typedef struct pt_config {
    uint32_t width;
    uint32_t height;
    uint32_t spp;      /* samples_per_pixel */
    uint32_t backend;  /* PT_BACKEND_* */
    uint64_t seed;     /* key of the counter-based RNG that stands in for rand::random (mod.rs:53) */
    uint32_t idx_begin; /* framebuffer-index band [idx_begin, idx_end) to render; 0,0 = whole frame */
    uint32_t idx_end;
    uint32_t rays_per_pass; /* wavefront: primary rays per pass (megakernel: primary samples per round); 0 = the library's own:
                             * passes sized by measured time, at most 512 Mi primary rays - cancel and progress are looked
                             * at between passes */
    uint32_t flags;
    /* Interleaved partition of the band for load balance across ranks (the cost of a pixel varies over the
     * image: contiguous eighths of cornell.json differ by up to 1.31x).  The band is cut into chunks of
     * chunk_pixels framebuffer indices; this call renders chunks chunk_first, chunk_first+chunk_step, ... and
     * writes them back to back into the output.  chunk_step = 0 or 1: the whole band (the other two ignored). */
    uint32_t chunk_pixels;
    uint32_t chunk_first;
    uint32_t chunk_step;
    /* Minimum interval between two progress callbacks, in milliseconds.  0 = 500, the reference's RenderUpdate cadence
     * (mod.rs:965-982); PT_PROGRESS_EVERY_PASS = at every pass boundary (a few milliseconds apart).  The cancel byte is
     * read at every pass boundary whatever this says (the reference polls it every 100 ms, mod.rs:947-958). */
    uint32_t progress_ms;
} pt_config;
#define PT_PROGRESS_EVERY_PASS 0xffffffffu

typedef struct pt_stats {
    uint64_t ray_bounces;        /* number of intersect_scene evaluations (mod.rs:663), exact */
    uint64_t samples;            /* primary samples traced */
    uint64_t intersect_rays;     /* rays processed by the dominant kernel (== ray_bounces for wavefront) */
    uint32_t intersect_launches; /* launches of the dominant kernel: k_pass (one per pass) or, for BVH scenes, k_intersect */
    uint32_t passes;
    double ms_total;     /* wall time of the call */
    double ms_device;    /* HIP-event time from first to last kernel of the call */
    double ms_intersect; /* HIP-event time summed over those launches (only if PT profiling on) */
} pt_stats;

/* Progress callback: fraction in [0,1], between passes (and between the parts of a very large call), at most every
 * pt_config.progress_ms, and once with 1.0 when the frame is complete and in the output buffer.  pt_ctx_render invokes it
 * on the calling thread; pt_render_multi and PT_FLAG_PIPELINES render on worker threads and invoke it from the worker of
 * rank / pipeline 0 - a GUI host has to marshal it - except for the final 1.0, which comes from the calling thread after
 * every rank / pipeline has finished.  It may raise the
 * cancel byte: the render then stops at that boundary.  It may call pt_ctx_snapshot on the context it was given to
 * (not under PT_FLAG_PIPELINES, where the accumulators live in child contexts: the snapshot reports an error). */
typedef void (*pt_progress_fn)(void *user, float fraction);

typedef struct pt_ctx pt_ctx;

const char *pt_version(void);
/* the back-end (-mllvm) switches the library was built with, "<general set> | flat: <set of the pass kernel without walks>": the
 * Makefile probes each against the compiler and drops the ones it rejects (they only steer instruction placement: same images
 * with any subset) */
const char *pt_build_flags(void);
/* the first 16 hex digits of sha256 over the device assembly the library's kernels were built from (Makefile: pt_kernels.s of
 * the same compile): the _traffic.json files under profiles/ name the hash of the library they were measured on, bench.py compares */
const char *pt_kernel_isa_hash(void);
const char *pt_last_error(void);
int pt_abi_version(void);
int pt_device_count(void);

/* a3 — CameraData::{lens_center, orthogonals} (mod.rs:211-232), host arithmetic in f32. */
int pt_camera_basis(const pt_camera *cam, float lens_center[3], float su[3], float sv[3]);

/* a10 — Mesh::new bounding sphere (mod.rs:450-499), including its `min + max*0.5` centre. */
int pt_mesh_bounding_sphere(const pt_triangle *tris, uint32_t n_tris, float center[3], float *radius);

/* One context = one GPU, one stream, device copies of one scene and the ray queues. */
int pt_ctx_create(int device, pt_ctx **out);
void pt_ctx_destroy(pt_ctx *ctx);
/* PT_ERR_INVALID, the context left as it was, pt_last_error naming the object and the field: an unknown kind or reflect_type, a
 * triangle range outside the array or shared by two objects, BVHs beyond pt_bvh_refs_fit, and a component of color or emission
 * that is negative or not finite (NaN included).  The last because radiance is summed in unsigned fixed point (see "progressive
 * accumulation" below): a contribution is a product of these components, and the conversion is defined for finite values >= 0
 * only.  pt_render and pt_render_multi refuse the same scenes, pt_ctx_set_object the same materials. */
int pt_ctx_set_scene(pt_ctx *ctx, const pt_camera *cam, const pt_object *objs, uint32_t n_objs,
                     const pt_triangle *tris, uint32_t n_tris);

/* Move the camera of the scene pt_ctx_set_scene gave, without building the scene again: what a viewport calls per frame.
 * REACH.  The device tables of a scene (BVH box paddings, bounding-sphere shortcuts, filter pads) rest on error bounds derived
 * from ONE box B = [lo, hi]: the box that bounds every ray origin - the objects and the lens centre (pt_camera_basis).  Nothing
 * else of the camera enters them, so they hold unchanged for every camera whose lens centre lies inside B.  pt_ctx_set_scene sets
 * B to the objects' box grown by its camera's lens centre (pt_scene_reach computes that box on the host, without a device);
 * pt_ctx_camera_reach returns the box in force.
 * SAME CAMERA: *cam bitwise equal to the context's (nine floats): nothing changes, both held frames stay, *rebuilt = 0.
 * FAST PATH (*rebuilt = 0): lo[a] <= lens[a] <= hi[a] on all three axes.  The context takes the camera, drops the frame
 * pt_ctx_accumulate holds and the held adaptive frame (their key includes the camera, as under pt_ctx_set_scene) and marks the
 * checkpoint fingerprint stale.  Nothing else: no flattening, no HIP call (but the release of a held frame's planes), no device
 * memory touched; the measured pass and round rates, the boxes of pt_ctx_set_mesh_bounds and the scratch of the denoisers,
 * pt_ctx_present and pt_ctx_reproject_var are kept.
 * SLOW PATH (*rebuilt = 1): the lens centre is outside B.  B grows geometrically, in binary32, per axis: lens[a] < lo[a] gives
 * lo[a] = lens[a] - (lo[a] - lens[a]); lens[a] > hi[a] gives hi[a] = lens[a] + (lens[a] - hi[a]); a bound that is not violated
 * stays.  The scene is flattened again for the new box from the context's host copies of the objects and triangles (it keeps
 * the triangles: 36 B each) and uploaded as pt_ctx_set_scene uploads it, then the camera is taken as on the fast path.  The
 * overshoot doubles: a dolly outwards costs O(log distance) rebuilds, an orbit is back on the fast path after a few.  The boxes of
 * pt_ctx_set_mesh_bounds and the measured rates survive.  If flattening fails the context is left as it was.
 * EQUIVALENCE.  After pt_ctx_set_camera(cam1), on either path, every entry point returns what it returns after
 * pt_ctx_set_scene(cam1, the same objects and triangles), bit for bit: frames, AOVs, queries, pt_stats.ray_bounces.  The device
 * tables may differ in their paddings; the results may not (the tables only ever decide what is tested exactly, never a result).
 * pt_ctx_accum_save / pt_ctx_adaptive_save write the fingerprint pt_ctx_set_scene(cam1, ...) would have given - computed at the
 * first save or load after a camera change, never by this call - so checkpoints interchange.
 * PT_ERR_INVALID, in this order, nothing changed: ctx NULL; cam NULL; no scene; a lens centre that is not finite.  rebuilt may
 * be NULL.  Like pt_ctx_set_scene, not to be called from a progress callback. */
int pt_ctx_set_camera(pt_ctx *ctx, const pt_camera *cam, int *rebuilt);
/* the box B in force (see pt_ctx_set_camera); PT_ERR_INVALID without a scene */
int pt_ctx_camera_reach(const pt_ctx *ctx, float lo[3], float hi[3]);
/* Pay pt_ctx_set_camera's rebuild once, up front: if [lo, hi] is not inside B, B becomes the union of the two and the scene is
 * rebuilt for it (*rebuilt = 1); otherwise nothing happens (*rebuilt = 0).  The camera does not change and the held frames stay.
 * PT_ERR_INVALID for lo[a] > hi[a], a bound that is not finite, or no scene. */
int pt_ctx_reserve_camera_reach(pt_ctx *ctx, const float lo[3], const float hi[3], int *rebuilt);
/* The box pt_ctx_set_scene would derive its bounds for: min / max in binary32 over the lens centre, every sphere's centre -/+
 * |radius| and every mesh vertex + the object's position.  Host only, no device. */
int pt_scene_reach(const pt_camera *cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris,
                   float lo[3], float hi[3]);

/* Replace object `index` of the scene pt_ctx_set_scene gave, without building the scene again: what a host calls per mouse move
 * while the user drags a sphere, nudges a mesh or changes a colour.  The triangle array is not touched.
 * REACH.  As under pt_ctx_set_camera: the device tables depend on the scene only through the box B (pt_ctx_camera_reach) that
 * bounds every ray origin, and otherwise each record on its own object.  So while an edited object stays inside B, only that
 * object's records change.  The object's bounds, in binary32: a sphere's centre -/+ |radius|; a mesh's object-local vertex box,
 * cached at pt_ctx_set_scene, plus position (addition is monotone, so this is what pt_scene_reach computes vertex by vertex).
 * SAME: *obj bitwise equal to the context's copy (nineteen words): nothing changes, both held frames stay, *rebuilt = 0.
 * MATERIAL path (*rebuilt = 0): only color, emission or reflect_type differ.  The object's material record, the surface records
 * at its ranks and the glass deferral, as pt_ctx_set_scene derives it, are updated; no geometry table is touched.
 * MOVE path, in reach (*rebuilt = 0): position, radius, bs_center or bs_radius differ (the material may too) and
 * lo[a] <= bounds.lo[a], bounds.hi[a] <= hi[a] on all three axes.  Only this object's records are rewritten, at their offsets in
 * the device tables.  A mesh with a BVH (16 triangles or more) keeps its tree and is REFIT ON THE DEVICE: the first such edit of
 * a mesh uploads its object-local triangles (36 B each) and a plan of its tree; from then on no triangle crosses to the device -
 * one lane per leaf recomputes the pair records, normals and padded boxes, one launch per height of the tree unites the boxes
 * bottom-up, one gathers the four-wide nodes.  Every edit recomputes from the object-local triangles: a sequence of moves does
 * not drift.  Smaller meshes and spheres are recomputed on the host by the code pt_ctx_set_scene runs.
 * OUT OF REACH (*rebuilt = 1): B grows per axis by pt_ctx_set_camera's rule applied to the violated bounds:
 * bounds.lo[a] < lo[a] gives lo[a] = bounds.lo[a] - (lo[a] - bounds.lo[a]); bounds.hi[a] > hi[a] gives
 * hi[a] = bounds.hi[a] + (bounds.hi[a] - hi[a]); the overshoot doubles.  The scene is flattened again for the new box from the
 * context's host copies and uploaded, exactly as on pt_ctx_set_camera's slow path.  If flattening fails the context is left as it was.
 * AFTERWARDS, on every path but SAME: the context's copy of the object is *obj; the frame pt_ctx_accumulate holds and the held
 * adaptive frame are dropped; the checkpoint fingerprint is marked stale (the next save or load computes the one
 * pt_ctx_set_scene would have given); the boxes of pt_ctx_set_mesh_bounds are marked dirty, because they take the object's
 * position.  The measured pass and round rates and the image passes' scratch are kept.  The call returns when the tables are final.
 * EQUIVALENCE.  After the call, on any path, every entry point returns what it returns after pt_ctx_set_scene(the context's
 * camera, the edited objects, the same triangles), bit for bit: frames on both backends and every scan form, AOVs,
 * pt_ctx_intersect*, pt_ctx_intersect_bounds, pt_ctx_orbit_point, pt_ctx_scatter, pt_stats.ray_bounces, checkpoints.  The tables
 * may differ in their paddings and, for a mesh with a BVH, in the tree's topology (a refit keeps the tree a build would choose
 * anew); the results may not.
 * PT_ERR_INVALID, in this order, nothing changed, before any device is touched: ctx NULL; obj NULL; no scene; index >= n_objs;
 * kind, tri_offset or tri_count differ from the object's (topology edits go through pt_ctx_set_scene);
 * reflect_type > PT_REFRACT; a position, radius, bs_center or bs_radius that is not finite; a component of color or emission
 * that is negative or not finite (as pt_ctx_set_scene refuses it).  rebuilt may be NULL.  One object per
 * call.  Like pt_ctx_set_scene, not to be called from a progress callback. */
int pt_ctx_set_object(pt_ctx *ctx, uint32_t index, const pt_object *obj, int *rebuilt);

/* Diagnostics: pt_siphash(1, 3, 0, 0, ...) over each device table of the scene, downloaded - what the tests compare a refit's
 * tables by.  On a scene whose arithmetic is exact (coordinates and moves that are multiples of 1/8, far below 2^20) an edited
 * context holds, under the same box B, the tables a fresh pt_ctx_set_scene builds, to the bit.  PT_ERR_INVALID without a scene. */
enum {
    PT_TABLE_OBJS = 0,
    PT_TABLE_OBJ_PAIRS,
    PT_TABLE_TRI_PAIRS,
    PT_TABLE_MATS,
    PT_TABLE_TRI_SHADE,
    PT_TABLE_BVH_NODES,
    PT_TABLE_BVH_NODES4,
    PT_TABLE_SPH_PAIRS,
    PT_TABLE_FLAT_PAIRS,
    PT_TABLE_CAND_PAIRS,
    PT_TABLE_RANK_ID,
    PT_TABLE_SURF,
    PT_TABLE_TRI_RANK,
    PT_TABLE_BVH_MESHES,
    PT_TABLE_COUNT
};
int pt_ctx_table_hashes(pt_ctx *ctx, uint64_t out[PT_TABLE_COUNT]);

/* Number of pixels a call with this config renders (the band, or this rank's chunks of it); 0 on a bad config. */
uint32_t pt_config_pixels(const pt_config *cfg);

/* Render the band [idx_begin, idx_end) (or this rank's chunks of it) into DEVICE memory: d_out_rgb holds
 * pt_config_pixels(cfg)*3 floats, pixel k of the call at element k*3+c, linear, clamped to [0,1] — for an
 * un-chunked band the memory image of the reference's Vec<Vec3> slice (mod.rs:1013-1014, 852-856).
 * `hip_stream` is a hipStream_t (NULL = the context's own stream).  Blocking.  Everything the call reads from or writes to the
 * caller's memory is ordered on that stream, after whatever is pending on it when the call is made, and has completed when the
 * call returns; the same holds for every entry point that takes a `hip_stream`, under every flag and backend.
 * Cancel (both backends): *cancel is read between passes (wavefront) / rounds (megakernel), which the library sizes by MEASURED
 * time when rays_per_pass is 0 - a tiny timed first pass of a scene, then as many samples as fit 100-120 ms, the rate kept with
 * the context - so a cancel comes back within about a tenth of a second whatever a ray of the scene costs (the reference polls
 * its flag every 100 ms, mod.rs:947-958); with an explicit rays_per_pass a pass is as long as asked for.  On PT_CANCELLED the
 * buffer holds every pixel averaged over the samples that were accumulated (stats->samples / pixels of the call), all zero if
 * none - the picture pt_ctx_snapshot would have given. */
int pt_ctx_render(pt_ctx *ctx, const pt_config *cfg, void *d_out_rgb, void *hip_stream,
                  const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats);

/* Device buffers for hosts that have no GPU allocator of their own (a Rust/C host driving pt_ctx_render;
 * tests).  Plain hipMalloc / hipFree / hipMemcpy on `device`. */
int pt_device_malloc(int device, size_t bytes, void **out);
int pt_device_free(int device, void *p);
int pt_device_download(int device, void *dst_host, const void *src_device, size_t bytes);

/* Size limit of one scene's BVHs (pt_ctx_set_scene fails with PT_ERR_INVALID beyond it): the walkers pack a node index or a
 * leaf code (first pair record << 1 | records - 1: a leaf is one or two pair records) into 26 bits of a queue entry - 2^26
 * nodes, 2^25 pair records (two triangles each) over all BVH meshes of the scene.  1 = fits. */
int pt_bvh_refs_fit(uint64_t n_bvh_nodes, uint64_t n_pair_records);

/* Device memory the wavefront backend may take for its ray queues in this context (bytes; 0 = the default: 85 % of what
 * the device reports free, divided among the contexts one call creates on it).  The default kernel (k_pass_cand) keeps
 * each wave's waiting rays on a stack of at most 1024 slots: K streams x 4 waves x 40 KB, whatever the pass holds (5.9 GB
 * for the 35 747 streams of a 1024x768 pass of 683 samples; small passes need less); the level-by-level forms (PT_FLAG_SEPARATE_KERNELS,
 * PT_FLAG_NO_BVH, PT_CAND_SCAN=0) hold rays_per_pass primary rays at 352 B each, 36 GB at their default.  A pass that does
 * not fit is halved until it does (a failed allocation does the same), which changes how the samples are batched and
 * nothing in the image.  A figure set here also bounds an explicit pt_config.rays_per_pass (the budget wins); without one
 * an explicit rays_per_pass is taken as given and only a failed allocation halves it. */
int pt_ctx_set_memory_budget(pt_ctx *ctx, size_t bytes);

/* Enable HIP-event timing of every launch of the dominant kernel (fills pt_stats.ms_intersect). */
int pt_ctx_set_profiling(pt_ctx *ctx, int enabled);
/* Name of the kernel the wavefront backend launches for this context's scene with these pt_config.flags - the one
 * pt_stats.intersect_launches / ms_intersect describe: "k_pass_cand" (one launch per pass, candidate scan: scenes
 * without BVH meshes), "k_pass_cand_bvh" (the same kernel's form for scenes with BVH meshes: candidate scan + parked
 * walks), "k_pass" (every triangle tested per ray), "k_pass_bvh" (scan + depth-first parked walks: PT_CAND_BVH=0),
 * or, with separate kernels, "k_intersect_cand" (the stand-alone intersect step with the candidate scan: scenes without BVH
 * meshes) / "k_intersect" (every triangle per ray, or scan + walks for BVH scenes).  For profilers and bench.py; NULL without
 * a scene. */
const char *pt_ctx_pass_kernel(const pt_ctx *ctx, uint32_t flags);

/* radiance(&ray, depth, &scene) (mod.rs:661-792) for ONE given ray, averaged over n_samples independent evaluations:
 * what the reference's own test_radiance does (src/render/test.rs:146-183: the sum of 10 000 calls with depth 0 divided
 * by their number), and the entry point through which hand-derived cases reach roulette / emission / specular / refract /
 * Fresnel on the device (tests/kats_shading.py; `depth` 2 and 5 put the first hit behind mod.rs:760 and mod.rs:677).
 * Sample i draws from the RNG stream (seed; counter = pixel, i, ...) exactly as sample i of framebuffer index `pixel`
 * would - `pixel` is only that counter, no frame is involved - so the oracle's pto_radiance_mean_at with the same
 * arguments walks the same paths.  depth < 12 (MAX_DEPTH, mod.rs:661).  backend / flags as in pt_config (PT_FLAG_PIPELINES
 * is refused).  out_rgb = the mean, NOT clamped (the reference clamps in render_pixel, mod.rs:852-856, not in radiance);
 * stats->ray_bounces = intersect_scene evaluations, exact.  Host pointers; blocking. */
int pt_ctx_radiance(pt_ctx *ctx, const float o[3], const float d[3], uint32_t depth, uint32_t n_samples, uint64_t seed,
                    uint32_t pixel, uint32_t backend, uint32_t flags, float out_rgb[3], pt_stats *stats);

/* Single-ray queries through the same device intersection code (a6): the callers are object
 * picking / click-debug / orbit pivot (src/views/viewport_tab.rs:240-246, render_tab.rs:177-205).
 * Host arrays: o,d = n*3 floats; outputs may be NULL.  object_id = -1 on a miss
 * (intersect_scene -> None), tri_id = index into the object's triangle list or -1 for spheres.
 * Bit-for-bit agreement with the reference's intersect_scene is guaranteed for rays like the path tracer's own:
 * direction of unit length (the reference normalises every direction it casts) and origin where its rays start - inside the bounding box of the scene's objects and of the camera given to
 * pt_ctx_set_scene: the error bounds behind the BVH boxes and the bounding-sphere shortcuts assume that distance
 * scale (pt_host.cpp).  A picking ray from a camera far outside the scene still gets the nearest hit, but a hit that
 * only exists through f32 round-off of the reference's arithmetic at that distance may be resolved differently. */
int pt_ctx_intersect(pt_ctx *ctx, const float *o, const float *d, uint32_t n, float *t,
                     int32_t *object_id, int32_t *tri_id, float *x, float *normal);

/* Diagnostics: intersect_scene (mod.rs:631-659) for n rays through the INTERSECT STEP OF THE WAVEFRONT PIPELINE itself - the
 * rays are laid out as ray streams and run through the kernel PT_FLAG_SEPARATE_KERNELS launches per depth (candidate scan:
 * conservative filters, per-wave ring, dense exact batches; with PT_FLAG_NO_BVH every triangle per ray; scenes with BVH
 * meshes: scan + parked walks) - where pt_ctx_intersect above goes through the single-ray query kernel.  t[i] = the hit
 * distance (+inf on a miss), id[i] = -1 (miss), the object index of a sphere, or n_objs + the flattened triangle index.
 * For ray-by-ray parity tests of the scan forms (rays that start ON a triangle included).  The same precondition as
 * pt_ctx_intersect above: bit-for-bit agreement with intersect_scene holds for directions of unit length and origins inside
 * the bounding box of the scene's objects and camera - the conservative filters and box tests these kernels run first
 * (pt_host.cpp) rest on error bounds that assume both. */
int pt_ctx_intersect_streams(pt_ctx *ctx, const float *o, const float *d, uint32_t n, uint32_t flags, float *t, int32_t *id);

/* SceneObjectData::intersect_bounds (mod.rs:282-290) of object `object` for n rays: a sphere is tested itself
 * (intersect_sphere), a mesh through Triangle::intersect over the 12 triangles of Mesh.bounding_box.  hit[i] = 1/0;
 * t / x / normal as Hit holds them (zero on a miss).  Outputs may be NULL. */
int pt_ctx_intersect_bounds(pt_ctx *ctx, uint32_t object, const float *o, const float *d, uint32_t n, int32_t *hit,
                            float *t, float *x, float *normal);
/* get_orbit_point (src/views/viewport_tab.rs:401-431): objects from the last to the first; an object whose bounds are
 * hit contributes its real hit if it has one, else the bounds hit; the nearest (strict <) wins.  found[i] = 1/0, point =
 * hit.intersection, object_id = the object that supplied it (-1), t = its distance. */
int pt_ctx_orbit_point(pt_ctx *ctx, const float *o, const float *d, uint32_t n, int32_t *found, float *point,
                       int32_t *object_id, float *t);
/* Mesh.bounding_box of a mesh object (12 object-local triangles).  pt_ctx_set_scene computes it as Mesh::new does
 * (mod.rs:452-476, 501-536); an inline Mesh of a scene file carries its own (deserialised verbatim, mod.rs:440-448) -
 * pass that one here (pt_scene_bounding_box) when it may differ. */
int pt_ctx_set_mesh_bounds(pt_ctx *ctx, uint32_t object, const pt_triangle box[12]);
/* bounding_box_to_triangles over the AABB of the triangles, as Mesh::new stores it (mod.rs:452-476, 501-536) */
int pt_mesh_bounding_box(const pt_triangle *tris, uint32_t n_tris, pt_triangle out[12]);

/* Diagnostics: evaluate the device's numerics contract (sin, cos, sqrt, 1/x on in[i]; Philox block for
 * counter (i, bits(in[i]), (i<<8)|(i&15), 0), key 0x0123456789abcdef) so tests can compare it bit for bit
 * with the host.  Host arrays of n (out_philox: 4n). */
int pt_ctx_numerics_probe(pt_ctx *ctx, const float *in, uint32_t n, float *out_sin, float *out_cos,
                          float *out_sqrt, float *out_rcp, uint32_t *out_philox);

/* Diagnostics, exhaustive: the device's f_sqrt against the compiler's IEEE square root on all 2^32 binary32 bit patterns
 * and its f_rcp against IEEE 1/d on every normal d with 2^-126 <= |d| <= 2^126 (the domain its callers keep to).
 * out[0], out[1] = inputs whose results differ in bits (NaN == NaN) - both must be 0; out[2], out[3] = inputs compared.
 * About a second of GPU time. */
int pt_ctx_numerics_sweep(pt_ctx *ctx, uint64_t out[4]);

/* Diagnostics, exhaustive: the device's sincos_f32 - the one transcendental of the path, cos / sin of r1 = 2 pi rand01()
 * in the diffuse bounce (mod.rs:691,703) - on ALL 2^24 arguments that expression can take (rand01() = k * 2^-24, rand
 * 0.8.5's f32 mapping) against the host instantiation of the same source (pt_host_sincos, which tests/test_abi.py holds to
 * the platform libm on the same arguments).  out[0] = arguments whose sine or cosine differs in bits (must be 0),
 * out[1] = arguments compared (2^24).  Uploads two 64 MB tables; well under a second of GPU time. */
int pt_ctx_sincos_sweep(pt_ctx *ctx, uint64_t out[2]);

/* Diagnostics: the per-sample part of render_pixel (mod.rs:805-843) - y = H-1 - idx/W, x = idx%W, the (s%2, (s/2)%2)
 * sub-pixel, the tent filter of two rand01() draws, sx / sy, sensor_pos = (position + su*sx) + sv*sy, direction =
 * (lens_center - sensor_pos).normalize(), origin = lens_center - ON THE DEVICE, through the functions the frame kernels
 * call, for n (framebuffer index, sample) pairs of a width x height frame with the context's camera; the two draws are
 * words 0 and 1 of the RNG block (seed; pixel, sample, tag 0).  form 0: as k_generate / k_mega / k_pass make it (column and
 * row by division), form 1: as k_pass_cand makes it (column and row handed in).  The oracle's pto_primary_ray is the
 * counterpart; tests/kats_camera.py holds both to an independent restatement, bit for bit.  Host arrays: o, d = n*3. */
int pt_ctx_primary_rays(pt_ctx *ctx, uint32_t width, uint32_t height, uint64_t seed, const uint32_t *pixel,
                        const uint32_t *sample, uint32_t n, uint32_t form, float *o, float *d);

/* Diagnostics: ONE radiance() invocation after its intersect_scene call (mod.rs:665-789) - the roulette verdict, the diffuse
 * basis and direction, the mirror direction, tdir, Re / Tr / P, the split, the children's depth and branch - ON THE DEVICE,
 * through the functions the frame kernels call (shade_surface, fetch_surface, fetch_surface_rank: called, not copied), for n
 * items.  An item is the ray, the throughput above it and its RNG key: the draws are words 0 (roulette), 1 (diffuse r1 / the
 * refract choice) and 2 (diffuse r2) of the block (seed; pixel, sample, tag (branch << 8) | (depth + 1)).  `form` says where
 * the surface comes from and which instantiation of the shading step runs:
 *   PT_SCATTER_GIVEN      surfaces[i] is the surface (hit point, normal, colour, emission, reflect type); max(colour) and its
 *                         reciprocal are filled in on the host by the routine that fills them for a scene's materials.  No scene
 *                         is needed; out[i].hit = 0.
 *   PT_SCATTER_BY_ID      the closest hit of pt_ctx_intersect's kernel function, then the surface by hit id (what k_shade, k_pass and
 *                         k_mega do).  `surfaces` is not read.
 *   PT_SCATTER_BY_RANK    the same hit mapped to its visiting rank, then the surface from the rank's record (what k_pass_cand and
 *                         k_mega_cand do).  A workgroup stages the leading ranks of the table in LDS exactly when k_pass_cand
 *                         would for this scene (the whole table does not fit beside the walk queues), so ranks below that head
 *                         come from LDS and the others from global memory.  Refused for a scene without candidate tables.
 *   | PT_SCATTER_DEFER_REFRACT   kShadeDeferRefract: a Refract surface comes back `deferred` with no rays and nothing else
 *                         defined; every other surface as without the flag.
 *   | PT_SCATTER_REFRACT_ONLY    kShadeRefractOnly.  The frame kernels only hand it Refract surfaces: with PT_SCATTER_GIVEN an item
 *                         whose surface is not Refract is refused; with the other two sources such an item comes back with hit
 *                         = PT_SCATTER_NOT_SHADED and nothing else defined.
 * out[i]: hit = -1 for a miss (nothing else defined), else the hit id (object index of a sphere, n_objs + flattened triangle
 * index); x; contrib = thr * emission and emits (some channel of the emission != 0); n_rays (0: the roulette or MAX_DEPTH ended the
 * path) continuation rays from x with directions d0, d1 and throughputs thr0, thr1 (d1, thr1: the transmitted ray of a split;
 * with fewer rays the unused ones hold what ShadeOut holds) and the depth and branch of each child.  Throughput goes DOWN
 * the path: thr0 = fl(fl(thr * colour') * factor) per channel, colour' the colour after the roulette's rescale.
 * This proves the functions, not each kernel's use of them: that stays with the bounce counts and the frame tests.
 * tests/kats_scatter.py is the independent restatement; the oracle's pto_dump_paths gives its paths with their keys.
 * Bit-for-bit agreement with it holds for directions and (PT_SCATTER_GIVEN) normals of unit length to within rounding, which
 * is all the frame kernels ever hand the step: its square roots of the diffuse basis, the diffuse direction and tdir skip the
 * range test of the general routine on the strength of that (csrc/pt_device.h states each bound).
 * PT_ERR_INVALID, all refused before any device is touched, checked in this order: NULL items or out; n == 0; unknown form
 * bits (or both mode flags, or source 3); PT_SCATTER_GIVEN without surfaces; an item with sample >= 2^24, depth > 11 or
 * branch outside 1..7; PT_SCATTER_GIVEN: a reflect type above 2, or PT_SCATTER_REFRACT_ONLY with a surface that is not Refract;
 * NULL ctx.  Then PT_ERR_NO_DEVICE without a device; then PT_ERR_INVALID for the other two sources without a scene, or
 * PT_SCATTER_BY_RANK on a scene without candidate tables.  Host arrays of n. */
#define PT_SCATTER_GIVEN 0u
#define PT_SCATTER_BY_ID 1u
#define PT_SCATTER_BY_RANK 2u
#define PT_SCATTER_DEFER_REFRACT 0x10u
#define PT_SCATTER_REFRACT_ONLY 0x20u
#define PT_SCATTER_NOT_SHADED (-2)
typedef struct pt_scatter_item {
    float o[3], d[3];   /* the ray of this radiance() call */
    float thr[3];       /* product of the weights above it ((1, 1, 1) for a primary ray) */
    uint32_t pixel;     /* framebuffer index: the RNG counter's first word */
    uint32_t sample;    /* < 2^24 */
    uint32_t depth;     /* the `depth` argument: 0..11 */
    uint32_t branch;    /* 1..7 (1: no split above) */
} pt_scatter_item;
typedef struct pt_scatter_surface {
    float x[3], n[3];   /* hit.intersection, hit.normal */
    float color[3], emission[3];
    uint32_t reflect;   /* PT_DIFFUSE / PT_SPECULAR / PT_REFRACT */
} pt_scatter_surface;
typedef struct pt_scatter_out {
    int32_t hit;
    uint32_t n_rays, emits, deferred;
    float x[3], contrib[3];
    float d0[3], thr0[3], d1[3], thr1[3];
    uint32_t depth0, branch0, depth1, branch1;
} pt_scatter_out;
int pt_ctx_scatter(pt_ctx *ctx, uint64_t seed, uint32_t form, const pt_scatter_item *items,
                   const pt_scatter_surface *surfaces /* PT_SCATTER_GIVEN only */, uint32_t n, pt_scatter_out *out);

/* The host instantiation of the shared numerics header's sincos (the same source the kernels compile). */
void pt_host_sincos(float y, float *s, float *c);

/* The drop-in for mod.rs:1017-1024: host buffers in, host framebuffer out (whole W*H*3 floats,
 * only the band is written).  Uses device 0 (or PT_DEVICE env).  Blocking.  PT_ERR_INVALID for a scene pt_ctx_set_scene
 * refuses, a negative or non-finite colour or emission component among them. */
int pt_render(const pt_config *cfg, const pt_camera *cam, const pt_object *objs, uint32_t n_objs,
              const pt_triangle *tris, uint32_t n_tris, float *out_rgb,
              const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats);

/* The same frame dealt to n_ranks ranks row by row - rank r renders image rows r, r+n_ranks, ... of the band (the
 * interleaved partition of pt_config.chunk_*: contiguous parts of a picture differ in cost) - one host thread and one
 * context per rank, rank r on device r mod pt_device_count(): single-process multi-GPU for hosts that want the image
 * in HOST memory (the CLI).  Each rank downloads its rows and copies them to their places in out_rgb, so no
 * device-to-device collective is involved; a host that keeps the framebuffer on the GPUs runs one process per GPU over
 * pt_ctx_render and gathers with pt_comm_gather_frame (RCCL) below.  The image is bit-identical for every n_ranks.
 * The progress callback comes from rank 0's worker thread. */
int pt_render_multi(const pt_config *cfg, uint32_t n_ranks, const pt_camera *cam, const pt_object *objs,
                    uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris, float *out_rgb,
                    const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats);

/* Progressive preview (RenderUpdate, mod.rs:881-885, sent every 500 ms by mod.rs:965-982): callable from the
 * progress callback of pt_ctx_render on the same thread.  Resolves what has been accumulated so far into
 * d_out_rgb (the call's layout, pt_config_pixels(cfg)*3 floats) and reports how many samples per pixel it holds.  The
 * reference's snapshot is a random subset of finished pixels; this one is every pixel at partial spp.  (A wavefront call
 * of more than 1.5 M pixels is rendered in parts of 2^20 pixels: the snapshot then shows the finished parts final, the
 * part in progress at partial spp - spp_done speaks of that part - and the parts not started black.) */
int pt_ctx_snapshot(pt_ctx *ctx, void *d_out_rgb, uint32_t *spp_done);

/* ---- progressive accumulation across calls: resume, refine, checkpoint -----------------------------------------
 * The RNG is keyed on (seed; pixel, sample, ...) and radiance is summed in u64 fixed point, whose sum does not depend on the
 * order of its terms; so a frame rendered to T samples over several calls is pt_ctx_render's frame at T, bit for bit.
 * THE SUMS.  A pixel channel is one u64 in 32.32 fixed point.  A contribution v (finite, >= 0: pt_ctx_set_scene keeps the others
 * out) adds c = min(v, 4294967040) as trunc(c) * 2^32 + trunc((c - trunc(c)) * 2^32), every step in binary32 and exact but the
 * truncations: one contribution SATURATES at 4294967040 = 2^32 - 256, the largest binary32 below 2^32.  The sum over all the
 * samples a pixel holds WRAPS at 2^32 radiance units and nothing detects it: mean x samples must stay below 4.29e9 - an emission
 * of 256 seen directly at 2^24 samples per pixel is the first frame that does not fit.  A frame is the sums resolved:
 * (float)((double)sum * 2^-32) / (float)samples, clamped to [0, 1] (pt_ctx_radiance: not clamped).
 *
 * pt_ctx_accumulate renders this frame up to cfg->spp samples per pixel IN TOTAL.  The samples come from an accumulator the
 * context keeps between calls, so only the samples it does not hold yet are traced.
 * - Frame key.  The held accumulator belongs to one frame: width, height, the band [idx_begin, idx_end), chunk_pixels /
 *   chunk_first / chunk_step (as pt_config reads them: all ignored when chunk_step <= 1), seed, and the scene as uploaded.
 *   backend, flags, rays_per_pass and progress_ms are NOT part of it - they give the same image - so a frame may switch
 *   backend, scan form (PT_FLAG_NO_BVH, PT_FLAG_SEPARATE_KERNELS) or pass size from one call to the next.
 * - A call whose key differs from the held one drops the held accumulator and starts from zero; pt_ctx_set_scene drops it too.
 *   pt_ctx_render neither reads nor disturbs it (the held sums live in a buffer of their own).
 * - Counts are kept per part, cut as pt_ctx_render cuts a call: one part up to 1.5 Mi pixels, otherwise parts of 2^20 pixels.
 *   A part whose count is c traces samples [c, cfg->spp) and nothing else; without a cancel every part ends at cfg->spp.  The
 *   megakernel renders the whole call at once when all counts are equal, otherwise part by part.
 * - d_out_rgb is laid out as for pt_ctx_render; each pixel is resolved over its own part's count, a pixel with count 0 is black.
 * - A cancelled call keeps every pass that finished and returns PT_CANCELLED; a later call with the same key continues from there.
 * - pt_ctx_snapshot from the progress callback shows every pixel at its own count (the parts this call has not reached at
 *   their earlier samples, not black); its spp_done describes the part in progress.
 * - PT_ERR_INVALID: cfg->spp below what is held (samples cannot be removed; pt_ctx_accum_reset starts over), PT_FLAG_PIPELINES
 *   (its accumulators live in child contexts), and whatever pt_ctx_render refuses (cfg->spp > 2^24 among them).
 * - stats counts only the work this call did; a call with nothing left to trace only resolves and reports zero rays.
 * - Memory: the held sums take 24 B per pixel of the call (403 MB at 4096^2), on top of and outside the ray-queue budget of
 *   pt_ctx_set_memory_budget; pt_ctx_accum_reset gives them back. */
int pt_ctx_accumulate(pt_ctx *ctx, const pt_config *cfg, void *d_out_rgb, void *hip_stream,
                      const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats);
/* Samples per pixel held for cfg's frame (min / max over its parts); 0, 0 if the held accumulator is of another frame or
 * there is none.  Host only. */
int pt_ctx_accum_info(const pt_ctx *ctx, const pt_config *cfg, uint32_t *spp_min, uint32_t *spp_max);
/* Drops the held accumulator and frees its memory. */
int pt_ctx_accum_reset(pt_ctx *ctx);
/* Checkpoint of the held accumulator (PT_ERR_INVALID if there is none), written to path + ".tmp" and renamed over `path`.
 * Little-endian: magic "PTACCUM1"; u32 format version 1; the frame key - u32 width, height, idx_begin, idx_end, chunk_pixels,
 * chunk_first, chunk_step, u64 seed; u64 scene fingerprint (pt_siphash(1, 3, 0, 0, ...) over u32 n_objs, u32 n_tris, then the
 * camera, objects and triangles as pt_ctx_set_scene got them); u32 call pixels, u32 part pixels, u32 number of parts; the
 * per-part counts (u32 each); the sums, 3 planes x call pixels of u64 (32.32 fixed point, pixel order); a trailing u64
 * pt_siphash(1, 3, 0, 0, ...) of everything before it. */
int pt_ctx_accum_save(pt_ctx *ctx, const char *path);
/* Replaces the held accumulator with a checkpoint's; the next pt_ctx_accumulate with its key continues from it.  Needs the
 * same scene set on ctx.  PT_ERR_IO: missing file or read error; PT_ERR_PARSE: wrong magic or version, bad trailing hash,
 * truncated file, sizes that do not fit each other; PT_ERR_INVALID: the scene fingerprint is not the context's scene.  On
 * each of these the held accumulator is left as it was.  No input crashes the loader. */
int pt_ctx_accum_load(pt_ctx *ctx, const char *path);

/* ---- how noisy is the held frame: half buffers, a per-pixel estimate, rendering to a target -------------------------
 * The dual-buffer estimate of Dammertz, Hanika, Keller and Lensch, "A Hierarchical Automatic Stopping Condition for Monte Carlo
 * Global Illumination" (2010): the samples of every pixel are dealt to two halves A and B, and the difference of the two
 * half images estimates the error of the whole.  Sums are u64 32.32 fixed point, so sums of disjoint sample sets add and
 * subtract exactly: the context keeps the sums of A beside the held sums (same layout, 24 B per pixel more), and B is
 * held - A, never stored.
 *
 * pt_ctx_accum_track_noise switches tracking on or off for the frames this context starts AFTER the call (off by default).
 * PT_ERR_INVALID for a NULL ctx and while an accumulator is held (call pt_ctx_accum_reset first).  With tracking off nothing
 * changes anywhere.  With tracking on, pt_ctx_accumulate's frame is still pt_ctx_render's frame at cfg->spp, bit for bit -
 * only the batching of the samples changes - and pt_stats counts the same samples and bounces; `passes` may be larger.
 * - A part (see pt_ctx_accumulate) holds c samples, nA of them in A, nB = c - nA in B.
 * - A call that brings the part from c to T traces [c, m) and then [m, T), m = min(T, c + 4 * ceil((T - c) / 8)): the first
 *   run is rounded up to whole groups of the four sub-pixels (s%2, (s/2)%2).  An empty second run is dropped.
 * - After a run, the samples it traced (fewer after a cancel) go to the half that holds fewer samples of that part; a tie
 *   goes to A.  So from zero: 0 -> 4 (A) -> 8 (B); then to 24: 8 -> 16 (A) -> 24 (B).
 * - The megakernel renders the whole call at once only when c AND nA are equal over all parts.
 * - WHICH samples A holds depends on the history of calls (and of cancels), not only on T: two hosts that reach T by
 *   different steps hold different halves, and so slightly different estimates.  What does not depend on history: the held
 *   sums, the output image, pt_ctx_accum_info.
 * - pt_ctx_accum_reset, pt_ctx_set_scene and a call with another frame key drop A with the held sums; pt_ctx_render touches
 *   neither; pt_ctx_snapshot is unchanged.
 * - Checkpoints.  pt_ctx_accum_save of a tracked frame keeps the magic "PTACCUM1" and writes format version 2: version 1 with
 *   the per-part nA (u32 each) after the counts and the planes of A (3 x call pixels of u64) after the sums; the trailing hash
 *   covers everything.  An untracked frame is written as version 1, byte for byte as before.  pt_ctx_accum_load reads both:
 *   a version-2 file gives a tracked frame whatever the context's switch says; a version-1 file loaded into a context with
 *   tracking on gives a tracked frame with nA = 0 and A = 0 - everything so far counts as B, the estimate starts with the next
 *   samples, and the weight w below handles unequal halves.  PT_ERR_PARSE also for a version-2 file with some nA > c. */
int pt_ctx_accum_track_noise(pt_ctx *ctx, int enabled);

/* THE NOISE ESTIMATE.  Every operation is IEEE binary32 + - * / and sqrt, correctly rounded, never contracted, in the order
 * the parentheses give, except the conversion of a sum, which is pt_ctx_render's: mean(S, n) = clamp((float)((double)S * 2^-32)
 * / (float)n) - the u64 to binary64, times 2^-32 (exact), rounded to binary32, divided in binary32 - with clamp(v) = v < 0 ? 0 :
 * (v > 1 ? 1 : v).  |v| is v with its sign bit cleared.  For pixel p of a part with nA > 0 and nB > 0, H_c / A_c its held / half-A
 * sums of channel c = r, g, b:
 *   a_c = mean(A_c, nA),  b_c = mean(H_c - A_c, nB),  m_c = mean(H_c, nA + nB)   (m: the value pt_ctx_accumulate writes)
 *   e(p) = (((|a_r - b_r| + |a_g - b_g|) + |a_b - b_b|) * w) / sqrt(2^-6 + ((m_r + m_g) + m_b))
 *   w = sqrt((float)nA * (float)nB) / ((float)nA + (float)nB), computed on the host in binary32 per part: 1/2 for equal halves;
 *       it makes |a - b| * w an estimate of the deviation of the whole pixel's mean for any split.
 * So 0 <= e(p) <= 3 * (1/2) / sqrt(2^-6) = 12.
 * Frame statistics, over the pixels with an estimate, in the same launch:
 * - sum = the sum of floor(e(p) * 2^28) as unsigned integers (36.28 fixed point in a u64, integer atomics: the order does not
 *   matter).  A term is below 2^32, pt_ctx_denoise's largest frame has 2^28 pixels and pt_ctx_accumulate's 2^31: the sum stays
 *   below 2^63.  mean_error = (double)sum * 2^-28 / (double)pixels.
 * - histogram: k = (the bits of e(p) as a u32) >> 21 - exponent and the top two mantissa bits, four bins per octave from 2^-12 -
 *   bin = k <= 460 ? 0 : (k >= 523 ? 63 : k - 460).  Bin b holds lo(b) <= e < hi(b), hi(b) = the float with bits (461 + b) << 21
 *   (hi(0) = 1.25 * 2^-12, hi(62) = 14), lo(b) = hi(b - 1); bin 0 also takes everything below, bin 63 everything from 14 on
 *   (its upper edge is +inf; it stays empty).  A host reads quantiles from it. */
typedef struct pt_noise_stats {
    uint32_t spp_min, spp_max;     /* as pt_ctx_accum_info */
    uint32_t spp_a_min, spp_b_min; /* smallest nA / nB over the parts */
    uint64_t pixels;               /* pixels with an estimate (parts with nA > 0 and nB > 0) */
    double mean_error;             /* mean of e(p) over those pixels */
    uint32_t histogram[64];        /* e(p) in the fixed bins above */
} pt_noise_stats;
/* The estimate of the held frame.  cfg names the frame as for pt_ctx_accum_info (its spp only has to be valid).  d_error: NULL,
 * or a device pointer of pt_config_pixels(cfg) floats that receives e(p) in the call's pixel order; a pixel of a part without
 * an estimate gets +inf.  `hip_stream` as for pt_ctx_render; blocking.  PT_ERR_INVALID: a NULL ctx, cfg or out; cfg is not the
 * held frame; the frame is not tracked; no part has nA > 0 and nB > 0.  Reads 48 B and writes 4 B per pixel; changes no state of
 * the context. */
int pt_ctx_accum_noise(pt_ctx *ctx, const pt_config *cfg, float *d_error, pt_noise_stats *out, void *hip_stream);

typedef struct pt_noise_target {
    float mean_error;     /* stop when stats.mean_error <= this; 0 = not used */
    float quantile;       /* in (0,1); 0 = not used */
    float quantile_error; /* stop when the upper edge of the histogram's quantile bin <= this */
    uint32_t min_spp;     /* 0 = 16 */
} pt_noise_target;
/* Renders cfg's frame until it is as clean as `tgt` asks, cfg->spp samples per pixel at most (the cap): a host loop over
 * pt_ctx_accumulate and pt_ctx_accum_noise.  It accumulates to max(samples held, min_spp), then to twice as many each step,
 * never beyond the cap; after each step it evaluates the noise, and stops at the first step where every criterion in use holds
 * (PT_OK), at the cap (PT_OK too: *noise tells which - noise->spp_max, noise->mean_error) or on a cancel (PT_CANCELLED; a later
 * call continues).  The quantile bin is the first bin at which the cumulative count reaches ceil(quantile * pixels).  A step
 * after which no part has both halves (a cap below 5) meets no criterion; *noise then has pixels 0 and mean_error +inf.
 * d_out_rgb holds pt_ctx_render's frame at the sample count reached, bit for bit.  stats (may be NULL) sums the steps.
 * Progress is the fraction of the cap's samples traced, and 1 at the end.
 * PT_ERR_INVALID, refused before any device is touched and checked in this order: NULL cfg, tgt, d_out_rgb or noise; a
 * mean_error, quantile or quantile_error that is negative or not finite; neither criterion in use; a quantile of 1 or more; NULL
 * ctx; the context is not tracking (or the held frame of cfg is not tracked); cfg->spp below what is held. */
int pt_ctx_accumulate_until(pt_ctx *ctx, const pt_config *cfg, const pt_noise_target *tgt, void *d_out_rgb, void *hip_stream,
                            const volatile uint8_t *cancel, pt_progress_fn cb, void *user, pt_stats *stats, pt_noise_stats *noise);

/* ---- adaptive sampling: every tile rendered to its own noise target -------------------------------------------------
 * pt_ctx_accumulate_until doubles the samples of the whole frame until the frame is clean; pt_ctx_render_adaptive does it tile by
 * tile (the step the paper above is about): a tile whose mean estimate meets the target takes no more samples, the others go on.
 * Because the RNG is keyed on (seed; pixel, sample) and radiance is summed in u64 fixed point, a pixel that ends with n samples is
 * pt_ctx_render's pixel at spp = n, bit for bit, whatever its neighbours hold.
 * - Frame.  cfg as for pt_ctx_render; cfg->spp is the CAP.  The band consists of whole image rows: idx_begin and idx_end are
 *   multiples of width (0, 0 = the whole frame).  A tile covers `tile` columns by `tile` rows of the band, counted from the band's
 *   first row and column 0: the pixel with call index k lies in tile row (k / width) / tile and tile column (k % width) / tile.
 *   Tiles at the right and bottom edges are partial.
 * - Levels.  n_0 = min_spp rounded up to a multiple of 8, n_(j+1) = min(2 * n_j, cap); a cap below n_0 is the only level.  Every
 *   open tile holds the same count.  The level that takes the open tiles from c to T traces [c, m) into half A and [m, T) into half
 *   B, m = min(T, c + 4 * ceil((T - c) / 8)): the rule of a tracked pt_ctx_accumulate call, so an open tile's halves after level j
 *   are those a tracked frame holds after pt_ctx_accumulate calls at n_0, ..., n_j (nA = the sum of the m - c, nB = T - nA).
 * - Decision.  After a level every pixel p of an open tile gets e(p) exactly as THE NOISE ESTIMATE defines it (the tiles' nA, nB,
 *   w on the host).  E = the sum over the tile's pixels of floor(e(p) * 2^28) as unsigned integers in a u64; the tile CLOSES iff
 *   E <= q * (pixels of the tile inside the frame), q = (uint64) floor((double) tile_error * 2^28) computed on the host.  A
 *   closed tile is never reopened.  The call ends when no tile is open or the cap is reached.  A level at which nB is 0 (a cap
 *   below 5) closes nothing and evaluates nothing.
 * - d_out_rgb (pt_config_pixels(cfg) * 3 floats, device): every pixel resolved over its own tile's count - pt_ctx_render's
 *   pixel at that count, bit for bit; a count of 0 (a cancel before the first level ended) gives black.
 * - d_spp (may be NULL; pt_config_pixels(cfg) u32, device): the count of every pixel, in the call's pixel order.
 * - d_error (may be NULL; pt_config_pixels(cfg) floats, device): e(p) of the tile's last evaluation, +inf where none was made.
 * - Cancel.  *cancel is read between levels (and after the progress callback made there); inside a level the tile pass runs in
 *   the time-sized rounds of the megakernel (pt_ctx_render), one level being the unit that is kept: PT_CANCELLED leaves every
 *   tile at the last count it completed, and the outputs are filled accordingly.
 * - Progress: the samples traced so far (partial tiles counted whole) over pixels * cap, between levels; 1.0 at the end.
 * - stats (may be NULL): samples = the sum of the counts = astats->samples; ray_bounces exact; passes = the tile pass's launches.
 * - astats.  level_spp[j] = n_j and tiles_closed[j] for the `levels` levels run; tiles_open = tiles still open at the end (at the
 *   cap, or at the cancel); mean_error = (double)(the sum of the tiles' last E) * 2^-28 / (double)pixels, +inf unless every tile
 *   has been evaluated.
 * - State.  The call is pt_ctx_adaptive_reset followed by pt_ctx_accumulate_adaptive (below): it starts from zero, replaces a
 *   held adaptive frame, and its own frame is held afterwards - pt_ctx_accumulate_adaptive continues it.  The held sums and half
 *   A's (48 B per pixel of the call), a count, nA and an E per tile, the open-tile list and the compact accumulator of a step's
 *   tiles (24 B per pixel of an open tile) live in the context, grow on demand and are reused between calls.  It changes no other
 *   state of the context: not pt_ctx_accumulate's held frame or counts, not the measured pass rates pt_ctx_render uses (its
 *   rounds keep a rate of their own).
 * - PT_ERR_INVALID, refused before any device is touched, checked in this order: NULL cfg, params, d_out_rgb or astats; a
 *   tile_error that is negative or not finite; a tile other than 0, 4, 8, 16, 32; NULL ctx; no scene; a band that is not whole
 *   rows; chunk_step > 1 or PT_FLAG_PIPELINES; whatever pt_ctx_render refuses; tiles that hold 2^32 pixels or more.
 * - backend is ignored: the call has one pass kernel, the megakernel's source compiled for the open-tile list (an item is a
 *   slot of the list, a pixel of the tile, a part of the level's samples).  PT_FLAG_NO_BVH selects the linear scan. */
typedef struct pt_adaptive_params {
    float tile_error;   /* a tile is finished when the mean of e(p) over its pixels <= this; finite, >= 0 */
    uint32_t tile;      /* tile edge in pixels: 4, 8, 16 or 32; 0 = 8 */
    uint32_t min_spp;   /* first level; 0 = 16; rounded up to a multiple of 8 */
} pt_adaptive_params;
typedef struct pt_adaptive_stats {
    uint32_t tiles, tiles_open;   /* tiles of the call; tiles that reached the cap (or the cancel) unfinished */
    uint32_t levels;              /* levels run */
    uint32_t level_spp[32];       /* samples per pixel a tile holds after level j */
    uint32_t tiles_closed[32];    /* tiles that finished at level j */
    uint64_t samples;             /* primary samples traced = sum over pixels of their count */
    double mean_error;            /* mean of e(p) over all pixels, each at its tile's last evaluation */
} pt_adaptive_stats;
int pt_ctx_render_adaptive(pt_ctx *ctx, const pt_config *cfg, const pt_adaptive_params *params,
                           void *d_out_rgb, uint32_t *d_spp, float *d_error, void *hip_stream,
                           const volatile uint8_t *cancel, pt_progress_fn cb, void *user,
                           pt_stats *stats, pt_adaptive_stats *astats);

/* ---- the adaptive frame held across calls: continue, refine, checkpoint -------------------------------------------
 * pt_ctx_accumulate_adaptive is pt_ctx_render_adaptive on a frame the context KEEPS: a cancelled frame is continued, a smaller
 * tile_error refines it, a higher cap extends it, and only the samples that are not held yet are traced.  Arguments, outputs
 * and refusals (in that order) are pt_ctx_render_adaptive's.
 * - Held adaptive frame and its key.  The context keeps one adaptive frame between calls.  Its key is pt_ctx_accumulate's frame
 *   key - width, height, the band, seed, and the scene as uploaded - plus the tile edge and n_0 = min_spp (0 = 16) rounded up to a
 *   multiple of 8, before any cap.  tile_error, the cap (cfg->spp), backend, flags, rays_per_pass and progress_ms are NOT part of
 *   it.  A call with another key, pt_ctx_set_scene and pt_ctx_adaptive_reset drop the frame; pt_ctx_render_adaptive replaces it.
 *   It is independent of pt_ctx_accumulate's held frame, in both directions.
 * - Per-tile state.  A tile holds a count c, nA of its samples in half A (nB = c - nA), and its last E or none.  The ladder is
 *   n_0, 2 n_0, 4 n_0, ...; a tile's next count after c is T = min(cap, the smallest ladder value > c) - min(cap, n_0) for c = 0.
 * - A call, 1: re-decide.  Every tile that has an E is closed iff E <= q * (its pixels inside the frame), q from THIS call's
 *   tile_error; a tile without an E is open.  So a smaller tile_error reopens tiles, and a larger one closes tiles without
 *   tracing anything.  A tile with c >= cap takes no samples; if it is not closed it counts in tiles_open (and in
 *   pt_adaptive_info.tiles_at_cap).  A cap below a tile's count is no error: samples are never removed.
 * - A call, 2: steps.  While some open tile has c < cap: the open tiles with the smallest c, among those the ones with the
 *   smallest nA, are a CLASS.  Every tile of the class is traced from c to T in two runs, [c, m) and [m, T), m = min(T, c + 4 *
 *   ceil((T - c) / 8)); an empty second run is dropped.  After each run its samples go to the half that holds fewer samples of
 *   the tile, a tie to A (pt_ctx_accumulate's rule for tracked frames).  After the last run every tile of the class is evaluated
 *   exactly as pt_ctx_render_adaptive evaluates a level - e(p), E, the decision; with nB = 0 nothing is evaluated.  From zero
 *   this is pt_ctx_render_adaptive's level sequence, halves and decisions; the two only differ after a cap that was not on the
 *   ladder.
 * - Cancel and progress.  *cancel is read between steps (and after the progress callback made there).  A step is kept whole or
 *   not at all: PT_CANCELLED leaves the frame held at the steps that completed, and the same call made again continues it.
 *   Progress: the samples held (the steps' partial tiles counted whole) over pixels * cap, between steps; 1.0 at the end.
 * - Outputs, over the held state: every pixel resolved over its tile's count (pt_ctx_render's pixel at that count, bit for
 *   bit), d_spp the counts, d_error e(p) of the tile's last evaluation - recomputed from the held sums, half A's, the count and
 *   nA, which are those of that evaluation - and +inf where the tile has no E.
 * - stats counts only this call's work: samples = the samples it added, ray_bounces and passes its own; a call with nothing to
 *   trace reports zero rays and still fills the outputs.  astats: level_spp[j] = the T of this call's step j and tiles_closed[j]
 *   the tiles its evaluation closed (steps beyond 32 run but are not recorded; `levels` saturates at 32); tiles, tiles_open,
 *   samples and mean_error describe the held frame after the call.
 * - Equality with a from-scratch render.  If tile_error never increased from call to call, and every earlier cap is a ladder
 *   value or equals the last call's cap, the held frame after the last call is the frame pt_ctx_render_adaptive gives from
 *   scratch with the last call's tile_error and cap: d_out_rgb, d_spp, d_error, samples and mean_error, bit for bit.  Otherwise
 *   every pixel is still pt_ctx_render's pixel at its own count; only which tiles hold which count may differ.
 * - Memory: 48 B per pixel of the call and 16 B per tile, outside the ray-queue budget; pt_ctx_adaptive_reset gives them back. */
int pt_ctx_accumulate_adaptive(pt_ctx *ctx, const pt_config *cfg, const pt_adaptive_params *params,
                               void *d_out_rgb, uint32_t *d_spp, float *d_error, void *hip_stream,
                               const volatile uint8_t *cancel, pt_progress_fn cb, void *user,
                               pt_stats *stats, pt_adaptive_stats *astats);
typedef struct pt_adaptive_info {
    uint32_t tiles, tiles_open, tiles_at_cap; /* tiles held; not closed under params->tile_error; of those, at cfg->spp or beyond */
    uint32_t spp_min, spp_max;                /* smallest / largest count over the tiles */
    uint64_t samples;                         /* sum over pixels of their count */
    double mean_error;                        /* as pt_adaptive_stats.mean_error */
} pt_adaptive_info;
/* The held adaptive frame of cfg / params, re-decided under params->tile_error and cfg->spp, without changing it.  All zeros
 * (PT_OK) if the key is not the held one.  Refusals as pt_ctx_render_adaptive's about cfg, params and ctx; blocking. */
int pt_ctx_adaptive_info(pt_ctx *ctx, const pt_config *cfg, const pt_adaptive_params *params, pt_adaptive_info *out);
/* Writes the three outputs (d_spp, d_error: may be NULL) from the held adaptive frame, as pt_ctx_accumulate_adaptive does at
 * its end.  Allowed from the progress callback of pt_ctx_accumulate_adaptive, in stream order after the steps issued: the
 * preview between steps (pt_ctx_snapshot does not know adaptive frames).  PT_ERR_INVALID if cfg's frame (width, height, band,
 * seed) is not the held one.  Blocking. */
int pt_ctx_adaptive_resolve(pt_ctx *ctx, const pt_config *cfg, void *d_out_rgb, uint32_t *d_spp, float *d_error, void *hip_stream);
/* Drops the held adaptive frame and frees its memory. */
int pt_ctx_adaptive_reset(pt_ctx *ctx);
/* Checkpoint of the held adaptive frame (PT_ERR_INVALID if there is none), written to path + ".tmp" and renamed over `path`.
 * Little-endian: magic "PTADAPT1"; u32 format version 1; the frame key as PTACCUM1 writes it (chunk fields 0), then u32 tile
 * edge and u32 n_0; the u64 scene fingerprint; u32 call pixels; u32 tiles; per tile u32 count, u32 nA, u64 E (all ones = none);
 * the held sums, then half A's, 3 planes x call pixels of u64 each; a trailing u64 pt_siphash(1, 3, 0, 0, ...) of everything
 * before it. */
int pt_ctx_adaptive_save(pt_ctx *ctx, const char *path);
/* Replaces the held adaptive frame with a checkpoint's; the next pt_ctx_accumulate_adaptive with its key continues from it.
 * Error codes as pt_ctx_accum_load's; PT_ERR_PARSE also for nA > count, a count above 2^24, an E of a tile one of whose halves
 * is empty, and sizes that do not fit the tile geometry.  On each of these the held frame is left as it was.  No input crashes
 * the loader. */
int pt_ctx_adaptive_load(pt_ctx *ctx, const char *path);

/* ---- first-hit AOVs: guide buffers for a denoiser, a pick map for a GUI ------------------------------------------
 * pt_ctx_render_aov covers the pixels pt_ctx_render covers with the same cfg - pt_config_pixels(cfg) of them, in the same
 * order (the band [idx_begin, idx_end) and the interleaved chunks included); pixel k of the call has framebuffer index p.
 * For each sample s in [0, cfg->spp) the ray is render_pixel's ray for (seed; p, s) (mod.rs:812-843), bit for bit what
 * pt_ctx_primary_rays returns and what the frame kernels trace - so these are the first cfg->spp samples of the frame with
 * that seed, a prefix of a frame rendered at more - and h = intersect_scene(ray) (mod.rs:631-659).  FIRST HIT only: a
 * mirror or glass surface gives its own colour and normal (pt_ctx_render_aov_ex, below, can follow the deterministic chain).
 * - albedo[3k+c] = sum over s of (colour[c] of the object hit, 0 on a miss) / spp
 * - normal[3k+c] = sum over s of (normal_towards_ray[c], 0 on a miss) / spp, not renormalised; normal_towards_ray is the hit
 *   normal flipped to face the ray, as radiance() computes it (mod.rs:669-673)
 * - depth[k] = sample 0's hit.distance, +inf on a miss
 * - object_id[k] = sample 0's object index (pt_ctx_set_scene order), -1 on a miss
 * Sums are 32.32 fixed point, as the frame accumulator's, so the result does not depend on how samples are spread over the
 * device: colours to_fixed(v), normal components sign(v) * to_fixed(|v|) summed in two's-complement int64; each mean is
 * (float)((double)sum * 2^-32) / (float)spp, not clamped.
 * Device pointers, pt_config_pixels(cfg) * 3 floats (albedo, normal) or * 1 (depth, object_id); any may be NULL and is then
 * skipped; all four NULL is PT_ERR_INVALID.  PT_FLAG_NO_BVH selects the linear scan (same results); backend, rays_per_pass,
 * progress_ms, PT_FLAG_SEPARATE_KERNELS and PT_FLAG_PIPELINES are ignored.  PT_ERR_INVALID also for a NULL ctx or cfg, no
 * scene, spp 0 or above 2^24, and whatever pt_ctx_render refuses about the band or the chunks; PT_ERR_HIP for HIP failures.
 * `hip_stream` as for pt_ctx_render (NULL = the context's own stream); blocking.  The call changes no other state of the
 * context: not the frame accumulators, not pt_ctx_accumulate's held sums or counts, not the measured pass rates. */
int pt_ctx_render_aov(pt_ctx *ctx, const pt_config *cfg, float *d_albedo, float *d_normal, float *d_depth,
                      int32_t *d_object_id, void *hip_stream);

/* ---- AOVs through mirror and glass surfaces: the guides of what a delta surface shows -----------------------------------
 * pt_ctx_render_aov_ex is pt_ctx_render_aov with parameters and a fifth output.  With params NULL or all zero it runs the
 * plain call - the same kernel, the same bits in the four buffers - and writes 0 to every word of d_chain.
 * With PT_AOV_THROUGH_DELTA a sample does not stop on a PT_SPECULAR or PT_REFRACT object: it follows the deterministic chain
 * to the first surface that is neither, and the guides describe THAT surface - the reflected wall, the refracted floor.  The
 * chain draws no random number, so it is stated bit for bit.  For sample s of pixel p (framebuffer index, as above) the first
 * ray is render_pixel's ray for (seed; p, s); thr = (1, 1, 1), L = +0, j = 0; then repeat h = intersect_scene(ray):
 * - a miss, at any stage: the sample adds 0 to albedo and normal; sample 0 gives depth +inf, object_id -1, chain j.
 * - a hit: L = L + h.distance (one binary32 addition per hit, in chain order).  If the object is PT_DIFFUSE or j == max_chain
 *   the hit is TERMINAL: the sample adds thr * colour to albedo (per channel one binary32 product) and normal_towards_ray of
 *   this hit against the current ray's direction (mod.rs:669-673) to normal; sample 0 gives depth L, object_id this object's
 *   index, chain j.  Otherwise thr = thr * colour, j = j + 1, and the next ray starts at hit.intersection with direction
 *   d - n*2*dot(n,d) on PT_SPECULAR (mod.rs:722-723, not renormalised) and on PT_REFRACT that same direction when cos2t < 0
 *   and tdir of mod.rs:746-749 otherwise - the values radiance() gives its recursive calls, what pt_ctx_scatter reports as
 *   d0 (mirror, total internal reflection) and d1 (a split's transmitted ray).  No roulette, no Fresnel weight, no draw: on
 *   glass the chain follows the transmitted ray wherever one exists.
 * Sums and their means are pt_ctx_render_aov's 32.32 fixed-point rules, so a frame that sees no delta surface gets the plain
 * call's bits (thr = 1 and L = +0 change nothing: 1 * c == c, 0 + t == t).  depth is the UNFOLDED path length to the terminal
 * surface, not a distance from the lens along the primary ray; object_id is the reflected or refracted object's, so a GUI's
 * pick map should keep using the plain call.  What pt_ctx_reproject* makes of an unfolded depth under a camera move has not
 * been studied.
 * - max_chain: the most delta steps a sample takes, 1..PT_AOV_MAX_CHAIN; 0 = 8.  A sample still on a delta surface after
 *   max_chain steps ends there with that surface's colour (times thr) and normal.
 * - d_chain: pt_config_pixels(cfg) uint32, sample 0's j; may be NULL, as each of the four others.
 * PT_ERR_INVALID before any device is touched, checked in this order: flag bits other than PT_AOV_THROUGH_DELTA; max_chain
 * above PT_AOV_MAX_CHAIN; max_chain != 0 without the flag; all five outputs NULL; then whatever pt_ctx_render_aov refuses.
 * Everything else - pixels covered, ignored cfg fields, PT_FLAG_NO_BVH, the stream, blocking, no other state of the context
 * changed - as pt_ctx_render_aov.  pt_aov_defaults writes the parameters of a through-delta call with every default written
 * out, {PT_AOV_THROUGH_DELTA, 8}; PT_ERR_INVALID for a NULL out. */
#define PT_AOV_THROUGH_DELTA 1u
#define PT_AOV_MAX_CHAIN 16u
typedef struct pt_aov_params {
    uint32_t flags;     /* PT_AOV_THROUGH_DELTA or 0 */
    uint32_t max_chain; /* 0 = 8; needs the flag */
} pt_aov_params;
int pt_aov_defaults(pt_aov_params *out);
int pt_ctx_render_aov_ex(pt_ctx *ctx, const pt_config *cfg, const pt_aov_params *params, float *d_albedo, float *d_normal,
                         float *d_depth, int32_t *d_object_id, uint32_t *d_chain, void *hip_stream);

/* ---- denoising a frame on the device with the first-hit guides ------------------------------------------------
 * pt_ctx_denoise runs an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a WHOLE frame in device memory,
 * guided by albedo, normal and depth: the consumer of pt_ctx_render_aov's buffers, for previews at few samples.
 * - Buffers: device pointers, width * height pixels in framebuffer order - d_color, d_albedo, d_normal, d_out 3 floats per
 *   pixel, d_depth 1 - the layouts pt_ctx_render / pt_ctx_render_aov write for a cfg without a band and without chunks.  Pixel
 *   idx has column x = idx % width and row y = idx / width (the filter is symmetric: the framebuffer's flip does not matter).
 * - d_albedo, d_normal, d_depth may each be NULL (see the arithmetic).  d_out may be d_color (the last level is the only
 *   writer of d_out, and d_color is read before the first); d_out may not alias a guide.
 * - `hip_stream` as for pt_ctx_render (NULL = the context's own stream); blocking.  No scene is needed.
 * - Scratch (48 B per pixel: two colour planes and the packed guides) lives in the context, grows when a frame needs more, is
 *   reused between calls, and is freed by pt_ctx_destroy.  The call changes no other state of the context: not the frame
 *   accumulators, not pt_ctx_accumulate's held sums or counts, not the measured pass rates.
 * - PT_ERR_INVALID, all refused before any device is touched: params->levels > 8, a sigma that is negative or not finite,
 *   sigma_normal_pow != 0, flag bits other than PT_DENOISE_NO_DEMODULATE, width or height 0, width * height > 2^28, NULL
 *   d_color or d_out, NULL ctx (checked in this order).  PT_ERR_HIP: a HIP call failed.  (PT_ERR_NO_DEVICE comes from
 *   pt_ctx_create: without a device there is no context.)
 * - pt_denoise_defaults fills in the values a zero field (or params == NULL) stands for: levels 5, sigma_color 2,
 *   sigma_depth 2^-5 (0.03125), flags 0.  They were chosen by the CPU study recorded in profiles/denoise_cpu_study.json.
 * - PT_DN_LDS_MAXSTEP (environment, read once at pt_ctx_create): levels whose step is at most this value stage their taps in
 *   LDS, the others read them through the caches.  Same bytes either way.
 *
 * THE ARITHMETIC.  Every operation is IEEE binary32 + - * / and sqrt, correctly rounded, never contracted, in the order the
 * parentheses give.  max(a, b) stands for (a > b ? a : b), pos(v) for (v > 0 ? v : 0) - a NaN gives 0 - and |v| for v with
 * its sign bit cleared.  +inf = the binary32 infinity.
 * 1. Prepare, for every pixel p:
 *    - hit(p) = depth[p] < +inf; without d_depth every pixel is a hit.
 *    - l = sqrt((nx*nx + ny*ny) + nz*nz) of normal[p]; N(p) = (nx / l, ny / l, nz / l) if l > 0, else (0, 0, 0).
 *    - per channel c: m_c(p) = albedo[p][c] > 2^-6 ? albedo[p][c] : 1; m_c = 1 without d_albedo or with
 *      PT_DENOISE_NO_DEMODULATE.  u_0(p)[c] = color[p][c] / m_c(p).
 * 2. Level i = 0 .. levels-1 with step s = 2^i, for every pixel p = (x, y):
 *    sum = (0, 0, 0), wsum = 0.  For dy = -2..2 (outer loop), dx = -2..2 (inner loop), q = (x + dx*s, y + dy*s):
 *    - q outside the frame: the tap is skipped.
 *    - h = B[|dy|] * B[|dx|] with B = {3/8, 1/4, 1/16} (the products are exact).
 *    - dx == 0 and dy == 0: w = h.
 *    - else if hit(p) != hit(q): the tap is skipped (a miss never blends with a hit).
 *    - else w = ((h * wn) * fall(xz)) * fall(xc), where
 *        wn = 1 without d_normal or if p and q both miss; else e = pos((N(p).x*N(q).x + N(p).y*N(q).y) + N(p).z*N(q).z),
 *             squared five times: e = e*e; e = e*e; e = e*e; e = e*e; wn = e*e  (e^32);
 *        xz = 0 without d_depth or if p and q both miss; else with zp = depth[p], zq = depth[q]:
 *             xz = |zp - zq| * (1 / (sds_i * max(zp, zq))), sds_i = sigma_depth * (float)s computed on the host in binary32;
 *        xc = ((dr*dr + dg*dg) + db*db) * rc_i with (dr, dg, db) = u_i(p) - u_i(q), rc_i = 1 / (sc_i * sc_i) and
 *             sc_i = sigma_color * 2^-i (2^-i exact), both computed on the host in binary32;
 *        fall(v): t = pos(1 - v * 0.125); t = t*t; t = t*t; fall = t*t  (t^8: exp(-v)'s stand-in, zero from v = 8 on, exact
 *             operations only, so that the device and a restatement in numpy agree bit for bit).
 *    - sum[c] = sum[c] + u_i(q)[c] * w for c = 0, 1, 2; wsum = wsum + w.
 *    u_{i+1}(p)[c] = sum[c] / wsum  (wsum >= 9/64: the centre tap).
 * 3. Finish: out[p][c] = clamp(u_levels(p)[c] * m_c(p)) with clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v), as pt_ctx_render clamps. */
typedef struct pt_denoise_params {
    uint32_t levels;        /* a-trous levels, step 1, 2, 4, ...; 0 = the default; at most 8 */
    float sigma_color;      /* 0 = the default */
    float sigma_normal_pow; /* reserved: must be 0 (the exponent of the normal weight is fixed at 32) */
    float sigma_depth;      /* 0 = the default */
    uint32_t flags;         /* PT_DENOISE_NO_DEMODULATE */
} pt_denoise_params;
#define PT_DENOISE_NO_DEMODULATE 1u
int pt_denoise_defaults(pt_denoise_params *out);
int pt_ctx_denoise(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_denoise_params *params,
                   const float *d_color, const float *d_albedo, const float *d_normal, const float *d_depth,
                   float *d_out, void *hip_stream);

/* ---- denoising what the frame's own noise estimate says is noise -----------------------------------------------
 * pt_ctx_denoise_var is pt_ctx_denoise with the fixed sigma_color replaced by a per-pixel variance taken from the frame's
 * noise estimate e(p): where the two half buffers agree the filter leaves the colour alone (a converged frame comes back
 * nearly untouched, detail on one surface survives), where they differ it smooths as far as they differ.  The variance is
 * prefiltered 3x3 and carried from level to level with the squares of the weights used (as SVGF does, Schied et al. 2017).
 * - Buffers, the aliasing rule (d_out may be d_color), `hip_stream`, blocking, the scratch and its ownership (the same 48 B per
 *   pixel, shared with pt_ctx_denoise), "no scene is needed" and "changes no other state of the context" are pt_ctx_denoise's.
 * - d_error: width * height floats in framebuffer order - the map pt_ctx_accum_noise writes for a cfg without a band and
 *   without chunks, or pt_ctx_render_adaptive's d_error.  +inf marks "no estimate".  It may not alias d_out.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: params->levels > 8, a sigma that is
 *   negative or not finite, flag bits other than PT_DENOISE_NO_DEMODULATE, width or height 0, width * height > 2^28, NULL
 *   d_color, NULL d_error (pt_ctx_denoise is the filter without an estimate), NULL d_out, NULL ctx.  PT_ERR_HIP: a HIP call
 *   failed.
 * - pt_denoise_var_defaults fills in the values a zero field (or params == NULL) stands for: levels 5, sigma_var 1,
 *   sigma_depth 2^-3 (0.125), flags 0.  They were chosen by the CPU study recorded in profiles/denoise_var_cpu_study.json.
 * - PT_DN_LDS_MAXSTEP selects the form of each level as for pt_ctx_denoise.  Same bytes either way.
 *
 * THE ARITHMETIC.  The rules are pt_ctx_denoise's: binary32 + - * / and sqrt, correctly rounded, never contracted, in the
 * order the parentheses give.  pos, fall, B, hit, N, m_c, wn, xz, sds_i, the order of the taps and the finish are those of
 * pt_ctx_denoise's contract above, word for word.  Only these things differ:
 * 1. Prepare, in addition, for every pixel p:
 *    - ev = error[p] < 12 ? pos(error[p]) : 12  (NaN and +inf give 12, the largest value an estimate can take).
 *    - d = ev * sqrt(2^-6 + ((color[p][0] + color[p][1]) + color[p][2])): e(p)'s normalisation undone, the weighted L1 half
 *      difference in colour units.
 *    - t_c = d / m_c(p) for c = 0, 1, 2; Vraw(p) = (t_0*t_0 + t_1*t_1) + t_2*t_2.
 * 2. Prefilter, for every pixel p = (x, y): sum = 0, gsum = 0.  For dy = -1..1 (outer loop), dx = -1..1 (inner loop),
 *    q = (x + dx, y + dy) inside the frame: g = G[|dy|] * G[|dx|] with G = {1/2, 1/4}; sum = sum + Vraw(q) * g;
 *    gsum = gsum + g.  V_0(p) = sum / gsum.  No guide weights are applied here.
 * 3. Level i = 0 .. levels-1 with step s = 2^i, for every pixel p:
 *    - r = 1 / ((kv * V_i(p)) + 2^-20), kv = sigma_var * sigma_var computed on the host in binary32.
 *    - the colour term of a tap that is not the centre is xc = ((dr*dr + dg*dg) + db*db) * r: constant over the levels, there
 *      is no 2^-i.  w is as in pt_ctx_denoise.
 *    - vs = 0 beside sum and wsum.  Every tap that is taken adds vs = vs + V_i(q) * (w * w); the centre adds
 *      V_i(p) * (h * h); a skipped tap adds nothing.
 *    - u_{i+1}(p) as in pt_ctx_denoise.  V_{i+1}(p) = vs / (wsum * wsum).
 * 4. Finish as in pt_ctx_denoise.
 * 5. Range: for colours in [0, 1] everything stays finite: Vraw <= 3 * (12 * sqrt(3 + 2^-6) * 64)^2.  For colours that are not
 *    finite the result is unspecified.  The constant 2^-20 and the factor-free Vraw (no 1/3, no 1/n) are deliberate:
 *    sigma_var absorbs the scale. */
typedef struct pt_denoise_var_params {
    uint32_t levels;     /* a-trous levels, step 1, 2, 4, ...; 0 = the default; at most 8 */
    float sigma_var;     /* 0 = the default; finite, >= 0 */
    float sigma_depth;   /* 0 = the default; finite, >= 0 */
    uint32_t flags;      /* PT_DENOISE_NO_DEMODULATE */
} pt_denoise_var_params;
int pt_denoise_var_defaults(pt_denoise_var_params *out);
int pt_ctx_denoise_var(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_denoise_var_params *params,
                       const float *d_color, const float *d_error, const float *d_albedo, const float *d_normal,
                       const float *d_depth, float *d_out, void *hip_stream);

/* ---- presenting a frame: fit to a window, gamma, 8 bits ----------------------------------------------------------
 * pt_ctx_present turns a linear float frame in device memory into what a window or an image file holds: gamma-corrected 8-bit
 * pixels at the size asked for, in display order.  The host downloads 4 B per window pixel instead of 12 B per frame pixel and
 * never calls powf.
 * - Buffers: device pointers.  d_rgb is width * height * 3 floats in framebuffer order - what pt_ctx_render,
 *   pt_ctx_accumulate*, pt_ctx_snapshot, pt_ctx_adaptive_resolve and the denoisers write for a whole frame (a cfg without a band
 *   and without chunks).  d_out is out_width * out_height * 4 (PT_PRESENT_RGBA8: r, g, b, 255) or * 3 (PT_PRESENT_RGB8) bytes,
 *   row-major from the top-left display pixel; for RGBA8 it is 4-byte aligned, as every device allocation is.  d_out may not
 *   alias d_rgb.
 * - `hip_stream` as for pt_ctx_render (NULL = the context's own stream); blocking.  No scene is needed.
 * - The call may be made from a progress callback, in stream order after pt_ctx_snapshot or pt_ctx_adaptive_resolve on the same
 *   stream.  It changes no other state of the context: not the frame accumulators, not the held frames, not the denoisers'
 *   scratch, not the measured pass rates.
 * - Scratch lives in the context, grows on demand, is reused between calls and is freed by pt_ctx_destroy; it is outside the
 *   ray-queue budget (pt_ctx_set_memory_budget): the 1 KB table, uploaded by the first call, and - only when the size changes -
 *   an intermediate of width * out_height * 24 B (the source rows an output row covers, summed per column and channel).  It
 *   shares nothing with the denoisers.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: an exposure that is negative, not finite
 *   or NaN; an unknown format; flag bits other than PT_PRESENT_FRAMEBUFFER_ORDER; width or height 0; exactly one of out_width,
 *   out_height 0; width * height or out_width * out_height above 2^28; NULL d_rgb; NULL d_out; NULL ctx.  PT_ERR_HIP: a HIP
 *   call failed (an intermediate that does not fit the device among them).
 *
 * THE ARITHMETIC.  All operations are IEEE binary32, correctly rounded, never contracted, except where integers or binary64
 * are named.  W, H = width, height; OW, OH = the output size (out_width, out_height, or W, H when both are 0).
 * 1. Display image.  Without PT_PRESENT_FRAMEBUFFER_ORDER D(x, y) = frame[W*H-1-(y*W+x)]: the order pt_write_ppm lists and the
 *    reference's canvas draws.  With the flag D(x, y) = frame[y*W+x].
 * 2. Per source value v: v' = v * exposure (one multiply; exposure 0 stands for 1); c(v') = v' > 0 ? (v' > 1 ? 1 : v') : 0.
 *    NaN and -0 give +0, +inf gives 1.
 * 3. Same size (OW == W and OH == H): m = c(v').  No fixed point: this path reproduces pt_write_ppm's numbers exactly.
 * 4. Otherwise, the area average in integers.  q = (uint64) floor(c(v') * 2^32) (the product is exact; q <= 2^32).  Output cell
 *    X covers [X*W, (X+1)*W) on an axis where source pixel x covers [x*OW, (x+1)*OW); wx(X, x) is the integer length of their
 *    overlap, wy(Y, y) likewise with H and OH, so sum_x wx = W and sum_y wy = H.  S = sum_y sum_x wy * wx * q in u64: below 2^60
 *    (at most W * H * 2^32), independent of the order of summation.  m = (float)((double)S / ((double)(W*H) * 4294967296.0)):
 *    the u64 -> binary64 conversion rounds to nearest even, the divisor is exact, one binary64 division, one rounding to
 *    binary32.  The same rule serves shrinking, enlarging and an axis whose size does not change.
 * 5. Eight bits: a table, not powf, is the contract on the device.  T[k], k = 1..255, is the bit pattern of the smallest
 *    binary32 x in [0, 1] with pt_to_int_with_gamma_correction(x) >= k, found on the host by bisection over bit patterns
 *    (non-negative floats order as their bits) with the host's own powf, once per process (thread-safe); T[0] = 0.  byte(m) =
 *    the number of k in 1..255 with bits(m) >= T[k].  It equals pt_to_int_with_gamma_correction(m) for every m iff that
 *    function does not decrease on [0, 1] - which holds for the libm this was checked against over all 1 065 353 217 bit
 *    patterns (tests/test_present_abi.py samples them).  The table's values belong to the host's libm: read them with
 *    pt_present_thresholds, never hard-code them.
 * pt_present_thresholds returns T.  pt_present_quantize_host applies steps 2 and 5 to n values on the host: the host
 * instantiation of the source the kernels compile (csrc/pt_present.h), to them what pt_host_sincos is to the device's sincos.
 * PT_ERR_INVALID for an exposure pt_ctx_present refuses and for a NULL pointer.  pt_write_ppm8 writes width * height * 3 bytes as
 * a binary PPM ("P6\n<width> <height>\n255\n" and the bytes); PT_ERR_INVALID for a NULL argument or an empty image, PT_ERR_IO
 * when the file cannot be written.  None of the three needs a device. */
#define PT_PRESENT_RGBA8 0u   /* r, g, b, 255 */
#define PT_PRESENT_RGB8  1u
#define PT_PRESENT_FRAMEBUFFER_ORDER 1u  /* flags: do not turn the frame into display order */
typedef struct pt_present_params {
    uint32_t out_width, out_height; /* 0, 0 = the frame's own size; one of them 0 alone: PT_ERR_INVALID */
    float exposure;                 /* 0 = 1; finite, > 0 otherwise */
    uint32_t format;                /* PT_PRESENT_* */
    uint32_t flags;
} pt_present_params;
int pt_ctx_present(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_present_params *params /* NULL = all zero */,
                   const float *d_rgb, uint8_t *d_out, void *hip_stream);
/* host only, no device needed */
int pt_present_thresholds(uint32_t out[256]);
int pt_present_quantize_host(const float *in, size_t n, float exposure, uint8_t *out);
int pt_write_ppm8(const char *path, const uint8_t *rgb8, uint32_t width, uint32_t height); /* binary P6, maxval 255 */

/* ---- reprojecting a preview frame's history across a camera move ---------------------------------------------------
 * pt_ctx_reproject carries last frame's colour into this frame's pixels through the depth and object-id guides and blends it
 * with this frame's colour by the history length: the temporal half of SVGF (Schied et al. 2017), whose spatial half the
 * denoisers are.  A pure image-space call on device buffers, for a viewport whose camera moves between frames of few samples.
 * - Buffers: device pointers, whole frames of width * height pixels in framebuffer order - d_color, d_normal, d_hist_color,
 *   d_hist_normal, d_out_color 3 floats per pixel; d_depth, d_hist_depth, d_hist_len, d_out_len 1 float; d_object_id,
 *   d_hist_object_id 1 int32 - the layouts pt_ctx_render / pt_ctx_render_aov write for a cfg without a band and without chunks.
 *   d_normal and d_hist_normal may each be NULL: the normal test runs only when both are given.
 * - History: after a call the host's history is the set (d_out_color, d_out_len, this call's d_depth, d_object_id, d_normal,
 *   cam).  The host swaps pointers; nothing is copied.  d_out_len is the history length in samples per pixel.
 * - First frame: d_hist_color, d_hist_len, d_hist_depth and d_hist_object_id are all NULL or none is.  When all are NULL
 *   hist_cam and d_hist_normal are not read, and the outputs are the colour and (float)weight everywhere.
 * - Aliasing: d_out_color may be d_color (a pixel reads its own colour before it writes).  No output may alias a history buffer
 *   or a guide: the kernel gathers neighbours.
 * - `hip_stream` as for pt_ctx_render (NULL = the context's own stream); blocking.  No scene is needed.  No scratch is taken.
 *   The call changes no state of the context: not the frame accumulators, not the held frames, not the denoisers' or
 *   pt_ctx_present's scratch, not the measured pass rates.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: a max_history or depth_tol that is
 *   negative or not finite; normal_min outside [-1, 1] or NaN; flags != 0; width or height 0; width * height above 2^28; NULL
 *   cam, d_color, d_depth, d_object_id, d_out_color or d_out_len; a partial set of history pointers; a full set of history
 *   pointers with NULL hist_cam; NULL ctx.  PT_ERR_HIP: a HIP call failed.  params == NULL stands for all zero.
 * - pt_reproject_defaults fills in the values a zero field stands for: weight 1, max_history 64, depth_tol 2^-3 (0.125),
 *   normal_min 0.9, flags 0.  They were chosen by the CPU study recorded in profiles/reproject_cpu_study.json.
 *
 * THE ARITHMETIC.  Every operation is IEEE binary32 + - * / and sqrt, correctly rounded, never contracted, in the order the
 * parentheses give - pt_ctx_denoise's rules.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; max(a, b) = a > b ? a : b; |v| is v
 * with its sign bit cleared; N(.) is pt_ctx_denoise's normalised normal, word for word.  (L, su, sv) and (L', su', sv') are
 * pt_camera_basis of cam and hist_cam, computed on the host in binary32; C is cam's position; C', D', f' are hist_cam's
 * position, direction (as stored) and focal length; W, H = width, height; wt = (float)weight (weight 0 stands for 1).
 * For pixel idx: x = idx % W, r = idx / W, y = H-1-r (render_pixel's row, mod.rs:805-806).
 * 1. No history.  If there is no history, or object_id[idx] < 0, or step 3 rejects, or step 4 ends with bsum > 0 false (every
 *    tap skipped, or taken with b = 0): out[c] = color[idx][c], len_out = wt.
 * 2. Same camera: all nine floats of cam and hist_cam are bitwise equal.  One tap, q = idx, with b = 1 and zexp = depth[idx];
 *    go to step 4.  A still camera is then an exact running mean.
 * 3. Projection.  sx = ((float)x + 0.5) / (float)W - 0.5; sy = ((float)y + 0.5) / (float)H - 0.5.
 *    S = (C + su*sx) + sv*sy per component; g = L - S; P = L + (g * (1 / sqrt(dot(g, g)))) * depth[idx]: the point the pixel
 *    centre's ray reaches at that distance, the direction made as render_pixel makes it.  The depth is sample 0's distance
 *    along a JITTERED ray while P uses the pixel centre: a sub-pixel error, which depth_tol and the bilinear taps are there for.
 *    v = P - L'; a = dot(v, D'); reject unless a > 0.  t = a / (f' * dot(D', D')); w = D'*f' - v / t per component (the sensor
 *    point minus C').  sx' = dot(w, su') / dot(su', su'); sy' = dot(w, sv') / dot(sv', sv').
 *    px = (sx' + 0.5) * (float)W - 0.5; py = (sy' + 0.5) * (float)H - 0.5; pr = (float)(H-1) - py.
 *    Reject unless px > -1 && px < W && pr > -1 && pr < H (a NaN rejects).
 *    x0 = floor(px), fx = px - (float)x0; r0 = floor(pr), fr = pr - (float)r0.  zexp = sqrt(dot(v, v)).
 *    The taps are q = (x0+i, r0+j), j = 0, 1 in the outer loop and i = 0, 1 in the inner loop, with
 *    b = (i ? fx : 1 - fx) * (j ? fr : 1 - fr).
 * 4. Tap test.  sum = (0, 0, 0), nsum = 0, bsum = 0.  A tap is skipped when q is outside the frame; when hist_len[q] > 0 does
 *    not hold; when hist_object_id[q] != object_id[idx]; when |zexp - hist_depth[q]| <= depth_tol * max(zexp, hist_depth[q])
 *    does not hold; when both normals are given and dot(N(idx), N'(q)) >= normal_min does not hold.  A tap that is taken adds
 *    sum[c] = sum[c] + hist_color[q][c] * b; nsum = nsum + hist_len[q] * b; bsum = bsum + b.
 * 5. Blend, if bsum > 0: h[c] = sum[c] / bsum; n = nsum / bsum; n' = n + wt; if n' > max_history, n' = max_history; if n' < wt,
 *    n' = wt; out[c] = h[c] + (color[idx][c] - h[c]) * (wt / n'); len_out = n'.
 * pt_reproject_project_host is the host instantiation of the projection the kernel compiles (csrc/pt_reproject.h): step 3 for
 * pixel idx at `depth`, from pt_camera_basis to zexp.  PT_OK and the three values; 1 for "no position" (step 3 rejected the
 * point; nothing is written); PT_ERR_INVALID for a NULL pointer, an empty frame, one above 2^28 pixels, or idx outside it.  It
 * needs no device. */
typedef struct pt_reproject_params {
    uint32_t weight;      /* samples per pixel the current frame holds; 0 = 1 */
    float max_history;    /* cap of the history length, in samples; 0 = the default; finite, >= 0 */
    float depth_tol;      /* relative depth tolerance; 0 = the default; finite, >= 0 */
    float normal_min;     /* smallest cosine between the two normals; 0 = the default; in [-1, 1] */
    uint32_t flags;       /* none defined: must be 0 */
} pt_reproject_params;
int pt_reproject_defaults(pt_reproject_params *out);
int pt_ctx_reproject(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_reproject_params *params,
                     const pt_camera *cam, const float *d_color, const float *d_depth,
                     const int32_t *d_object_id, const float *d_normal /* may be NULL */,
                     const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len,
                     const float *d_hist_depth, const int32_t *d_hist_object_id,
                     const float *d_hist_normal /* may be NULL */,
                     float *d_out_color, float *d_out_len, void *hip_stream);
/* host only, no device: the host instantiation of the projection the kernel compiles */
int pt_reproject_project_host(const pt_camera *cam, const pt_camera *hist_cam, uint32_t width,
                              uint32_t height, uint32_t idx, float depth,
                              float *px, float *pr, float *zexp);

/* ---- reprojection with temporal moments and a noise map per frame -----------------------------------------------
 * pt_ctx_reproject_var is pt_ctx_reproject plus the rest of SVGF's temporal pass: the first and second moment of s = (r + g) + b
 * are carried through the same reprojection as the colour and turned into a per-pixel variance; where the history is too short
 * to trust (the first frame, disocclusions) a spatial estimate over a window of the current frame stands in.  The result is an
 * error map in the units of THE NOISE ESTIMATE's e(p), which pt_ctx_denoise_var reads as it is: a viewport's loop is
 * pt_ctx_reproject_var -> pt_ctx_denoise_var -> pt_ctx_present.  pt_ctx_reproject itself is unchanged, and everything it states
 * about buffers, `hip_stream`, blocking, "no scene is needed" and the first-frame form carries over.  The differences:
 * - Moments planes: d_hist_moments and d_out_moments hold 2 floats per pixel, (m1, m2), in framebuffer order, 8-byte aligned.
 *   d_hist_moments belongs to the history set: all five history pointers (d_hist_color, d_hist_len, d_hist_moments,
 *   d_hist_depth, d_hist_object_id) are NULL, or none is.  After a call the host's history is the set (d_out_color, d_out_len,
 *   d_out_moments, this call's d_depth, d_object_id, d_normal, cam).
 * - Error map: d_error is 1 float per pixel, e below, in the units of THE NOISE ESTIMATE's e(p); it can be handed to
 *   pt_ctx_denoise_var as it is.  +inf means "no estimate".
 * - Aliasing: d_out_color may be d_color, as for pt_ctx_reproject.  d_out_moments and d_error may alias no input and no other
 *   output.
 * - Scratch: the in-place rule makes the call take a scratch plane of 4 B per pixel in the context - this frame's s values,
 *   written before any colour is overwritten.  It grows on demand, is reused between calls and is freed by pt_ctx_destroy; it
 *   lies outside the ray-queue budget and is shared with nothing.  The call changes no other state of the context.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: a max_history or depth_tol that is
 *   negative or not finite; normal_min outside [-1, 1] or NaN; radius above 3; flags != 0; width or height 0; width * height
 *   above 2^28; NULL cam, d_color, d_depth, d_object_id, d_out_color, d_out_len, d_out_moments or d_error; a partial set of the
 *   five history pointers; a full set of history pointers with NULL hist_cam; NULL ctx.  PT_ERR_HIP: a HIP call failed.
 *   params == NULL stands for all zero.
 * - pt_reproject_var_defaults fills in the values a zero field stands for: weight 1, max_history 64, depth_tol 2^-3 (0.125),
 *   normal_min 0.9 (pt_reproject_defaults' three), min_frames 2, radius 3, flags 0.  min_frames and radius were chosen by the
 *   CPU study recorded in profiles/reproject_var_cpu_study.json.
 *
 * THE ARITHMETIC, under pt_ctx_reproject's rules: binary32, correctly rounded, never contracted, in the order the parentheses
 * give; max(a, b) = a > b ? a : b; pos(v) = v > 0 ? v : 0 (a NaN gives 0); wt, W as there.
 * Colour and length.  d_out_color and d_out_len are pt_ctx_reproject's, bit for bit: its steps 1-5 with the same taps taken
 *    and the same b.
 * Moments.  s = (color[idx][0] + color[idx][1]) + color[idx][2], of the input colour; q2 = s*s.  Where pt_ctx_reproject's step 1
 *    applies to the pixel: m1 = s, m2 = q2.  Otherwise, over the taps that were taken and in their order:
 *    a1 = a1 + hist_m[q][0]*b; a2 = a2 + hist_m[q][1]*b; then h1 = a1/bsum; h2 = a2/bsum; k = wt/n';
 *    m1 = h1 + (s - h1)*k; m2 = h2 + (q2 - h2)*k: the colour's blend applied to the pair (s, s*s).
 * Temporal variance.  vt = pos(m2 - m1*m1); k = wt / len_out; long = len_out >= (float)min_frames * wt, the product formed on
 *    the host in binary32.
 * Spatial estimate, for pixels that are not long.  The pixel sits at column x and row r = idx / W; R = radius.  Loop dy = -R..R
 *    outside, dx = -R..R inside, over q = (x+dx, r+dy) inside the frame (a q outside it is skipped, not clamped).  The centre is
 *    always taken.  Another q is taken iff object_id[q] == object_id[idx] and either object_id[idx] < 0 or
 *    |depth[idx] - depth[q]| <= depth_tol * max(depth[idx], depth[q]).  A taken q adds S1 = S1 + s_q; S2 = S2 + s_q*s_q;
 *    cnt = cnt + 1, where s_q comes from the INPUT colour at q and cnt is an integer.  mean = S1/(float)cnt;
 *    vs = pos(S2/(float)cnt - mean*mean); v = max(vs, vt).  With cnt < 2 there is no estimate: e = +inf.
 * Long pixels.  v = vt.
 * Error.  e = sqrt(v*k) / sqrt(2^-6 + ((out[0] + out[1]) + out[2])), over the blended colour; if !(e < 12), e = 12. */
typedef struct pt_reproject_var_params {
    uint32_t weight;      /* as pt_reproject_params */
    float max_history;    /* as pt_reproject_params */
    float depth_tol;      /* as pt_reproject_params; also the spatial window's depth test */
    float normal_min;     /* as pt_reproject_params */
    uint32_t min_frames;  /* a history shorter than min_frames * weight samples takes the spatial estimate; 0 = the default */
    uint32_t radius;      /* spatial window (2*radius+1)^2; 0 = the default; at most 3 */
    uint32_t flags;       /* none defined: must be 0 */
} pt_reproject_var_params;
int pt_reproject_var_defaults(pt_reproject_var_params *out);
int pt_ctx_reproject_var(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_reproject_var_params *params,
                         const pt_camera *cam, const float *d_color, const float *d_depth,
                         const int32_t *d_object_id, const float *d_normal /* may be NULL */,
                         const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len,
                         const float *d_hist_moments, const float *d_hist_depth,
                         const int32_t *d_hist_object_id, const float *d_hist_normal /* may be NULL */,
                         float *d_out_color, float *d_out_len, float *d_out_moments, float *d_error,
                         void *hip_stream);

/* ---- reprojecting history through object edits: per-object motion ------------------------------------------------------
 * pt_ctx_reproject and pt_ctx_reproject_var follow the camera: step 3 puts the point a pixel sees into the history camera as if
 * the world had stood still.  pt_ctx_reproject_moved and pt_ctx_reproject_var_moved take a table of per-object motion records as
 * well, so that a frame in which pt_ctx_set_object moved an object keeps the object's history.
 *
 * THE RECORD.  motion[i] says where the surface point of object i that is now at P was in the history frame:
 * Pm[a] = P[a]*scale + offset[a] - two binary32 operations per component, never fused.  That covers every geometry edit
 * pt_ctx_set_object takes: a translation of a sphere or a mesh, and a sphere's radius.  Translation and uniform scale keep
 * normals, so the normal test is unchanged.
 * - IDENTITY, "did not move", is recognised by its bits: the scale word equals 1.0f and the three offset words equal +0.0f.
 * - A record with scale == 0 is the MARKER "this object has no usable history".
 * - Any other record needs a finite scale > 0 and finite offsets.
 * pt_object_motion_between(now, before, out) makes the record of one edit.  The marker when kind, tri_offset or tri_count differ;
 * when any word of color, emission or reflect_type differs (the object's old radiance is then not its new radiance); when a
 * sphere's now->radius is 0; when a position or (of a sphere) a radius is not finite.  Sphere: scale = |before.radius| /
 * |now.radius|; offset[a] = before.position[a] - now.position[a]*scale.  Mesh: scale = 1; offset[a] = before.position[a] -
 * now.position[a]; bs_center and bs_radius are not read.  Equal geometry then yields IDENTITY exactly (a difference of -0.0f is
 * stored as +0.0f).  Should the arithmetic leave the finite numbers, or a sphere's scale come out 0, the record is the marker.
 * PT_ERR_INVALID for a NULL pointer.  Host only.
 *
 * `motion` is a HOST array of n_motion records, indexed by object id.  The call copies it into scratch of the context, 16 B per
 * record, on the call's stream: the scratch grows on demand, lies outside the ray-queue budget, is freed by pt_ctx_destroy and is
 * shared with nothing.  The call changes no other state of the context (pt_ctx_reproject_var_moved: but for
 * pt_ctx_reproject_var's plane of s values).
 *
 * THE ARITHMETIC of pt_ctx_reproject_moved is pt_ctx_reproject's, word for word, with this inserted ahead of step 2 for a pixel
 * with id = object_id[idx] >= 0:
 *    rec = (uint32)id < n_motion ? motion[id] : IDENTITY.  An id beyond the table is never an error and never a read outside it.
 *    rec is the marker: step 1 - out = color, len_out = wt.
 *    rec is IDENTITY: steps 2-5 exactly as they are.
 *    Otherwise step 2 is never taken, not even under bitwise-equal cameras, and step 3 runs with v = Pm - L'.  The rest is
 *    unchanged: a, t, w, px, pr, zexp = sqrt(dot(v, v)), the four taps and their tests, the blend.
 * pt_ctx_reproject_var_moved is pt_ctx_reproject_var with "colour, length and taps are pt_ctx_reproject_moved's": the moments
 * ride the same taps; the spatial estimate does not read the table.
 * - Delegation: with motion == NULL, n_motion == 0, or every record IDENTITY (the host checks in O(n_motion)), the call is
 *   today's launch of pt_ctx_reproject / pt_ctx_reproject_var, unchanged, and copies nothing: their bytes by construction, and
 *   a loop in which nothing moves pays nothing.
 * - PT_ERR_INVALID, all refused before any device is touched: pt_ctx_reproject's (pt_ctx_reproject_var's) own in their order,
 *   then n_motion above 2^20; motion == NULL with n_motion != 0; a record that is neither IDENTITY nor a marker and has a
 *   non-finite or negative scale or a non-finite offset.
 * - Out of scope: the table describes the FIRST-HIT guides.  With PT_AOV_THROUGH_DELTA guides the id is the reflected object's and
 *   the depth is unfolded, so the map is meaningless there.  Light that changed elsewhere - the moved object's shadow, its bounce
 *   light - is stale history that no reprojection detects: a matter for the max_history policy on frames in which something
 *   moved (profiles/reproject_moved_cpu_study.json).
 * pt_reproject_project_moved_host is pt_reproject_project_host with the record `rec` (not NULL; a marker is refused with
 * PT_ERR_INVALID, as a record the calls refuse is): step 3 with the mapped point, the host instantiation of what the moved
 * kernels compile.  With an IDENTITY record it is pt_reproject_project_host. */
typedef struct pt_object_motion {
    float offset[3];
    float scale;
} pt_object_motion; /* 16 B */
int pt_object_motion_between(const pt_object *now, const pt_object *before, pt_object_motion *out); /* host only */
int pt_ctx_reproject_moved(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_reproject_params *params,
                           const pt_camera *cam, const float *d_color, const float *d_depth,
                           const int32_t *d_object_id, const float *d_normal /* may be NULL */,
                           const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len,
                           const float *d_hist_depth, const int32_t *d_hist_object_id,
                           const float *d_hist_normal /* may be NULL */,
                           float *d_out_color, float *d_out_len,
                           const pt_object_motion *motion /* host */, uint32_t n_motion, void *hip_stream);
int pt_ctx_reproject_var_moved(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_reproject_var_params *params,
                               const pt_camera *cam, const float *d_color, const float *d_depth,
                               const int32_t *d_object_id, const float *d_normal /* may be NULL */,
                               const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len,
                               const float *d_hist_moments, const float *d_hist_depth,
                               const int32_t *d_hist_object_id, const float *d_hist_normal /* may be NULL */,
                               float *d_out_color, float *d_out_len, float *d_out_moments, float *d_error,
                               const pt_object_motion *motion /* host */, uint32_t n_motion, void *hip_stream);
/* host only, no device */
int pt_reproject_project_moved_host(const pt_camera *cam, const pt_camera *hist_cam, uint32_t width,
                                    uint32_t height, uint32_t idx, float depth, const pt_object_motion *rec,
                                    float *px, float *pr, float *zexp);

/* ---- tracing at low resolution and filling the frame in through the guides ---------------------------------------------
 * pt_ctx_upsample fills a frame of width x height pixels from a colour frame traced at lo_width x lo_height: a joint bilateral
 * upsampler (Kopf et al. 2007) over the first-hit guides of BOTH sizes.  The paths, about nine intersections per sample, are
 * traced at a fraction of the resolution; the guides, one intersection per sample, at full resolution, so edges stay where they
 * are.  Its tap tests are pt_ctx_reproject's: object id, relative depth, normal cosine.  A pure image-space call on device
 * buffers; a viewport's loop is pt_ctx_render + pt_ctx_render_aov at the low size, pt_ctx_render_aov at the full size,
 * pt_ctx_upsample, then pt_ctx_reproject_var -> pt_ctx_denoise_var -> pt_ctx_present as before.
 * - Buffers: device pointers to whole frames in framebuffer order - what pt_ctx_render / pt_ctx_render_aov write for a cfg
 *   without a band and without chunks.  The d_lo_ planes hold lo_width * lo_height pixels, rendered with the SAME camera and
 *   scene at that size (the sensor does not depend on the pixel counts: both frames see the same picture); the others hold
 *   width * height pixels.  Colour, normal and albedo 3 floats per pixel; depth and weight 1 float; object id 1 int32.  Any
 *   sizes may be combined: smaller, equal or larger on either axis.
 * - Optional guides: the normal test runs only when both normals are given; demodulation runs only when both albedos are given.
 * - d_out_weight (may be NULL) receives the sum of the bilinear weights of the taps that passed the tests: 0 where none did
 *   and the fallback was used - "how sure" the pixel is.
 * - Aliasing: no output may alias any input or the other output.
 * - `hip_stream` as for pt_ctx_render (NULL = the context's own stream); blocking.  No scene is needed.  No scratch is taken.
 *   The call changes no state of the context.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: a depth_tol that is negative or not
 *   finite; normal_min outside [-1, 1] or NaN; flags != 0; one of the four sizes 0; one of the four sizes above 2^14 (16384:
 *   with that bound the integers of step 1 fit 32 bits and frac never reaches 1); NULL d_lo_color, d_lo_depth, d_lo_object_id,
 *   d_depth, d_object_id or d_out_color; NULL ctx.  PT_ERR_HIP: a HIP call failed.  params == NULL stands for all zero.
 * - pt_upsample_defaults fills in the values a zero field stands for: depth_tol 2^-2 (0.25), normal_min 0.95, flags 0.  They
 *   were chosen by the CPU study recorded in profiles/upsample_cpu_study.json.
 *
 * THE ARITHMETIC.  The rules are pt_ctx_denoise's: every operation is IEEE binary32 + - * /, correctly rounded and never
 * contracted, in the order the parentheses give.  max(a, b) = a > b ? a : b; |v| is v with its sign bit cleared;
 * clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v); dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; N(.) is pt_ctx_denoise's normalised
 * normal, word for word; m_c(.) is pt_ctx_denoise's demodulation factor, albedo[c] > 2^-6 ? albedo[c] : 1 - and 1 for every
 * channel unless BOTH albedo planes are given.  W, H are the frame's size and w, h the low-resolution size.  For frame pixel
 * idx: x = idx % W, r = idx / W.
 * 1. Tap position, in unsigned 32-bit integers.  ax = (2x + 1) * w + W; x0 = (int)(ax / (2W)) - 1; ex = ax % (2W);
 *    fx = (float)ex / (float)(2W).  Likewise ar = (2r + 1) * h + H, which gives r0, er and fr = (float)er / (float)(2H).  The
 *    centre of frame pixel x lies at x0 + fx on the axis whose integers are the low-resolution pixel centres.  It follows that
 *    -1 <= x0 <= w-1 and 0 <= fx < 1; equal sizes give x0 = x, fx = 0; wherever one tap of an axis is outside the
 *    low-resolution frame, the other one's weight is > 0.
 * 2. Taps.  q = (x0 + i, r0 + j), with j = 0, 1 in the outer loop and i = 0, 1 in the inner loop;
 *    b = (i ? fx : 1 - fx) * (j ? fr : 1 - fr); u_q[c] = lo_color[q][c] / m_c^lo(q).
 * 3. Tested pass.  sum = (0, 0, 0), bsum = 0.  A tap is skipped when q is outside the low-resolution frame; when
 *    lo_object_id[q] != object_id[idx]; when object_id[idx] >= 0 and
 *    |depth[idx] - lo_depth[q]| <= depth_tol * max(depth[idx], lo_depth[q]) does not hold; when object_id[idx] >= 0, both
 *    normals are given and dot(N(idx), N_lo(q)) >= normal_min does not hold.  A miss (id < 0) is held to the id test alone: its
 *    depth is +inf.  A tap that is taken adds sum[c] = sum[c] + u_q[c] * b; bsum = bsum + b.  A taken tap with b = 0 adds zeros.
 * 4. If bsum > 0: weight = bsum.  Otherwise the fallback: the same loop again, with only the taps outside the low-resolution
 *    frame skipped; weight = 0.  By step 1 its bsum is > 0.
 * 5. out[c] = clamp((sum[c] / bsum) * m_c(idx)).
 * Colours are expected finite; for others the result is unspecified.  With equal sizes and the low-resolution guides equal to
 * the frame's, the output is clamp(color): the colour itself for a rendered frame, bit for bit (without the albedo planes; with
 * them (c / m) * m may differ from c in the last bit).
 * pt_upsample_tap_host is the host instantiation of the tap position the kernel compiles (csrc/pt_upsample.h): step 1 for one
 * coordinate of one axis, *first = x0 and *frac = fx.  PT_ERR_INVALID for a NULL pointer, a size that is 0 or above 2^14, or
 * coord >= size.  It needs no device. */
typedef struct pt_upsample_params {
    float depth_tol;    /* relative depth tolerance of a tap; 0 = the default; finite, >= 0 */
    float normal_min;   /* smallest cosine between the two normals; 0 = the default; in [-1, 1] */
    uint32_t flags;     /* none defined: must be 0 */
} pt_upsample_params;
int pt_upsample_defaults(pt_upsample_params *out);
int pt_ctx_upsample(pt_ctx *ctx, uint32_t width, uint32_t height, uint32_t lo_width, uint32_t lo_height,
                    const pt_upsample_params *params /* NULL = all zero */,
                    const float *d_lo_color, const float *d_lo_depth, const int32_t *d_lo_object_id,
                    const float *d_lo_normal /* may be NULL */, const float *d_lo_albedo /* may be NULL */,
                    const float *d_depth, const int32_t *d_object_id,
                    const float *d_normal /* may be NULL */, const float *d_albedo /* may be NULL */,
                    float *d_out_color, float *d_out_weight /* may be NULL */, void *hip_stream);
/* host only, no device: the host instantiation of the tap position the kernel compiles */
int pt_upsample_tap_host(uint32_t size, uint32_t lo_size, uint32_t coord, int32_t *first, float *frac);

/* ---- retracing chosen pixels of a frame ---------------------------------------------------------------------------------
 * Two passes of the viewport loop say which pixels they could not serve: pt_ctx_upsample writes d_out_weight = 0 where no tap
 * passed and the pixel took the bilinear fallback, pt_ctx_reproject* write d_out_len = weight where a pixel found no history.
 * pt_ctx_select_pixels turns such planes into a byte mask and counts it; pt_ctx_render_masked traces the masked pixels of a
 * frame and writes them into it, each one pt_ctx_render's pixel bit for bit.  The loop with both:
 *   pt_ctx_upsample(..., d_up, d_weight) -> pt_ctx_select_pixels(weight_max = 0, d_weight) -> pt_ctx_render_masked(cfg at the
 *   LOW-RESOLUTION spp, d_mask, d_up) -> pt_ctx_reproject_var -> ...
 *
 * pt_ctx_select_pixels: an image pass on device buffers.
 * - The planes are whole frames of width * height floats in framebuffer order; either may be NULL, not both.  d_mask receives
 *   width * height bytes.  No output may alias an input.
 * - THE PREDICATE, in IEEE binary32 comparisons:
 *     mask[p] = ((d_weight && !(weight[p] > weight_max)) || (d_len && !(len[p] > len_max))) ? 1 : 0.
 *   A NaN in a plane selects the pixel (no comparison with a NaN holds).  The thresholds are taken literally: there are no
 *   defaults; a threshold of +inf selects every pixel, one of -inf only the pixels that hold -inf or a NaN.
 * - *n_selected (host memory, may be NULL) is the number of ones, counted with integer atomics in the same launch: exact,
 *   whatever the order.
 * - `hip_stream` as for pt_ctx_render (NULL = the context's own stream); blocking.  No scene is needed.  The call changes no
 *   state of the context beyond a scratch word for the count.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: a NaN threshold; flags != 0; width or
 *   height 0; width * height > 2^28; both planes NULL; NULL d_mask; NULL params; NULL ctx.  PT_ERR_HIP: a HIP call failed.
 *
 * pt_ctx_render_masked: a frame call.
 * - d_mask: pt_config_pixels(cfg) bytes in the call's pixel order (byte k is pixel idx_begin + k of the frame); nonzero means
 *   selected, whatever the value.  d_rgb: the call's frame, pt_config_pixels(cfg) * 3 floats in pt_ctx_render's layout, input
 *   and output.
 * - Every selected pixel k gets d_rgb[3k + c] = what pt_ctx_render with the same cfg writes there: samples [0, cfg->spp), the
 *   same fixed-point sums, the same mean and clamp, bit for bit.  No other float of d_rgb is written.  *n_pixels (host memory,
 *   may be NULL) is the number of selected pixels.
 * - The band and the flags follow pt_ctx_render_adaptive: the band is whole image rows, chunk_step <= 1, `backend` is ignored
 *   (but must be a valid one), PT_FLAG_NO_BVH selects the linear scan (same bytes), PT_FLAG_PIPELINES is refused; cfg->spp as
 *   pt_ctx_render bounds it.
 * - An empty mask: PT_OK, *n_pixels = 0, zero stats; nothing is traced or written.
 * - `cancel` is read before the trace and between its rounds (sized as the megakernel's: about a tenth of a second).  On
 *   PT_CANCELLED d_rgb is untouched: the call is kept whole or not at all.  There is no progress callback.
 * - stats (may be NULL): samples = *n_pixels * spp, ray_bounces exact, passes = the trace's launches.
 * - State: the list of selected pixels (4 B each) and the compact accumulator (24 B each) are scratch of the context, grown on
 *   demand and freed by pt_ctx_destroy; the rounds keep a measured rate of their own, which pt_ctx_set_scene forgets.  Nothing
 *   else changes: not the frame pt_ctx_accumulate holds, not the adaptive frame, not the other calls' rates.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: NULL cfg, d_mask or d_rgb; NULL ctx; no
 *   scene; a band that is not whole rows; chunk_step > 1 or PT_FLAG_PIPELINES; whatever pt_ctx_render refuses of a cfg.
 *   PT_ERR_HIP: a HIP call failed.  PT_ERR_OVERFLOW as for the megakernel. */
typedef struct pt_select_params {
    float weight_max;   /* taken literally, no default; not NaN */
    float len_max;      /* taken literally, no default; not NaN */
    uint32_t flags;     /* none defined: must be 0 */
} pt_select_params;
int pt_ctx_select_pixels(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_select_params *params,
                         const float *d_weight /* may be NULL */, const float *d_len /* may be NULL */,
                         uint8_t *d_mask, uint32_t *n_selected /* host, may be NULL */, void *hip_stream);
int pt_ctx_render_masked(pt_ctx *ctx, const pt_config *cfg, const uint8_t *d_mask, void *d_rgb,
                         void *hip_stream, const volatile uint8_t *cancel, pt_stats *stats,
                         uint32_t *n_pixels /* host, may be NULL */);

/* ---- reprojection with per-pixel sample counts ---------------------------------------------------------------------------
 * pt_ctx_reproject_var and pt_ctx_reproject_var_moved assume that every pixel of the frame holds the same number of samples,
 * pt_reproject_var_params.weight: that one number is the blend factor's numerator, the history length that is carried, the
 * `long` test and the scale k of the error map.  Two calls produce frames for which it is false: pt_ctx_render_adaptive /
 * pt_ctx_accumulate_adaptive, whose d_spp holds every pixel's own count, and pt_ctx_select_pixels + pt_ctx_render_masked at a
 * multiple of the frame's samples.  pt_ctx_reproject_var_weighted is pt_ctx_reproject_var_moved with one more input, d_spp: a
 * plane of width * height uint32 in framebuffer order, device memory, the samples each pixel of d_color holds - the layout
 * pt_ctx_render_adaptive writes as its d_spp for a cfg without a band.  A count of 0 means "this pixel was not traced this
 * frame": its colour is not data, and its history is carried through as it is, so a host may trace a subset of the pixels per
 * frame under a still or slowly moving camera.
 * - Everything pt_ctx_reproject_var_moved states carries over word for word: the buffers, the history set, aliasing, the scratch
 *   plane of s values, the motion table and its scratch, `hip_stream`, blocking, "no scene is needed".  d_spp may alias no output.
 * - PT_ERR_INVALID: pt_ctx_reproject_var_moved's refusals in its order.  d_spp is never refused.
 * - Delegation: with d_spp == NULL the call is pt_ctx_reproject_var_moved with the same arguments: that call's launches, and its
 *   bytes by construction.
 *
 * THE ARITHMETIC is pt_ctx_reproject_var_moved's, with these changes and no others.  w0 = (float)weight (0 stands for 1), the
 * uniform value as before.  For pixel idx, c = spp[idx] and wp = (float)c; a count above 2^24 is converted round-to-nearest
 * and is not checked.
 * c > 0.  Every wt in steps 1 and 5 of pt_ctx_reproject, in the moments and in k = wt / len_out, is wp.
 *    long = len_out >= (float)min_frames * wp; the product is formed on the device in binary32 (exact for the counts the
 *    library produces).
 * c == 0.  Where step 1 applies (no history, id < 0, the marker, rejected, no tap with bsum > 0): out = color[idx] as stored,
 *    len_out = 0, m1 = s, m2 = s*s, e = +inf.  Otherwise h, h1, h2 and n = nsum / bsum as before; n' = n, and if
 *    n' > max_history, n' = max_history; out[c] = h[c], m1 = h1, m2 = h2 - the values themselves, not h + (x - h)*0: a NaN
 *    colour does not leak and -0 stays -0; len_out = n'; long = len_out >= (float)min_frames * w0 (the host-formed product);
 *    long: e = the error of pos(m2 - m1*m1) with k = w0 / len_out over out; not long: e = +inf - there is no spatial
 *    estimate without a colour.
 * Spatial estimate (pixels with c > 0 that are not long).  As before, with one more condition on every q but the centre:
 *    spp[q] == spp[idx].  A neighbour with another count holds values of another variance; one with count 0 holds no data.
 *    k = wp / len_out.
 * The plane of s values is written for every pixel as before; the value of a c == 0 pixel is never read by a taken tap.
 * CONSEQUENCE.  A plane that holds the constant w everywhere gives, bit for bit, pt_ctx_reproject_var_moved with weight = w,
 * on all four outputs.
 *
 * pt_ctx_spp_plane builds the plane of a boosted frame: spp[p] = (d_mask && mask[p] != 0) ? masked : base, with d_mask
 * pt_ctx_select_pixels' byte mask (width * height bytes, device; may be NULL) and d_spp width * height uint32 (device).
 * - An image pass: no scene is needed, no scratch is taken, no state of the context changes; `hip_stream` as for
 *   pt_ctx_render; blocking.  d_spp may not alias d_mask.
 * - PT_ERR_INVALID, all refused before any device is touched, checked in this order: width or height 0; width * height above
 *   2^28; NULL d_spp; NULL ctx.  PT_ERR_HIP: a HIP call failed. */
int pt_ctx_reproject_var_weighted(pt_ctx *ctx, uint32_t width, uint32_t height, const pt_reproject_var_params *params,
                                  const pt_camera *cam, const float *d_color, const float *d_depth,
                                  const int32_t *d_object_id, const float *d_normal /* may be NULL */,
                                  const uint32_t *d_spp /* width*height u32, device; NULL = uniform */,
                                  const pt_camera *hist_cam, const float *d_hist_color, const float *d_hist_len,
                                  const float *d_hist_moments, const float *d_hist_depth,
                                  const int32_t *d_hist_object_id, const float *d_hist_normal /* may be NULL */,
                                  float *d_out_color, float *d_out_len, float *d_out_moments, float *d_error,
                                  const pt_object_motion *motion /* host, may be NULL */, uint32_t n_motion, void *hip_stream);
int pt_ctx_spp_plane(pt_ctx *ctx, uint32_t width, uint32_t height, uint32_t base, const uint8_t *d_mask /* may be NULL */,
                     uint32_t masked, uint32_t *d_spp, void *hip_stream);

/* ---- the one collective of the path: the framebuffer gather over RCCL (xGMI) ---------------------------------
 * One process (or thread) per GPU renders its rows with pt_ctx_render (chunk_first = rank, chunk_step = n_ranks) into
 * device memory; pt_comm_gather_frame then gives EVERY rank the whole frame in device memory: one in-place
 * ncclAllGather of the rank buffers (padded to the largest) and one kernel that puts the rows back in framebuffer order.
 * librccl is loaded on first use (dlopen; PT_RCCL_LIB overrides the name), so hosts that never gather do not need it. */
typedef struct pt_comm pt_comm;
#define PT_COMM_ID_BYTES 128
/* rank 0: a fresh id (ncclGetUniqueId); the host carries the bytes to the other ranks by its own means */
int pt_comm_unique_id(uint8_t id[PT_COMM_ID_BYTES]);
/* every rank, collectively: ncclCommInitRank on `device` */
int pt_comm_create(int device, int rank, int n_ranks, const uint8_t id[PT_COMM_ID_BYTES], pt_comm **out);
void pt_comm_destroy(pt_comm *comm);
/* cfg: the frame (width, height, band) and the chunk size the ranks rendered with (chunk_pixels; chunk_first /
 * chunk_step are taken from the communicator).  d_local_rgb: this rank's pt_ctx_render output; d_frame_rgb: band
 * pixels * 3 floats on this rank's device.  `hip_stream`: NULL = the communicator's own stream.  Blocking. */
int pt_comm_gather_frame(pt_comm *comm, const pt_config *cfg, const void *d_local_rgb, void *d_frame_rgb, void *hip_stream);

/* Image.hash (mod.rs:897-926): Rust's DefaultHasher (SipHash-1-3, zero key) over the f32 bit patterns of the
 * pixels in order; the GUI uses it to invalidate its canvas cache (src/views/render_tab.rs:248-256). */
uint64_t pt_image_hash(const float *rgb, size_t n_floats);
/* the underlying SipHash-c-d (k0, k1 = key) so that the implementation can be pinned on the published
 * SipHash-2-4 test vector */
uint64_t pt_siphash(uint32_t c_rounds, uint32_t d_rounds, uint64_t k0, uint64_t k1, const uint8_t *data, size_t len);

/* ---- formats either side of the path (host only, no GPU needed) ------------------------- */

typedef struct pt_scene pt_scene;

/* SceneDescriptor::load + to_data (mod.rs:92-110, 304-318) and load_off (load_off.rs:8-85).
 * `path` is the JSON file; MeshFile paths are resolved against `base_dir` (the reference
 * resolves them against the process CWD; pass "." for that behaviour). */
int pt_scene_load(const char *path, const char *base_dir, pt_scene **out);
/* flags = PT_LOAD_TRIANGULATE additionally accepts OFF faces with more than 3 vertices (meshes/hdodec.off has
 * pentagons) and fan-triangulates them.  An extension: the reference's load_off rejects such files
 * (load_off.rs:73-76), so there is no reference behaviour to match beyond "a triangle stays a triangle". */
#define PT_LOAD_TRIANGULATE 1u
int pt_scene_load_ex(const char *path, const char *base_dir, uint32_t flags, pt_scene **out);
/* SceneData::to_descriptor + SceneDescriptor::save (mod.rs:112-117, 127-149): the same bytes
 * serde_json::to_string_pretty writes (MeshFile objects keep their path/scale, inline meshes their
 * bounding_sphere / bounding_box). */
int pt_scene_save(const pt_scene *s, const char *path);
int pt_scene_set_camera(pt_scene *s, const pt_camera *cam);
/* setup_scenes (src/render/scenes.rs:43-318): the scenes the reference builds in code and saves when scenes/ holds
 * no *.json (load_scene_ids, scenes.rs:28-38) - "single-sphere", "cartesian", "two-spheres", "three-spheres",
 * "cornell", "mesh" in that order.  `base_dir` is where "mesh" finds meshes/mctri.off. */
uint32_t pt_builtin_scene_count(void);
const char *pt_builtin_scene_id(uint32_t i);
int pt_scene_builtin(const char *id, const char *base_dir, pt_scene **out);
void pt_scene_free(pt_scene *s);
const char *pt_scene_id(const pt_scene *s);
const pt_camera *pt_scene_camera(const pt_scene *s);
const pt_object *pt_scene_objects(const pt_scene *s, uint32_t *n);
const pt_triangle *pt_scene_triangles(const pt_scene *s, uint32_t *n);
/* Mesh.bounding_box of object i as the scene file stored it, or as Mesh::new computes it for MeshFile objects and meshes
 * built through the API; NULL for spheres.  12 triangles, valid until the scene is freed. */
const pt_triangle *pt_scene_bounding_box(const pt_scene *s, uint32_t object);

/* load_off (load_off.rs:8-85): returns a malloc'ed triangle array (free with pt_free). */
int pt_load_off(const char *path, float scale, pt_triangle **tris, uint32_t *n_tris);
int pt_load_off_ex(const char *path, float scale, uint32_t flags, pt_triangle **tris, uint32_t *n_tris);
void pt_free(void *p);

/* gamma (mod.rs:57-63) and the P3 writer (mod.rs:1043-1076). */
float pt_gamma_correction(float x);
uint32_t pt_to_int_with_gamma_correction(float x);
int pt_write_ppm(const char *path, const float *rgb, uint32_t width, uint32_t height, uint32_t spp,
                 const char *scene_id, uint64_t seconds);
/* A whole frame (framebuffer order, width * height * channels floats) as a little-endian PFM: "PF" for 3 channels, "Pf" for 1
 * (any other count: PT_ERR_INVALID), scale -1.0; PT_ERR_IO when the file cannot be written.  Placed pixel for pixel over
 * pt_write_ppm's image of the same frame: the PPM lists framebuffer index i as pixel W*H-1-i from the top left, and PFM
 * stores rows bottom-up, so PFM row q (from the bottom), column c holds framebuffer index q*W + (W-1-c) - each framebuffer
 * row in turn, its columns reversed. */
int pt_write_pfm(const char *path, const float *data, uint32_t width, uint32_t height, uint32_t channels);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_H */
