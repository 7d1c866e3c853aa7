//! src/render/hip.rs — binding of libptrace_hip.so (include/ptrace.h, ABI 5) for filippo-orru/path-tracer-rust.
//!
//! NOT COMPILED HERE: the build image has no Rust toolchain.  This is the file a maintainer adds as `mod hip;` in
//! `src/render/mod.rs` (a child module of `render`, so it may read the private fields of `Mesh` and
//! `StandaloneSphere`), plus the few lines in `render()` shown at the bottom.  Every struct mirrors a `typedef struct`
//! of include/ptrace.h field by field (sizes 36 / 36 / 72 / 56 / 56 bytes, checked from Python in tests/test_abi.py).
//!
//! Line references are to the reference's src/render/mod.rs.
use super::{ReflectType, RenderConfig, SceneData, SceneObject, SceneObjectData};
use glam::Vec3;
use std::ffi::{c_void, CStr};
use std::os::raw::c_char;
use std::sync::atomic::{AtomicBool, AtomicUsize, Ordering};
use std::sync::Mutex;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct PtCamera {
    pub position: [f32; 3],
    pub direction: [f32; 3],
    pub focal_length: f32,
    pub sensor_width: f32,
    pub aspect_ratio: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct PtTriangle {
    pub a: [f32; 3],
    pub b: [f32; 3],
    pub c: [f32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct PtObject {
    pub kind: u32, // 0 = PT_SPHERE, 1 = PT_MESH
    pub position: [f32; 3],
    pub radius: f32,
    pub color: [f32; 3],
    pub emission: [f32; 3],
    pub reflect_type: u32, // enum order of ReflectType (:71-76)
    pub tri_offset: u32,
    pub tri_count: u32,
    pub bs_center: [f32; 3], // Mesh.bounding_sphere.position, object-local, as stored (:268 adds `position`)
    pub bs_radius: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct PtConfig {
    pub width: u32,
    pub height: u32,
    pub spp: u32,
    pub backend: u32, // 0 wavefront, 1 megakernel
    pub seed: u64,
    pub idx_begin: u32, // 0, 0 = whole frame
    pub idx_end: u32,
    pub rays_per_pass: u32, // 0 = library default
    pub flags: u32,
    pub chunk_pixels: u32,
    pub chunk_first: u32,
    pub chunk_step: u32,
    pub progress_ms: u32, // 0 = 500 ms, the cadence of the reference's progress thread (:965-982)
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtStats {
    pub ray_bounces: u64,
    pub samples: u64,
    pub intersect_rays: u64,
    pub intersect_launches: u32,
    pub passes: u32,
    pub ms_total: f64,
    pub ms_device: f64,
    pub ms_intersect: f64,
}

// pt_ctx_denoise_var's parameters; a zero field = the library's default (pt_denoise_var_defaults)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtDenoiseVarParams {
    pub levels: u32,
    pub sigma_var: f32,
    pub sigma_depth: f32,
    pub flags: u32,
}

// pt_ctx_overlay's parameters (the editing cues drawn on a frame before pt_ctx_present); all zero = nothing drawn.
// pt_overlay_defaults writes the defaults out, with the grid sized for a camera.
pub const PT_OVERLAY_SKY: u32 = 1;
pub const PT_OVERLAY_GRID: u32 = 2;
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtOverlayParams {
    pub flags: u32,
    pub n_selected: u32,
    pub selected: [i32; 16],
    pub radius: u32,
    pub outline_color: [f32; 3],
    pub outline_alpha: f32,
    pub fill_color: [f32; 3],
    pub fill_alpha: f32,
    pub sky_top: [f32; 3],
    pub sky_bottom: [f32; 3],
    pub grid_color: [f32; 3],
    pub grid_alpha: f32,
    pub grid_y: f32,
    pub grid_spacing: f32,
    pub grid_half_width: f32,
    pub grid_extent: f32,
}

// pt_ctx_solid's parameters (a lit solid view from the first-hit guides); every field is taken as it stands - there is no
// "0 = default": pt_solid_defaults writes the defaults out, and a NULL pointer stands for them.
pub const PT_SOLID_HEADLIGHT: u32 = 1;
pub const PT_SOLID_REFLECT_SKY: u32 = 2;
pub const PT_SOLID_MAX_SHININESS_LOG2: u32 = 10;
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtSolidParams {
    pub flags: u32,
    pub light: [f32; 3],
    pub ambient: f32,
    pub diffuse: f32,
    pub specular: f32,
    pub shininess_log2: u32,
    pub background: [f32; 3],
    pub sky_top: [f32; 3],
    pub sky_bottom: [f32; 3],
}

// one record of pt_ctx_solid's looks table, a host array indexed by object id (pt_solid_look_of fills one from a PtObject)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtSolidLook {
    pub emission: [f32; 3],
    pub reflect_type: u32,
}

// the tone stage (include/ptrace_tone.h): the meter's rectangle and flags, what it counts, pt_meter_exposure's parameters, and
// pt_ctx_tonemap's - every field of those taken as it stands; pt_tonemap_defaults / pt_meter_exposure_defaults write the defaults out
pub const PT_METER_SKIP_MISSES: u32 = 1;
pub const PT_METER_BINS: u32 = 256;
pub const PT_TONE_CLAMP: u32 = 0;
pub const PT_TONE_REINHARD: u32 = 1;
pub const PT_TONE_ACES: u32 = 2;
pub const PT_TONE_LUMA: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtMeterParams {
    pub flags: u32,
    pub x0: u32,
    pub y0: u32,
    pub x1: u32,
    pub y1: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PtMeterStats {
    pub pixels: u64,
    pub dark: u64,
    pub histogram: [u32; 256],
    pub max_luminance: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtMeterExposureParams {
    pub key: f32,
    pub low_fraction: f32,
    pub high_fraction: f32,
    pub min_exposure: f32,
    pub max_exposure: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtTonemapParams {
    pub curve: u32,
    pub flags: u32,
    pub exposure: f32,
    pub white: f32,
}

// the firefly stage (include/ptrace_despike.h): pt_ctx_despike's parameters, every field taken as it stands
// (pt_despike_defaults writes the defaults out), and what it counts
pub const PT_DESPIKE_SAME_OBJECT: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtDespikeParams {
    pub radius: u32,
    pub rank: u32,
    pub flags: u32,
    pub threshold: f32,
    pub floor: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtDespikeStats {
    pub pixels: u64,
    pub spikes: u64,
    pub nonfinite: u64,
}

// pt_ctx_present's parameters; all zero = the frame's own size, exposure 1, RGBA8, display order
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtPresentParams {
    pub out_width: u32,
    pub out_height: u32,
    pub exposure: f32,
    pub format: u32,
    pub flags: u32,
}

// pt_ctx_reproject's parameters; a zero field = the library's default (pt_reproject_defaults)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtReprojectParams {
    pub weight: u32,
    pub max_history: f32,
    pub depth_tol: f32,
    pub normal_min: f32,
    pub flags: u32,
}

// pt_ctx_reproject_var's parameters; a zero field = the library's default (pt_reproject_var_defaults)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtReprojectVarParams {
    pub weight: u32,
    pub max_history: f32,
    pub depth_tol: f32,
    pub normal_min: f32,
    pub min_frames: u32,
    pub radius: u32,
    pub flags: u32,
}

// one record of pt_ctx_reproject_moved's per-object motion table: the surface point now at P was at P * scale + offset in the
// history frame; (0, 0, 0, 1) bit for bit = did not move, scale 0 = no usable history (pt_object_motion_between makes one)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PtObjectMotion {
    pub offset: [f32; 3],
    pub scale: f32,
}

// pt_ctx_upsample's parameters; a zero field = the library's default (pt_upsample_defaults)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtUpsampleParams {
    pub depth_tol: f32,
    pub normal_min: f32,
    pub flags: u32,
}

// pt_ctx_select_pixels' thresholds: taken literally, no defaults
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtSelectParams {
    pub weight_max: f32,
    pub len_max: f32,
    pub flags: u32,
}

// pt_ctx_scatter (a parity probe: one radiance() invocation on the device): an item, a given surface, what the step decided
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtScatterItem {
    pub o: [f32; 3],
    pub d: [f32; 3],
    pub thr: [f32; 3],
    pub pixel: u32,
    pub sample: u32,
    pub depth: u32,
    pub branch: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtScatterSurface {
    pub x: [f32; 3],
    pub n: [f32; 3],
    pub color: [f32; 3],
    pub emission: [f32; 3],
    pub reflect: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtScatterOut {
    pub hit: i32,
    pub n_rays: u32,
    pub emits: u32,
    pub deferred: u32,
    pub x: [f32; 3],
    pub contrib: [f32; 3],
    pub d0: [f32; 3],
    pub thr0: [f32; 3],
    pub d1: [f32; 3],
    pub thr1: [f32; 3],
    pub depth0: u32,
    pub branch0: u32,
    pub depth1: u32,
    pub branch1: u32,
}

pub const PT_SCATTER_GIVEN: u32 = 0;
pub const PT_SCATTER_BY_ID: u32 = 1;
pub const PT_SCATTER_BY_RANK: u32 = 2;
pub const PT_SCATTER_DEFER_REFRACT: u32 = 0x10;
pub const PT_SCATTER_REFRACT_ONLY: u32 = 0x20;
pub const PT_SCATTER_NOT_SHADED: i32 = -2;

// pt_ctx_denoise's parameters; a zero field = the library's default (pt_denoise_defaults)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtDenoiseParams {
    pub levels: u32,
    pub sigma_color: f32,
    pub sigma_normal_pow: f32,
    pub sigma_depth: f32,
    pub flags: u32,
}

// pt_ctx_render_aov_ex's parameters: flags PT_AOV_THROUGH_DELTA or 0; max_chain 0 = 8, at most PT_AOV_MAX_CHAIN, needs the flag
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtAovParams {
    pub flags: u32,
    pub max_chain: u32,
}

// pt_ctx_accum_noise's frame statistics: the error estimate e(p) from the two halves of a noise-tracked frame's samples
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PtNoiseStats {
    pub spp_min: u32,
    pub spp_max: u32,
    pub spp_a_min: u32,
    pub spp_b_min: u32,
    pub pixels: u64,
    pub mean_error: f64,
    pub histogram: [u32; 64],
}

// pt_ctx_accumulate_until's stopping rule; a zero criterion is not used
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtNoiseTarget {
    pub mean_error: f32,
    pub quantile: f32,
    pub quantile_error: f32,
    pub min_spp: u32,
}

// pt_ctx_render_adaptive: a tile (4, 8, 16 or 32 pixels square; 0 = 8) takes no more samples once the mean of its error
// estimate is at most tile_error; min_spp is the first level (0 = 16)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtAdaptiveParams {
    pub tile_error: f32,
    pub tile: u32,
    pub min_spp: u32,
}

// what an adaptive frame did: the levels run, the tiles that closed at each, the samples traced
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PtAdaptiveStats {
    pub tiles: u32,
    pub tiles_open: u32,
    pub levels: u32,
    pub level_spp: [u32; 32],
    pub tiles_closed: [u32; 32],
    pub samples: u64,
    pub mean_error: f64,
}

// the adaptive frame a context holds, re-decided under a target and a cap (pt_ctx_adaptive_info)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PtAdaptiveInfo {
    pub tiles: u32,
    pub tiles_open: u32,
    pub tiles_at_cap: u32,
    pub spp_min: u32,
    pub spp_max: u32,
    pub samples: u64,
    pub mean_error: f64,
}
/// pt_ctx_table_hashes: the index of each device table in its output (PT_TABLE_* of ptrace.h)
pub const PT_TABLE_OBJS: usize = 0;
pub const PT_TABLE_OBJ_PAIRS: usize = 1;
pub const PT_TABLE_TRI_PAIRS: usize = 2;
pub const PT_TABLE_MATS: usize = 3;
pub const PT_TABLE_TRI_SHADE: usize = 4;
pub const PT_TABLE_BVH_NODES: usize = 5;
pub const PT_TABLE_BVH_NODES4: usize = 6;
pub const PT_TABLE_SPH_PAIRS: usize = 7;
pub const PT_TABLE_FLAT_PAIRS: usize = 8;
pub const PT_TABLE_CAND_PAIRS: usize = 9;
pub const PT_TABLE_RANK_ID: usize = 10;
pub const PT_TABLE_SURF: usize = 11;
pub const PT_TABLE_TRI_RANK: usize = 12;
pub const PT_TABLE_BVH_MESHES: usize = 13;
pub const PT_TABLE_COUNT: usize = 14;
pub const PT_DENOISE_NO_DEMODULATE: u32 = 1;
pub const PT_AOV_THROUGH_DELTA: u32 = 1;
pub const PT_AOV_MAX_CHAIN: u32 = 16;
pub const PT_PRESENT_RGBA8: u32 = 0;
pub const PT_PRESENT_RGB8: u32 = 1;
pub const PT_PRESENT_FRAMEBUFFER_ORDER: u32 = 1;

pub const PT_OK: i32 = 0;
pub const PT_CANCELLED: i32 = -4;

pub type PtProgressFn = extern "C" fn(user: *mut c_void, fraction: f32);

/// opaque `pt_ctx` of include/ptrace.h: one GPU, one stream, the device copies of one scene and the ray queues
#[repr(C)]
pub struct PtCtx {
    _private: [u8; 0],
}

#[link(name = "ptrace_hip")]
extern "C" {
    pub fn pt_render(
        cfg: *const PtConfig,
        cam: *const PtCamera,
        objs: *const PtObject,
        n_objs: u32,
        tris: *const PtTriangle,
        n_tris: u32,
        out_rgb: *mut f32,
        cancel: *const u8,
        cb: Option<PtProgressFn>,
        user: *mut c_void,
        stats: *mut PtStats,
    ) -> i32;
    // the resident form: scene tables and ray queues stay in HBM across frames, the frame is written to device memory,
    // and the progress callback may pull what has been accumulated so far (pt_ctx_snapshot)
    pub fn pt_ctx_create(device: i32, out: *mut *mut PtCtx) -> i32;
    pub fn pt_ctx_destroy(ctx: *mut PtCtx);
    pub fn pt_ctx_set_scene(
        ctx: *mut PtCtx,
        cam: *const PtCamera,
        objs: *const PtObject,
        n_objs: u32,
        tris: *const PtTriangle,
        n_tris: u32,
    ) -> i32;
    // the camera of the scene moved without building the scene again (a viewport's call per frame); `rebuilt` may be null
    pub fn pt_ctx_set_camera(ctx: *mut PtCtx, cam: *const PtCamera, rebuilt: *mut i32) -> i32;
    pub fn pt_ctx_camera_reach(ctx: *const PtCtx, lo: *mut f32, hi: *mut f32) -> i32;
    pub fn pt_ctx_reserve_camera_reach(ctx: *mut PtCtx, lo: *const f32, hi: *const f32, rebuilt: *mut i32) -> i32;
    pub fn pt_ctx_set_object(ctx: *mut PtCtx, index: u32, obj: *const PtObject, rebuilt: *mut i32) -> i32;
    pub fn pt_ctx_table_hashes(ctx: *mut PtCtx, out: *mut u64) -> i32;
    pub fn pt_scene_reach(
        cam: *const PtCamera,
        objs: *const PtObject,
        n_objs: u32,
        tris: *const PtTriangle,
        n_tris: u32,
        lo: *mut f32,
        hi: *mut f32,
    ) -> i32;
    pub fn pt_ctx_render(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        d_out_rgb: *mut c_void,
        hip_stream: *mut c_void,
        cancel: *const u8,
        cb: Option<PtProgressFn>,
        user: *mut c_void,
        stats: *mut PtStats,
    ) -> i32;
    pub fn pt_ctx_snapshot(ctx: *mut PtCtx, d_out_rgb: *mut c_void, spp_done: *mut u32) -> i32;
    // progressive accumulation: the frame up to cfg.spp samples IN TOTAL, from the samples the context holds for it (Stop
    // keeps them, Continue / "more samples" traces only the rest); checkpoints of the held samples on disk
    pub fn pt_ctx_accumulate(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        d_out_rgb: *mut c_void,
        hip_stream: *mut c_void,
        cancel: *const u8,
        cb: Option<PtProgressFn>,
        user: *mut c_void,
        stats: *mut PtStats,
    ) -> i32;
    pub fn pt_ctx_accum_info(ctx: *const PtCtx, cfg: *const PtConfig, spp_min: *mut u32, spp_max: *mut u32) -> i32;
    pub fn pt_ctx_accum_reset(ctx: *mut PtCtx) -> i32;
    pub fn pt_ctx_accum_save(ctx: *mut PtCtx, path: *const c_char) -> i32;
    pub fn pt_ctx_accum_load(ctx: *mut PtCtx, path: *const c_char) -> i32;
    // noise tracking: half of every pixel's samples is summed a second time, so that the frame's error can be estimated
    pub fn pt_ctx_accum_track_noise(ctx: *mut PtCtx, enabled: i32) -> i32;
    pub fn pt_ctx_accum_noise(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        d_error: *mut f32,
        out: *mut PtNoiseStats,
        hip_stream: *mut c_void,
    ) -> i32;
    // pt_ctx_accumulate until the estimate meets tgt; cfg.spp is the cap
    pub fn pt_ctx_accumulate_until(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        tgt: *const PtNoiseTarget,
        d_out_rgb: *mut c_void,
        hip_stream: *mut c_void,
        cancel: *const u8,
        cb: Option<PtProgressFn>,
        user: *mut c_void,
        stats: *mut PtStats,
        noise: *mut PtNoiseStats,
    ) -> i32;
    // the frame with every tile rendered to its own noise target; cfg.spp is the cap; d_spp (the count per pixel: a GUI's
    // heat map) and d_error may be null
    pub fn pt_ctx_render_adaptive(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        params: *const PtAdaptiveParams,
        d_out_rgb: *mut c_void,
        d_spp: *mut u32,
        d_error: *mut f32,
        hip_stream: *mut c_void,
        cancel: *const u8,
        cb: Option<PtProgressFn>,
        user: *mut c_void,
        stats: *mut PtStats,
        astats: *mut PtAdaptiveStats,
    ) -> i32;
    // pt_ctx_render_adaptive on the adaptive frame the context keeps: Stop keeps it, the same call continues it, a smaller
    // tile_error refines it, a higher cap extends it; checkpoints of it on disk
    pub fn pt_ctx_accumulate_adaptive(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        params: *const PtAdaptiveParams,
        d_out_rgb: *mut c_void,
        d_spp: *mut u32,
        d_error: *mut f32,
        hip_stream: *mut c_void,
        cancel: *const u8,
        cb: Option<PtProgressFn>,
        user: *mut c_void,
        stats: *mut PtStats,
        astats: *mut PtAdaptiveStats,
    ) -> i32;
    pub fn pt_ctx_adaptive_info(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        params: *const PtAdaptiveParams,
        out: *mut PtAdaptiveInfo,
    ) -> i32;
    // the preview between steps: allowed from pt_ctx_accumulate_adaptive's progress callback
    pub fn pt_ctx_adaptive_resolve(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        d_out_rgb: *mut c_void,
        d_spp: *mut u32,
        d_error: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_ctx_adaptive_reset(ctx: *mut PtCtx) -> i32;
    pub fn pt_ctx_adaptive_save(ctx: *mut PtCtx, path: *const c_char) -> i32;
    pub fn pt_ctx_adaptive_load(ctx: *mut PtCtx, path: *const c_char) -> i32;
    // first-hit AOVs of the frame cfg describes (device buffers, any may be null): mean albedo and ray-facing normal over the
    // first cfg.spp samples, sample 0's depth and object id - a denoiser's guides, a pick map
    pub fn pt_ctx_render_aov(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        d_albedo: *mut f32,
        d_normal: *mut f32,
        d_depth: *mut f32,
        d_object_id: *mut i32,
        hip_stream: *mut c_void,
    ) -> i32;
    // the same with parameters (null = the plain call) and sample 0's chain length per pixel: with PT_AOV_THROUGH_DELTA the
    // guides are those of the first surface behind the mirrors and the glass - for the filters, not for a pick map
    pub fn pt_aov_defaults(out: *mut PtAovParams) -> i32;
    pub fn pt_ctx_render_aov_ex(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        params: *const PtAovParams,
        d_albedo: *mut f32,
        d_normal: *mut f32,
        d_depth: *mut f32,
        d_object_id: *mut i32,
        d_chain: *mut u32,
        hip_stream: *mut c_void,
    ) -> i32;
    // edge-avoiding a-trous filter over a whole frame in device memory, guided by pt_ctx_render_aov's buffers (each guide may
    // be null; d_out may be d_color); params null = defaults
    pub fn pt_denoise_defaults(out: *mut PtDenoiseParams) -> i32;
    pub fn pt_ctx_denoise(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtDenoiseParams,
        d_color: *const f32,
        d_albedo: *const f32,
        d_normal: *const f32,
        d_depth: *const f32,
        d_out: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    // the same filter with its colour weight taken from the frame's noise estimate (pt_ctx_accum_noise's or
    // pt_ctx_render_adaptive's d_error, one f32 per pixel) in place of one sigma_color; params null = defaults
    pub fn pt_denoise_var_defaults(out: *mut PtDenoiseVarParams) -> i32;
    pub fn pt_ctx_denoise_var(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtDenoiseVarParams,
        d_color: *const f32,
        d_error: *const f32,
        d_albedo: *const f32,
        d_normal: *const f32,
        d_depth: *const f32,
        d_out: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    // a float frame in device memory as gamma-corrected 8-bit pixels at the size asked for, in the canvas's order (the
    // reference's gamma_correction per pixel and redraw, src/views/render_tab.rs:278-296, done once on the device)
    pub fn pt_ctx_present(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtPresentParams,
        d_rgb: *const f32,
        d_out: *mut u8,
        hip_stream: *mut c_void,
    ) -> i32;
    // last frame's colour carried into this frame's pixels through the depth and object-id guides, blended by history length:
    // what lets the viewport tab (src/views/viewport_tab.rs) keep its samples while the camera orbits
    pub fn pt_reproject_defaults(out: *mut PtReprojectParams) -> i32;
    pub fn pt_ctx_reproject(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtReprojectParams,
        cam: *const PtCamera,
        d_color: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        d_normal: *const f32,
        hist_cam: *const PtCamera,
        d_hist_color: *const f32,
        d_hist_len: *const f32,
        d_hist_depth: *const f32,
        d_hist_object_id: *const i32,
        d_hist_normal: *const f32,
        d_out_color: *mut f32,
        d_out_len: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    // the same with the temporal moments of (r + g) + b carried along and a per-pixel error map out of them, in the units
    // pt_ctx_denoise_var reads: the viewport's loop is reproject_var -> denoise_var -> present
    pub fn pt_reproject_var_defaults(out: *mut PtReprojectVarParams) -> i32;
    pub fn pt_ctx_reproject_var(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtReprojectVarParams,
        cam: *const PtCamera,
        d_color: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        d_normal: *const f32,
        hist_cam: *const PtCamera,
        d_hist_color: *const f32,
        d_hist_len: *const f32,
        d_hist_moments: *const f32,
        d_hist_depth: *const f32,
        d_hist_object_id: *const i32,
        d_hist_normal: *const f32,
        d_out_color: *mut f32,
        d_out_len: *mut f32,
        d_out_moments: *mut f32,
        d_error: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    // the two calls with a per-object motion table (a HOST array, copied by the call): history carried on objects that
    // pt_ctx_set_object moved; motion null, n_motion 0 or all records IDENTITY = the plain calls
    pub fn pt_object_motion_between(now: *const PtObject, before: *const PtObject, out: *mut PtObjectMotion) -> i32;
    pub fn pt_ctx_reproject_moved(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtReprojectParams,
        cam: *const PtCamera,
        d_color: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        d_normal: *const f32,
        hist_cam: *const PtCamera,
        d_hist_color: *const f32,
        d_hist_len: *const f32,
        d_hist_depth: *const f32,
        d_hist_object_id: *const i32,
        d_hist_normal: *const f32,
        d_out_color: *mut f32,
        d_out_len: *mut f32,
        motion: *const PtObjectMotion,
        n_motion: u32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_ctx_reproject_var_moved(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtReprojectVarParams,
        cam: *const PtCamera,
        d_color: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        d_normal: *const f32,
        hist_cam: *const PtCamera,
        d_hist_color: *const f32,
        d_hist_len: *const f32,
        d_hist_moments: *const f32,
        d_hist_depth: *const f32,
        d_hist_object_id: *const i32,
        d_hist_normal: *const f32,
        d_out_color: *mut f32,
        d_out_len: *mut f32,
        d_out_moments: *mut f32,
        d_error: *mut f32,
        motion: *const PtObjectMotion,
        n_motion: u32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_reproject_project_moved_host(
        cam: *const PtCamera,
        hist_cam: *const PtCamera,
        width: u32,
        height: u32,
        idx: u32,
        depth: f32,
        rec: *const PtObjectMotion,
        px: *mut f32,
        pr: *mut f32,
        zexp: *mut f32,
    ) -> i32;
    pub fn pt_reproject_project_host(
        cam: *const PtCamera,
        hist_cam: *const PtCamera,
        width: u32,
        height: u32,
        idx: u32,
        depth: f32,
        px: *mut f32,
        pr: *mut f32,
        zexp: *mut f32,
    ) -> i32;
    // a colour frame traced at lo_width x lo_height filled in at width x height through the first-hit guides of both sizes: the
    // viewport traces a quarter of the paths while the camera moves ("pixel size" 2)
    pub fn pt_upsample_defaults(out: *mut PtUpsampleParams) -> i32;
    pub fn pt_ctx_upsample(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        lo_width: u32,
        lo_height: u32,
        params: *const PtUpsampleParams,
        d_lo_color: *const f32,
        d_lo_depth: *const f32,
        d_lo_object_id: *const i32,
        d_lo_normal: *const f32,
        d_lo_albedo: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        d_normal: *const f32,
        d_albedo: *const f32,
        d_out_color: *mut f32,
        d_out_weight: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_upsample_tap_host(size: u32, lo_size: u32, coord: u32, first: *mut i32, frac: *mut f32) -> i32;
    // the pixels a pass could not serve (upsample weight 0, no history) as a byte mask, and those pixels of a frame traced again
    // and written into it: each one pt_ctx_render's pixel, bit for bit
    pub fn pt_ctx_select_pixels(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtSelectParams,
        d_weight: *const f32,
        d_len: *const f32,
        d_mask: *mut u8,
        n_selected: *mut u32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_ctx_render_masked(
        ctx: *mut PtCtx,
        cfg: *const PtConfig,
        d_mask: *const u8,
        d_rgb: *mut c_void,
        hip_stream: *mut c_void,
        cancel: *const u8,
        stats: *mut PtStats,
        n_pixels: *mut u32,
    ) -> i32;
    // pt_ctx_reproject_var_moved with a plane of per-pixel sample counts (what pt_ctx_render_adaptive writes as d_spp, or
    // pt_ctx_spp_plane makes of a mask): count 0 = not traced this frame, the history is carried through; d_spp null = the moved call
    pub fn pt_ctx_reproject_var_weighted(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtReprojectVarParams,
        cam: *const PtCamera,
        d_color: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        d_normal: *const f32,
        d_spp: *const u32,
        hist_cam: *const PtCamera,
        d_hist_color: *const f32,
        d_hist_len: *const f32,
        d_hist_moments: *const f32,
        d_hist_depth: *const f32,
        d_hist_object_id: *const i32,
        d_hist_normal: *const f32,
        d_out_color: *mut f32,
        d_out_len: *mut f32,
        d_out_moments: *mut f32,
        d_error: *mut f32,
        motion: *const PtObjectMotion,
        n_motion: u32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_ctx_spp_plane(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        base: u32,
        d_mask: *const u8,
        masked: u32,
        d_spp: *mut u32,
        hip_stream: *mut c_void,
    ) -> i32;
    // host arrays of n; `surfaces` is read by PT_SCATTER_GIVEN alone
    pub fn pt_ctx_scatter(
        ctx: *mut PtCtx,
        seed: u64,
        form: u32,
        items: *const PtScatterItem,
        surfaces: *const PtScatterSurface,
        n: u32,
        out: *mut PtScatterOut,
    ) -> i32;
    pub fn pt_write_pfm(path: *const c_char, data: *const f32, width: u32, height: u32, channels: u32) -> i32;
    pub fn pt_device_malloc(device: i32, bytes: usize, out: *mut *mut c_void) -> i32;
    pub fn pt_device_free(device: i32, p: *mut c_void) -> i32;
    pub fn pt_device_download(device: i32, dst_host: *mut c_void, src_device: *const c_void, bytes: usize) -> i32;
    pub fn pt_last_error() -> *const c_char;
    pub fn pt_device_count() -> i32;
    pub fn pt_image_hash(rgb: *const f32, n_floats: usize) -> u64;
}

// include/ptrace_overlay.h: pt_ctx_overlay has a header of its own, and so a block of its own here
extern "C" {
    // what the viewport tab (src/views/viewport_tab.rs) draws around the picture - backdrop, ground grid, the selected object's
    // outline - on the device frame, between the denoiser and pt_ctx_present; the context's own stream, no stream argument
    pub fn pt_overlay_defaults(cam: *const PtCamera, out: *mut PtOverlayParams) -> i32;
    pub fn pt_ctx_overlay(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtOverlayParams,
        cam: *const PtCamera,
        d_rgb: *const f32,
        d_object_id: *const i32,
        d_depth: *const f32,
        d_out: *mut f32,
    ) -> i32;
    pub fn pt_overlay_pixel_host(
        cam: *const PtCamera,
        width: u32,
        height: u32,
        params: *const PtOverlayParams,
        idx: u32,
        object_id: i32,
        depth: f32,
        selected: i32,
        outlined: i32,
        rgb_in: *const f32,
        rgb_out: *mut f32,
    ) -> i32;
}

// include/ptrace_solid.h: pt_ctx_solid has a header of its own too, and so a block of its own here
extern "C" {
    // what the viewport tab (src/views/viewport_tab.rs) shows while the scene is edited - the objects lit and solid - from one
    // sample of pt_ctx_render_aov's planes; `looks` is a host array; hip_stream as for pt_ctx_render
    pub fn pt_solid_defaults(out: *mut PtSolidParams) -> i32;
    pub fn pt_solid_look_of(obj: *const PtObject, out: *mut PtSolidLook) -> i32;
    pub fn pt_ctx_solid(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtSolidParams,
        cam: *const PtCamera,
        d_albedo: *const f32,
        d_normal: *const f32,
        d_depth: *const f32,
        d_object_id: *const i32,
        looks: *const PtSolidLook,
        n_looks: u32,
        d_out: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_solid_pixel_host(
        cam: *const PtCamera,
        width: u32,
        height: u32,
        params: *const PtSolidParams,
        idx: u32,
        object_id: i32,
        depth: f32,
        albedo: *const f32,
        normal: *const f32,
        look: *const PtSolidLook,
        rgb_out: *mut f32,
    ) -> i32;
}

// include/ptrace_tone.h: the tone stage has a header of its own as well, and so a block of its own here
extern "C" {
    // the frame pt_ctx_accumulate holds, resolved without the clamp to [0, 1]; hip_stream as for pt_ctx_render
    pub fn pt_ctx_accum_hdr(ctx: *mut PtCtx, cfg: *const PtConfig, d_out_rgb: *mut f32, hip_stream: *mut c_void) -> i32;
    // a luminance histogram of a float frame on the device, and the host's way from it to an exposure
    pub fn pt_ctx_meter(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtMeterParams,
        d_rgb: *const f32,
        d_object_id: *const i32,
        out: *mut PtMeterStats,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_meter_bin_host(luminance: f32, bin: *mut i32) -> i32;
    pub fn pt_meter_exposure_defaults(out: *mut PtMeterExposureParams) -> i32;
    pub fn pt_meter_exposure(stats: *const PtMeterStats, params: *const PtMeterExposureParams, exposure: *mut f32) -> i32;
    pub fn pt_meter_exposure_weights(stats: *const PtMeterStats, params: *const PtMeterExposureParams, kept: *mut f64) -> i32;
    pub fn pt_meter_adapt(current: f32, target: f32, dt: f32, tau: f32, next: *mut f32) -> i32;
    // exposure and a curve: a float frame to a display-linear float frame in [0, 1]; d_out may be d_rgb
    pub fn pt_tonemap_defaults(out: *mut PtTonemapParams) -> i32;
    pub fn pt_ctx_tonemap(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtTonemapParams,
        d_rgb: *const f32,
        d_out: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_tonemap_pixel_host(params: *const PtTonemapParams, rgb: *const f32, out: *mut f32) -> i32;
}

// include/ptrace_despike.h: the firefly stage has a header of its own as well, and so a block of its own here
extern "C" {
    pub fn pt_despike_defaults(out: *mut PtDespikeParams) -> i32;
    // fireflies of a float frame clipped in front of the denoiser; d_out may not be d_rgb; hip_stream as for pt_ctx_render
    pub fn pt_ctx_despike(
        ctx: *mut PtCtx,
        width: u32,
        height: u32,
        params: *const PtDespikeParams,
        d_rgb: *const f32,
        d_object_id: *const i32,
        d_out: *mut f32,
        d_mask: *mut u8,
        out: *mut PtDespikeStats,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn pt_despike_frame_host(
        width: u32,
        height: u32,
        params: *const PtDespikeParams,
        rgb: *const f32,
        object_id: *const i32,
        out_rgb: *mut f32,
        mask: *mut u8,
        out: *mut PtDespikeStats,
    ) -> i32;
}

fn v3(v: Vec3) -> [f32; 3] {
    [v.x, v.y, v.z]
}

/// SceneData -> the flat arrays of the C ABI.  Nothing is recomputed: every value is copied as the reference holds it
/// (`direction` un-normalised as stored, `bounding_sphere` as deserialised or as Mesh::new made it, :450-499), and the
/// triangles of all meshes are laid end to end in object order (object-local coordinates; the library adds `position`
/// exactly as Triangle::transformed does, :546-552).
pub fn flatten(scene: &SceneData) -> (PtCamera, Vec<PtObject>, Vec<PtTriangle>) {
    let cam = PtCamera {
        position: v3(scene.camera.position),
        direction: v3(scene.camera.direction()),
        focal_length: scene.camera.focal_length,
        sensor_width: scene.camera.sensor_width,
        aspect_ratio: scene.camera.aspect_ratio,
    };
    let mut objs: Vec<PtObject> = Vec::with_capacity(scene.objects.len());
    let mut tris: Vec<PtTriangle> = Vec::new();
    for o in scene.objects.iter() {
        let o: &SceneObjectData = o;
        let mut p = PtObject {
            position: v3(o.position),
            color: v3(o.material.color),
            emission: v3(o.material.emmission), // sic
            reflect_type: match o.material.reflect_type {
                ReflectType::Diffuse => 0,
                ReflectType::Specular => 1,
                ReflectType::Refract => 2,
            },
            ..Default::default()
        };
        match &o.type_ {
            SceneObject::Sphere { radius } => {
                p.kind = 0;
                p.radius = *radius;
            }
            SceneObject::Mesh { mesh, file: _ } => {
                p.kind = 1;
                p.tri_offset = tris.len() as u32;
                p.tri_count = mesh.triangles.len() as u32;
                p.bs_center = v3(mesh.bounding_sphere.position);
                p.bs_radius = mesh.bounding_sphere.radius;
                tris.extend(mesh.triangles.iter().map(|t| PtTriangle {
                    a: v3(t.a),
                    b: v3(t.b),
                    c: v3(t.c),
                }));
            }
        }
        objs.push(p);
    }
    (cam, objs, tris)
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(pt_last_error()) }.to_string_lossy().into_owned()
}

/// One side of a viewport's temporal history, all in device memory: a colour frame with its history length and the first-hit
/// guides it was rendered with (pt_ctx_render, pt_ctx_render_aov), and the camera it was seen from.  d_moments: the temporal
/// moments, 2 floats per pixel, which reproject_var_and_swap carries (reproject_and_swap does not read it: it may be null there).
pub struct ReprojectFrame {
    pub cam: PtCamera,
    pub d_color: *mut f32,
    pub d_len: *mut f32,
    pub d_moments: *mut f32,
    pub d_depth: *mut f32,
    pub d_object_id: *mut i32,
    pub d_normal: *mut f32,
}

/// `cur` holds the frame just rendered (colour, guides, camera); its colour and length become the blend with `hist`
/// (pt_ctx_reproject, in place: d_out_color = d_color), and the two swap roles: on return `hist` is the new history and `cur`
/// the set of buffers the next frame renders into.  Pointers change hands; nothing is copied.  `have_history`: false for the
/// first frame after a scene change.  `weight`: the samples per pixel `cur` was rendered with.
///
/// Dragging an object (the GUI's selection): pick once, then per mouse move replace the object and render - no pt_ctx_set_scene:
/// ```ignore
/// let mut obj = objects[picked];                        // the host's copy of the object pt_ctx_orbit_point named
/// obj.position = dragged_position();
/// let mut rebuilt = 0i32;
/// unsafe { pt_ctx_set_object(ctx, picked as u32, &obj, &mut rebuilt) };   // rebuilt != 0: it left the scene's reach (rare)
/// have_history = false;                                 // a frame in which an object moved passes no history on
/// ```
///
/// One turn of a viewport: the scene is set once (pt_ctx_set_scene), the camera moves per frame (pt_ctx_set_camera):
/// ```ignore
/// let mut rebuilt = 0i32;
/// cur.cam = camera_from_the_gui();
/// unsafe {
///     pt_ctx_set_camera(ctx, &cur.cam, &mut rebuilt);   // rebuilt != 0: the lens centre left the scene's reach (rare)
///     pt_ctx_render(ctx, &cfg, cur.d_color as *mut c_void, null_mut(), null(), None, null_mut(), &mut stats);
///     pt_ctx_render_aov(ctx, &cfg, d_albedo, cur.d_normal, cur.d_depth, cur.d_object_id, null_mut());
/// }
/// reproject_and_swap(ctx, (cfg.width, cfg.height), cfg.spp, &mut cur, &mut hist, have_history);
/// have_history = true;
/// ```
pub fn reproject_and_swap(
    ctx: *mut PtCtx,
    frame: (u32, u32),
    weight: u32,
    cur: &mut ReprojectFrame,
    hist: &mut ReprojectFrame,
    have_history: bool,
) -> i32 {
    let pp = PtReprojectParams { weight, ..Default::default() };
    let null = std::ptr::null::<f32>();
    let rc = unsafe {
        if have_history {
            pt_ctx_reproject(
                ctx, frame.0, frame.1, &pp, &cur.cam, cur.d_color, cur.d_depth, cur.d_object_id, cur.d_normal, &hist.cam,
                hist.d_color, hist.d_len, hist.d_depth, hist.d_object_id, hist.d_normal, cur.d_color, cur.d_len,
                std::ptr::null_mut(),
            )
        } else {
            pt_ctx_reproject(
                ctx, frame.0, frame.1, &pp, &cur.cam, cur.d_color, cur.d_depth, cur.d_object_id, cur.d_normal,
                std::ptr::null(), null, null, null, std::ptr::null(), null, cur.d_color, cur.d_len, std::ptr::null_mut(),
            )
        }
    };
    if rc == PT_OK {
        std::mem::swap(cur, hist);
    }
    rc
}

/// reproject_and_swap with the moments carried along and the frame's noise map out of them (pt_ctx_reproject_var): `cur`'s colour
/// is blended in place, its d_len and d_moments are written, and `d_error` - width * height floats, no part of either side -
/// receives the estimate pt_ctx_denoise_var reads.  Then the two sides swap roles as there: pointers change hands, nothing is
/// copied.
pub fn reproject_var_and_swap(
    ctx: *mut PtCtx,
    frame: (u32, u32),
    weight: u32,
    cur: &mut ReprojectFrame,
    hist: &mut ReprojectFrame,
    d_error: *mut f32,
    have_history: bool,
) -> i32 {
    let pp = PtReprojectVarParams { weight, ..Default::default() };
    let null = std::ptr::null::<f32>();
    let rc = unsafe {
        if have_history {
            pt_ctx_reproject_var(
                ctx, frame.0, frame.1, &pp, &cur.cam, cur.d_color, cur.d_depth, cur.d_object_id, cur.d_normal, &hist.cam,
                hist.d_color, hist.d_len, hist.d_moments, hist.d_depth, hist.d_object_id, hist.d_normal, cur.d_color, cur.d_len,
                cur.d_moments, d_error, std::ptr::null_mut(),
            )
        } else {
            pt_ctx_reproject_var(
                ctx, frame.0, frame.1, &pp, &cur.cam, cur.d_color, cur.d_depth, cur.d_object_id, cur.d_normal,
                std::ptr::null(), null, null, null, null, std::ptr::null(), null, cur.d_color, cur.d_len, cur.d_moments,
                d_error, std::ptr::null_mut(),
            )
        }
    };
    if rc == PT_OK {
        std::mem::swap(cur, hist);
    }
    rc
}

/// The first-hit guides of one frame in device memory (pt_ctx_render_aov), and for the low-resolution side the colour traced
/// at that size (pt_ctx_render); d_color is not read on the full-resolution side.  d_normal and d_albedo may be null.
pub struct UpsampleGuides {
    pub width: u32,
    pub height: u32,
    pub d_color: *const f32,
    pub d_depth: *const f32,
    pub d_object_id: *const i32,
    pub d_normal: *const f32,
    pub d_albedo: *const f32,
}

/// `lo` traced at a fraction of the resolution, filled in at `full`'s size through the guides of both (pt_ctx_upsample, the
/// library's defaults): `d_out_color` - full.width * full.height * 3 floats, no part of either side - is the frame that goes
/// on to reproject_var_and_swap with `weight` = the samples per pixel `lo` was traced with.
pub fn upsample_into(ctx: *mut PtCtx, lo: &UpsampleGuides, full: &UpsampleGuides, d_out_color: *mut f32) -> i32 {
    unsafe {
        pt_ctx_upsample(
            ctx, full.width, full.height, lo.width, lo.height, std::ptr::null(), lo.d_color, lo.d_depth, lo.d_object_id,
            lo.d_normal, lo.d_albedo, full.d_depth, full.d_object_id, full.d_normal, full.d_albedo, d_out_color,
            std::ptr::null_mut(), std::ptr::null_mut(),
        )
    }
}

/// The fallback pixels of an upsampled frame traced again at full size: `d_weight` is the plane pt_ctx_upsample wrote beside
/// `d_color` (upsample_into passes none: a host that retraces calls pt_ctx_upsample with one), `d_mask` full-size scratch of one
/// byte per pixel, `cfg` the full-size frame at the LOW-RESOLUTION samples per pixel, so that reproject_var_and_swap's uniform
/// `weight` stays true for every pixel.  Returns the library's code; `retraced` is the number of pixels replaced.
pub fn retrace_fallback(ctx: *mut PtCtx, cfg: &PtConfig, d_weight: *const f32, d_mask: *mut u8, d_color: *mut f32, retraced: &mut u32) -> i32 {
    let sel = PtSelectParams { weight_max: 0.0, len_max: 0.0, flags: 0 };
    unsafe {
        let rc = pt_ctx_select_pixels(
            ctx, cfg.width, cfg.height, &sel, d_weight, std::ptr::null(), d_mask, std::ptr::null_mut(), std::ptr::null_mut(),
        );
        if rc != PT_OK {
            return rc;
        }
        pt_ctx_render_masked(
            ctx, cfg, d_mask, d_color as *mut c_void, std::ptr::null_mut(), std::ptr::null(), std::ptr::null_mut(), retraced,
        )
    }
}

/// The window a preview is shown in: its size in pixels and the bytes the canvas draws, width * height * 4 (r, g, b, 255),
/// row-major from the top left - gamma-corrected and in the canvas's order already (pt_ctx_present).  The GUI uploads them
/// as a texture as they are; it neither walks the frame backwards nor calls gamma_correction (render_tab.rs:278-296).
pub struct PreviewWindow {
    pub width: u32,
    pub height: u32,
    pub rgba: Mutex<Vec<u8>>,
}

/// what the progress callback needs: the counter and the pixel buffer the reference's 500 ms thread reads (:960-976), and,
/// for a host that shows a window, the window and its device buffer
struct Preview<'a> {
    ctx: *mut PtCtx,
    d_snap: *mut c_void,
    d_rgba: *mut u8,
    frame: (u32, u32),
    window: Option<&'a PreviewWindow>,
    pixels: &'a Mutex<Vec<Vec3>>,
    processed_pixel_count: &'a AtomicUsize,
    grid_size: usize,
}

/// d_rgb (the frame, in device memory) at the window's size into the window's bytes: one device call, 4 B per window pixel
/// downloaded
fn present_to_window(ctx: *mut PtCtx, frame: (u32, u32), d_rgb: *const c_void, d_rgba: *mut u8, win: &PreviewWindow) -> i32 {
    let pp = PtPresentParams {
        out_width: win.width,
        out_height: win.height,
        ..Default::default() // exposure 1, RGBA8, the canvas's order
    };
    let rc = unsafe { pt_ctx_present(ctx, frame.0, frame.1, &pp, d_rgb as *const f32, d_rgba, std::ptr::null_mut()) };
    if rc != PT_OK {
        return rc;
    }
    let n = win.width as usize * win.height as usize * 4;
    let mut local = vec![0u8; n];
    let rc = unsafe { pt_device_download(0, local.as_mut_ptr() as *mut c_void, d_rgba as *const c_void, n) };
    if rc == PT_OK {
        *win.rgba.lock().unwrap() = local;
    }
    rc
}

/// Called by the library between passes, at most every 500 ms (pt_config.progress_ms = 0: the reference's RenderUpdate
/// cadence, :965-982), on the thread that called pt_ctx_render.  Drives the counter the progress thread reads (:966-968) and
/// puts the picture accumulated so far into `pixels`, so that the RenderUpdate that thread sends next (:969-972) carries a
/// partial image: pt_ctx_snapshot resolves the accumulators into device memory (every pixel over the samples it has so far
/// - the reference's partial image is a random subset of finished pixels, this one is the whole frame at partial spp),
/// With a window, pt_ctx_present then fits the snapshot to the window on the device and 4 B per WINDOW pixel come down;
/// without one, the floats do: one download, one copy under the mutex (held for a memcpy, as render_pixel_to_vec holds it for one store, :1013-1014).
extern "C" fn on_progress(user: *mut c_void, fraction: f32) {
    let p = unsafe { &*(user as *const Preview) };
    p.processed_pixel_count
        .store((fraction * p.grid_size as f32) as usize, Ordering::Relaxed);
    if fraction >= 1.0 {
        return; // the finished frame is copied by render_pixels_hip itself
    }
    let mut spp_done: u32 = 0;
    if unsafe { pt_ctx_snapshot(p.ctx, p.d_snap, &mut spp_done) } != PT_OK {
        return; // nothing accumulated yet
    }
    if let Some(win) = p.window {
        // same stream as the snapshot (the context's own): in stream order after it
        let _ = present_to_window(p.ctx, p.frame, p.d_snap as *const c_void, p.d_rgba, win);
        return;
    }
    let mut local = vec![Vec3::default(); p.grid_size];
    let bytes = p.grid_size * 3 * std::mem::size_of::<f32>();
    if unsafe { pt_device_download(0, local.as_mut_ptr() as *mut c_void, p.d_snap, bytes) } == PT_OK {
        p.pixels.lock().unwrap().copy_from_slice(&local);
    }
}

/// Replaces the parallel section :1017-1024: fills `pixels` (index (H-1-y)*W+x, :805-806; glam::Vec3 is
/// #[repr(C)] 3 x f32, so the Vec's memory IS the out_rgb layout) and keeps it filled with the partial picture while the
/// frame renders.  `cancel` is the flag render() already owns (`stop_render`, :943): one byte, read by the library between
/// passes (a few milliseconds apart; the reference polls it every 100 ms, :947-958).
pub fn render_pixels_hip(
    cfg: &RenderConfig,
    pixels: &Mutex<Vec<Vec3>>,
    cancel: &AtomicBool,
    processed_pixel_count: &AtomicUsize,
    seed: u64,
    window: Option<&PreviewWindow>,
) -> Result<PtStats, String> {
    let (cam, objs, tris) = flatten(&cfg.scene);
    let grid_size = cfg.resolution.width * cfg.resolution.height;
    let bytes = grid_size * 3 * std::mem::size_of::<f32>();
    let c = PtConfig {
        width: cfg.resolution.width as u32,
        height: cfg.resolution.height as u32,
        spp: cfg.samples_per_pixel as u32,
        seed,
        ..Default::default() // progress_ms = 0: a callback at most every 500 ms
    };
    let mut ctx: *mut PtCtx = std::ptr::null_mut();
    let (mut d_out, mut d_snap): (*mut c_void, *mut c_void) = (std::ptr::null_mut(), std::ptr::null_mut());
    let mut d_rgba: *mut c_void = std::ptr::null_mut();
    let mut st = PtStats::default();
    let rc = unsafe {
        let mut rc = pt_ctx_create(0, &mut ctx);
        if rc == PT_OK {
            rc = pt_ctx_set_scene(ctx, &cam, objs.as_ptr(), objs.len() as u32, tris.as_ptr(), tris.len() as u32);
        }
        if rc == PT_OK {
            rc = pt_device_malloc(0, bytes, &mut d_out);
        }
        if rc == PT_OK {
            rc = pt_device_malloc(0, bytes, &mut d_snap);
        }
        if let (true, Some(win)) = (rc == PT_OK, window) {
            rc = pt_device_malloc(0, win.width as usize * win.height as usize * 4, &mut d_rgba);
        }
        if rc == PT_OK {
            let preview = Preview {
                ctx,
                d_snap,
                d_rgba: d_rgba as *mut u8,
                frame: (c.width, c.height),
                window,
                pixels,
                processed_pixel_count,
                grid_size,
            };
            rc = pt_ctx_render(
                ctx,
                &c,
                d_out,
                std::ptr::null_mut(),
                cancel.as_ptr() as *const u8,
                Some(on_progress),
                &preview as *const Preview as *mut c_void,
                &mut st,
            );
        }
        if rc == PT_OK || rc == PT_CANCELLED {
            // the finished frame - or, cancelled, every pixel over the samples that were accumulated (the reference's
            // cancelled image holds its finished pixels and black elsewhere, :1003-1016)
            let mut local = vec![Vec3::default(); grid_size];
            let rc2 = pt_device_download(0, local.as_mut_ptr() as *mut c_void, d_out, bytes);
            if rc2 == PT_OK {
                pixels.lock().unwrap().copy_from_slice(&local);
            } else {
                rc = rc2;
            }
            // ... and the window shows it
            if let (true, Some(win)) = (rc2 == PT_OK, window) {
                let rc3 = present_to_window(ctx, (c.width, c.height), d_out, d_rgba as *mut u8, win);
                if rc3 != PT_OK {
                    rc = rc3;
                }
            }
        }
        rc
    };
    let msg = if rc == PT_OK || rc == PT_CANCELLED { String::new() } else { last_error() };
    unsafe {
        pt_device_free(0, d_rgba);
        pt_device_free(0, d_snap);
        pt_device_free(0, d_out);
        pt_ctx_destroy(ctx);
    }
    match rc {
        PT_OK | PT_CANCELLED => Ok(st),
        _ => Err(msg),
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The edit in render() (:1001-1024).  `pixels` is the Arc<Mutex<Vec<Vec3>>> render() already owns (:938) and the 500 ms
// thread clones under its lock (:969-972); render_pixels_hip only takes the lock for a memcpy.
//
//     let render_pixel_to_vec = ...;                       // unchanged (CPU path)
//     if hip::pt_device_count() > 0 && !MOCK_RANDOM {
//         let seed = rand::random::<u64>();                // the reference is OS-seeded too (:53)
//         match hip::render_pixels_hip(&render_config, &pixels, &stop_render, &processed_pixel_count, seed, None) {
//             Ok(stats) => println!("GPU: {} ray bounces in {:.1} ms", stats.ray_bounces, stats.ms_total),
//             Err(msg) => panic!("libptrace_hip: {msg}"),  // the reference unwraps its own errors (:1032,1042)
//         }
//     } else if MOCK_RANDOM { ... } else { ... rayon ... } // unchanged
//
// RenderUpdate { progress, image } (:969-972) then carries the growing picture every 500 ms exactly as with the CPU path:
// the progress thread is untouched, it finds `pixels` refreshed by on_progress.  A host that renders many frames of one
// scene (the GUI re-renders on every camera move) keeps the PtCtx and the two device buffers instead of creating them per
// frame: pt_ctx_set_scene only when the scene changed, pt_ctx_set_camera when only the camera moved.
