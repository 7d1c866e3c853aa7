// ptrace_cli.cpp — command-line host above the C ABI with the UX of the reference's (dead) CLI,
// src/cmd_render.rs:16-44 / .vscode/launch.json: `ptrace <spp> <res_y> <scene id or index>`.
// Width defaults to res_y*3/2 (src/render/mod.rs:872-879, src/main.rs:174-177); the scene is looked up as
// scenes/{id}.json (mod.rs:94) or by index into the sorted scenes/*.json listing (scenes.rs:10-41); the
// image goes to out/<timestamp>-scene-<id>-spp<N>-res<H>-.ppm plus a latest.ppm symlink (mod.rs:1031-1088).
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/ptrace.h"
#include "../../include/ptrace_overlay.h"
#include "../../include/ptrace_solid.h"
#include "../../include/ptrace_tone.h"
#include "../../include/ptrace_despike.h"

// --aov-chain [K]: the guides every pass of this program reads come from pt_ctx_render_aov_ex with PT_AOV_THROUGH_DELTA
static bool g_aov_chain = false;
static pt_aov_params g_aov = {0u, 0u};

// the guides of one frame: the plain call, byte for byte what it always wrote - or, with --aov-chain, the chain call
static int render_guides(pt_ctx *ctx, const pt_config *cfg, float *d_albedo, float *d_normal, float *d_depth, int32_t *d_id,
                         uint32_t *d_chain = nullptr) {
    if (!g_aov_chain) return pt_ctx_render_aov(ctx, cfg, d_albedo, d_normal, d_depth, d_id, nullptr);
    return pt_ctx_render_aov_ex(ctx, cfg, &g_aov, d_albedo, d_normal, d_depth, d_id, d_chain, nullptr);
}

// --select / --outline-radius / --sky / --grid: the editing cues drawn on the frame a --preview shows (pt_ctx_overlay)
struct OverlayOpts {
    bool on = false;
    uint32_t flags = 0, radius = 0;  // radius 0: the library's default
    std::vector<int32_t> selected;
};
static OverlayOpts g_overlay;

// pt_overlay_defaults for the frame's camera with what the command line names on top, applied in place
static int draw_overlay(pt_ctx *ctx, uint32_t w, uint32_t h, const pt_camera *cam, float *d_rgb, const int32_t *d_id, const float *d_depth) {
    pt_overlay_params op;
    int rc = pt_overlay_defaults(cam, &op);
    if (rc) return rc;
    op.flags = g_overlay.flags;
    op.n_selected = (uint32_t)g_overlay.selected.size();
    for (size_t i = 0; i < g_overlay.selected.size(); ++i) op.selected[i] = g_overlay.selected[i];
    if (g_overlay.radius) op.radius = g_overlay.radius;
    return pt_ctx_overlay(ctx, w, h, &op, cam, d_rgb, d_id, d_depth, d_rgb);
}

// --solid [N]: the frame a --preview shows is not the traced one but pt_ctx_solid of an N-sample pt_ctx_render_aov (0: off)
static uint32_t g_solid = 0;

// The guides at g_solid samples into the four planes given, then the lit solid view of them into d_out: the looks from the scene's
// objects, a headlight, mirrors showing the sky - in --sky's two colours (pt_overlay_defaults') when --sky is given
static int draw_solid(pt_ctx *ctx, const pt_config *frame, const pt_camera *cam, const pt_object *objs, uint32_t n_objs, float *d_albedo,
                      float *d_normal, float *d_depth, int32_t *d_id, float *d_out) {
    pt_config guides = *frame;
    guides.spp = g_solid;
    int rc = pt_ctx_render_aov(ctx, &guides, d_albedo, d_normal, d_depth, d_id, nullptr);
    std::vector<pt_solid_look> looks(n_objs);
    for (uint32_t i = 0; i < n_objs && !rc; ++i) rc = pt_solid_look_of(&objs[i], &looks[i]);
    pt_solid_params sp;
    if (!rc) rc = pt_solid_defaults(&sp);
    if (rc) return rc;
    sp.flags = PT_SOLID_HEADLIGHT | PT_SOLID_REFLECT_SKY;
    if (g_overlay.flags & PT_OVERLAY_SKY) {
        pt_overlay_params op;
        rc = pt_overlay_defaults(cam, &op);
        if (rc) return rc;
        memcpy(sp.sky_top, op.sky_top, sizeof sp.sky_top);
        memcpy(sp.sky_bottom, op.sky_bottom, sizeof sp.sky_bottom);
    }
    return pt_ctx_solid(ctx, frame->width, frame->height, &sp, cam, d_albedo, d_normal, d_depth, d_id, looks.data(), n_objs, d_out, nullptr);
}

// --hdr / --tonemap / --auto-exposure: the tone stage (ptrace_tone.h) between the frame and the cues of a --preview.  Any of them
// turns the frame's render into pt_ctx_accumulate + pt_ctx_accum_hdr: the frame that follows is the radiance, not clamped.
struct ToneOptions {
    std::string hdr;                 // --hdr FILE.pfm: the unclamped frame
    bool curve_on = false;           // --tonemap was given
    uint32_t curve = PT_TONE_ACES;
    bool luma = false;               // --tone-luma
    float white = 4.0f;              // --white W
    bool auto_on = false;            // --auto-exposure [KEY]
    float key = 0.0f;                // 0: pt_meter_exposure_defaults'
    bool despike_on = false;         // --despike [T]
    float despike_t = 0.0f;          // 0: pt_despike_defaults'
    bool any() const { return !hdr.empty() || curve_on || auto_on || despike_on; }
};
static ToneOptions g_tone;
// --orbit adapts the metered exposure over a fixed frame interval (the files do not depend on the machine's speed)
static const float kOrbitFrameSeconds = 1.0f / 30.0f, kAdaptSeconds = 0.5f;

// The frame cfg names, rendered through the held sums and resolved without the clamp into d_out (fresh: the held frame is dropped first)
static int render_hdr(pt_ctx *ctx, const pt_config *cfg, float *d_out, bool fresh, pt_progress_fn cb, pt_stats *st) {
    int rc = fresh ? pt_ctx_accum_reset(ctx) : PT_OK;
    if (!rc) rc = pt_ctx_accumulate(ctx, cfg, d_out, nullptr, nullptr, cb, nullptr, st);
    if (!rc) rc = pt_ctx_accum_hdr(ctx, cfg, d_out, nullptr);
    return rc;
}

// --despike [T]: pt_ctx_despike at its defaults (T: the threshold) from the radiance in d_rgb into d_out, in front of every filter
// and of the meter.  Without PT_DESPIKE_SAME_OBJECT, also under --orbit where the ids are at hand: the defaults are the study's
// choice (profiles/despike_study.json), and with the flag that setting is the grid's worst.  The line on stderr
// is printed at once, or with later == true by despike_report() - the single frame's, once the progress line has been closed.
static pt_despike_stats g_despike_stats;
static bool g_despike_pending = false;
static void despike_report() {
    fprintf(stderr, "despike: %llu spikes, %llu non-finite of %llu pixels\n", (unsigned long long)g_despike_stats.spikes,
            (unsigned long long)g_despike_stats.nonfinite, (unsigned long long)g_despike_stats.pixels);
    g_despike_pending = false;
}
static int despike_frame(pt_ctx *ctx, uint32_t w, uint32_t h, const float *d_rgb, float *d_out, bool later) {
    pt_despike_params dp;
    pt_despike_stats &ds = g_despike_stats;
    int rc = pt_despike_defaults(&dp);
    if (rc) return rc;
    if (g_tone.despike_t > 0.0f) dp.threshold = g_tone.despike_t;
    rc = pt_ctx_despike(ctx, w, h, &dp, d_rgb, nullptr, d_out, nullptr, &ds, nullptr);
    g_despike_pending = !rc && later;
    if (!rc && !later) despike_report();
    return rc;
}

// meter -> pt_meter_exposure (-> pt_meter_adapt from *adapted, which it updates; NULL or 0: no adaptation) -> pt_ctx_tonemap in
// place.  d_id: the ids of the frame when misses are to be skipped, else NULL.  `exposure`: --exposure's (0: none given); what
// pt_ctx_present still has to apply comes back in *present_exposure (0 once a curve has applied it).
static int tone_frame(pt_ctx *ctx, uint32_t w, uint32_t h, float *d_rgb, const int32_t *d_id, float exposure, float *adapted,
                      float *present_exposure) {
    float e = exposure > 0.0f ? exposure : 1.0f;
    int rc = PT_OK;
    if (g_tone.auto_on) {
        pt_meter_params mp;
        memset(&mp, 0, sizeof mp);
        mp.flags = d_id ? PT_METER_SKIP_MISSES : 0u;
        pt_meter_stats ms;
        pt_meter_exposure_params ep;
        rc = pt_ctx_meter(ctx, w, h, &mp, d_rgb, d_id, &ms, nullptr);
        if (!rc) rc = pt_meter_exposure_defaults(&ep);
        if (!rc && g_tone.key > 0.0f) ep.key = g_tone.key;
        if (!rc) rc = pt_meter_exposure(&ms, &ep, &e);
        if (!rc && adapted) {
            if (*adapted > 0.0f) rc = pt_meter_adapt(*adapted, e, kOrbitFrameSeconds, kAdaptSeconds, &e);
            *adapted = e;
        }
        if (rc) return rc;
    }
    *present_exposure = g_tone.auto_on ? e : exposure;
    if (g_tone.curve_on) {
        const pt_tonemap_params tp = {g_tone.curve, g_tone.luma ? PT_TONE_LUMA : 0u, e, g_tone.white};
        rc = pt_ctx_tonemap(ctx, w, h, &tp, d_rgb, d_rgb, nullptr);
        *present_exposure = 0.0f;
    }
    return rc;
}

// --hdr: the device frame as it stands, through pt_write_pfm
static int write_hdr(int dev, const float *d_rgb, uint32_t w, uint32_t h, const std::string &path) {
    std::vector<float> img((size_t)w * h * 3);
    int rc = pt_device_download(dev, img.data(), d_rgb, img.size() * sizeof(float));
    if (!rc) rc = pt_write_pfm(path.c_str(), img.data(), w, h, 3);
    if (rc)
        fprintf(stderr, "cannot write %s (%d): %s\n", path.c_str(), rc, pt_last_error());
    else
        printf("wrote %s\n", path.c_str());
    return rc;
}

static void usage() {
    fprintf(stderr,
            "usage: ptrace <samplesPerPixel> <y-resolution> <scene id|index> [--width W] [--backend wavefront|megakernel]\n"
            "              [--seed S] [--gpus N] [--root DIR] [--out DIR] [--no-ppm] [--checkpoint FILE] [--aov N]\n"
            "              [--aov-chain [K]]\n"
            "              [--denoise [N]] [--noise-target X [--noise-map FILE.pfm]]\n"
            "              [--adaptive X [--tile N] [--spp-map FILE.pfm] [--error-map FILE.pfm] [--adaptive-checkpoint FILE]]\n"
            "              [--denoise-var [N]] [--preview FILE.ppm [--preview-size WxH] [--exposure E]]\n"
            "              [--select I[,J...]] [--outline-radius R] [--sky] [--grid] [--solid [N]]\n"
            "              [--hdr FILE.pfm] [--tonemap clamp|reinhard|aces [--tone-luma] [--white W]] [--auto-exposure [KEY]]\n"
            "              [--despike [T]]\n"
            "              [--trace-scale K [--retrace]]\n"
            "              [--orbit N [--orbit-step DEG] [--move I:DX,DY,DZ [--move-history [F]]] [--boost K]]\n"
            "  --checkpoint FILE: continue from the samples FILE holds (if it exists), render up to <samplesPerPixel> in all and\n"
            "                     save them to FILE; one GPU only; the seed defaults to 0 instead of the clock, so that the same\n"
            "                     command continues the same frame\n"
            "  --aov N: after the frame, first-hit AOVs over its first N samples on one GPU, written next to the image as\n"
            "           PFM files: ...-beauty.pfm (the linear frame), -albedo, -normal, -depth (+inf on a miss) and -id (the\n"
            "           object index as a float, -1 on a miss)\n"
            "  --aov-chain [K]: guides THROUGH mirror and glass surfaces (pt_ctx_render_aov_ex, PT_AOV_THROUGH_DELTA, at most K = 1..16\n"
            "           steps, default 8): --aov then also writes ...-chain.pfm (sample 0's number of steps), its -depth is the\n"
            "           path's whole length and its -id the reflected object's; --denoise, --denoise-var, --trace-scale and --orbit\n"
            "           take their guides from that call\n"
            "  --denoise [N]: after the frame, denoise it on the GPU (pt_ctx_denoise, default parameters) with first-hit guides over\n"
            "           its first N samples (default 16), written next to the image as ...-denoised.ppm and ...-denoised.pfm; one\n"
            "           GPU only\n"
            "  --noise-target X: <samplesPerPixel> becomes a cap: render until the frame's mean estimated error (pt_ctx_accum_noise)\n"
            "           is at most X, doubling the samples from 16; prints the samples reached and the error; one GPU only;\n"
            "           with --checkpoint the file keeps the half buffers too (format version 2)\n"
            "  --noise-map FILE.pfm: with --noise-target, the per-pixel estimate e(p) of the final frame as a 1-channel PFM\n"
            "  --adaptive X: <samplesPerPixel> becomes a cap: every tile (--tile N: 4, 8, 16 or 32 pixels square, default 8) is\n"
            "           rendered until its mean estimated error is at most X (pt_ctx_render_adaptive); one GPU; not with\n"
            "           --checkpoint or --noise-target\n"
            "  --adaptive-checkpoint FILE: with --adaptive, continue the adaptive frame FILE holds (if it exists) to this X and\n"
            "           this cap - only tiles still above X take samples - and save FILE again (pt_ctx_accumulate_adaptive);\n"
            "           the seed defaults to 0 then\n"
            "  --spp-map FILE.pfm: with --adaptive, the samples every pixel got as a 1-channel PFM\n"
            "  --error-map FILE.pfm: with --adaptive, the estimate e(p) every pixel ended with (+inf: none) as a 1-channel PFM\n"
            "  --denoise-var [N]: with --noise-target or --adaptive: after the frame, denoise it on the GPU as far as its own noise\n"
            "           estimate says (pt_ctx_denoise_var, default parameters), guides and files as for --denoise; one GPU only;\n"
            "           not with --denoise\n"
            "  --preview FILE.ppm: after the frame (after --denoise / --denoise-var: of the denoised frame), turn it into 8-bit display\n"
            "           pixels on the GPU (pt_ctx_present, RGB8) and write them as a binary PPM; --preview-size WxH fits the frame to\n"
            "           that size by area averaging (default: the frame's own), --exposure E scales it first (default 1); one GPU\n"
            "           only\n"
            "  --select I[,J...], --outline-radius R, --sky, --grid: with --preview (the single frame or every frame of --orbit): draw\n"
            "           the editing cues on the frame before it is presented (pt_ctx_overlay, after the denoisers): an outline of R\n"
            "           frame pixels (1..8, default 2) around the objects listed (at most 16 indices), a sky gradient where the first\n"
            "           hit missed, the ground grid in y = 0 where no object hides it - pt_overlay_defaults for the frame's camera\n"
            "           otherwise; the single frame takes a 1-sample pt_ctx_render_aov for the object ids and depths\n"
            "  --hdr FILE.pfm, --tonemap CURVE, --auto-exposure [KEY]: with --preview (the single frame or every frame of --orbit): the\n"
            "           tone stage.  Any of them renders the frame through pt_ctx_accumulate + pt_ctx_accum_hdr: radiance, not clamped\n"
            "           to [0, 1].  --hdr writes that frame (under --orbit FILE-000.pfm, ...: the frame shown, before the curve).\n"
            "           --tonemap applies pt_ctx_tonemap's curve before the cues and pt_ctx_present (--tone-luma: on the luminance;\n"
            "           --white W: Reinhard's white point, default 4); --exposure E then scales the radiance before the curve.\n"
            "           --auto-exposure meters the frame (pt_ctx_meter, pt_meter_exposure, KEY default 0.18) in place of --exposure;\n"
            "           under --orbit the exposure follows through pt_meter_adapt at 30 frames per second, half a second's time\n"
            "           constant; with --sky or --solid the pixels that missed are not metered.  Not with --trace-scale, --adaptive\n"
            "           or --boost.\n"
            "  --despike [T]: with --preview (the single frame or every frame of --orbit): the radiance frame (as for --hdr) goes through\n"
            "           pt_ctx_despike at its defaults, T its threshold (default 2), before --hdr writes it and before --denoise,\n"
            "           --denoise-var, --auto-exposure and --tonemap see it: a pixel brighter than T times its third brightest\n"
            "           neighbour plus 0.25 is scaled down to that limit.  One line on stderr per frame:\n"
            "           despike: S spikes, N non-finite of P pixels.\n"
            "  --solid [N]: with --preview (the single frame or every frame of --orbit): the frame shown is not the traced one but the\n"
            "           objects lit and solid (pt_ctx_solid: ambient, diffuse and a highlight from a light at the lens, times the\n"
            "           albedo, plus the objects' emission; mirrors show the sky) from an N-sample pt_ctx_render_aov (default 1), the\n"
            "           cues of --select, --sky and --grid drawn on it; under --orbit a frame is pt_ctx_set_camera / pt_ctx_set_object,\n"
            "           pt_ctx_render_aov, pt_ctx_solid, pt_ctx_overlay, pt_ctx_present - no path is traced, nothing reprojected or\n"
            "           denoised; not with --aov-chain (its ids and depths are the reflected object's), --trace-scale, --retrace,\n"
            "           --boost or --move-history (nothing for them to act on)\n"
            "  --trace-scale K: K = 2..8: trace the paths at ceil(W/K) x ceil(H/K), the first-hit guides at both sizes, and fill the\n"
            "           frame in through the guides with albedo and normals (pt_ctx_upsample, default parameters); the image written\n"
            "           is the full-size frame; combines with --denoise and --preview; one GPU only; not with --checkpoint,\n"
            "           --noise-target or --adaptive\n"
            "  --retrace: with --trace-scale: the pixels for which no low-resolution tap passed the tests (pt_ctx_upsample's weight 0:\n"
            "           they took the bilinear fallback across an edge) are selected (pt_ctx_select_pixels) and traced at full size\n"
            "           with <samplesPerPixel> samples into the filled-in frame (pt_ctx_render_masked); prints their number\n"
            "  --orbit N: with --preview FILE.ppm: N frames of a viewport whose camera turns about the vertical axis through the\n"
            "           origin, frame k by k * DEG degrees (--orbit-step DEG, default 2) from the scene's own camera: per frame\n"
            "           pt_ctx_set_camera, pt_ctx_render at <samplesPerPixel>, the first-hit guides, pt_ctx_reproject_var against\n"
            "           frame k-1, pt_ctx_denoise_var (sigma_var 2), pt_ctx_overlay if asked for, and pt_ctx_present; the frames go to FILE-000.ppm, FILE-001.ppm,\n"
            "           ..., one line per frame to stderr (the camera update's milliseconds, whether it rebuilt the scene, the\n"
            "           frame's total); one GPU only; not with --trace-scale, --adaptive, --noise-target, --checkpoint, --denoise or\n"
            "           --denoise-var\n"
            "  --move I:DX,DY,DZ: with --orbit: in frame k object I stands at its position + k * (DX, DY, DZ), in binary32, set\n"
            "           through pt_ctx_set_object - no pt_ctx_set_scene per frame; a frame in which the object moved passes no\n"
            "           history to the reprojection; the frame's stderr line adds what the edit took and whether it rebuilt\n"
            "  --move-history [F]: with --move: a frame in which the object moved passes its history on after all, through\n"
            "           pt_ctx_reproject_var_moved with the object's record (pt_object_motion_between of the object in frame k and in\n"
            "           frame k-1); with F, max_history on such a frame is F frames' samples (F * <samplesPerPixel>), which bounds how\n"
            "           long the light the object changed elsewhere stays; without F it stays pt_reproject_var_defaults' 64 samples,\n"
            "           the pick of profiles/reproject_moved_cpu_study.json; not with --aov-chain\n"
            "  --boost K: with --orbit: the pixels that find no history (pt_ctx_reproject's length <= the frame's samples,\n"
            "           pt_ctx_select_pixels) are traced again at K * <samplesPerPixel> (pt_ctx_render_masked, K = 2..64), and the frame\n"
            "           enters the loop with its true per-pixel counts (pt_ctx_spp_plane, pt_ctx_reproject_var_weighted); prints\n"
            "           'Boosted N of W*H pixels' per frame\n");
}

static std::vector<std::string> scene_ids(const std::string &root) {
    std::vector<std::string> ids;
    DIR *d = opendir((root + "/scenes").c_str());
    if (!d) return ids;
    while (dirent *e = readdir(d)) {
        std::string n = e->d_name;
        if (n.size() > 5 && n.substr(n.size() - 5) == ".json") ids.push_back(n.substr(0, n.size() - 5));
    }
    closedir(d);
    std::sort(ids.begin(), ids.end());
    return ids;
}

static void progress(void *, float f) {
    fprintf(stderr, "\rRendering ... %5.1f%%", 100.0 * f);
    fflush(stderr);
}

constexpr int kCliExit = 1000;  // render_on_context: the message is out, exit 1

// a frame that stays on its GPU after the render (--denoise and --denoise-var filter it there)
struct DeviceFrame {
    int dev = 0;
    pt_ctx *ctx = nullptr;
    void *d_out = nullptr;
    bool want_error = false;  // --denoise-var: keep the frame's estimate e(p) too
    void *d_error = nullptr;
};

// --noise-target: render to a mean error of at most `target` (0: not asked for), cfg->spp at most; *spp_reached = the samples
// per pixel the frame ended with
struct NoiseRun {
    float target = 0.0f;
    std::string map;  // --noise-map
    uint32_t spp_reached = 0;
};

// --noise-map: e(p) of the held frame through pt_write_pfm, one channel
static int write_noise_map(int dev, pt_ctx *ctx, const pt_config *cfg, const std::string &path) {
    const size_t npix = (size_t)cfg->width * cfg->height;
    std::vector<float> err(npix);
    void *d_err = nullptr;
    pt_noise_stats ns;
    int rc = pt_device_malloc(dev, npix * sizeof(float), &d_err);
    if (!rc) rc = pt_ctx_accum_noise(ctx, cfg, (float *)d_err, &ns, nullptr);
    if (!rc) rc = pt_device_download(dev, err.data(), d_err, npix * sizeof(float));
    if (d_err) pt_device_free(dev, d_err);
    if (!rc) rc = pt_write_pfm(path.c_str(), err.data(), cfg->width, cfg->height, 1);
    if (rc)
        fprintf(stderr, "cannot write the noise map %s: %s\n", path.c_str(), pt_last_error());
    else
        printf("wrote %s\n", path.c_str());
    return rc;
}

// --adaptive: every tile to a mean error of at most `target` (negative: not asked for), cfg->spp at most
struct AdaptiveRun {
    float target = -1.0f;
    uint32_t tile = 0;
    std::string map;        // --spp-map
    std::string error_map;  // --error-map
    std::string file;       // --adaptive-checkpoint
};

// --adaptive on one context on one GPU: the frame into img, the counts and the estimate through pt_write_pfm (one channel).
// `keep` takes the context, the device frame and its estimate instead of their being freed.
static int render_adaptive(const pt_config *cfg, pt_scene *sc, const AdaptiveRun &run, std::vector<float> &img, pt_stats *st,
                           DeviceFrame *keep) {
    int dev = 0;
    if (const char *e = getenv("PT_DEVICE")) dev = atoi(e);
    uint32_t n_objs = 0, n_tris = 0;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    const size_t npix = (size_t)cfg->width * cfg->height;
    pt_ctx *ctx = nullptr;
    void *d_out = nullptr, *d_spp = nullptr, *d_err = nullptr;
    pt_adaptive_params par;
    memset(&par, 0, sizeof par);
    par.tile_error = run.target;
    par.tile = run.tile;
    pt_adaptive_stats as;
    int rc = pt_ctx_create(dev, &ctx);
    if (!rc) rc = pt_ctx_set_scene(ctx, pt_scene_camera(sc), objs, n_objs, tris, n_tris);
    if (!rc) rc = pt_device_malloc(dev, npix * 3 * sizeof(float), &d_out);
    if (!rc && !run.map.empty()) rc = pt_device_malloc(dev, npix * sizeof(uint32_t), &d_spp);
    if (!rc && (keep || !run.error_map.empty())) rc = pt_device_malloc(dev, npix * sizeof(float), &d_err);
    if (!rc && !run.file.empty() && access(run.file.c_str(), F_OK) == 0) {
        rc = pt_ctx_adaptive_load(ctx, run.file.c_str());
        pt_adaptive_info held;
        if (!rc) rc = pt_ctx_adaptive_info(ctx, cfg, &par, &held);
        if (rc) {
            fprintf(stderr, "cannot resume from %s (%d): %s\n", run.file.c_str(), rc, pt_last_error());
            pt_ctx_destroy(ctx);
            return kCliExit;
        }
        if (held.tiles == 0u) {
            fprintf(stderr, "checkpoint %s is of another frame (size, seed, tile or scene): not resumed\n", run.file.c_str());
            pt_ctx_destroy(ctx);
            return kCliExit;
        }
        printf("Resuming from %.1f samples per pixel on average, %u of %u tiles open\n", (double)held.samples / (double)npix,
               held.tiles_open, held.tiles);
        fflush(stdout);
    }
    if (!rc)
        rc = pt_ctx_accumulate_adaptive(ctx, cfg, &par, d_out, (uint32_t *)d_spp, (float *)d_err, nullptr, nullptr, progress, nullptr,
                                        st, &as);
    if (!rc && !run.file.empty()) {
        rc = pt_ctx_adaptive_save(ctx, run.file.c_str());
        if (rc) fprintf(stderr, "cannot save checkpoint %s: %s\n", run.file.c_str(), pt_last_error());
    }
    if (!rc) rc = pt_device_download(dev, img.data(), d_out, npix * 3 * sizeof(float));
    if (!rc) {
        printf("\nAdaptive, tile error %g: %u of %u tiles finished in %u levels, %.1f samples per pixel on average (cap %u), mean error %.6g\n",
               (double)run.target, as.tiles - as.tiles_open, as.tiles, as.levels, (double)as.samples / (double)npix, cfg->spp,
               as.mean_error);
        fflush(stdout);
    }
    if (!rc && d_spp) {
        std::vector<uint32_t> cnt(npix);
        std::vector<float> f(npix);
        rc = pt_device_download(dev, cnt.data(), d_spp, npix * sizeof(uint32_t));
        for (size_t i = 0; i < npix; ++i) f[i] = (float)cnt[i];
        if (!rc) rc = pt_write_pfm(run.map.c_str(), f.data(), cfg->width, cfg->height, 1);
        if (rc) {
            fprintf(stderr, "cannot write the sample-count map %s: %s\n", run.map.c_str(), pt_last_error());
            rc = kCliExit;
        } else {
            printf("wrote %s\n", run.map.c_str());
        }
    }
    if (!rc && !run.error_map.empty()) {
        std::vector<float> err(npix);
        rc = pt_device_download(dev, err.data(), d_err, npix * sizeof(float));
        if (!rc) rc = pt_write_pfm(run.error_map.c_str(), err.data(), cfg->width, cfg->height, 1);
        if (rc) {
            fprintf(stderr, "cannot write the error map %s: %s\n", run.error_map.c_str(), pt_last_error());
            rc = kCliExit;
        } else {
            printf("wrote %s\n", run.error_map.c_str());
        }
    }
    if (d_spp) pt_device_free(dev, d_spp);
    if (!rc && keep) {
        keep->dev = dev;
        keep->ctx = ctx;
        keep->d_out = d_out;
        keep->d_error = d_err;
        return rc;
    }
    if (d_err) pt_device_free(dev, d_err);
    if (d_out) pt_device_free(dev, d_out);
    if (ctx) pt_ctx_destroy(ctx);
    return rc;
}

// --checkpoint / --denoise / --noise-target: one context on one GPU.  With FILE the frame is accumulated from what FILE holds up
// to cfg->spp and FILE is saved again; without, it is rendered.  `keep` takes the context and the device frame instead of their
// being freed.
static int render_on_context(const pt_config *cfg, pt_scene *sc, const std::string &file, std::vector<float> &img, pt_stats *st,
                             DeviceFrame *keep, NoiseRun *noise) {
    int dev = 0;
    if (const char *e = getenv("PT_DEVICE")) dev = atoi(e);
    uint32_t n_objs = 0, n_tris = 0;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    pt_ctx *ctx = nullptr;
    int rc = pt_ctx_create(dev, &ctx);
    if (!rc) rc = pt_ctx_set_scene(ctx, pt_scene_camera(sc), objs, n_objs, tris, n_tris);
    if (!rc && noise->target > 0.0f) rc = pt_ctx_accum_track_noise(ctx, 1);
    if (!rc && !file.empty() && access(file.c_str(), F_OK) == 0) {
        rc = pt_ctx_accum_load(ctx, file.c_str());
        if (rc) {
            fprintf(stderr, "cannot resume from %s (%d): %s\n", file.c_str(), rc, pt_last_error());
            pt_ctx_destroy(ctx);
            return kCliExit;
        }
        uint32_t lo = 0, hi = 0;
        rc = pt_ctx_accum_info(ctx, cfg, &lo, &hi);
        if (!rc && hi == 0u) {
            fprintf(stderr, "checkpoint %s is of another frame (size, seed or scene): not resumed\n", file.c_str());
            pt_ctx_destroy(ctx);
            return kCliExit;
        }
        if (!rc && hi > cfg->spp) {
            fprintf(stderr, "checkpoint %s holds %u samples per pixel, more than the %u asked for\n", file.c_str(), hi, cfg->spp);
            pt_ctx_destroy(ctx);
            return kCliExit;
        }
        if (!rc) {
            if (lo == hi)
                printf("Resuming from %u samples per pixel\n", lo);
            else
                printf("Resuming from %u samples per pixel (up to %u)\n", lo, hi);
            fflush(stdout);
        }
    }
    void *d_out = nullptr;
    const size_t bytes = img.size() * sizeof(float);
    if (!rc) rc = pt_device_malloc(dev, bytes, &d_out);
    noise->spp_reached = cfg->spp;
    if (!rc && noise->target > 0.0f) {
        pt_noise_target tgt;
        memset(&tgt, 0, sizeof tgt);
        tgt.mean_error = noise->target;
        pt_noise_stats ns;
        rc = pt_ctx_accumulate_until(ctx, cfg, &tgt, d_out, nullptr, nullptr, progress, nullptr, st, &ns);
        if (!rc) {
            noise->spp_reached = ns.spp_max;
            printf("\nNoise target %g: reached %u samples per pixel, mean error %.6g%s\n", (double)noise->target, ns.spp_max,
                   ns.mean_error, ns.mean_error <= (double)noise->target ? "" : " (the cap: target not met)");
            fflush(stdout);
            if (!noise->map.empty() && write_noise_map(dev, ctx, cfg, noise->map)) rc = kCliExit;
        }
    } else if (!rc) {
        rc = file.empty() && !g_tone.any() ? pt_ctx_render(ctx, cfg, d_out, nullptr, nullptr, progress, nullptr, st)
                                           : pt_ctx_accumulate(ctx, cfg, d_out, nullptr, nullptr, progress, nullptr, st);
    }
    if (!rc) rc = pt_device_download(dev, img.data(), d_out, bytes);
    // the tone stage takes the radiance: the frame kept on the device is the held sums without the clamp (img keeps the clamped one)
    if (!rc && keep && g_tone.any() && !g_tone.despike_on) rc = pt_ctx_accum_hdr(ctx, cfg, (float *)d_out, nullptr);
    if (!rc && keep && g_tone.despike_on) {  // the pass gathers: the radiance goes to a frame of its own, the clipped one to d_out
        void *d_hdr = nullptr;
        rc = pt_device_malloc(dev, bytes, &d_hdr);
        if (!rc) rc = pt_ctx_accum_hdr(ctx, cfg, (float *)d_hdr, nullptr);
        if (!rc) rc = despike_frame(ctx, cfg->width, cfg->height, (const float *)d_hdr, (float *)d_out, true);
        if (d_hdr) pt_device_free(dev, d_hdr);
    }
    if (!rc && !file.empty()) {
        rc = pt_ctx_accum_save(ctx, file.c_str());
        if (rc) fprintf(stderr, "cannot save checkpoint %s: %s\n", file.c_str(), pt_last_error());
    }
    void *d_err = nullptr;
    if (!rc && keep && keep->want_error) {  // the held frame's e(p), where --noise-map's comes from
        pt_noise_stats ns;
        rc = pt_device_malloc(dev, (img.size() / 3) * sizeof(float), &d_err);
        if (!rc) rc = pt_ctx_accum_noise(ctx, cfg, (float *)d_err, &ns, nullptr);
    }
    if (!rc && keep) {
        keep->dev = dev;
        keep->ctx = ctx;
        keep->d_out = d_out;
        keep->d_error = d_err;
        return rc;
    }
    if (d_err) pt_device_free(dev, d_err);
    if (d_out) pt_device_free(dev, d_out);
    if (ctx) pt_ctx_destroy(ctx);
    return rc;
}

// --trace-scale K: one context on one GPU.  The paths at ceil(W/K) x ceil(H/K), the first-hit guides over the frame's samples at
// both sizes, then pt_ctx_upsample with albedo and normals at its defaults: the full-size frame into img.  `retrace`: the pixels
// the upsampler could not serve (weight 0) are then traced at full size, with the low-resolution frame's samples per pixel, into
// that frame.  `keep` takes the context and the device frame instead of their being freed.
static int render_scaled(const pt_config *cfg, pt_scene *sc, uint32_t scale, bool retrace, std::vector<float> &img, pt_stats *st,
                         DeviceFrame *keep) {
    int dev = 0;
    if (const char *e = getenv("PT_DEVICE")) dev = atoi(e);
    uint32_t n_objs = 0, n_tris = 0;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    pt_config lo = *cfg;
    lo.width = (cfg->width + scale - 1u) / scale;
    lo.height = (cfg->height + scale - 1u) / scale;
    const size_t npix = (size_t)cfg->width * cfg->height, nlo = (size_t)lo.width * lo.height;
    pt_ctx *ctx = nullptr;
    void *d_out = nullptr, *d_lo = nullptr, *d_full = nullptr, *d_sel = nullptr;  // d_sel: the weight plane, then the mask
    uint32_t retraced = 0;
    int rc = pt_ctx_create(dev, &ctx);
    if (!rc) rc = pt_ctx_set_scene(ctx, pt_scene_camera(sc), objs, n_objs, tris, n_tris);
    if (!rc) rc = pt_device_malloc(dev, npix * 3 * sizeof(float), &d_out);
    if (!rc) rc = pt_device_malloc(dev, nlo * 11 * sizeof(float), &d_lo);      // colour, albedo, normal, depth, id
    if (!rc) rc = pt_device_malloc(dev, npix * 8 * sizeof(float), &d_full);  // albedo, normal, depth, id
    if (!rc && retrace) rc = pt_device_malloc(dev, npix * (sizeof(float) + 1), &d_sel);
    if (!rc) {
        float *lo_color = (float *)d_lo, *lo_albedo = lo_color + nlo * 3, *lo_normal = lo_albedo + nlo * 3, *lo_depth = lo_normal + nlo * 3;
        int32_t *lo_id = (int32_t *)(lo_depth + nlo);
        float *albedo = (float *)d_full, *normal = albedo + npix * 3, *depth = normal + npix * 3;
        int32_t *id = (int32_t *)(depth + npix);
        rc = pt_ctx_render(ctx, &lo, lo_color, nullptr, nullptr, progress, nullptr, st);
        if (!rc) rc = render_guides(ctx, &lo, lo_albedo, lo_normal, lo_depth, lo_id);
        if (!rc) rc = render_guides(ctx, cfg, albedo, normal, depth, id);
        if (!rc)
            rc = pt_ctx_upsample(ctx, cfg->width, cfg->height, lo.width, lo.height, nullptr, lo_color, lo_depth, lo_id, lo_normal, lo_albedo,
                                 depth, id, normal, albedo, (float *)d_out, (float *)d_sel, nullptr);
        if (!rc && retrace) {
            const pt_select_params sel = {0.0f, 0.0f, 0u};
            uint8_t *mask = (uint8_t *)((float *)d_sel + npix);
            rc = pt_ctx_select_pixels(ctx, cfg->width, cfg->height, &sel, (const float *)d_sel, nullptr, mask, nullptr, nullptr);
            if (!rc) rc = pt_ctx_render_masked(ctx, cfg, mask, d_out, nullptr, nullptr, nullptr, &retraced);
        }
    }
    if (!rc) rc = pt_device_download(dev, img.data(), d_out, npix * 3 * sizeof(float));
    if (!rc) {
        printf("\nTraced at %ux%u (--trace-scale %u), filled in to %ux%u\n", lo.width, lo.height, scale, cfg->width, cfg->height);
        if (retrace) printf("Retraced %u of %zu pixels\n", retraced, npix);
        fflush(stdout);
    }
    if (d_lo) pt_device_free(dev, d_lo);
    if (d_full) pt_device_free(dev, d_full);
    if (d_sel) pt_device_free(dev, d_sel);
    if (!rc && keep) {
        keep->dev = dev;
        keep->ctx = ctx;
        keep->d_out = d_out;
        return rc;
    }
    if (d_out) pt_device_free(dev, d_out);
    if (ctx) pt_ctx_destroy(ctx);
    return rc;
}

// --denoise / --denoise-var: first-hit guides over the frame's first `spp` samples, pt_ctx_denoise - or, with the frame's
// estimate, pt_ctx_denoise_var - in place on the device frame, and the two files at `stem`
static int write_denoised(const pt_config *frame, uint32_t spp, const DeviceFrame &df, const std::string &stem, const char *scene_id) {
    pt_config cfg = *frame;
    cfg.spp = spp;
    const size_t npix = (size_t)cfg.width * cfg.height;
    std::vector<float> img(npix * 3);
    void *d_buf = nullptr;
    int rc = pt_device_malloc(df.dev, npix * 7 * sizeof(float), &d_buf);
    if (!rc) {
        float *d_albedo = (float *)d_buf, *d_normal = d_albedo + npix * 3, *d_depth = d_normal + npix * 3;
        rc = render_guides(df.ctx, &cfg, d_albedo, d_normal, d_depth, nullptr);
        if (!rc && df.d_error)
            rc = pt_ctx_denoise_var(df.ctx, cfg.width, cfg.height, nullptr, (const float *)df.d_out, (const float *)df.d_error,
                                    d_albedo, d_normal, d_depth, (float *)df.d_out, nullptr);
        else if (!rc)
            rc = pt_ctx_denoise(df.ctx, cfg.width, cfg.height, nullptr, (const float *)df.d_out, d_albedo, d_normal, d_depth,
                                (float *)df.d_out, nullptr);
        if (!rc) rc = pt_device_download(df.dev, img.data(), df.d_out, npix * 3 * sizeof(float));
    }
    if (d_buf) pt_device_free(df.dev, d_buf);
    if (rc) {
        fprintf(stderr, "denoising failed (%d): %s\n", rc, pt_last_error());
        return rc;
    }
    const std::string ppm = stem + "denoised.ppm", pfm = stem + "denoised.pfm";
    rc = pt_write_ppm(ppm.c_str(), img.data(), cfg.width, cfg.height, frame->spp, scene_id, 0);
    if (!rc) printf("wrote %s\n", ppm.c_str());
    if (!rc) rc = pt_write_pfm(pfm.c_str(), img.data(), cfg.width, cfg.height, 3);
    if (!rc) printf("wrote %s\n", pfm.c_str());
    if (rc) fprintf(stderr, "cannot write the denoised frame: %s\n", pt_last_error());
    return rc;
}

// --preview: the device frame as 8-bit display pixels (pt_ctx_present, RGB8) at ow x oh (0, 0: the frame's size), and the P6 file
static int write_preview(const pt_config *frame, const DeviceFrame &df, const std::string &path, uint32_t ow, uint32_t oh,
                         float exposure, pt_scene *sc) {
    const pt_camera *cam = pt_scene_camera(sc);
    pt_present_params pp;
    memset(&pp, 0, sizeof pp);
    pp.out_width = ow;
    pp.out_height = oh;
    pp.exposure = exposure;
    pp.format = PT_PRESENT_RGB8;
    if (!ow) ow = frame->width, oh = frame->height;
    std::vector<uint8_t> px((size_t)ow * oh * 3);
    void *d_px = nullptr, *d_guides = nullptr;
    int rc = pt_device_malloc(df.dev, px.size(), &d_px);
    if (!rc && g_solid) {
        // the lit solid view of the frame's first-hit guides takes the traced frame's place, then the cues in place
        const size_t npix = (size_t)frame->width * frame->height;
        uint32_t n_objs = 0;
        const pt_object *objs = pt_scene_objects(sc, &n_objs);
        rc = pt_device_malloc(df.dev, npix * 8 * sizeof(float), &d_guides);
        float *d_albedo = (float *)d_guides, *d_normal = d_albedo + npix * 3, *d_depth = d_normal + npix * 3;
        int32_t *d_id = (int32_t *)(d_depth + npix);
        if (!rc) rc = draw_solid(df.ctx, frame, cam, objs, n_objs, d_albedo, d_normal, d_depth, d_id, (float *)df.d_out);
        // (the meter leaves the background out: misses are skipped)
        if (!rc && (g_tone.curve_on || g_tone.auto_on))
            rc = tone_frame(df.ctx, frame->width, frame->height, (float *)df.d_out, d_id, exposure, nullptr, &pp.exposure);
        if (!rc && g_overlay.on) rc = draw_overlay(df.ctx, frame->width, frame->height, cam, (float *)df.d_out, d_id, d_depth);
    } else if (!rc && g_overlay.on) {
        // nothing has produced ids and depths for this frame: one sample of first-hit guides, then the cues in place
        const size_t npix = (size_t)frame->width * frame->height;
        pt_config one = *frame;
        one.spp = 1;
        rc = pt_device_malloc(df.dev, npix * 8, &d_guides);
        float *d_depth = (float *)d_guides;
        int32_t *d_id = (int32_t *)(d_depth + npix);
        if (!rc) rc = pt_ctx_render_aov(df.ctx, &one, nullptr, nullptr, d_depth, d_id, nullptr);
        // the curve before the cues; with --sky the meter leaves out the pixels the sky will fill
        if (!rc && (g_tone.curve_on || g_tone.auto_on))
            rc = tone_frame(df.ctx, frame->width, frame->height, (float *)df.d_out, (g_overlay.flags & PT_OVERLAY_SKY) ? d_id : nullptr, exposure,
                            nullptr, &pp.exposure);
        if (!rc) rc = draw_overlay(df.ctx, frame->width, frame->height, cam, (float *)df.d_out, d_id, d_depth);
    } else if (!rc && (g_tone.curve_on || g_tone.auto_on)) {
        rc = tone_frame(df.ctx, frame->width, frame->height, (float *)df.d_out, nullptr, exposure, nullptr, &pp.exposure);
    }
    if (d_guides) pt_device_free(df.dev, d_guides);
    if (!rc) rc = pt_ctx_present(df.ctx, frame->width, frame->height, &pp, (const float *)df.d_out, (uint8_t *)d_px, nullptr);
    if (!rc) rc = pt_device_download(df.dev, px.data(), d_px, px.size());
    if (d_px) pt_device_free(df.dev, d_px);
    if (!rc) rc = pt_write_ppm8(path.c_str(), px.data(), ow, oh);
    if (rc)
        fprintf(stderr, "cannot write the preview %s (%d): %s\n", path.c_str(), rc, pt_last_error());
    else
        printf("wrote %s\n", path.c_str());
    return rc;
}

// --aov: the frame's first-hit AOVs at `spp` samples (pt_ctx_render_aov) on one GPU, and the five PFM files at `stem`; with
// --aov-chain the chain call's, and a sixth file, the chain plane as floats
static int write_aovs(const pt_config *frame, uint32_t spp, pt_scene *sc, const std::vector<float> &img, const std::string &stem) {
    int dev = 0;
    if (const char *e = getenv("PT_DEVICE")) dev = atoi(e);
    uint32_t n_objs = 0, n_tris = 0;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    pt_config cfg = *frame;
    cfg.spp = spp;
    const size_t npix = (size_t)cfg.width * cfg.height;
    std::vector<float> albedo(npix * 3), normal(npix * 3), depth(npix), id_f(npix);
    std::vector<int32_t> id(npix);
    std::vector<uint32_t> chain(g_aov_chain ? npix : 0);
    std::vector<float> chain_f(chain.size());
    pt_ctx *ctx = nullptr;
    void *d_buf = nullptr;
    int rc = pt_ctx_create(dev, &ctx);
    if (!rc) rc = pt_ctx_set_scene(ctx, pt_scene_camera(sc), objs, n_objs, tris, n_tris);
    if (!rc) rc = pt_device_malloc(dev, npix * (g_aov_chain ? 10 : 9) * sizeof(float), &d_buf);
    if (!rc) {
        float *d_albedo = (float *)d_buf, *d_normal = d_albedo + npix * 3, *d_depth = d_normal + npix * 3;
        int32_t *d_id = (int32_t *)(d_depth + npix);
        uint32_t *d_chain = g_aov_chain ? (uint32_t *)(d_id + npix) : nullptr;
        rc = render_guides(ctx, &cfg, d_albedo, d_normal, d_depth, d_id, d_chain);
        if (!rc && d_chain) rc = pt_device_download(dev, chain.data(), d_chain, npix * sizeof(uint32_t));
        if (!rc) rc = pt_device_download(dev, albedo.data(), d_albedo, npix * 3 * sizeof(float));
        if (!rc) rc = pt_device_download(dev, normal.data(), d_normal, npix * 3 * sizeof(float));
        if (!rc) rc = pt_device_download(dev, depth.data(), d_depth, npix * sizeof(float));
        if (!rc) rc = pt_device_download(dev, id.data(), d_id, npix * sizeof(int32_t));
    }
    if (d_buf) pt_device_free(dev, d_buf);
    if (ctx) pt_ctx_destroy(ctx);
    if (rc) {
        fprintf(stderr, "AOVs failed (%d): %s\n", rc, pt_last_error());
        return rc;
    }
    for (size_t i = 0; i < npix; ++i) id_f[i] = (float)id[i];
    const struct {
        const char *name;
        const float *data;
        uint32_t channels;
    } files[] = {{"beauty", img.data(), 3}, {"albedo", albedo.data(), 3}, {"normal", normal.data(), 3}, {"depth", depth.data(), 1},
                 {"id", id_f.data(), 1}, {"chain", chain_f.data(), 1}};
    for (size_t i = 0; i < chain.size(); ++i) chain_f[i] = (float)chain[i];
    for (const auto &f : files) {
        if (!g_aov_chain && !strcmp(f.name, "chain")) continue;
        const std::string path = stem + f.name + ".pfm";
        rc = pt_write_pfm(path.c_str(), f.data, cfg.width, cfg.height, f.channels);
        if (rc) {
            fprintf(stderr, "cannot write %s: %s\n", path.c_str(), pt_last_error());
            return rc;
        }
        printf("wrote %s\n", path.c_str());
    }
    return 0;
}

// --orbit: the scene's camera turned by `degrees` about the vertical axis through the origin - binary64 arithmetic, rounded to
// binary32 once (always from camera 0, never from the frame before)
static pt_camera orbit_camera(const pt_camera &cam, double degrees) {
    const double a = degrees * (M_PI / 180.0), c = cos(a), s = sin(a);
    pt_camera o = cam;
    const float *in[2] = {cam.position, cam.direction};
    float *out[2] = {o.position, o.direction};
    for (int i = 0; i < 2; ++i) {
        const double x = in[i][0], z = in[i][2];
        out[i][0] = (float)(c * x + s * z);
        out[i][2] = (float)(-s * x + c * z);
    }
    return o;
}

// one side of the orbit loop's history: device planes of one frame
struct OrbitSide {
    float *color, *len, *moments, *depth, *normal;
    int32_t *id;
};

// --orbit N: the viewport loop of INTEGRATION.md on one context on one GPU, the camera moved with pt_ctx_set_camera
// --move I:DX,DY,DZ: object `index` stands at its position + k * d in frame k (index < 0: nothing moves)
// --move-history [F]: carry: a move frame keeps its history, capped at `history` frames' samples (0: the library's default)
struct OrbitMove {
    long index = -1;
    float d[3] = {0.0f, 0.0f, 0.0f};
    bool carry = false;
    float history = 0.0f;
};

// --boost K (0: off): the pixels without history traced again at K times the frame's samples, the frame blended by its true counts
static int render_orbit(const pt_config *cfg, pt_scene *sc, uint32_t frames, double step, const std::string &preview, uint32_t ow,
                        uint32_t oh, float exposure, const OrbitMove &mv, uint32_t boost) {
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    int dev = 0;
    if (const char *e = getenv("PT_DEVICE")) dev = atoi(e);
    uint32_t n_objs = 0, n_tris = 0;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    const pt_camera cam0 = *pt_scene_camera(sc);
    const uint32_t w = cfg->width, h = cfg->height;
    const size_t npix = (size_t)w * h;
    pt_present_params pp;
    memset(&pp, 0, sizeof pp);
    pp.out_width = ow;
    pp.out_height = oh;
    pp.exposure = exposure;
    pp.format = PT_PRESENT_RGB8;
    if (!ow) ow = w, oh = h;
    std::vector<uint8_t> px((size_t)ow * oh * 3);
    const std::string stem = preview.size() > 4 && preview.substr(preview.size() - 4) == ".ppm" ? preview.substr(0, preview.size() - 4) : preview;
    pt_ctx *ctx = nullptr;
    // two sides of 11 floats per pixel, then albedo (3), the error (1) and the frame shown (3)
    void *d_buf = nullptr, *d_px = nullptr;
    int rc = pt_ctx_create(dev, &ctx);
    if (!rc) rc = pt_ctx_set_scene(ctx, &cam0, objs, n_objs, tris, n_tris);
    if (!rc) rc = pt_device_malloc(dev, npix * 29 * sizeof(float), &d_buf);
    if (!rc) rc = pt_device_malloc(dev, px.size(), &d_px);
    // --boost: the plane of counts (4 B per pixel), then the mask (1)
    void *d_boost = nullptr;
    if (!rc && boost) rc = pt_device_malloc(dev, npix * 5, &d_boost);
    uint32_t *const d_spp = (uint32_t *)d_boost;
    uint8_t *const d_mask = d_boost ? (uint8_t *)d_boost + npix * 4 : nullptr;
    OrbitSide side[2];
    float *d_albedo = nullptr, *d_error = nullptr, *d_shown = nullptr;
    if (!rc) {
        float *f = (float *)d_buf;
        for (OrbitSide &s : side) {
            s.color = f, s.len = f + npix * 3, s.moments = f + npix * 4, s.depth = f + npix * 6, s.normal = f + npix * 7;
            s.id = (int32_t *)(f + npix * 10);
            f += npix * 11;
        }
        d_albedo = f, d_error = f + npix * 3, d_shown = f + npix * 4;
    }
    OrbitSide *cur = &side[0], *hist = &side[1];
    pt_camera hist_cam = cam0;
    float adapted = 0.0f;  // --auto-exposure: the exposure of the frame before (0: none yet)
    const bool tone = g_tone.curve_on || g_tone.auto_on;
    for (uint32_t k = 0; k < frames && !rc; ++k) {
        const pt_camera cam = orbit_camera(cam0, (double)k * step);
        // a frame in which an object moved passes no history on: the reprojection follows the camera, not the objects - unless
        // --move-history hands it the object's record
        const bool moves = mv.index >= 0 && k != 0u && (mv.d[0] != 0.0f || mv.d[1] != 0.0f || mv.d[2] != 0.0f);
        const bool carried = moves && mv.carry;
        const bool hh = k != 0u && (!moves || carried);
        int rebuilt = 0, edit_rebuilt = 0;
        pt_stats st;
        const clk::time_point t0 = clk::now();
        rc = pt_ctx_set_camera(ctx, &cam, &rebuilt);
        const clk::time_point t1 = clk::now();
        if (!rc && mv.index >= 0) {
            pt_object o = objs[mv.index];
            for (int a = 0; a < 3; ++a) o.position[a] = objs[mv.index].position[a] + (float)k * mv.d[a];
            rc = pt_ctx_set_object(ctx, (uint32_t)mv.index, &o, &edit_rebuilt);
        }
        const clk::time_point t1b = clk::now();
        if (g_solid) {
            // --solid: the guides, the lit solid view of them, the cues, the display pixels - no path is traced
            if (!rc) rc = draw_solid(ctx, cfg, &cam, objs, n_objs, d_albedo, cur->normal, cur->depth, cur->id, d_shown);
            if (!rc && tone) rc = tone_frame(ctx, w, h, d_shown, cur->id, exposure, &adapted, &pp.exposure);
            if (!rc && g_overlay.on) rc = draw_overlay(ctx, w, h, &cam, d_shown, cur->id, cur->depth);
            if (!rc) rc = pt_ctx_present(ctx, w, h, &pp, d_shown, (uint8_t *)d_px, nullptr);
            if (!rc) rc = pt_device_download(dev, px.data(), d_px, px.size());
            const clk::time_point t2 = clk::now();
            if (rc) break;
            char name[32];
            snprintf(name, sizeof name, "-%03u.ppm", k);
            const std::string path = stem + name;
            rc = pt_write_ppm8(path.c_str(), px.data(), ow, oh);
            if (rc) break;
            fprintf(stderr, "frame %u: pt_ctx_set_camera %.3f ms (%s), solid frame %.3f ms\n", k, ms(t0, t1), rebuilt ? "rebuilt" : "not rebuilt",
                    ms(t0, t2));
            printf("wrote %s\n", path.c_str());
            continue;
        }
        // with a tone option the frame is the radiance: the camera moved, so the held sums start over
        // (--despike: into d_shown, which nothing uses before the filter, and from there clipped into the frame)
        if (!rc)
            rc = g_tone.any() ? render_hdr(ctx, cfg, g_tone.despike_on ? d_shown : cur->color, true, nullptr, &st)
                              : pt_ctx_render(ctx, cfg, cur->color, nullptr, nullptr, nullptr, nullptr, &st);
        if (!rc) rc = render_guides(ctx, cfg, d_albedo, cur->normal, cur->depth, cur->id);
        if (!rc && g_tone.despike_on) rc = despike_frame(ctx, w, h, d_shown, cur->color, false);
        pt_reproject_var_params rp;
        memset(&rp, 0, sizeof rp);
        rp.weight = cfg->spp;
        std::vector<pt_object_motion> table;
        if (!rc && carried) {
            pt_object now = objs[mv.index], before = objs[mv.index];
            for (int a = 0; a < 3; ++a) {
                now.position[a] = objs[mv.index].position[a] + (float)k * mv.d[a];
                before.position[a] = objs[mv.index].position[a] + (float)(k - 1u) * mv.d[a];
            }
            table.assign(n_objs, pt_object_motion{{0.0f, 0.0f, 0.0f}, 1.0f});
            rc = pt_object_motion_between(&now, &before, &table[mv.index]);
            rp.max_history = mv.history * (float)cfg->spp;  // 0: the default
        }
        if (!rc && boost) {
            // the lengths of the plain blend (into the planes the filter fills later) say which pixels found no history; those
            // are traced again at boost * spp into the frame, and the frame is blended by the counts it then holds
            const pt_reproject_params lp = {rp.weight, rp.max_history, 0.0f, 0.0f, 0u};
            const pt_select_params sel = {0.0f, (float)cfg->spp, 0u};
            pt_config cfg_b = *cfg;
            cfg_b.spp = boost * cfg->spp;
            uint32_t boosted = 0;
            rc = pt_ctx_reproject_moved(ctx, w, h, &lp, &cam, cur->color, cur->depth, cur->id, cur->normal, hh ? &hist_cam : nullptr,
                                        hh ? hist->color : nullptr, hh ? hist->len : nullptr, hh ? hist->depth : nullptr,
                                        hh ? hist->id : nullptr, hh ? hist->normal : nullptr, d_shown, d_error,
                                        table.empty() ? nullptr : table.data(), (uint32_t)table.size(), nullptr);
            if (!rc) rc = pt_ctx_select_pixels(ctx, w, h, &sel, nullptr, d_error, d_mask, nullptr, nullptr);
            if (!rc) rc = pt_ctx_render_masked(ctx, &cfg_b, d_mask, cur->color, nullptr, nullptr, nullptr, &boosted);
            if (!rc) rc = pt_ctx_spp_plane(ctx, w, h, cfg->spp, d_mask, cfg_b.spp, d_spp, nullptr);
            if (!rc)
                rc = pt_ctx_reproject_var_weighted(ctx, w, h, &rp, &cam, cur->color, cur->depth, cur->id, cur->normal, d_spp,
                                                   hh ? &hist_cam : nullptr, hh ? hist->color : nullptr, hh ? hist->len : nullptr,
                                                   hh ? hist->moments : nullptr, hh ? hist->depth : nullptr, hh ? hist->id : nullptr,
                                                   hh ? hist->normal : nullptr, cur->color, cur->len, cur->moments, d_error,
                                                   table.empty() ? nullptr : table.data(), (uint32_t)table.size(), nullptr);
            if (!rc) printf("Boosted %u of %zu pixels\n", boosted, npix);
        } else if (!rc && carried) {
            rc = pt_ctx_reproject_var_moved(ctx, w, h, &rp, &cam, cur->color, cur->depth, cur->id, cur->normal, &hist_cam, hist->color,
                                            hist->len, hist->moments, hist->depth, hist->id, hist->normal, cur->color, cur->len,
                                            cur->moments, d_error, table.data(), n_objs, nullptr);
        } else if (!rc)
            rc = pt_ctx_reproject_var(ctx, w, h, &rp, &cam, cur->color, cur->depth, cur->id, cur->normal, hh ? &hist_cam : nullptr,
                                      hh ? hist->color : nullptr, hh ? hist->len : nullptr, hh ? hist->moments : nullptr,
                                      hh ? hist->depth : nullptr, hh ? hist->id : nullptr, hh ? hist->normal : nullptr, cur->color,
                                      cur->len, cur->moments, d_error, nullptr);
        pt_denoise_var_params dp;
        memset(&dp, 0, sizeof dp);
        dp.sigma_var = 2.0f;
        if (!rc) rc = pt_ctx_denoise_var(ctx, w, h, &dp, cur->color, d_error, d_albedo, cur->normal, cur->depth, d_shown, nullptr);
        if (!rc && !g_tone.hdr.empty()) {
            char hname[32];
            snprintf(hname, sizeof hname, "-%03u.pfm", k);
            const std::string &hp = g_tone.hdr;
            if (write_hdr(dev, d_shown, w, h, (hp.size() > 4 && hp.substr(hp.size() - 4) == ".pfm" ? hp.substr(0, hp.size() - 4) : hp) + hname)) rc = PT_ERR_IO;
        }
        if (!rc && tone)
            rc = tone_frame(ctx, w, h, d_shown, (g_overlay.flags & PT_OVERLAY_SKY) ? cur->id : nullptr, exposure, &adapted, &pp.exposure);
        if (!rc && g_overlay.on) rc = draw_overlay(ctx, w, h, &cam, d_shown, cur->id, cur->depth);
        if (!rc) rc = pt_ctx_present(ctx, w, h, &pp, d_shown, (uint8_t *)d_px, nullptr);
        if (!rc) rc = pt_device_download(dev, px.data(), d_px, px.size());
        const clk::time_point t2 = clk::now();
        if (rc) break;
        std::swap(cur, hist);
        hist_cam = cam;
        char name[32];
        snprintf(name, sizeof name, "-%03u.ppm", k);
        const std::string path = stem + name;
        rc = pt_write_ppm8(path.c_str(), px.data(), ow, oh);
        if (rc) break;
        if (mv.index >= 0)
            fprintf(stderr, "frame %u: pt_ctx_set_camera %.3f ms (%s), pt_ctx_set_object %.3f ms (%s), frame %.3f ms\n", k, ms(t0, t1),
                    rebuilt ? "rebuilt" : "not rebuilt", ms(t1, t1b), edit_rebuilt ? "rebuilt" : "not rebuilt", ms(t0, t2));
        else
            fprintf(stderr, "frame %u: pt_ctx_set_camera %.3f ms (%s), frame %.3f ms\n", k, ms(t0, t1), rebuilt ? "rebuilt" : "not rebuilt",
                    ms(t0, t2));
        printf("wrote %s\n", path.c_str());
    }
    if (rc) fprintf(stderr, "--orbit failed (%d): %s\n", rc, pt_last_error());
    if (d_boost) pt_device_free(dev, d_boost);
    if (d_px) pt_device_free(dev, d_px);
    if (d_buf) pt_device_free(dev, d_buf);
    if (ctx) pt_ctx_destroy(ctx);
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        usage();
        return 1;
    }
    const uint32_t spp = (uint32_t)strtoul(argv[1], nullptr, 10);
    const uint32_t res_y = (uint32_t)strtoul(argv[2], nullptr, 10);
    std::string scene_arg = argv[3], root = ".", out_dir = "out", backend = "wavefront";
    uint32_t width = res_y * 3 / 2;
    uint64_t seed = (uint64_t)time(nullptr);
    bool seed_given = false;
    std::string checkpoint;
    bool write_ppm = true;
    uint32_t gpus = 1, aov_spp = 0, denoise_spp = 0, denoise_var_spp = 0, trace_scale = 0;
    bool retrace = false;
    NoiseRun noise;
    AdaptiveRun adaptive;
    std::string preview;
    uint32_t preview_w = 0, preview_h = 0;
    float exposure = 0.0f;
    uint32_t orbit_frames = 0;
    double orbit_step = 2.0;
    bool orbit_step_given = false;
    OrbitMove orbit_move;
    uint32_t boost = 0;
    for (int i = 4; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--width") width = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--backend") backend = next();
        else if (a == "--seed") {
            seed = strtoull(next(), nullptr, 10);
            seed_given = true;
        }
        else if (a == "--checkpoint") {
            checkpoint = next();
            if (checkpoint.empty()) {
                usage();
                return 1;
            }
        }
        else if (a == "--gpus") gpus = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--root") root = next();
        else if (a == "--out") out_dir = next();
        else if (a == "--no-ppm") write_ppm = false;
        else if (a == "--preview") {
            preview = next();
            if (preview.empty()) {
                usage();
                return 1;
            }
        }
        else if (a == "--preview-size") {
            char x = 0, rest = 0;
            if (sscanf(next(), "%u%c%u%c", &preview_w, &x, &preview_h, &rest) != 3 || x != 'x' || !preview_w || !preview_h) {
                fprintf(stderr, "--preview-size needs WxH, both positive\n");
                return 1;
            }
        }
        else if (a == "--select") {
            const char *v = next();
            g_overlay.selected.clear();
            for (const char *q = v; *q;) {
                char *e = nullptr;
                const long id = strtol(q, &e, 10);
                if (e == q || id < 0 || id > INT32_MAX || (*e && *e != ',') || (*e == ',' && !e[1]) || g_overlay.selected.size() == PT_OVERLAY_MAX_SELECTED) {
                    g_overlay.selected.clear();
                    break;
                }
                g_overlay.selected.push_back((int32_t)id);
                q = *e ? e + 1 : e;
            }
            if (g_overlay.selected.empty()) {
                fprintf(stderr, "--select needs I[,J...]: 1 to 16 object indices, none negative\n");
                return 1;
            }
            g_overlay.on = true;
        }
        else if (a == "--outline-radius") {
            char *e = nullptr;
            const char *v = next();
            const unsigned long r = strtoul(v, &e, 10);
            if (e == v || *e || r < 1 || r > PT_OVERLAY_MAX_RADIUS) {
                fprintf(stderr, "--outline-radius needs R = 1..8 frame pixels\n");
                return 1;
            }
            g_overlay.radius = (uint32_t)r;
            g_overlay.on = true;
        }
        else if (a == "--sky") {
            g_overlay.flags |= PT_OVERLAY_SKY;
            g_overlay.on = true;
        }
        else if (a == "--grid") {
            g_overlay.flags |= PT_OVERLAY_GRID;
            g_overlay.on = true;
        }
        else if (a == "--solid") {
            g_solid = 1;
            // the count is optional: taken when the next argument is a number
            if (i + 1 < argc && argv[i + 1][0] != '\0' && strspn(argv[i + 1], "0123456789") == strlen(argv[i + 1])) {
                const char *v = argv[++i];
                g_solid = strlen(v) < 6 ? (uint32_t)strtoul(v, nullptr, 10) : 0u;
                if (!g_solid) {
                    fprintf(stderr, "--solid takes N = 1..99999 samples of guides (or none: 1)\n");
                    return 1;
                }
            }
        }
        else if (a == "--exposure") {
            char *e = nullptr;
            const char *v = next();
            exposure = strtof(v, &e);
            if (e == v || *e || !(exposure > 0.0f) || !(exposure < INFINITY)) {
                fprintf(stderr, "--exposure needs a positive finite number\n");
                return 1;
            }
        }
        else if (a == "--hdr") {
            g_tone.hdr = next();
            if (g_tone.hdr.empty()) {
                fprintf(stderr, "--hdr needs FILE.pfm\n");
                return 1;
            }
        } else if (a == "--tonemap") {
            const std::string c = next();
            if (c != "clamp" && c != "reinhard" && c != "aces") {
                fprintf(stderr, "--tonemap takes clamp, reinhard or aces\n");
                return 1;
            }
            g_tone.curve_on = true;
            g_tone.curve = c == "clamp" ? PT_TONE_CLAMP : c == "reinhard" ? PT_TONE_REINHARD : PT_TONE_ACES;
        } else if (a == "--tone-luma") {
            g_tone.luma = true;
        } else if (a == "--white") {
            const char *v = next();
            char *e = nullptr;
            g_tone.white = strtof(v, &e);
            if (e == v || *e || !(g_tone.white > 0.0f) || !(g_tone.white < INFINITY)) {
                fprintf(stderr, "--white needs a positive finite number\n");
                return 1;
            }
        } else if (a == "--auto-exposure") {
            g_tone.auto_on = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') {
                char *e = nullptr;
                g_tone.key = strtof(argv[++i], &e);
                if (*e || !(g_tone.key > 0.0f) || !(g_tone.key < INFINITY)) {
                    fprintf(stderr, "--auto-exposure takes a positive finite KEY (or none: 0.18)\n");
                    return 1;
                }
            }
        }
        else if (a == "--despike") {
            g_tone.despike_on = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') {
                char *e = nullptr;
                g_tone.despike_t = strtof(argv[++i], &e);
                if (*e || !(g_tone.despike_t >= 1.0f) || !(g_tone.despike_t < INFINITY)) {
                    fprintf(stderr, "--despike takes a finite threshold T >= 1 (or none: 2)\n");
                    return 1;
                }
            }
        }
        else if (a == "--aov") {
            aov_spp = (uint32_t)strtoul(next(), nullptr, 10);
            if (!aov_spp) {
                usage();
                return 1;
            }
        }
        else if (a == "--aov-chain") {
            g_aov_chain = true;
            g_aov.flags = PT_AOV_THROUGH_DELTA;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) {  // the optional K
                const char *v = argv[++i];
                const unsigned long k = *v && strspn(v, "0123456789") == strlen(v) && strlen(v) < 4 ? strtoul(v, nullptr, 10) : 0ul;
                if (k < 1ul || k > PT_AOV_MAX_CHAIN) {
                    fprintf(stderr, "--aov-chain takes K = 1..%u steps (or none: 8)\n", PT_AOV_MAX_CHAIN);
                    return 1;
                }
                g_aov.max_chain = (uint32_t)k;
            }
        }
        else if (a == "--noise-target") {
            noise.target = strtof(next(), nullptr);
            if (!(noise.target > 0.0f)) {
                usage();
                return 1;
            }
        }
        else if (a == "--noise-map") {
            noise.map = next();
            if (noise.map.empty()) {
                usage();
                return 1;
            }
        }
        else if (a == "--adaptive") {
            const char *v = next();
            char *end = nullptr;
            adaptive.target = strtof(v, &end);
            if (end == v || !(adaptive.target >= 0.0f)) {
                usage();
                return 1;
            }
        }
        else if (a == "--adaptive-checkpoint") {
            adaptive.file = next();
            if (adaptive.file.empty()) {
                usage();
                return 1;
            }
        }
        else if (a == "--tile") adaptive.tile = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--spp-map") {
            adaptive.map = next();
            if (adaptive.map.empty()) {
                usage();
                return 1;
            }
        }
        else if (a == "--error-map") {
            adaptive.error_map = next();
            if (adaptive.error_map.empty()) {
                usage();
                return 1;
            }
        }
        else if (a == "--trace-scale") {
            const char *v = next();
            trace_scale = strspn(v, "0123456789") == strlen(v) ? (uint32_t)strtoul(v, nullptr, 10) : 0u;
            if (trace_scale < 2u || trace_scale > 8u) {
                fprintf(stderr, "--trace-scale needs K = 2..8\n");
                return 1;
            }
        }
        else if (a == "--retrace")
            retrace = true;
        else if (a == "--orbit") {
            const char *v = next();
            orbit_frames = *v && strspn(v, "0123456789") == strlen(v) ? (uint32_t)strtoul(v, nullptr, 10) : 0u;
            if (!orbit_frames || orbit_frames > 1000u) {
                fprintf(stderr, "--orbit needs N = 1..1000 frames\n");
                return 1;
            }
        }
        else if (a == "--move") {
            const char *v = next();
            char colon = 0, rest = 0;
            if (sscanf(v, "%ld%c%f,%f,%f%c", &orbit_move.index, &colon, &orbit_move.d[0], &orbit_move.d[1], &orbit_move.d[2], &rest) != 5 ||
                colon != ':' || orbit_move.index < 0 || !std::isfinite(orbit_move.d[0]) || !std::isfinite(orbit_move.d[1]) ||
                !std::isfinite(orbit_move.d[2])) {
                fprintf(stderr, "--move needs I:DX,DY,DZ, an object index and three finite numbers\n");
                return 1;
            }
        }
        else if (a == "--move-history") {
            orbit_move.carry = true;
            // the optional F: taken when the next argument is a number
            char *e = nullptr;
            const float f = i + 1 < argc ? strtof(argv[i + 1], &e) : 0.0f;
            if (i + 1 < argc && e != argv[i + 1] && !*e) {
                ++i;
                orbit_move.history = f;
                if (!(f >= 1.0f) || !std::isfinite(f)) {
                    fprintf(stderr, "--move-history takes F >= 1 frames, a finite number (or none: the library's max_history)\n");
                    return 1;
                }
            }
        }
        else if (a == "--boost") {
            const char *v = next();
            boost = *v && strspn(v, "0123456789") == strlen(v) ? (uint32_t)strtoul(v, nullptr, 10) : 0u;
            if (boost < 2u || boost > 64u) {
                fprintf(stderr, "--boost needs K = 2..64\n");
                return 1;
            }
        }
        else if (a == "--orbit-step") {
            char *e = nullptr;
            const char *v = next();
            orbit_step = strtod(v, &e);
            orbit_step_given = true;
            if (e == v || *e || !std::isfinite(orbit_step)) {
                fprintf(stderr, "--orbit-step needs a finite number of degrees\n");
                return 1;
            }
        }
        else if (a == "--denoise-var") {
            denoise_var_spp = 16;
            if (i + 1 < argc && argv[i + 1][0] != '\0' && strspn(argv[i + 1], "0123456789") == strlen(argv[i + 1])) {
                denoise_var_spp = (uint32_t)strtoul(argv[++i], nullptr, 10);
                if (!denoise_var_spp) {
                    fprintf(stderr, "--denoise-var needs a positive number of guide samples\n");
                    return 1;
                }
            }
        }
        else if (a == "--denoise") {
            denoise_spp = 16;
            // the count is optional: taken when the next argument is a number
            if (i + 1 < argc && argv[i + 1][0] != '\0' && strspn(argv[i + 1], "0123456789") == strlen(argv[i + 1])) {
                denoise_spp = (uint32_t)strtoul(argv[++i], nullptr, 10);
                if (!denoise_spp) {
                    usage();
                    return 1;
                }
            }
        }
        else {
            usage();
            return 1;
        }
    }
    if (!spp || !res_y || !width) {
        usage();
        return 1;
    }
    if (g_aov_chain && !(aov_spp || denoise_spp || denoise_var_spp || trace_scale || orbit_frames)) {
        fprintf(stderr, "--aov-chain goes with --aov, --denoise, --denoise-var, --trace-scale or --orbit: nothing else reads guides\n");
        return 1;
    }
    if (orbit_step_given && !orbit_frames) {
        fprintf(stderr, "--orbit-step goes with --orbit N\n");
        return 1;
    }
    if (boost && !orbit_frames) {
        fprintf(stderr, "--boost goes with --orbit N: it boosts the pixels that find no history\n");
        return 1;
    }
    if (orbit_move.index >= 0 && !orbit_frames) {
        fprintf(stderr, "--move goes with --orbit N\n");
        return 1;
    }
    if (orbit_move.carry && (orbit_move.index < 0 || g_aov_chain)) {
        fprintf(stderr, "--move-history goes with --move I:DX,DY,DZ and not with --aov-chain: it carries the moved object's history\n");
        return 1;
    }
    if (orbit_frames && preview.empty()) {
        fprintf(stderr, "--orbit needs --preview FILE.ppm: the frames are written as FILE-000.ppm, FILE-001.ppm, ...\n");
        return 1;
    }
    if (orbit_frames && (gpus > 1 || trace_scale || adaptive.target >= 0.0f || noise.target > 0.0f || !checkpoint.empty() || denoise_spp || denoise_var_spp ||
                         aov_spp)) {
        fprintf(stderr, "--orbit works with one GPU only and not with --trace-scale, --adaptive, --noise-target, --checkpoint, --denoise, "
                        "--denoise-var or --aov\n");
        return 1;
    }
    if (!checkpoint.empty() && gpus > 1) {
        fprintf(stderr, "--checkpoint works with one GPU only (--gpus %u)\n", gpus);
        return 1;
    }
    if (denoise_spp && gpus > 1) {
        fprintf(stderr, "--denoise works with one GPU only (--gpus %u)\n", gpus);
        return 1;
    }
    if (noise.target > 0.0f && gpus > 1) {
        fprintf(stderr, "--noise-target works with one GPU only (--gpus %u)\n", gpus);
        return 1;
    }
    if (!noise.map.empty() && !(noise.target > 0.0f)) {
        fprintf(stderr, "--noise-map needs --noise-target\n");
        return 1;
    }
    const bool is_adaptive = adaptive.target >= 0.0f;
    if (is_adaptive && (!checkpoint.empty() || noise.target > 0.0f)) {
        fprintf(stderr, "--adaptive cannot be combined with --checkpoint or --noise-target\n");
        return 1;
    }
    if (is_adaptive && (gpus > 1 || denoise_spp)) {
        fprintf(stderr, "--adaptive works with one GPU only and not with --denoise\n");
        return 1;
    }
    if ((!adaptive.map.empty() || adaptive.tile) && !is_adaptive) {
        fprintf(stderr, "--tile and --spp-map need --adaptive\n");
        return 1;
    }
    if (!adaptive.error_map.empty() && !is_adaptive) {
        fprintf(stderr, "--error-map needs --adaptive\n");
        return 1;
    }
    if (!adaptive.file.empty() && !is_adaptive) {
        fprintf(stderr, "--adaptive-checkpoint needs --adaptive\n");
        return 1;
    }
    if (!preview.empty() && gpus > 1) {
        fprintf(stderr, "--preview works with one GPU only (--gpus %u)\n", gpus);
        return 1;
    }
    if (preview.empty() && (preview_w || exposure != 0.0f)) {
        fprintf(stderr, "--preview-size and --exposure go with --preview FILE.ppm\n");
        return 1;
    }
    if (g_solid && preview.empty()) {
        fprintf(stderr, "--solid goes with --preview FILE.ppm\n");
        return 1;
    }
    if ((g_tone.any() || g_tone.luma) && preview.empty()) {
        fprintf(stderr, "--hdr, --tonemap, --tone-luma, --auto-exposure and --despike go with --preview FILE.ppm\n");
        return 1;
    }
    if (g_tone.luma && !g_tone.curve_on) {
        fprintf(stderr, "--tone-luma goes with --tonemap\n");
        return 1;
    }
    if (g_tone.any() && (trace_scale || is_adaptive || boost)) {
        fprintf(stderr, "--hdr, --tonemap, --auto-exposure and --despike cannot be combined with %s: the frame is not the one pt_ctx_accumulate holds\n",
                trace_scale ? "--trace-scale" : boost ? "--boost" : "--adaptive");
        return 1;
    }
    if (!g_tone.hdr.empty() && g_solid && orbit_frames) {
        fprintf(stderr, "--hdr cannot be combined with --solid under --orbit: no path is traced\n");
        return 1;
    }
    if (g_tone.despike_on && g_solid) {
        fprintf(stderr, "--despike cannot be combined with --solid: the frame shown is not a traced one\n");
        return 1;
    }
    if (g_solid && g_aov_chain) {
        fprintf(stderr, "--solid cannot be combined with --aov-chain: the chain's ids and depths are the reflected object's\n");
        return 1;
    }
    if (g_solid && (trace_scale || retrace || boost || orbit_move.carry)) {
        fprintf(stderr, "--solid cannot be combined with %s: no path is traced, so it has nothing to act on\n",
                trace_scale ? "--trace-scale" : retrace ? "--retrace" : boost ? "--boost" : "--move-history");
        return 1;
    }
    if (preview.empty() && g_overlay.on) {
        fprintf(stderr, "--select, --outline-radius, --sky and --grid go with --preview FILE.ppm\n");
        return 1;
    }
    if (denoise_var_spp && denoise_spp) {
        fprintf(stderr, "--denoise-var cannot be combined with --denoise\n");
        return 1;
    }
    if (denoise_var_spp && !is_adaptive && !(noise.target > 0.0f)) {
        fprintf(stderr, "--denoise-var needs a frame with a noise estimate: --noise-target or --adaptive\n");
        return 1;
    }
    if (trace_scale && (gpus > 1 || !checkpoint.empty() || noise.target > 0.0f || is_adaptive)) {
        fprintf(stderr, "--trace-scale works with one GPU only and not with --checkpoint, --noise-target or --adaptive\n");
        return 1;
    }
    if (retrace && !trace_scale) {
        fprintf(stderr, "--retrace needs --trace-scale\n");
        return 1;
    }
    if ((!checkpoint.empty() || !adaptive.file.empty()) && !seed_given) seed = 0;
    // load_scene_ids (scenes.rs:28-38): a scenes/ directory without any *.json is filled with the built-in scenes
    if (scene_ids(root).empty()) {
        mkdir((root + "/scenes").c_str(), 0777);
        for (uint32_t i = 0; i < pt_builtin_scene_count(); ++i) {
            const char *bid = pt_builtin_scene_id(i);
            pt_scene *b = nullptr;
            if (pt_scene_builtin(bid, root.c_str(), &b) != PT_OK ||
                pt_scene_save(b, (root + "/scenes/" + bid + ".json").c_str()) != PT_OK)
                fprintf(stderr, "Failed to save scene '%s': %s\n", bid, pt_last_error());
            pt_scene_free(b);
        }
    }
    // SceneId::Int(i) -> nth scene of the listing, SceneId::String -> by id (cmd_render.rs:19-30)
    std::string id = scene_arg;
    char *endp = nullptr;
    unsigned long idx = strtoul(scene_arg.c_str(), &endp, 10);
    if (*endp == '\0' && !scene_arg.empty()) {
        std::vector<std::string> ids = scene_ids(root);
        if (idx >= ids.size()) {
            fprintf(stderr, "scene index %lu out of range (%zu scenes)\n", idx, ids.size());
            return 1;
        }
        id = ids[idx];
    }
    pt_scene *sc = nullptr;
    int rc = pt_scene_load((root + "/scenes/" + id + ".json").c_str(), root.c_str(), &sc);
    if (rc) {
        fprintf(stderr, "cannot load scene '%s': %s\n", id.c_str(), pt_last_error());
        return 1;
    }
    uint32_t n_objs = 0, n_tris = 0;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    printf("Rendering scene %s (%u objects), %u samples per pixel, %ux%u resolution\n", pt_scene_id(sc), n_objs, spp,
           width, res_y);  // mod.rs:987-995
    pt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = width;
    cfg.height = res_y;
    cfg.spp = spp;
    cfg.backend = backend == "megakernel" ? PT_BACKEND_MEGAKERNEL : PT_BACKEND_WAVEFRONT;
    cfg.seed = seed;
    if (orbit_frames) {
        if (orbit_move.index >= (long)n_objs) {
            fprintf(stderr, "--move: object %ld is not one of the scene's %u\n", orbit_move.index, n_objs);
            pt_scene_free(sc);
            return 1;
        }
        rc = render_orbit(&cfg, sc, orbit_frames, orbit_step, preview, preview_w, preview_h, exposure, orbit_move, boost);
        pt_scene_free(sc);
        return rc ? 2 : 0;
    }
    std::vector<float> img((size_t)width * res_y * 3, 0.0f);
    pt_stats st;
    DeviceFrame df;
    df.want_error = denoise_var_spp != 0;
    const bool keep_frame = denoise_spp || denoise_var_spp || !preview.empty();  // the frame stays on its GPU for what follows
    if (trace_scale)
        rc = render_scaled(&cfg, sc, trace_scale, retrace, img, &st, keep_frame ? &df : nullptr);
    else if (is_adaptive)
        rc = render_adaptive(&cfg, sc, adaptive, img, &st, keep_frame ? &df : nullptr);
    else if (checkpoint.empty() && !keep_frame && !(noise.target > 0.0f))
        rc = pt_render_multi(&cfg, gpus ? gpus : 1, pt_scene_camera(sc), objs, n_objs, tris, n_tris, img.data(), nullptr,
                             progress, nullptr, &st);
    else
        rc = render_on_context(&cfg, sc, checkpoint, img, &st, keep_frame ? &df : nullptr, &noise);
    const uint32_t spp_out = noise.target > 0.0f && !rc ? noise.spp_reached : spp;  // the samples the frame holds
    cfg.spp = spp_out;
    auto release = [&]() {
        if (df.d_error) pt_device_free(df.dev, df.d_error);
        if (df.d_out) pt_device_free(df.dev, df.d_out);
        if (df.ctx) pt_ctx_destroy(df.ctx);
        pt_scene_free(sc);
    };
    if (rc == kCliExit) {
        release();
        return 1;
    }
    fprintf(stderr, "\n");
    if (g_despike_pending) despike_report();
    if (rc) {
        fprintf(stderr, "render failed (%d): %s\n", rc, pt_last_error());
        release();
        return 2;
    }
    printf("Rendering complete\n");
    printf("{\"ray_bounces\": %llu, \"samples\": %llu, \"ms_total\": %.3f, \"ms_device\": %.3f, \"ray_bounces_per_sec\": %.4g}\n",
           (unsigned long long)st.ray_bounces, (unsigned long long)st.samples, st.ms_total, st.ms_device,
           st.ray_bounces / (st.ms_total * 1e-3));
    // out/<stamp>-scene-<id>-spp<N>-res<H>- : the image's name without ".ppm" (mod.rs:1035-1041); the AOV files share it
    char stamp[64];
    time_t now = time(nullptr);
    strftime(stamp, sizeof stamp, "%Y-%m-%d_%H:%M:%S", localtime(&now));
    const std::string stem = out_dir + "/" + stamp + "-scene-" + pt_scene_id(sc) + "-spp" + std::to_string(spp_out) + "-res" +
                             std::to_string(res_y) + "-";
    if (write_ppm || aov_spp || denoise_spp || denoise_var_spp) mkdir(out_dir.c_str(), 0755);  // create_dir_all("out"), mod.rs:1032
    if (write_ppm) {
        const std::string path = stem + ".ppm";
        rc = pt_write_ppm(path.c_str(), img.data(), width, res_y, spp_out, pt_scene_id(sc), (uint64_t)(st.ms_total / 1000.0));
        if (rc) {
            fprintf(stderr, "cannot write %s: %s\n", path.c_str(), pt_last_error());
            release();
            return 3;
        }
        unlink("latest.ppm");  // mod.rs:1079-1088
        if (symlink(path.c_str(), "latest.ppm") != 0)
            printf("Could not create symlink to latest image. You can find it at %s\n", path.c_str());
        printf("wrote %s\n", path.c_str());
    }
    if (!g_tone.hdr.empty() && write_hdr(df.dev, (const float *)df.d_out, width, res_y, g_tone.hdr)) {
        release();
        return 3;
    }
    if (aov_spp && write_aovs(&cfg, aov_spp, sc, img, stem)) {
        release();
        return 3;
    }
    if ((denoise_spp || denoise_var_spp) &&
        write_denoised(&cfg, denoise_spp ? denoise_spp : denoise_var_spp, df, stem, pt_scene_id(sc))) {
        release();
        return 3;
    }
    if (!preview.empty() && write_preview(&cfg, df, preview, preview_w, preview_h, exposure, sc)) {
        release();
        return 3;
    }
    release();
    return 0;
}
