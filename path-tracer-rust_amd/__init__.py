"""Python binding of libptrace_hip.so (C ABI in include/ptrace.h) for bench.py, smoke() and the rank harness.

Import with importlib.import_module("path-tracer-rust_amd").  This module is plumbing only: it loads the
in-tree shared library (and fails loudly if it is missing — there is no Python or CPU fallback), re-exports the
structs and constants of abi.py, and provides the band partition / framebuffer gather used when one process per GPU renders a
contiguous band of the reference's `pixels` vector (src/render/mod.rs:1017-1024: pixels are independent).
"""
import ctypes as C
import os

from . import abi
from .abi import (PT_AOV_MAX_CHAIN, PT_AOV_THROUGH_DELTA, PT_CANCELLED, PT_DENOISE_NO_DEMODULATE, PT_ERR_HIP, PT_ERR_INVALID,  # noqa: F401
                  PT_ERR_IO, PT_ERR_NO_DEVICE, PT_ERR_PARSE, PT_FLAG_NO_BVH, PT_FLAG_SEPARATE_KERNELS, PT_OK,
                  PT_PRESENT_FRAMEBUFFER_ORDER, PT_PRESENT_RGB8, PT_PRESENT_RGBA8, PT_SCATTER_BY_ID, PT_SCATTER_BY_RANK,
                  PT_SCATTER_DEFER_REFRACT, PT_SCATTER_GIVEN, PT_SCATTER_NOT_SHADED, PT_SCATTER_REFRACT_ONLY, TABLE_NAMES, f3,
                  pt_adaptive_info, pt_adaptive_params, pt_adaptive_stats, pt_aov_params, pt_camera, pt_config, pt_denoise_params,
                  pt_denoise_var_params, pt_noise_stats, pt_noise_target, pt_object, pt_object_motion, pt_present_params,
                  pt_reproject_params, pt_reproject_var_params, pt_scatter_item, pt_scatter_out, pt_scatter_surface,
                  pt_select_params, pt_stats, pt_triangle, pt_upsample_params)
from .overlay_abi import PT_OVERLAY_GRID, PT_OVERLAY_SKY, pt_overlay_params  # noqa: F401  (include/ptrace_overlay.h)
from .solid_abi import (PT_SOLID_HEADLIGHT, PT_SOLID_MAX_SHININESS_LOG2, PT_SOLID_REFLECT_SKY, pt_solid_look,  # noqa: F401
                        pt_solid_params)  # (include/ptrace_solid.h)
from .tone_abi import (PT_METER_BINS, PT_METER_SKIP_MISSES, PT_TONE_ACES, PT_TONE_CLAMP, PT_TONE_LUMA, PT_TONE_REINHARD,  # noqa: F401
                       pt_meter_exposure_params, pt_meter_params, pt_meter_stats, pt_tonemap_params)  # (include/ptrace_tone.h)
from .despike_abi import PT_DESPIKE_SAME_OBJECT, pt_despike_params, pt_despike_stats  # noqa: F401  (include/ptrace_despike.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PT_LIB") or os.path.join(_HERE, "libptrace_hip.so")  # PT_LIB: A/B builds when tuning


class PtraceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ptrace error %d: %s" % (code, msg))
        self.code = code


BACKEND_WAVEFRONT, BACKEND_MEGAKERNEL = abi.PT_BACKEND_WAVEFRONT, abi.PT_BACKEND_MEGAKERNEL
BACKENDS = {"wavefront": BACKEND_WAVEFRONT, "megakernel": BACKEND_MEGAKERNEL}

_lib = None


def lib():
    """The loaded C ABI.  Raises if the HIP library has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build it with `make -C %s` (hipcc, gfx950); there is no fallback path"
                          % (LIB_PATH, _HERE))
    _lib = abi.load(LIB_PATH)
    return _lib


def _check(rc):
    if rc != PT_OK:
        raise PtraceError(rc, lib().pt_last_error().decode())


class Scene:
    """SceneDescriptor::load + to_data through the C ABI (pt_scene_load)."""

    def __init__(self, path, base_dir=None):
        L = lib()
        base_dir = base_dir or os.path.dirname(os.path.dirname(os.path.abspath(path)))
        self._h = C.c_void_p()
        _check(L.pt_scene_load(path.encode(), base_dir.encode(), C.byref(self._h)))
        n, m = C.c_uint32(), C.c_uint32()
        self.objects = L.pt_scene_objects(self._h, C.byref(n))
        self.triangles = L.pt_scene_triangles(self._h, C.byref(m))
        self.n_objects, self.n_triangles = n.value, m.value
        self.camera = L.pt_scene_camera(self._h)
        self.id = L.pt_scene_id(self._h).decode()

    def close(self):
        if self._h:
            lib().pt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """pt_ctx: one GPU, one scene, the ray streams."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().pt_ctx_create(device, C.byref(self._h)))

    def set_scene(self, scene):
        _check(lib().pt_ctx_set_scene(self._h, scene.camera, scene.objects, scene.n_objects, scene.triangles,
                                      scene.n_triangles))

    def set_camera(self, cam):
        """Move the camera of the scene set_scene gave (pt_ctx_set_camera): a pt_camera, a pointer to one or a dict of its fields.
        Returns whether the scene had to be rebuilt (the lens centre left camera_reach()); False on the fast path."""
        rebuilt = C.c_int(0)
        _check(lib().pt_ctx_set_camera(self._h, _camera(cam), C.byref(rebuilt)))
        return bool(rebuilt.value)

    def camera_reach(self):
        """The box (lo, hi), three floats each, of lens centres the scene's tables hold for (pt_ctx_camera_reach)."""
        lo, hi = f3(), f3()
        _check(lib().pt_ctx_camera_reach(self._h, lo, hi))
        return tuple(lo), tuple(hi)

    def reserve_camera_reach(self, lo, hi):
        """Grow camera_reach() to hold the box [lo, hi] now, rebuilding the scene once if it does not
        (pt_ctx_reserve_camera_reach).  Returns whether it rebuilt."""
        rebuilt = C.c_int(0)
        _check(lib().pt_ctx_reserve_camera_reach(self._h, f3(*lo), f3(*hi), C.byref(rebuilt)))
        return bool(rebuilt.value)

    def set_object(self, index, obj):
        """Replace object `index` of the scene set_scene gave (pt_ctx_set_object): a pt_object with the kind and triangle range of
        the one it replaces.  A move inside camera_reach() rewrites that object's records only - a mesh with a BVH is refit on
        the device.  Returns whether the scene had to be rebuilt (the object left camera_reach()); False otherwise."""
        rebuilt = C.c_int(0)
        _check(lib().pt_ctx_set_object(self._h, index, C.byref(obj), C.byref(rebuilt)))
        return bool(rebuilt.value)

    def table_hashes(self):
        """Diagnostics (pt_ctx_table_hashes): {table name: hash of the device table, downloaded}, in TABLE_NAMES' order."""
        out = (C.c_uint64 * len(TABLE_NAMES))()
        _check(lib().pt_ctx_table_hashes(self._h, out))
        return dict(zip(TABLE_NAMES, out))

    def pass_kernel(self, separate_kernels=False):
        """Name of the kernel a wavefront pass of this scene launches (see pt_ctx_pass_kernel)."""
        n = lib().pt_ctx_pass_kernel(self._h, PT_FLAG_SEPARATE_KERNELS if separate_kernels else 0)
        return n.decode() if n else None

    def set_profiling(self, on):
        _check(lib().pt_ctx_set_profiling(self._h, 1 if on else 0))

    @staticmethod
    def _config(width, height, spp, seed=1, backend="wavefront", band=None, rays_per_pass=0, chunks=None, pipelines=1,
                separate_kernels=False):
        cfg = pt_config(width, height, spp, BACKENDS[backend], seed, 0, 0, rays_per_pass,
                        (((pipelines & 15) << 8) if pipelines > 1 else 0) | (PT_FLAG_SEPARATE_KERNELS if separate_kernels else 0))
        if band is not None:
            cfg.idx_begin, cfg.idx_end = band
        if chunks is not None:
            cfg.chunk_pixels, cfg.chunk_first, cfg.chunk_step = chunks
        return cfg

    def render(self, out_ptr, width, height, spp, seed=1, backend="wavefront", band=None, rays_per_pass=0,
               stream=None, chunks=None, pipelines=1, separate_kernels=False):
        """Render band [begin,end) (default whole frame) — or, with chunks=(chunk_pixels, first, step), this rank's
        interleaved chunks of it — into device memory at out_ptr (owned pixels * 3 floats)."""
        cfg = self._config(width, height, spp, seed, backend, band, rays_per_pass, chunks, pipelines, separate_kernels)
        st = pt_stats()
        _check(lib().pt_ctx_render(self._h, C.byref(cfg), C.c_void_p(out_ptr), C.c_void_p(stream or 0), None, None,
                                   None, C.byref(st)))
        return st

    def accumulate(self, out_ptr, width, height, spp, seed=1, backend="wavefront", band=None, rays_per_pass=0,
                   stream=None, chunks=None, pipelines=1, separate_kernels=False):
        """The frame of render() with the same arguments, up to `spp` samples per pixel IN TOTAL: the context keeps the
        samples of earlier calls for this frame and traces only the rest (pt_ctx_accumulate).  Returns this call's pt_stats."""
        cfg = self._config(width, height, spp, seed, backend, band, rays_per_pass, chunks, pipelines, separate_kernels)
        st = pt_stats()
        _check(lib().pt_ctx_accumulate(self._h, C.byref(cfg), C.c_void_p(out_ptr), C.c_void_p(stream or 0), None, None,
                                       None, C.byref(st)))
        return st

    def accum_info(self, width, height, seed=1, band=None, chunks=None):
        """(min, max) samples per pixel held for this frame; (0, 0) if the context holds another frame or none."""
        cfg = self._config(width, height, 1, seed, band=band, chunks=chunks)
        lo, hi = C.c_uint32(), C.c_uint32()
        _check(lib().pt_ctx_accum_info(self._h, C.byref(cfg), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def render_aov(self, width, height, spp, seed=1, band=None, chunks=None, albedo=None, normal=None, depth=None,
                   object_id=None, no_bvh=False, stream=None, through_delta=False, max_chain=0, chain=None):
        """First-hit AOVs of the frame render() would draw with the same width, height, seed, band and chunks, over its first
        `spp` samples (pt_ctx_render_aov): device pointers, each optional - albedo / normal: pixels * 3 float32 (the means
        over the samples), depth: pixels float32 (sample 0's hit distance, +inf on a miss), object_id: pixels int32 (sample
        0's object, -1 on a miss).
        through_delta=True (pt_ctx_render_aov_ex with PT_AOV_THROUGH_DELTA): a sample that hits a mirror or glass surface
        follows the deterministic chain, at most max_chain steps (0 = 8, at most PT_AOV_MAX_CHAIN), and the guides describe
        the surface that ends it; depth is then the path's whole length.  chain: pixels uint32, sample 0's number of delta
        steps (zeros without through_delta).  Without through_delta, max_chain and chain this is the plain call."""
        cfg = self._config(width, height, spp, seed, band=band, chunks=chunks)
        if no_bvh:
            cfg.flags |= PT_FLAG_NO_BVH
        ptr = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        if not through_delta and not max_chain and not chain:
            _check(lib().pt_ctx_render_aov(self._h, C.byref(cfg), ptr(albedo), ptr(normal), ptr(depth), ptr(object_id),
                                           C.c_void_p(stream or 0)))
            return
        params = pt_aov_params(PT_AOV_THROUGH_DELTA if through_delta else 0, max_chain)
        _check(lib().pt_ctx_render_aov_ex(self._h, C.byref(cfg), C.byref(params), ptr(albedo), ptr(normal), ptr(depth),
                                          ptr(object_id), ptr(chain), C.c_void_p(stream or 0)))

    def denoise(self, width, height, color, out, albedo=None, normal=None, depth=None, stream=None, **params):
        """Denoise a whole width x height frame in device memory (pt_ctx_denoise): `color` and `out` are device pointers to
        pixels * 3 float32 (out may be color); the guides albedo / normal (pixels * 3) and depth (pixels) are optional - what
        render_aov writes for the same frame.  params: levels, sigma_color, sigma_depth (0 or absent = denoise_defaults()),
        no_demodulate=True for PT_DENOISE_NO_DEMODULATE."""
        p = pt_denoise_params()
        p.flags = PT_DENOISE_NO_DEMODULATE if params.pop("no_demodulate", False) else 0
        for k in ("levels", "sigma_color", "sigma_depth", "sigma_normal_pow"):
            if k in params:
                setattr(p, k, params.pop(k))
        if params:
            raise TypeError("denoise() got unexpected parameters %r" % sorted(params))
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_denoise(self._h, width, height, C.byref(p), ptr(color), ptr(albedo), ptr(normal), ptr(depth),
                                    ptr(out), C.c_void_p(stream or 0)))

    def denoise_var(self, width, height, color, error, out, albedo=None, normal=None, depth=None, levels=0, sigma_var=0.0,
                    sigma_depth=0.0, no_demodulate=False, stream=None):
        """Denoise a whole width x height frame in device memory as far as its own noise estimate says it needs
        (pt_ctx_denoise_var): as denoise(), with `error` a device pointer to pixels float32 - what accum_noise(error=...) or
        render_adaptive(error=...) wrote for the same frame.  levels, sigma_var, sigma_depth: 0 = denoise_var_defaults()."""
        p = pt_denoise_var_params(levels, sigma_var, sigma_depth, PT_DENOISE_NO_DEMODULATE if no_demodulate else 0)
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_denoise_var(self._h, width, height, C.byref(p), ptr(color), ptr(error), ptr(albedo), ptr(normal),
                                        ptr(depth), ptr(out), C.c_void_p(stream or 0)))

    def present(self, width, height, rgb, out, out_size=None, exposure=0.0, rgb8=False, framebuffer_order=False, stream=None):
        """A whole width x height float frame in device memory as gamma-corrected 8-bit pixels (pt_ctx_present): `rgb` is a
        device pointer to pixels * 3 float32, `out` one to out pixels * 4 bytes (r, g, b, 255) or * 3 with rgb8=True, row-major
        from the top-left display pixel.  out_size=(w, h) fits the frame to that size by area averaging; exposure 0 = 1;
        framebuffer_order=True keeps the frame's own order instead of the display's."""
        ow, oh = out_size if out_size else (0, 0)
        p = pt_present_params(ow, oh, exposure, PT_PRESENT_RGB8 if rgb8 else PT_PRESENT_RGBA8,
                              PT_PRESENT_FRAMEBUFFER_ORDER if framebuffer_order else 0)
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_present(self._h, width, height, C.byref(p), ptr(rgb), ptr(out), C.c_void_p(stream or 0)))

    def overlay(self, width, height, rgb, out, params=None, cam=None, object_id=None, depth=None):
        """The editing cues on a whole width x height float frame in device memory (pt_ctx_overlay): the sky where object_id < 0,
        the ground grid where depth does not hide it, and the tint and outline of the objects listed in `params`
        (a pt_overlay_params; overlay_defaults(cam) gives one to fill in; None = copy).  Device pointers: `rgb` and `out`
        pixels * 3 float32 (out may be rgb), `object_id` pixels int32, `depth` pixels float32 - the planes of render_aov.  Runs on
        the context's own stream: there is no stream argument."""
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_overlay(self._h, width, height, C.byref(params) if params is not None else None,
                                    C.byref(cam) if cam is not None else None, ptr(rgb), ptr(object_id), ptr(depth), ptr(out)))

    def solid(self, width, height, normal, depth, object_id, out, cam, albedo=None, params=None, looks=None, stream=None):
        """A lit solid view of a whole width x height frame from the first-hit guides in device memory (pt_ctx_solid): ambient,
        diffuse and one highlight, times the albedo, plus the objects' emission.  Device pointers, the planes of render_aov:
        `normal`, `albedo` (None: a clay view) and `out` pixels * 3 float32 (out may be albedo or normal), `depth` pixels
        float32, `object_id` pixels int32.  `cam`: as for set_camera().  `params`: a pt_solid_params (solid_defaults() gives one; None = the defaults);
        `looks`: a ctypes array of pt_solid_look indexed by object id (solid_looks(objects)), host memory, or None."""
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_solid(self._h, width, height, C.byref(params) if params is not None else None, _camera(cam), ptr(albedo),
                                  ptr(normal), ptr(depth), ptr(object_id), looks, len(looks) if looks is not None else 0, ptr(out),
                                  C.c_void_p(stream or 0)))

    def accum_hdr(self, out_ptr, width, height, seed=1, band=None, chunks=None, stream=None):
        """The frame accumulate() holds for these arguments, resolved WITHOUT the clamp to [0, 1] (pt_ctx_accum_hdr): into device
        memory at out_ptr, laid out as accumulate() lays its output out.  Raises if the context holds another frame or none."""
        cfg = self._config(width, height, 1, seed, band=band, chunks=chunks)
        _check(lib().pt_ctx_accum_hdr(self._h, C.byref(cfg), C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    def meter(self, width, height, rgb, object_id=None, rect=None, skip_misses=False, stream=None):
        """The luminance histogram of a whole width x height float frame in device memory (pt_ctx_meter): a pt_meter_stats -
        256 bins, eight per octave from 2^-20, the dark pixels apart, and the largest luminance.  `rgb`: device pointer to
        pixels * 3 float32; rect=(x0, y0, x1, y1) meters that half-open rectangle only; skip_misses=True leaves out the pixels
        whose `object_id` (device pointer, pixels int32) is below 0.  meter_exposure() turns the result into an exposure."""
        x0, y0, x1, y1 = rect if rect else (0, 0, 0, 0)
        p = pt_meter_params(PT_METER_SKIP_MISSES if skip_misses else 0, x0, y0, x1, y1)
        out = pt_meter_stats()
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_meter(self._h, width, height, C.byref(p), ptr(rgb), ptr(object_id), C.byref(out), C.c_void_p(stream or 0)))
        return out

    def tonemap(self, width, height, rgb, out, params=None, stream=None):
        """Exposure and a tone curve on a whole width x height float frame in device memory (pt_ctx_tonemap): `rgb` and `out` are
        device pointers to pixels * 3 float32 (out may be rgb); the result is display-linear in [0, 1], what overlay() and
        present() take.  `params`: a pt_tonemap_params (tonemap_defaults() gives one; None = the defaults)."""
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_tonemap(self._h, width, height, C.byref(params) if params is not None else None, ptr(rgb), ptr(out),
                                    C.c_void_p(stream or 0)))

    def despike(self, width, height, rgb, out, params=None, object_id=None, mask=None, stats=True, stream=None):
        """Fireflies of a whole width x height float frame in device memory clipped (pt_ctx_despike), in front of denoise(): a
        pixel brighter than threshold * (the rank-th largest luminance of its neighbours) + floor is scaled down to that limit,
        a non-finite one written as 0.  `rgb` and `out` are device pointers to pixels * 3 float32 and may not be the same;
        `params`: a pt_despike_params (despike_defaults() gives one; None = the defaults); `object_id` (device pointer, pixels
        int32) is read with PT_DESPIKE_SAME_OBJECT in params.flags; `mask` (device pointer, pixels bytes) receives 0 / 1 (spike) /
        2 (non-finite), the plane render_masked() reads.  Returns a pt_despike_stats, or None with stats=False (nothing is then
        counted or downloaded)."""
        st = pt_despike_stats() if stats else None
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_despike(self._h, width, height, C.byref(params) if params is not None else None, ptr(rgb), ptr(object_id),
                                    ptr(out), ptr(mask), C.byref(st) if stats else None, C.c_void_p(stream or 0)))
        return st

    def _reproject(self, entry, params, width, height, cam, frame, history, outs, motion=None, stream=None):
        """The one call of the five reproject methods.  `params`: the entry point's struct, filled - pt_reproject_var_params
        brings the "moments" of `history` along; `frame`: this frame's planes in the entry point's order, `outs`: its outputs;
        motion None: the entry point takes no table."""
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        h = history or {}
        var = isinstance(params, pt_reproject_var_params)
        keys = ("color", "len", "moments", "depth", "object_id", "normal") if var else ("color", "len", "depth", "object_id", "normal")
        table = () if motion is None else (_motion_table(motion), len(motion))
        _check(getattr(lib(), entry)(self._h, width, height, C.byref(params), _camera(cam), *map(ptr, frame),
                                     _camera(h["cam"]) if history else None, *(ptr(h.get(k)) for k in keys), *map(ptr, outs), *table,
                                     C.c_void_p(stream or 0)))

    def reproject(self, width, height, cam, color, depth, object_id, out_color, out_len, normal=None, history=None, weight=1,
                  max_history=0.0, depth_tol=0.0, normal_min=0.0, stream=None):
        """Carry a preview frame's history across a camera move and blend it with this frame (pt_ctx_reproject).  Device pointers
        to whole width x height frames: color, normal, out_color pixels * 3 float32; depth, out_len pixels float32; object_id
        pixels int32 - what render() and render_aov() write.  `cam`: this frame's camera (a pt_camera, a pointer to one, or a dict
        of its fields).  `history`: None for the first frame, else a dict with "cam", "color", "len", "depth", "object_id" and
        optionally "normal" - after the call the next frame's history is dict(cam=cam, color=out_color, len=out_len, depth=depth,
        object_id=object_id, normal=normal): pointers are swapped, nothing is copied.  weight: the samples per pixel `color`
        holds; max_history, depth_tol, normal_min: 0 = reproject_defaults().  out_color may be color."""
        self._reproject("pt_ctx_reproject", pt_reproject_params(weight, max_history, depth_tol, normal_min, 0), width, height, cam,
                        (color, depth, object_id, normal), history, (out_color, out_len), stream=stream)

    def reproject_var(self, width, height, cam, color, depth, object_id, out_color, out_len, out_moments, error, normal=None,
                      history=None, weight=1, max_history=0.0, depth_tol=0.0, normal_min=0.0, min_frames=0, radius=0, stream=None):
        """reproject() with the temporal moments of (r + g) + b carried along and a noise map per frame out of them
        (pt_ctx_reproject_var).  As reproject(), and: out_moments pixels * 2 float32, error pixels float32 - the estimate
        denoise_var() reads, +inf where there is none; `history` also holds "moments" - after the call the next frame's history
        is dict(cam=cam, color=out_color, len=out_len, moments=out_moments, depth=depth, object_id=object_id, normal=normal).
        min_frames, radius: 0 = reproject_var_defaults().  out_color may be color; out_moments and error alias nothing."""
        p = pt_reproject_var_params(weight, max_history, depth_tol, normal_min, min_frames, radius, 0)
        self._reproject("pt_ctx_reproject_var", p, width, height, cam, (color, depth, object_id, normal), history,
                        (out_color, out_len, out_moments, error), stream=stream)

    def reproject_var_moved(self, width, height, cam, color, depth, object_id, out_color, out_len, out_moments, error, motion,
                            normal=None, history=None, weight=1, max_history=0.0, depth_tol=0.0, normal_min=0.0, min_frames=0,
                            radius=0, stream=None):
        """reproject_var() with history carried on objects that set_object() moved (pt_ctx_reproject_var_moved).  `motion`: a
        sequence indexed by object id of pt_object_motion records or (ox, oy, oz, scale) tuples, as object_motion_between()
        makes them - host data, copied by the call; empty, or all (0, 0, 0, 1), is reproject_var() itself."""
        p = pt_reproject_var_params(weight, max_history, depth_tol, normal_min, min_frames, radius, 0)
        self._reproject("pt_ctx_reproject_var_moved", p, width, height, cam, (color, depth, object_id, normal), history,
                        (out_color, out_len, out_moments, error), motion, stream)

    def reproject_var_weighted(self, width, height, cam, color, depth, object_id, out_color, out_len, out_moments, error, spp=None,
                               motion=None, normal=None, history=None, weight=1, max_history=0.0, depth_tol=0.0, normal_min=0.0,
                               min_frames=0, radius=0, stream=None):
        """reproject_var_moved() for a frame whose pixels hold different numbers of samples (pt_ctx_reproject_var_weighted).
        `spp`: a device pointer to pixels uint32, the samples each pixel of `color` holds - render_adaptive()'s spp plane, or
        what spp_plane() makes of a mask; a count of 0 means "not traced this frame": the pixel's history is carried through as
        it is.  spp=None is reproject_var_moved(); motion=None is an empty table.  `weight` stays the uniform value: it scales
        the error of the pixels without samples."""
        p = pt_reproject_var_params(weight, max_history, depth_tol, normal_min, min_frames, radius, 0)
        self._reproject("pt_ctx_reproject_var_weighted", p, width, height, cam, (color, depth, object_id, normal, spp), history,
                        (out_color, out_len, out_moments, error), () if motion is None else motion, stream)

    def spp_plane(self, width, height, spp, base, mask=None, masked=0, stream=None):
        """The plane of counts of a boosted frame (pt_ctx_spp_plane): spp[p] = masked where mask[p] != 0, else base.  Device
        pointers: `spp` pixels uint32, `mask` pixels bytes (select_pixels()'s) or None."""
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_spp_plane(self._h, width, height, base, ptr(mask), masked, ptr(spp), C.c_void_p(stream or 0)))

    def reproject_moved(self, width, height, cam, color, depth, object_id, out_color, out_len, motion, normal=None, history=None,
                        weight=1, max_history=0.0, depth_tol=0.0, normal_min=0.0, stream=None):
        """reproject() with history carried on objects that set_object() moved (pt_ctx_reproject_moved); `motion` as for
        reproject_var_moved()."""
        self._reproject("pt_ctx_reproject_moved", pt_reproject_params(weight, max_history, depth_tol, normal_min, 0), width, height,
                        cam, (color, depth, object_id, normal), history, (out_color, out_len), motion, stream)

    def upsample(self, width, height, lo_width, lo_height, lo, depth, object_id, out_color, normal=None, albedo=None,
                 out_weight=None, depth_tol=0.0, normal_min=0.0, stream=None):
        """Fill a width x height frame from a colour frame traced at lo_width x lo_height, through the first-hit guides of both
        sizes (pt_ctx_upsample).  Device pointers to whole frames: `lo` is a dict with "color", "depth", "object_id" and
        optionally "normal", "albedo" - what render() and render_aov() write at the low size with the same camera and scene;
        depth, object_id, normal, albedo: render_aov()'s at the full size; out_color pixels * 3 float32; out_weight, if given,
        pixels float32 - the bilinear weight of the taps that passed, 0 where none did.  The normal test needs both normals,
        demodulation both albedos.  depth_tol, normal_min: 0 = upsample_defaults().  No output may alias an input."""
        p = pt_upsample_params(depth_tol, normal_min, 0)
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        _check(lib().pt_ctx_upsample(self._h, width, height, lo_width, lo_height, C.byref(p), ptr(lo["color"]), ptr(lo["depth"]),
                                     ptr(lo["object_id"]), ptr(lo.get("normal")), ptr(lo.get("albedo")), ptr(depth), ptr(object_id),
                                     ptr(normal), ptr(albedo), ptr(out_color), ptr(out_weight), C.c_void_p(stream or 0)))

    def select_pixels(self, width, height, mask, weight=None, len=None, weight_max=0.0, len_max=0.0, stream=None):
        """Turn the loop's planes into a byte mask (pt_ctx_select_pixels): mask[p] = 1 where weight[p] <= weight_max or
        len[p] <= len_max or either holds a NaN, else 0.  Device pointers to whole frames: `weight` is upsample()'s out_weight,
        `len` is reproject()'s out_len (pixels float32 each, at least one given); `mask` pixels bytes.  The thresholds are taken
        literally.  Returns the number of selected pixels."""
        p = pt_select_params(weight_max, len_max, 0)
        ptr = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        n = C.c_uint32(0)
        _check(lib().pt_ctx_select_pixels(self._h, width, height, C.byref(p), ptr(weight), ptr(len), ptr(mask), C.byref(n),
                                          C.c_void_p(stream or 0)))
        return n.value

    def scatter(self, items, seed=1, form=PT_SCATTER_BY_ID, surfaces=None):
        """One radiance() invocation per item on the device, through the functions the frame kernels call (pt_ctx_scatter, a
        parity probe).  `items`: a ctypes array of pt_scatter_item; `surfaces`: one of pt_scatter_surface with PT_SCATTER_GIVEN.
        `form`: PT_SCATTER_GIVEN / _BY_ID / _BY_RANK, optionally | PT_SCATTER_DEFER_REFRACT or PT_SCATTER_REFRACT_ONLY.  Returns a
        ctypes array of pt_scatter_out."""
        out = (pt_scatter_out * len(items))()
        _check(lib().pt_ctx_scatter(self._h, seed, form, items, surfaces, len(items), out))
        return out

    def render_masked(self, mask, rgb, width, height, spp, seed=1, band=None, no_bvh=False, rays_per_pass=0, stream=None):
        """Trace the pixels of the frame whose mask byte is not zero and write them into `rgb` (pt_ctx_render_masked): each gets
        what render() with the same arguments writes there, bit for bit; no other float of `rgb` is written.  `mask`: the
        band's pixels bytes, `rgb`: the band's pixels * 3 float32, device pointers; the band is whole rows.  Returns
        (pt_stats, the number of pixels traced)."""
        cfg = self._config(width, height, spp, seed, "megakernel", band, rays_per_pass)
        if no_bvh:
            cfg.flags |= PT_FLAG_NO_BVH
        st, n = pt_stats(), C.c_uint32(0)
        _check(lib().pt_ctx_render_masked(self._h, C.byref(cfg), C.c_void_p(mask), C.c_void_p(rgb), C.c_void_p(stream or 0), None,
                                          C.byref(st), C.byref(n)))
        return st, n.value

    def accum_track_noise(self, on=True):
        """Keep half of every pixel's samples in a second accumulator for the frames started from now on
        (pt_ctx_accum_track_noise), so that accum_noise() / accumulate_until() can estimate the frame's error."""
        _check(lib().pt_ctx_accum_track_noise(self._h, 1 if on else 0))

    def accum_noise(self, width, height, seed=1, band=None, chunks=None, error=None, stream=None):
        """The error estimate of the held, noise-tracked frame (pt_ctx_accum_noise): returns pt_noise_stats; `error`, if
        given, is a device pointer to pixels float32 that receives the per-pixel estimate."""
        cfg = self._config(width, height, 1, seed, band=band, chunks=chunks)
        ns = pt_noise_stats()
        _check(lib().pt_ctx_accum_noise(self._h, C.byref(cfg), C.c_void_p(error) if error else None, C.byref(ns),
                                        C.c_void_p(stream or 0)))
        return ns

    def accumulate_until(self, out_ptr, width, height, max_spp, mean_error=0.0, quantile=0.0, quantile_error=0.0, min_spp=0,
                         seed=1, backend="wavefront", band=None, rays_per_pass=0, stream=None, chunks=None):
        """accumulate() in doubling steps until the estimated error meets the target or max_spp is reached
        (pt_ctx_accumulate_until).  Returns (pt_stats summed over the steps, pt_noise_stats of the frame it ended with)."""
        cfg = self._config(width, height, max_spp, seed, backend, band, rays_per_pass, chunks)
        tgt = pt_noise_target(mean_error, quantile, quantile_error, min_spp)
        st, ns = pt_stats(), pt_noise_stats()
        _check(lib().pt_ctx_accumulate_until(self._h, C.byref(cfg), C.byref(tgt), C.c_void_p(out_ptr), C.c_void_p(stream or 0),
                                             None, None, None, C.byref(st), C.byref(ns)))
        return st, ns

    def render_adaptive(self, out_ptr, width, height, max_spp, tile_error, tile=0, min_spp=0, seed=1, band=None, spp_map=None,
                        error=None, no_bvh=False, rays_per_pass=0, stream=None):
        """The frame with every tile rendered until the mean of its error estimate meets tile_error, max_spp samples per
        pixel at most (pt_ctx_render_adaptive).  `spp_map` (pixels uint32: the samples each pixel got) and `error` (pixels
        float32: the estimate) are optional device pointers.  Returns (pt_stats, pt_adaptive_stats)."""
        cfg = self._config(width, height, max_spp, seed, "megakernel", band, rays_per_pass)
        if no_bvh:
            cfg.flags |= PT_FLAG_NO_BVH
        par = pt_adaptive_params(tile_error, tile, min_spp)
        st, ast = pt_stats(), pt_adaptive_stats()
        ptr = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        _check(lib().pt_ctx_render_adaptive(self._h, C.byref(cfg), C.byref(par), C.c_void_p(out_ptr), ptr(spp_map), ptr(error),
                                            C.c_void_p(stream or 0), None, None, None, C.byref(st), C.byref(ast)))
        return st, ast

    def accumulate_adaptive(self, out_ptr, width, height, max_spp, tile_error, tile=0, min_spp=0, seed=1, band=None,
                            spp_map=None, error=None, no_bvh=False, rays_per_pass=0, stream=None):
        """render_adaptive() on the adaptive frame the context keeps between calls (pt_ctx_accumulate_adaptive): a cancelled
        frame is continued, a smaller tile_error refines it, a higher max_spp extends it; only the samples not held yet are
        traced.  Returns (this call's pt_stats, pt_adaptive_stats)."""
        cfg = self._config(width, height, max_spp, seed, "megakernel", band, rays_per_pass)
        if no_bvh:
            cfg.flags |= PT_FLAG_NO_BVH
        par = pt_adaptive_params(tile_error, tile, min_spp)
        st, ast = pt_stats(), pt_adaptive_stats()
        ptr = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        _check(lib().pt_ctx_accumulate_adaptive(self._h, C.byref(cfg), C.byref(par), C.c_void_p(out_ptr), ptr(spp_map),
                                                ptr(error), C.c_void_p(stream or 0), None, None, None, C.byref(st), C.byref(ast)))
        return st, ast

    def adaptive_info(self, width, height, max_spp, tile_error, tile=0, min_spp=0, seed=1, band=None):
        """The held adaptive frame re-decided under tile_error and max_spp (pt_ctx_adaptive_info): pt_adaptive_info, all zeros
        if the context holds another adaptive frame or none."""
        cfg = self._config(width, height, max_spp, seed, "megakernel", band)
        par, out = pt_adaptive_params(tile_error, tile, min_spp), pt_adaptive_info()
        _check(lib().pt_ctx_adaptive_info(self._h, C.byref(cfg), C.byref(par), C.byref(out)))
        return out

    def adaptive_resolve(self, out_ptr, width, height, seed=1, band=None, spp_map=None, error=None, stream=None):
        """Write the image, and optionally the count and error maps, of the held adaptive frame (pt_ctx_adaptive_resolve)."""
        cfg = self._config(width, height, 1, seed, "megakernel", band)
        ptr = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        _check(lib().pt_ctx_adaptive_resolve(self._h, C.byref(cfg), C.c_void_p(out_ptr), ptr(spp_map), ptr(error),
                                             C.c_void_p(stream or 0)))

    def adaptive_reset(self):
        _check(lib().pt_ctx_adaptive_reset(self._h))

    def adaptive_save(self, path):
        _check(lib().pt_ctx_adaptive_save(self._h, os.fsencode(path)))

    def adaptive_load(self, path):
        """Continue from a checkpoint of adaptive_save; the scene it was rendered from must be set."""
        _check(lib().pt_ctx_adaptive_load(self._h, os.fsencode(path)))

    def accum_reset(self):
        _check(lib().pt_ctx_accum_reset(self._h))

    def accum_save(self, path):
        _check(lib().pt_ctx_accum_save(self._h, os.fsencode(path)))

    def accum_load(self, path):
        """Continue from a checkpoint of accum_save; the scene it was rendered from must be set."""
        _check(lib().pt_ctx_accum_load(self._h, os.fsencode(path)))

    def close(self):
        if self._h:
            lib().pt_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """pt_comm: the RCCL framebuffer gather behind the C ABI (include/ptrace.h).  `unique_id()` on rank 0, the 128
    bytes carried to the other ranks by the host's own means (bench.py: the torch.distributed store), then every rank
    constructs Comm(device, rank, world, id) collectively."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(Comm.ID_BYTES)
        _check(lib().pt_comm_unique_id(buf))
        return buf.raw

    def __init__(self, device, rank, world, ident):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        _check(lib().pt_comm_create(device, rank, world, C.create_string_buffer(ident, Comm.ID_BYTES), C.byref(self._h)))

    def gather_frame(self, local_ptr, frame_ptr, width, height, chunk_pixels, band=None, stream=None):
        """Every rank gets the whole band in device memory at frame_ptr (one ncclAllGather + the un-permute kernel)."""
        cfg = pt_config(width, height, 1, 0, 0, 0, 0, 0, 0)
        if band is not None:
            cfg.idx_begin, cfg.idx_end = band
        cfg.chunk_pixels = chunk_pixels
        _check(lib().pt_comm_gather_frame(self._h, C.byref(cfg), C.c_void_p(local_ptr), C.c_void_p(frame_ptr),
                                          C.c_void_p(stream or 0)))

    def close(self):
        if self._h:
            lib().pt_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_pfm(path, array):
    """A frame as a PFM file (pt_write_pfm): `array` is (height, width, 3) or (height, width) in framebuffer order (row
    i // width of index i); a 3-channel array gives "PF", a 1-channel one "Pf".  Placed over write_ppm's image pixel for
    pixel."""
    import numpy as np

    a = np.ascontiguousarray(array, dtype=np.float32)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0].copy()
    if a.ndim not in (2, 3):
        raise ValueError("write_pfm wants a (height, width[, channels]) array, not shape %r" % (a.shape,))
    channels = a.shape[2] if a.ndim == 3 else 1
    _check(lib().pt_write_pfm(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0], channels))


def write_ppm8(path, array):
    """8-bit pixels as a binary PPM (pt_write_ppm8): `array` is (height, width, 3) uint8 from the top-left pixel - what
    Context.present(rgb8=True) wrote, downloaded."""
    import numpy as np

    a = np.ascontiguousarray(array, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_ppm8 wants a (height, width, 3) array, not shape %r" % (a.shape,))
    _check(lib().pt_write_ppm8(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]))


def overlay_defaults(cam=None):
    """pt_ctx_overlay's defaults written out (pt_overlay_defaults): with a pt_camera the grid is sized for its distance."""
    p = pt_overlay_params()
    _check(lib().pt_overlay_defaults(C.byref(cam) if cam is not None else None, C.byref(p)))
    return p


def solid_defaults():
    """pt_ctx_solid's defaults written out (pt_solid_defaults): a headlight, ambient 0.1, diffuse 1, specular 0.5 at exponent 32."""
    p = pt_solid_params()
    _check(lib().pt_solid_defaults(C.byref(p)))
    return p


def solid_looks(objects):
    """pt_ctx_solid's looks table for a sequence (or ctypes array) of pt_object, one pt_solid_look each (pt_solid_look_of)."""
    arr = (pt_solid_look * len(objects))()
    for i, o in enumerate(objects):
        _check(lib().pt_solid_look_of(C.byref(o), C.byref(arr[i])))
    return arr


def despike_defaults():
    """pt_ctx_despike's defaults written out (pt_despike_defaults): radius 1, rank 3, no flags, threshold 2, floor 0.25."""
    p = pt_despike_params()
    _check(lib().pt_despike_defaults(C.byref(p)))
    return p


def despike_frame(rgb, width, height, params=None, object_id=None):
    """pt_ctx_despike's arithmetic for a whole frame on the host (pt_despike_frame_host): `rgb` a float32 array of pixels * 3
    values, `object_id` an int32 array of pixels.  Returns (out, mask, pt_despike_stats) with out and mask numpy arrays."""
    import numpy as np
    src = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1)
    ids = np.ascontiguousarray(object_id, dtype=np.int32).reshape(-1) if object_id is not None else None
    out, mask, st = np.zeros_like(src), np.zeros(width * height, dtype=np.uint8), pt_despike_stats()
    _check(lib().pt_despike_frame_host(width, height, C.byref(params) if params is not None else None, src.ctypes.data_as(C.c_void_p),
                                       ids.ctypes.data_as(C.c_void_p) if ids is not None else None, out.ctypes.data_as(C.c_void_p),
                                       mask.ctypes.data_as(C.c_void_p), C.byref(st)))
    return out.reshape(-1, 3), mask, st


def tonemap_defaults():
    """pt_ctx_tonemap's defaults written out (pt_tonemap_defaults): the ACES fit, no flags, exposure 1, white 4."""
    p = pt_tonemap_params()
    _check(lib().pt_tonemap_defaults(C.byref(p)))
    return p


def tonemap_pixel(rgb, params=None):
    """pt_ctx_tonemap's arithmetic for one pixel on the host (pt_tonemap_pixel_host): (r, g, b) -> (r, g, b)."""
    v, o = (C.c_float * 3)(*rgb), (C.c_float * 3)()
    _check(lib().pt_tonemap_pixel_host(C.byref(params) if params is not None else None, v, o))
    return tuple(o)


def meter_bin(luminance):
    """pt_ctx_meter's bin of one luminance (pt_meter_bin_host): 0..255, or -1 for a dark pixel."""
    b = C.c_int32()
    _check(lib().pt_meter_bin_host(luminance, C.byref(b)))
    return b.value


def meter_exposure_defaults():
    """pt_meter_exposure's defaults written out: key 0.18, the darkest 5 % and the brightest 2 % dropped, range [2^-8, 2^8]."""
    p = pt_meter_exposure_params()
    _check(lib().pt_meter_exposure_defaults(C.byref(p)))
    return p


def meter_exposure(stats, params=None):
    """The exposure that maps the log-average luminance of a pt_meter_stats (Context.meter) to the key (pt_meter_exposure)."""
    e = C.c_float()
    _check(lib().pt_meter_exposure(C.byref(stats), C.byref(params) if params is not None else None, C.byref(e)))
    return e.value


def meter_adapt(current, target, dt, tau):
    """One step of eye adaptation in log2 exposure from `current` towards `target` over dt with time constant tau (pt_meter_adapt)."""
    e = C.c_float()
    _check(lib().pt_meter_adapt(current, target, dt, tau, C.byref(e)))
    return e.value


def present_thresholds():
    """pt_ctx_present's table (pt_present_thresholds): 256 bit patterns, T[k] the smallest float that maps to at least k."""
    t = (C.c_uint32 * 256)()
    _check(lib().pt_present_thresholds(t))
    return list(t)


def present_quantize_host(values, exposure=0.0):
    """pt_ctx_present's per-value mapping on the host (pt_present_quantize_host): float32 values to bytes, same shape."""
    import numpy as np

    a = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(a.shape, dtype=np.uint8)
    _check(lib().pt_present_quantize_host(a.ctypes.data_as(C.POINTER(C.c_float)), a.size, exposure,
                                          out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def _camera(cam):
    """a pt_camera, a pointer to one, or a dict of its fields, as an argument for POINTER(pt_camera)"""
    if isinstance(cam, dict):
        return C.pointer(pt_camera(f3(*cam["position"]), f3(*cam["direction"]), cam["focal_length"], cam["sensor_width"],
                                   cam["aspect_ratio"]))
    return C.pointer(cam) if isinstance(cam, pt_camera) else cam


def scene_reach(scene, cam=None):
    """The box (lo, hi) Context.set_scene(scene) derives its bounds for - with `cam`, for that camera in place of the scene's own
    (pt_scene_reach: host only, no device)."""
    lo, hi = f3(), f3()
    _check(lib().pt_scene_reach(scene.camera if cam is None else _camera(cam), scene.objects, scene.n_objects, scene.triangles,
                                scene.n_triangles, lo, hi))
    return tuple(lo), tuple(hi)


def reproject_defaults():
    """The values pt_ctx_reproject uses for a zero field: {"weight", "max_history", "depth_tol", "normal_min"}
    (pt_reproject_defaults)."""
    p = pt_reproject_params()
    _check(lib().pt_reproject_defaults(C.byref(p)))
    return {"weight": p.weight, "max_history": p.max_history, "depth_tol": p.depth_tol, "normal_min": p.normal_min}


def reproject_var_defaults():
    """The values pt_ctx_reproject_var uses for a zero field: reproject_defaults()' four and {"min_frames", "radius"}
    (pt_reproject_var_defaults)."""
    p = pt_reproject_var_params()
    _check(lib().pt_reproject_var_defaults(C.byref(p)))
    return {"weight": p.weight, "max_history": p.max_history, "depth_tol": p.depth_tol, "normal_min": p.normal_min,
            "min_frames": p.min_frames, "radius": p.radius}


def upsample_defaults():
    """The values pt_ctx_upsample uses for a zero field: {"depth_tol", "normal_min"} (pt_upsample_defaults)."""
    p = pt_upsample_params()
    _check(lib().pt_upsample_defaults(C.byref(p)))
    return {"depth_tol": p.depth_tol, "normal_min": p.normal_min}


def upsample_tap_host(size, lo_size, coord):
    """Where the centre of pixel `coord` of an axis of `size` pixels lies among the centres of an axis of `lo_size` pixels
    (pt_upsample_tap_host, the host instantiation of the tap position the kernel compiles): (first, frac) - the taps are first
    and first + 1, with weights 1 - frac and frac."""
    first, frac = C.c_int32(), C.c_float()
    _check(lib().pt_upsample_tap_host(size, lo_size, coord, C.byref(first), C.byref(frac)))
    return first.value, frac.value


def _motion_table(motion):
    """a ctypes array of pt_object_motion (None when empty) from records or (ox, oy, oz, scale) tuples"""
    if not len(motion):
        return None
    arr = (pt_object_motion * len(motion))()
    for i, r in enumerate(motion):
        arr[i] = r if isinstance(r, pt_object_motion) else pt_object_motion((C.c_float * 3)(*r[:3]), r[3])
    return arr


def object_motion_between(now, before):
    """The motion record of one set_object() edit: where the surface point of `now` (a pt_object) was on `before`
    (pt_object_motion_between) - (0, 0, 0, 1) for equal geometry, scale 0 (the marker: no usable history) when the material or
    the kind changed."""
    r = pt_object_motion()
    _check(lib().pt_object_motion_between(C.byref(now), C.byref(before), C.byref(r)))
    return r


def reproject_project_host(cam, hist_cam, width, height, idx, depth):
    """Where the point pixel `idx` of `cam` sees at `depth` lies in hist_cam's frame (pt_reproject_project_host, the host
    instantiation of the kernel's projection): (px, pr, zexp) - column, row and expected history depth - or None when the point
    has no position there (behind the lens, outside the frame)."""
    out = [C.c_float() for _ in range(3)]
    rc = lib().pt_reproject_project_host(_camera(cam), _camera(hist_cam), width, height, idx, depth, *[C.byref(o) for o in out])
    if rc == 1:
        return None
    _check(rc)
    return tuple(o.value for o in out)


def denoise_defaults():
    """The values pt_ctx_denoise uses for a zero field: {"levels", "sigma_color", "sigma_depth"} (pt_denoise_defaults)."""
    p = pt_denoise_params()
    _check(lib().pt_denoise_defaults(C.byref(p)))
    return {"levels": p.levels, "sigma_color": p.sigma_color, "sigma_depth": p.sigma_depth}


def aov_defaults():
    """The parameters of a through-delta render_aov with every default written out: {"through_delta", "max_chain"}
    (pt_aov_defaults)."""
    p = pt_aov_params()
    _check(lib().pt_aov_defaults(C.byref(p)))
    return {"through_delta": bool(p.flags & PT_AOV_THROUGH_DELTA), "max_chain": p.max_chain}


def denoise_var_defaults():
    """The values pt_ctx_denoise_var uses for a zero field: {"levels", "sigma_var", "sigma_depth"} (pt_denoise_var_defaults)."""
    p = pt_denoise_var_params()
    _check(lib().pt_denoise_var_defaults(C.byref(p)))
    return {"levels": p.levels, "sigma_var": p.sigma_var, "sigma_depth": p.sigma_depth}


def build_flags():
    """The back-end (-mllvm) switches the library was built with (the Makefile drops the ones the compiler rejects)."""
    return lib().pt_build_flags().decode()


def kernel_isa_hash():
    """Hash of the device assembly the loaded library's kernels were built from (profiles name the one they measured)."""
    return lib().pt_kernel_isa_hash().decode()


# the -mllvm set the Makefile asks for (instruction placement only; worth 3.5 % on mesh.json): a library built without some of
# them - its compiler did not know them - still renders the same images
# (two sets, "general | flat: k_pass_cand without walks" - that kernel is a translation unit of its own, pt_kernels_flat.hip)
BUILD_FLAGS_WANTED = ("-amdgpu-sched-strategy=max-ilp", "-disable-machine-licm", "-disable-machine-sink")
BUILD_FLAGS_WANTED_FLAT = ("-amdgpu-sched-strategy=iterative-minreg", "-disable-machine-licm")


def build_flags_complete():
    general, _, flat = build_flags().partition("| flat:")
    return all(f in general for f in BUILD_FLAGS_WANTED) and all(f in flat for f in BUILD_FLAGS_WANTED_FLAT)


def image_hash(frame):
    """Image.hash (mod.rs:916-926) of a [pixels, 3] float32 torch tensor (any device): pt_image_hash over its bits."""
    host = frame.detach().to("cpu").contiguous()
    return int(lib().pt_image_hash(C.cast(host.data_ptr(), C.POINTER(C.c_float)), host.numel()))


def band_for_rank(npix, rank, world):
    """Contiguous band of framebuffer indices for `rank` of `world`: [rank*npix/world, (rank+1)*npix/world).
    idx = (H-1-y)*W + x is row-major (mod.rs:805-806), so a band is one contiguous slice of the image."""
    if not (0 <= rank < world):
        raise ValueError("rank outside world")
    return (npix * rank) // world, (npix * (rank + 1)) // world


def chunk_counts(npix, world, chunk_pixels):
    """Pixels owned by each rank under the interleaved partition (chunk c belongs to rank c % world), by arithmetic."""
    n_chunks = (npix + chunk_pixels - 1) // chunk_pixels
    last = npix - (n_chunks - 1) * chunk_pixels  # pixels of the last (possibly short) chunk
    counts = []
    for r in range(world):
        mine = (n_chunks - r + world - 1) // world if n_chunks > r else 0
        c = mine * chunk_pixels
        if mine and (n_chunks - 1) % world == r:
            c -= chunk_pixels - last
        counts.append(c)
    return counts


def chunk_owner_map(npix, world, chunk_pixels):
    """Interleaved partition spelled out: chunk c (chunk_pixels consecutive framebuffer indices) belongs to rank
    c % world.  Returns (counts, index) with index[r] = the framebuffer indices of rank r's pixels in the order
    pt_ctx_render writes them.  O(npix * world): the explicit form the tests hold the arithmetic against."""
    import torch
    idx = torch.arange(npix, dtype=torch.int64)
    owner = (idx // chunk_pixels) % world
    index = [idx[owner == r] for r in range(world)]
    return [int(i.numel()) for i in index], index


def gather_chunks(local, npix, rank, world, chunk_pixels, dist=None, force_collective=False):
    """One all-gather of the per-rank chunk buffers ([owned pixels, 3]) and the permutation back to framebuffer
    order.  Equal shares (npix a multiple of world*chunk_pixels) use all_gather_into_tensor + a strided view copy;
    ragged shares pad every rank to whole chunks and copy rank r's chunks to the frame's chunks r, r+world, ...
    (one strided copy per rank: O(npix) bytes, no index tensors).  world == 1 is the identity unless
    force_collective asks for the collective anyway (hardware check of the RCCL path on a one-GPU box)."""
    import torch
    if world == 1 and not force_collective:
        return local
    if dist is None:
        import torch.distributed as dist
    counts = chunk_counts(npix, world, chunk_pixels)
    assert local.shape[0] == counts[rank]
    if len(set(counts)) == 1 and npix % (world * chunk_pixels) == 0:
        flat = torch.empty((npix, 3), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(flat, local.contiguous())
        rounds = npix // (world * chunk_pixels)
        # flat is [rank][round][chunk_pixels]; the frame is [round][rank][chunk_pixels]
        return flat.view(world, rounds, chunk_pixels, 3).permute(1, 0, 2, 3).reshape(npix, 3)
    n_chunks = (npix + chunk_pixels - 1) // chunk_pixels
    per_rank = [len(range(r, n_chunks, world)) for r in range(world)]  # chunks of each rank (the last may be short)
    m = max(per_rank) * chunk_pixels
    padded = torch.zeros((m, 3), dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    frame = torch.empty((n_chunks, chunk_pixels, 3), dtype=local.dtype, device=local.device)
    for r in range(world):
        if per_rank[r]:
            frame[r::world] = parts[r][: per_rank[r] * chunk_pixels].view(per_rank[r], chunk_pixels, 3)
    return frame.view(n_chunks * chunk_pixels, 3)[:npix]


def gather_bands(local, npix, rank, world, dist=None):
    """All-gather the per-rank bands (torch tensors of shape [band_pixels, 3]) into the full [npix, 3] image.
    One collective: all_gather_into_tensor when the bands are equal, all_gather on padded bands otherwise."""
    import torch
    if world == 1:
        return local
    if dist is None:
        import torch.distributed as dist
    sizes = [band_for_rank(npix, r, world)[1] - band_for_rank(npix, r, world)[0] for r in range(world)]
    if len(set(sizes)) == 1:
        full = torch.empty((npix, 3), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(full, local.contiguous())
        return full
    m = max(sizes)
    padded = torch.zeros((m, 3), dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    return torch.cat([parts[r][: sizes[r]] for r in range(world)], dim=0)
