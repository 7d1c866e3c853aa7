"""The C ABI of libptrace_hip.so (include/ptrace.h) as ctypes: the one place that describes the header to Python.

Structs and constants carry the header's names; SIGNATURES has one entry per function the header declares.  Everything
else in the tree - the package's wrappers, tests/ptlib.py, the scripts under tools/ - loads the library through load() and
takes its struct classes from here; tests/test_abi.py checks this file against the header and against the C compiler.

How a parameter is typed: a struct pointer is POINTER(struct); a string is c_char_p; a device buffer, a stream, a callback or
an opaque handle (pt_ctx, pt_scene, pt_comm) is c_void_p, which takes ints, None, arrays, byref() and function pointers; a
host array or out-parameter of fixed element type is POINTER(elem) where every caller passes that, else c_void_p.
"""
from ctypes import (CDLL, CFUNCTYPE, POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_uint32,
                    c_uint64, c_ulonglong, c_void_p)

f3 = c_float * 3
pt_progress_fn = CFUNCTYPE(None, c_void_p, c_float)


# ------------------------------------------------------------------------------------------------ structs
class pt_camera(Structure):
    _fields_ = [("position", f3), ("direction", f3), ("focal_length", c_float), ("sensor_width", c_float),
                ("aspect_ratio", c_float)]


class pt_triangle(Structure):
    _fields_ = [("a", f3), ("b", f3), ("c", f3)]


class pt_object(Structure):
    _fields_ = [("kind", c_uint32), ("position", f3), ("radius", c_float), ("color", f3), ("emission", f3),
                ("reflect_type", c_uint32), ("tri_offset", c_uint32), ("tri_count", c_uint32), ("bs_center", f3),
                ("bs_radius", c_float)]


class pt_config(Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("spp", c_uint32), ("backend", c_uint32), ("seed", c_uint64),
                ("idx_begin", c_uint32), ("idx_end", c_uint32), ("rays_per_pass", c_uint32), ("flags", c_uint32),
                ("chunk_pixels", c_uint32), ("chunk_first", c_uint32), ("chunk_step", c_uint32), ("progress_ms", c_uint32)]


class pt_stats(Structure):
    _fields_ = [("ray_bounces", c_uint64), ("samples", c_uint64), ("intersect_rays", c_uint64),
                ("intersect_launches", c_uint32), ("passes", c_uint32), ("ms_total", c_double), ("ms_device", c_double),
                ("ms_intersect", c_double)]


class pt_scatter_item(Structure):
    _fields_ = [("o", f3), ("d", f3), ("thr", f3), ("pixel", c_uint32), ("sample", c_uint32), ("depth", c_uint32),
                ("branch", c_uint32)]


class pt_scatter_surface(Structure):
    _fields_ = [("x", f3), ("n", f3), ("color", f3), ("emission", f3), ("reflect", c_uint32)]


class pt_scatter_out(Structure):
    _fields_ = [("hit", c_int32), ("n_rays", c_uint32), ("emits", c_uint32), ("deferred", c_uint32), ("x", f3), ("contrib", f3),
                ("d0", f3), ("thr0", f3), ("d1", f3), ("thr1", f3), ("depth0", c_uint32), ("branch0", c_uint32),
                ("depth1", c_uint32), ("branch1", c_uint32)]


class pt_noise_stats(Structure):
    _fields_ = [("spp_min", c_uint32), ("spp_max", c_uint32), ("spp_a_min", c_uint32), ("spp_b_min", c_uint32),
                ("pixels", c_uint64), ("mean_error", c_double), ("histogram", c_uint32 * 64)]


class pt_noise_target(Structure):
    _fields_ = [("mean_error", c_float), ("quantile", c_float), ("quantile_error", c_float), ("min_spp", c_uint32)]


class pt_adaptive_params(Structure):
    _fields_ = [("tile_error", c_float), ("tile", c_uint32), ("min_spp", c_uint32)]


class pt_adaptive_stats(Structure):
    _fields_ = [("tiles", c_uint32), ("tiles_open", c_uint32), ("levels", c_uint32), ("level_spp", c_uint32 * 32),
                ("tiles_closed", c_uint32 * 32), ("samples", c_uint64), ("mean_error", c_double)]


class pt_adaptive_info(Structure):
    _fields_ = [("tiles", c_uint32), ("tiles_open", c_uint32), ("tiles_at_cap", c_uint32), ("spp_min", c_uint32),
                ("spp_max", c_uint32), ("samples", c_uint64), ("mean_error", c_double)]


class pt_aov_params(Structure):
    _fields_ = [("flags", c_uint32), ("max_chain", c_uint32)]


class pt_denoise_params(Structure):
    _fields_ = [("levels", c_uint32), ("sigma_color", c_float), ("sigma_normal_pow", c_float), ("sigma_depth", c_float),
                ("flags", c_uint32)]


class pt_denoise_var_params(Structure):
    _fields_ = [("levels", c_uint32), ("sigma_var", c_float), ("sigma_depth", c_float), ("flags", c_uint32)]


class pt_present_params(Structure):
    _fields_ = [("out_width", c_uint32), ("out_height", c_uint32), ("exposure", c_float), ("format", c_uint32),
                ("flags", c_uint32)]


class pt_reproject_params(Structure):
    _fields_ = [("weight", c_uint32), ("max_history", c_float), ("depth_tol", c_float), ("normal_min", c_float),
                ("flags", c_uint32)]


class pt_reproject_var_params(Structure):
    _fields_ = [("weight", c_uint32), ("max_history", c_float), ("depth_tol", c_float), ("normal_min", c_float),
                ("min_frames", c_uint32), ("radius", c_uint32), ("flags", c_uint32)]


class pt_object_motion(Structure):
    _fields_ = [("offset", f3), ("scale", c_float)]


class pt_upsample_params(Structure):
    _fields_ = [("depth_tol", c_float), ("normal_min", c_float), ("flags", c_uint32)]


class pt_select_params(Structure):
    _fields_ = [("weight_max", c_float), ("len_max", c_float), ("flags", c_uint32)]


# ------------------------------------------------------------------------------------------------ constants
PT_ABI_VERSION = 5
PT_OK, PT_ERR_INVALID, PT_ERR_NO_DEVICE, PT_ERR_HIP, PT_CANCELLED = 0, -1, -2, -3, -4
PT_ERR_OVERFLOW, PT_ERR_IO, PT_ERR_PARSE, PT_ERR_COMM = -5, -6, -7, -8
PT_DIFFUSE, PT_SPECULAR, PT_REFRACT = 0, 1, 2
PT_SPHERE, PT_MESH = 0, 1
PT_BACKEND_WAVEFRONT, PT_BACKEND_MEGAKERNEL = 0, 1
PT_FLAG_NO_BVH, PT_FLAG_SEPARATE_KERNELS = 1, 2
PT_PROGRESS_EVERY_PASS = 0xffffffff
PT_SCATTER_GIVEN, PT_SCATTER_BY_ID, PT_SCATTER_BY_RANK = 0, 1, 2
PT_SCATTER_DEFER_REFRACT, PT_SCATTER_REFRACT_ONLY = 0x10, 0x20
PT_SCATTER_NOT_SHADED = -2
PT_AOV_THROUGH_DELTA, PT_AOV_MAX_CHAIN = 1, 16
PT_DENOISE_NO_DEMODULATE = 1
PT_PRESENT_RGBA8, PT_PRESENT_RGB8 = 0, 1
PT_PRESENT_FRAMEBUFFER_ORDER = 1
PT_COMM_ID_BYTES = 128
PT_LOAD_TRIANGULATE = 1


def PT_FLAG_PIPELINES(n):
    return (n & 15) << 8


# the device tables of a scene, by their PT_TABLE_* index (pt_ctx_table_hashes)
TABLE_NAMES = ("objs", "obj_pairs", "tri_pairs", "mats", "tri_shade", "bvh_nodes", "bvh_nodes4", "sph_pairs", "flat_pairs", "cand_pairs",
               "rank_id", "surf", "tri_rank", "bvh_meshes")
(PT_TABLE_OBJS, PT_TABLE_OBJ_PAIRS, PT_TABLE_TRI_PAIRS, PT_TABLE_MATS, PT_TABLE_TRI_SHADE, PT_TABLE_BVH_NODES, PT_TABLE_BVH_NODES4,
 PT_TABLE_SPH_PAIRS, PT_TABLE_FLAT_PAIRS, PT_TABLE_CAND_PAIRS, PT_TABLE_RANK_ID, PT_TABLE_SURF, PT_TABLE_TRI_RANK, PT_TABLE_BVH_MESHES,
 PT_TABLE_COUNT) = range(15)

# ------------------------------------------------------------------------------------------------ signatures
P, vp = POINTER, c_void_p
SIGNATURES = {  # name: (restype, argtypes), in the header's order
    "pt_version": (c_char_p, []),
    "pt_build_flags": (c_char_p, []),
    "pt_kernel_isa_hash": (c_char_p, []),
    "pt_last_error": (c_char_p, []),
    "pt_abi_version": (c_int, []),
    "pt_device_count": (c_int, []),
    "pt_camera_basis": (c_int, [P(pt_camera), P(c_float), P(c_float), P(c_float)]),
    "pt_mesh_bounding_sphere": (c_int, [P(pt_triangle), c_uint32, P(c_float), P(c_float)]),
    "pt_ctx_create": (c_int, [c_int, P(vp)]),
    "pt_ctx_destroy": (None, [vp]),
    "pt_ctx_set_scene": (c_int, [vp, P(pt_camera), P(pt_object), c_uint32, P(pt_triangle), c_uint32]),
    "pt_ctx_set_camera": (c_int, [vp, P(pt_camera), P(c_int)]),
    "pt_ctx_camera_reach": (c_int, [vp, P(c_float), P(c_float)]),
    "pt_ctx_reserve_camera_reach": (c_int, [vp, P(c_float), P(c_float), P(c_int)]),
    "pt_scene_reach": (c_int, [P(pt_camera), P(pt_object), c_uint32, P(pt_triangle), c_uint32, P(c_float), P(c_float)]),
    "pt_ctx_set_object": (c_int, [vp, c_uint32, P(pt_object), P(c_int)]),
    "pt_ctx_table_hashes": (c_int, [vp, P(c_uint64)]),
    "pt_config_pixels": (c_uint32, [P(pt_config)]),
    "pt_ctx_render": (c_int, [vp, P(pt_config), vp, vp, vp, vp, vp, P(pt_stats)]),
    "pt_device_malloc": (c_int, [c_int, c_size_t, P(vp)]),
    "pt_device_free": (c_int, [c_int, vp]),
    "pt_device_download": (c_int, [c_int, vp, vp, c_size_t]),
    "pt_bvh_refs_fit": (c_int, [c_uint64, c_uint64]),
    "pt_ctx_set_memory_budget": (c_int, [vp, c_size_t]),
    "pt_ctx_set_profiling": (c_int, [vp, c_int]),
    "pt_ctx_pass_kernel": (c_char_p, [vp, c_uint32]),
    "pt_ctx_radiance": (c_int, [vp, P(c_float), P(c_float), c_uint32, c_uint32, c_uint64, c_uint32, c_uint32, c_uint32,
        P(c_float), P(pt_stats)]),
    "pt_ctx_intersect": (c_int, [vp, P(c_float), P(c_float), c_uint32, P(c_float), P(c_int32), P(c_int32), P(c_float),
        P(c_float)]),
    "pt_ctx_intersect_streams": (c_int, [vp, P(c_float), P(c_float), c_uint32, c_uint32, P(c_float), P(c_int32)]),
    "pt_ctx_intersect_bounds": (c_int, [vp, c_uint32, P(c_float), P(c_float), c_uint32, P(c_int32), P(c_float), P(c_float),
        P(c_float)]),
    "pt_ctx_orbit_point": (c_int, [vp, P(c_float), P(c_float), c_uint32, P(c_int32), P(c_float), P(c_int32), P(c_float)]),
    "pt_ctx_set_mesh_bounds": (c_int, [vp, c_uint32, P(pt_triangle)]),
    "pt_mesh_bounding_box": (c_int, [P(pt_triangle), c_uint32, P(pt_triangle)]),
    "pt_ctx_numerics_probe": (c_int, [vp, P(c_float), c_uint32, P(c_float), P(c_float), P(c_float), P(c_float), P(c_uint32)]),
    "pt_ctx_numerics_sweep": (c_int, [vp, P(c_uint64)]),
    "pt_ctx_sincos_sweep": (c_int, [vp, P(c_uint64)]),
    "pt_ctx_primary_rays": (c_int, [vp, c_uint32, c_uint32, c_uint64, P(c_uint32), P(c_uint32), c_uint32, c_uint32, P(c_float),
        P(c_float)]),
    "pt_ctx_scatter": (c_int, [vp, c_uint64, c_uint32, P(pt_scatter_item), P(pt_scatter_surface), c_uint32, P(pt_scatter_out)]),
    "pt_host_sincos": (None, [c_float, P(c_float), P(c_float)]),
    "pt_render": (c_int, [P(pt_config), P(pt_camera), P(pt_object), c_uint32, P(pt_triangle), c_uint32, P(c_float), vp, vp, vp,
        P(pt_stats)]),
    "pt_render_multi": (c_int, [P(pt_config), c_uint32, P(pt_camera), P(pt_object), c_uint32, P(pt_triangle), c_uint32,
        P(c_float), vp, vp, vp, P(pt_stats)]),
    "pt_ctx_snapshot": (c_int, [vp, vp, P(c_uint32)]),
    "pt_ctx_accumulate": (c_int, [vp, P(pt_config), vp, vp, vp, vp, vp, P(pt_stats)]),
    "pt_ctx_accum_info": (c_int, [vp, P(pt_config), P(c_uint32), P(c_uint32)]),
    "pt_ctx_accum_reset": (c_int, [vp]),
    "pt_ctx_accum_save": (c_int, [vp, c_char_p]),
    "pt_ctx_accum_load": (c_int, [vp, c_char_p]),
    "pt_ctx_accum_track_noise": (c_int, [vp, c_int]),
    "pt_ctx_accum_noise": (c_int, [vp, P(pt_config), vp, P(pt_noise_stats), vp]),
    "pt_ctx_accumulate_until": (c_int, [vp, P(pt_config), P(pt_noise_target), vp, vp, vp, vp, vp, P(pt_stats),
        P(pt_noise_stats)]),
    "pt_ctx_render_adaptive": (c_int, [vp, P(pt_config), P(pt_adaptive_params), vp, vp, vp, vp, vp, vp, vp, P(pt_stats),
        P(pt_adaptive_stats)]),
    "pt_ctx_accumulate_adaptive": (c_int, [vp, P(pt_config), P(pt_adaptive_params), vp, vp, vp, vp, vp, vp, vp, P(pt_stats),
        P(pt_adaptive_stats)]),
    "pt_ctx_adaptive_info": (c_int, [vp, P(pt_config), P(pt_adaptive_params), P(pt_adaptive_info)]),
    "pt_ctx_adaptive_resolve": (c_int, [vp, P(pt_config), vp, vp, vp, vp]),
    "pt_ctx_adaptive_reset": (c_int, [vp]),
    "pt_ctx_adaptive_save": (c_int, [vp, c_char_p]),
    "pt_ctx_adaptive_load": (c_int, [vp, c_char_p]),
    "pt_ctx_render_aov": (c_int, [vp, P(pt_config), vp, vp, vp, vp, vp]),
    "pt_aov_defaults": (c_int, [P(pt_aov_params)]),
    "pt_ctx_render_aov_ex": (c_int, [vp, P(pt_config), P(pt_aov_params), vp, vp, vp, vp, vp, vp]),
    "pt_denoise_defaults": (c_int, [P(pt_denoise_params)]),
    "pt_ctx_denoise": (c_int, [vp, c_uint32, c_uint32, P(pt_denoise_params), vp, vp, vp, vp, vp, vp]),
    "pt_denoise_var_defaults": (c_int, [P(pt_denoise_var_params)]),
    "pt_ctx_denoise_var": (c_int, [vp, c_uint32, c_uint32, P(pt_denoise_var_params), vp, vp, vp, vp, vp, vp, vp]),
    "pt_ctx_present": (c_int, [vp, c_uint32, c_uint32, P(pt_present_params), vp, vp, vp]),
    "pt_present_thresholds": (c_int, [P(c_uint32)]),
    "pt_present_quantize_host": (c_int, [vp, c_size_t, c_float, vp]),
    "pt_write_ppm8": (c_int, [c_char_p, vp, c_uint32, c_uint32]),
    "pt_reproject_defaults": (c_int, [P(pt_reproject_params)]),
    "pt_ctx_reproject": (c_int, [vp, c_uint32, c_uint32, P(pt_reproject_params), P(pt_camera), vp, vp, vp, vp, P(pt_camera), vp,
        vp, vp, vp, vp, vp, vp, vp]),
    "pt_reproject_project_host": (c_int, [P(pt_camera), P(pt_camera), c_uint32, c_uint32, c_uint32, c_float, P(c_float),
        P(c_float), P(c_float)]),
    "pt_reproject_var_defaults": (c_int, [P(pt_reproject_var_params)]),
    "pt_ctx_reproject_var": (c_int, [vp, c_uint32, c_uint32, P(pt_reproject_var_params), P(pt_camera), vp, vp, vp, vp,
        P(pt_camera), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pt_object_motion_between": (c_int, [P(pt_object), P(pt_object), P(pt_object_motion)]),
    "pt_ctx_reproject_moved": (c_int, [vp, c_uint32, c_uint32, P(pt_reproject_params), P(pt_camera), vp, vp, vp, vp,
        P(pt_camera), vp, vp, vp, vp, vp, vp, vp, P(pt_object_motion), c_uint32, vp]),
    "pt_ctx_reproject_var_moved": (c_int, [vp, c_uint32, c_uint32, P(pt_reproject_var_params), P(pt_camera), vp, vp, vp, vp,
        P(pt_camera), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, P(pt_object_motion), c_uint32, vp]),
    "pt_reproject_project_moved_host": (c_int, [P(pt_camera), P(pt_camera), c_uint32, c_uint32, c_uint32, c_float,
        P(pt_object_motion), P(c_float), P(c_float), P(c_float)]),
    "pt_upsample_defaults": (c_int, [P(pt_upsample_params)]),
    "pt_ctx_upsample": (c_int, [vp, c_uint32, c_uint32, c_uint32, c_uint32, P(pt_upsample_params), vp, vp, vp, vp, vp, vp, vp,
        vp, vp, vp, vp, vp]),
    "pt_upsample_tap_host": (c_int, [c_uint32, c_uint32, c_uint32, P(c_int32), P(c_float)]),
    "pt_ctx_select_pixels": (c_int, [vp, c_uint32, c_uint32, P(pt_select_params), vp, vp, vp, P(c_uint32), vp]),
    "pt_ctx_render_masked": (c_int, [vp, P(pt_config), vp, vp, vp, vp, P(pt_stats), P(c_uint32)]),
    "pt_ctx_reproject_var_weighted": (c_int, [vp, c_uint32, c_uint32, P(pt_reproject_var_params), P(pt_camera), vp, vp, vp, vp, vp,
        P(pt_camera), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, P(pt_object_motion), c_uint32, vp]),
    "pt_ctx_spp_plane": (c_int, [vp, c_uint32, c_uint32, c_uint32, vp, c_uint32, vp, vp]),
    "pt_comm_unique_id": (c_int, [c_char_p]),
    "pt_comm_create": (c_int, [c_int, c_int, c_int, c_char_p, P(vp)]),
    "pt_comm_destroy": (None, [vp]),
    "pt_comm_gather_frame": (c_int, [vp, P(pt_config), vp, vp, vp]),
    "pt_image_hash": (c_uint64, [P(c_float), c_size_t]),
    "pt_siphash": (c_uint64, [c_uint32, c_uint32, c_uint64, c_uint64, c_char_p, c_size_t]),
    "pt_scene_load": (c_int, [c_char_p, c_char_p, P(vp)]),
    "pt_scene_load_ex": (c_int, [c_char_p, c_char_p, c_uint32, P(vp)]),
    "pt_scene_save": (c_int, [vp, c_char_p]),
    "pt_scene_set_camera": (c_int, [vp, P(pt_camera)]),
    "pt_builtin_scene_count": (c_uint32, []),
    "pt_builtin_scene_id": (c_char_p, [c_uint32]),
    "pt_scene_builtin": (c_int, [c_char_p, c_char_p, P(vp)]),
    "pt_scene_free": (None, [vp]),
    "pt_scene_id": (c_char_p, [vp]),
    "pt_scene_camera": (P(pt_camera), [vp]),
    "pt_scene_objects": (P(pt_object), [vp, P(c_uint32)]),
    "pt_scene_triangles": (P(pt_triangle), [vp, P(c_uint32)]),
    "pt_scene_bounding_box": (P(pt_triangle), [vp, c_uint32]),
    "pt_load_off": (c_int, [c_char_p, c_float, P(P(pt_triangle)), P(c_uint32)]),
    "pt_load_off_ex": (c_int, [c_char_p, c_float, c_uint32, P(P(pt_triangle)), P(c_uint32)]),
    "pt_free": (None, [vp]),
    "pt_gamma_correction": (c_float, [c_float]),
    "pt_to_int_with_gamma_correction": (c_uint32, [c_float]),
    "pt_write_ppm": (c_int, [c_char_p, vp, c_uint32, c_uint32, c_uint32, c_char_p, c_uint64]),
    "pt_write_pfm": (c_int, [c_char_p, vp, c_uint32, c_uint32, c_uint32]),
}
# what the diagnostic builds of the Makefile export on top (walk, phases, tail, ranges); declared where a library has them
DEBUG_SIGNATURES = {
    "pt_debug_walk_stats": (c_int, [vp, P(c_ulonglong)]),
    "pt_debug_phase_stats": (c_int, [vp, P(c_ulonglong), c_uint32]),
    "pt_debug_tail_stats": (c_int, [vp, vp, c_uint32]),
    "pt_debug_range_stats_flat": (c_int, [P(c_ulonglong), c_uint32]),
    "pt_debug_range_stats_tile": (c_int, [P(c_ulonglong), c_uint32]),
    "pt_debug_range_stats_main": (c_int, [P(c_ulonglong), c_uint32]),
}


def declare(cdll, partial=False):
    """Give every function of SIGNATURES its restype and argtypes on a loaded library and return the library.
    A symbol the library lacks raises, naming all that are missing; partial=True skips them (a library built from an
    older header)."""
    from . import overlay_abi  # include/ptrace_overlay.h: a header of its own has a table of its own (imported here: it imports this module)
    from . import solid_abi  # include/ptrace_solid.h: likewise
    from . import tone_abi  # include/ptrace_tone.h: likewise
    from . import despike_abi  # include/ptrace_despike.h: likewise

    missing = []
    for table in (SIGNATURES, overlay_abi.SIGNATURES, solid_abi.SIGNATURES, tone_abi.SIGNATURES, despike_abi.SIGNATURES, DEBUG_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            try:
                fn = getattr(cdll, name)
            except AttributeError:
                if table is not DEBUG_SIGNATURES:
                    missing.append(name)
                continue
            fn.restype, fn.argtypes = restype, argtypes
    if missing and not partial:
        raise AttributeError("%s does not export %s" % (cdll._name, ", ".join(missing)))
    return cdll


def load(path):
    return declare(CDLL(path))
