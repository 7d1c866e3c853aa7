"""include/ptrace_overlay.h (pt_ctx_overlay) as ctypes: to that header what abi.py is to include/ptrace.h - the struct and the
constants under the header's names and one SIGNATURES entry per function it declares, typed by abi.py's rules.  abi.declare() gives
these functions their prototypes together with ptrace.h's, so a library loaded through abi.load() has them.  A module of its own
because the header is one: tests/test_abi.py holds abi.py to ptrace.h struct for struct; tests/test_overlay_abi.py holds this
module to ptrace_overlay.h the same way, the C compiler's layout included."""
from ctypes import POINTER as P
from ctypes import Structure, c_float, c_int, c_int32, c_uint32, c_void_p

from .abi import f3, pt_camera

vp = c_void_p


class pt_overlay_params(Structure):
    _fields_ = [("flags", c_uint32), ("n_selected", c_uint32), ("selected", c_int32 * 16), ("radius", c_uint32),
                ("outline_color", f3), ("outline_alpha", c_float), ("fill_color", f3), ("fill_alpha", c_float), ("sky_top", f3),
                ("sky_bottom", f3), ("grid_color", f3), ("grid_alpha", c_float), ("grid_y", c_float), ("grid_spacing", c_float),
                ("grid_half_width", c_float), ("grid_extent", c_float)]


PT_OVERLAY_SKY, PT_OVERLAY_GRID = 1, 2
PT_OVERLAY_MAX_SELECTED, PT_OVERLAY_MAX_RADIUS = 16, 8

SIGNATURES = {
    "pt_overlay_defaults": (c_int, [P(pt_camera), P(pt_overlay_params)]),
    "pt_ctx_overlay": (c_int, [vp, c_uint32, c_uint32, P(pt_overlay_params), P(pt_camera), vp, vp, vp, vp]),
    "pt_overlay_pixel_host": (c_int, [P(pt_camera), c_uint32, c_uint32, P(pt_overlay_params), c_uint32, c_int32, c_float, c_int, c_int,
                                      P(c_float), P(c_float)]),
}
