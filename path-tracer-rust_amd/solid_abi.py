"""include/ptrace_solid.h (pt_ctx_solid) as ctypes: to that header what overlay_abi.py is to include/ptrace_overlay.h - the two
structs and the constants under the header's names and one SIGNATURES entry per function it declares, typed by abi.py's rules.
abi.declare() gives these functions their prototypes together with ptrace.h's, so a library loaded through abi.load() has them.
A module of its own because the header is one: tests/test_abi.py holds abi.py to ptrace.h struct for struct;
tests/test_solid_abi.py holds this module to ptrace_solid.h the same way, the C compiler's layout included."""
from ctypes import POINTER as P
from ctypes import Structure, c_float, c_int, c_int32, c_uint32, c_void_p

from .abi import f3, pt_camera, pt_object

vp = c_void_p


class pt_solid_params(Structure):
    _fields_ = [("flags", c_uint32), ("light", f3), ("ambient", c_float), ("diffuse", c_float), ("specular", c_float),
                ("shininess_log2", c_uint32), ("background", f3), ("sky_top", f3), ("sky_bottom", f3)]


class pt_solid_look(Structure):
    _fields_ = [("emission", f3), ("reflect_type", c_uint32)]


PT_SOLID_HEADLIGHT, PT_SOLID_REFLECT_SKY = 1, 2
PT_SOLID_MAX_SHININESS_LOG2 = 10

SIGNATURES = {
    "pt_solid_defaults": (c_int, [P(pt_solid_params)]),
    "pt_solid_look_of": (c_int, [P(pt_object), P(pt_solid_look)]),
    "pt_ctx_solid": (c_int, [vp, c_uint32, c_uint32, P(pt_solid_params), P(pt_camera), vp, vp, vp, vp, P(pt_solid_look), c_uint32, vp, vp]),
    "pt_solid_pixel_host": (c_int, [P(pt_camera), c_uint32, c_uint32, P(pt_solid_params), c_uint32, c_int32, c_float, P(c_float),
                                    P(c_float), P(pt_solid_look), P(c_float)]),
}
