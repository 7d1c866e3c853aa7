"""include/ptrace_tone.h (pt_ctx_accum_hdr, pt_ctx_meter, pt_ctx_tonemap) as ctypes: to that header what solid_abi.py is to
include/ptrace_solid.h - the four structs and the constants under the header's names and one SIGNATURES entry per function it
declares, typed by abi.py's rules.  abi.declare() gives these functions their prototypes together with ptrace.h's, so a library
loaded through abi.load() has them.  A module of its own because the header is one: tests/test_abi.py holds abi.py to ptrace.h
struct for struct; tests/test_tone_abi.py holds this module to ptrace_tone.h the same way, the C compiler's layout included."""
from ctypes import POINTER as P
from ctypes import Structure, c_double, c_float, c_int, c_int32, c_uint32, c_uint64, c_void_p

from .abi import pt_config

vp = c_void_p

PT_METER_SKIP_MISSES = 1
PT_METER_BINS = 256
PT_TONE_CLAMP, PT_TONE_REINHARD, PT_TONE_ACES = 0, 1, 2
PT_TONE_LUMA = 1


class pt_meter_params(Structure):
    _fields_ = [("flags", c_uint32), ("x0", c_uint32), ("y0", c_uint32), ("x1", c_uint32), ("y1", c_uint32)]


class pt_meter_stats(Structure):
    _fields_ = [("pixels", c_uint64), ("dark", c_uint64), ("histogram", c_uint32 * PT_METER_BINS), ("max_luminance", c_float)]


class pt_meter_exposure_params(Structure):
    _fields_ = [("key", c_float), ("low_fraction", c_float), ("high_fraction", c_float), ("min_exposure", c_float),
                ("max_exposure", c_float)]


class pt_tonemap_params(Structure):
    _fields_ = [("curve", c_uint32), ("flags", c_uint32), ("exposure", c_float), ("white", c_float)]


SIGNATURES = {
    "pt_ctx_accum_hdr": (c_int, [vp, P(pt_config), vp, vp]),
    "pt_ctx_meter": (c_int, [vp, c_uint32, c_uint32, P(pt_meter_params), vp, vp, P(pt_meter_stats), vp]),
    "pt_meter_bin_host": (c_int, [c_float, P(c_int32)]),
    "pt_meter_exposure_defaults": (c_int, [P(pt_meter_exposure_params)]),
    "pt_meter_exposure": (c_int, [P(pt_meter_stats), P(pt_meter_exposure_params), P(c_float)]),
    "pt_meter_exposure_weights": (c_int, [P(pt_meter_stats), P(pt_meter_exposure_params), P(c_double)]),
    "pt_meter_adapt": (c_int, [c_float, c_float, c_float, c_float, P(c_float)]),
    "pt_tonemap_defaults": (c_int, [P(pt_tonemap_params)]),
    "pt_ctx_tonemap": (c_int, [vp, c_uint32, c_uint32, P(pt_tonemap_params), vp, vp, vp]),
    "pt_tonemap_pixel_host": (c_int, [P(pt_tonemap_params), P(c_float), P(c_float)]),
}
