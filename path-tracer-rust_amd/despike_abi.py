"""include/ptrace_despike.h (pt_ctx_despike) as ctypes: to that header what tone_abi.py is to include/ptrace_tone.h - the two
structs and the constant under the header's names and one SIGNATURES entry per function it declares, typed by abi.py's rules.
abi.declare() gives these functions their prototypes together with ptrace.h's, so a library loaded through abi.load() has them.
A module of its own because the header is one: tests/test_abi.py holds abi.py to ptrace.h struct for struct;
tests/test_despike_abi.py holds this module to ptrace_despike.h the same way, the C compiler's layout included."""
from ctypes import POINTER as P
from ctypes import Structure, c_float, c_int, c_uint32, c_uint64, c_void_p

vp = c_void_p

PT_DESPIKE_SAME_OBJECT = 1


class pt_despike_params(Structure):
    _fields_ = [("radius", c_uint32), ("rank", c_uint32), ("flags", c_uint32), ("threshold", c_float), ("floor", c_float)]


class pt_despike_stats(Structure):
    _fields_ = [("pixels", c_uint64), ("spikes", c_uint64), ("nonfinite", c_uint64)]


SIGNATURES = {
    "pt_despike_defaults": (c_int, [P(pt_despike_params)]),
    "pt_ctx_despike": (c_int, [vp, c_uint32, c_uint32, P(pt_despike_params), vp, vp, vp, vp, P(pt_despike_stats), vp]),
    "pt_despike_frame_host": (c_int, [c_uint32, c_uint32, P(pt_despike_params), vp, vp, vp, vp, P(pt_despike_stats)]),
}
