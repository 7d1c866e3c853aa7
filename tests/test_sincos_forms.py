"""csrc/pt_math.h's sincos_f32 is a fused form of glibc's sinf / cosf: every a + b * c one fma, the quadrant's sign applied to the two
binary32 results.  host/sincos_check.cpp holds it to an in-file restatement of the UNFUSED form (each product and sum rounded on
its own, the sign carried by x and the cosine table) on all 2^24 arguments the path tracer reaches, bit for bit, under
AddressSanitizer and UBSan; `make sincos-check` builds and runs it.  This test runs that rule and reads the two counts.
(The pins of the values themselves are elsewhere and unchanged: tests/test_abi.py against the oracle and libm on the same 2^24
arguments, pt_ctx_sincos_sweep for the device against the host.)"""
import re

import ptlib


def test_fused_sincos_equals_unfused_on_every_argument():
    out = ptlib.host_check("sincos")
    m = re.search(r"sincos_check: (\d+) arguments, sin mismatches (\d+), cos mismatches (\d+)", out)
    assert m, out[-4000:]
    assert int(m.group(1)) == 1 << 24
    assert int(m.group(2)) == 0 and int(m.group(3)) == 0, m.group(0)
