"""pt_ctx_select_pixels and pt_ctx_render_masked at the ABI, without a device.

- The header declares pt_select_params and the two functions; the library exports them; PT_ABI_VERSION is still 5; the Rust
  shim and the Python binding mirror them.
- Every refusal of both calls, in the header's order.  Both check the context last (pt_ctx_select_pixels) or second
  (pt_ctx_render_masked), so a NULL context reaches every earlier refusal without a device.
- A NaN threshold is refused, infinite ones are not.
- The restatement of the predicate (tests/masked_ref.py) on the values that matter.
- `make select-check` - the validators and the predicate under AddressSanitizer and UBSan as a stand-alone program - builds
  and exits 0.
The GPU side is tests/test_gpu_masked.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import masked_ref as ref
import ptlib
from masked_ref import F32
from ptlib import PtConfig, PtSelectParams

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
SELECT_NAMES = ["ctx", "width", "height", "params", "d_weight", "d_len", "d_mask", "n_selected", "hip_stream"]
MASKED_NAMES = ["ctx", "cfg", "d_mask", "d_rgb", "hip_stream", "cancel", "stats", "n_pixels"]


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


@pytest.fixture(scope="module")
def L():
    return ptlib.product()


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_them():
    h = _header()
    body = re.search(r"typedef struct pt_select_params \{(.*?)\} pt_select_params;", h, flags=re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"\b(uint32_t|float)\s+([\w\s,]+);", body) for n in names.split(",")]
    assert fields == [("float", "weight_max"), ("float", "len_max"), ("uint32_t", "flags")]
    assert [n for n, _ in PtSelectParams._fields_] == [n for _, n in fields]
    assert C.sizeof(PtSelectParams) == 12
    for name, kinds, names in (("pt_ctx_select_pixels", "piippppp" + "p", SELECT_NAMES), ("pt_ctx_render_masked", "p" * 8, MASKED_NAMES)):
        m = re.search(r"\bint %s\((.*?)\);" % name, h, flags=re.S)
        params = [q.strip() for q in m.group(1).split(",")]
        assert "".join("p" if "*" in q else "i" for q in params) == kinds, name
        assert [q.split()[-1].lstrip("*") for q in params] == names, name
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)  # symbols were added, nothing changed


def test_header_states_the_contract():
    def norm(t):
        return " ".join(t.replace("*", " ").split())

    text = _header(strip=False)
    at = text.index("retracing chosen pixels of a frame")
    doc = norm(text[at:text.index("typedef struct pt_select_params", at)])
    for phrase in ("mask[p] = ((d_weight && !(weight[p] > weight_max)) || (d_len && !(len[p] > len_max))) ? 1 : 0",
                   "A NaN in a plane selects the pixel", "taken literally", "integer atomics", "No scene is needed",
                   "nonzero means selected", "bit for bit", "No other float of d_rgb is written", "whole image rows",
                   "PT_FLAG_PIPELINES is refused", "An empty mask", "On PT_CANCELLED d_rgb is untouched", "no progress callback",
                   "samples = n_pixels spp", "4 B each", "24 B each", "pt_ctx_set_scene forgets"):
        assert norm(phrase) in doc, phrase
    first = doc.index("pt_ctx_select_pixels: an image pass")
    second = doc.index("pt_ctx_render_masked: a frame call")
    for start, order in ((first, ["a NaN threshold", "flags != 0", "width or height 0", "> 2^28", "both planes NULL", "NULL d_mask",
                                  "NULL params", "NULL ctx"]),
                         (second, ["NULL cfg, d_mask or d_rgb", "NULL ctx", "no scene", "not whole rows", "chunk_step > 1 or",
                                   "whatever pt_ctx_render refuses"])):
        at = doc.index("checked in this order", start)
        where = [doc.index(p, at) for p in order]
        assert where == sorted(where), order


def test_library_exports_them_and_the_abi_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pt_ctx_select_pixels", "pt_ctx_render_masked"} <= exported
    assert L.pt_abi_version() == 5


def test_rust_shim_mirrors_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct PtSelectParams \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("weight_max", "f32"), ("len_max", "f32"), ("flags", "u32")]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for name, names, types in (
            ("pt_ctx_select_pixels", SELECT_NAMES, ["*mut PtCtx", "u32", "u32", "*const PtSelectParams", "*const f32", "*const f32",
                                                    "*mut u8", "*mut u32", "*mut c_void"]),
            ("pt_ctx_render_masked", MASKED_NAMES, ["*mut PtCtx", "*const PtConfig", "*const u8", "*mut c_void", "*mut c_void",
                                                    "*const u8", "*mut PtStats", "*mut u32"])):
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*i32;" % name, ext, flags=re.S)
        params = [(q.split(":", 1)[0].strip(), q.split(":", 1)[1].strip()) for q in m.group(1).split(",") if ":" in q]
        assert [n for n, _ in params] == names and [t for _, t in params] == types, name
    helper = rust[rust.index("pub fn retrace_fallback("):]
    helper = helper[:helper.index("\n}\n")]
    assert "pt_ctx_select_pixels(" in helper and "pt_ctx_render_masked(" in helper and "pt_device_download" not in helper


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    assert [n for n, _ in pkg.pt_select_params._fields_] == [n for n, _ in PtSelectParams._fields_]
    assert C.sizeof(pkg.pt_select_params) == 12
    assert callable(pkg.Context.select_pixels) and callable(pkg.Context.render_masked)
    lib = pkg.lib()
    assert len(lib.pt_ctx_select_pixels.argtypes) == 9 and len(lib.pt_ctx_render_masked.argtypes) == 8


# -------------------------------------------------------------------------------------------------------- refusals
def test_select_refusals_in_order_without_a_device(L):
    """Each call breaks one rule and every rule checked AFTER it: the message names the first.  The context is NULL throughout."""
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(3)]  # never dereferenced: every call is refused before a device is touched
    P = PtSelectParams
    nan, inf = float("nan"), float("inf")

    def call(w, h, prm, weight, length, mask):
        rc = L.pt_ctx_select_pixels(None, w, h, C.byref(prm) if prm is not None else None, weight, length, mask, None, None)
        return rc, L.pt_last_error().decode()

    cases = [
        (call(0, 0, P(nan, 0.0, 6), None, None, None), "NaN"),
        (call(0, 0, P(0.0, nan, 6), None, None, None), "NaN"),
        (call(0, 0, P(inf, -inf, 6), None, None, None), "flags"),  # the infinities are thresholds like any other
        (call(0, 1 << 20, P(0.0, 0.0, 0), None, None, None), "must be positive"),
        (call(1 << 20, 0, P(0.0, 0.0, 0), None, None, None), "must be positive"),
        (call(1 << 14, (1 << 14) + 1, P(0.0, 0.0, 0), None, None, None), "2^28"),
        (call(4, 4, None, None, None, None), "both NULL"),
        (call(4, 4, None, p[0], None, None), "d_mask"),
        (call(4, 4, None, None, p[1], None), "d_mask"),
        (call(4, 4, None, p[0], p[1], p[2]), "params"),
        (call(4, 4, P(0.0, 0.0, 0), p[0], p[1], p[2]), "ctx"),
        (call(4, 4, P(inf, -inf, 0), p[0], None, p[2]), "ctx"),
        (call(4, 4, P(-inf, inf, 0), None, p[1], p[2]), "ctx"),
        (call(1 << 14, 1 << 14, P(0.0, 0.0, 0), p[0], p[1], p[2]), "ctx"),  # 2^28 pixels are allowed
    ]
    for i, ((rc, msg), word) in enumerate(cases):
        assert rc == PT_ERR_INVALID and word in msg, (i, rc, msg, word)


def test_render_masked_refusals_without_a_device(L):
    """NULL cfg, d_mask or d_rgb comes before the context; everything after it needs one (tests/test_gpu_masked.py)."""
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(2)]
    cfg = PtConfig(8, 8, 1, 1, 1, 0, 0, 0, 0)
    bad = PtConfig(0, 0, 0, 7, 1, 3, 2, 0, 0x200, 0, 0, 5)  # every later rule broken too
    n = C.c_uint32(77)
    for args in ((None, p[0], p[1]), (C.byref(bad), None, p[1]), (C.byref(bad), p[0], None)):
        assert L.pt_ctx_render_masked(None, args[0], args[1], args[2], None, None, None, C.byref(n)) == PT_ERR_INVALID
        assert "NULL argument" in L.pt_last_error().decode()
    for c in (cfg, bad):
        assert L.pt_ctx_render_masked(None, C.byref(c), p[0], p[1], None, None, None, C.byref(n)) == PT_ERR_INVALID
        assert "ctx" in L.pt_last_error().decode()
    assert n.value == 77  # a refused call writes nothing


# -------------------------------------------------------------------------------------------------- the restatement
def test_ref_predicate_on_the_values_that_matter():
    t = F32(0.25)
    v = np.array([0.0, -0.0, 0.25, np.nextafter(t, F32(1)), np.nextafter(t, F32(0)), 1.0, np.nan, np.inf, -np.inf], dtype=F32)
    mask, n = ref.select(weight=v, weight_max=0.25)
    assert mask.tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1] and n == 6 and mask.dtype == np.uint8
    assert ref.select(length=v, len_max=0.25)[0].tolist() == mask.tolist()
    # either plane selects; a plane that is not given selects nothing
    w = np.array([0.0, 1.0, 1.0, 0.0], dtype=F32)
    ln = np.array([16.0, 8.0, 16.0, 8.0], dtype=F32)
    assert ref.select(w, ln, 0.0, 8.0)[0].tolist() == [1, 1, 0, 1]
    assert ref.select(weight=w, weight_max=0.0)[0].tolist() == [1, 0, 0, 1]
    assert ref.select(length=ln, len_max=8.0)[0].tolist() == [0, 1, 0, 1]
    # infinite thresholds: +inf selects everything, -inf only -inf and NaN
    assert ref.select(weight=v, weight_max=np.inf)[1] == len(v)
    assert ref.select(weight=v, weight_max=-np.inf)[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("size", ref.SIZES, ids=["%dx%d" % s for s in ref.SIZES])
def test_the_gpu_tests_planes_hold_every_kind_of_value(size):
    n = size[0] * size[1]
    for key, seed in (("weight_max", 1), ("len_max", 2)):
        v = ref.plane(n, ref.PARAMS[key], seed + n)
        assert v.dtype == F32 and len(v) == n
        if n >= 8:
            t = F32(ref.PARAMS[key])
            assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any() and (v == t).any()
            assert (v == np.nextafter(t, F32(np.inf))).any() and (v == np.nextafter(t, F32(-np.inf))).any()
            assert ((v == 0) & np.signbit(v)).any()
            m, ones = ref.select(weight=v, weight_max=t)
            assert 0 < ones < n


# -------------------------------------------------------------------------------------------- the stand-alone program
def test_select_check_builds_and_passes():
    ptlib.host_check("select")
