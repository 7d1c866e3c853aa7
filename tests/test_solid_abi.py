"""pt_ctx_solid at the ABI and its contract, without a device.

- include/ptrace_solid.h declares pt_solid_params, pt_solid_look, pt_ctx_solid and the three host functions and states the
  contract; the library exports them; solid_abi.py, the Rust shim and the Python binding mirror them - the structs' layout and the
  constants as the C compiler sees the header; PT_ABI_VERSION is still 5; ptrace.h and ptrace_overlay.h know nothing of the pass.
- Every refusal, in the header's order, with a NULL context (the last thing checked): none needs a device.
- pt_solid_defaults against the header's list, pt_solid_look_of against a pt_object.
- pt_solid_pixel_host == tests/solid_ref.py, bit for bit, on a few thousand random pixels per flag combination, with and without
  albedo: NaN payloads, -0, denormals and infinities in albedo and normal, ids on both sides of n_looks, misses, zero normals.
- host/solid_check.cpp under the sanitizers (make solid-check).
The GPU side is tests/test_gpu_solid.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import overlay_ref
import ptlib
import solid_ref as ref
from solid_ref import F32, HEADLIGHT, REFLECT_SKY, PtSolidLook, PtSolidParams

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
PARAM_FIELDS = [("uint32_t", "flags"), ("float", "light[3]"), ("float", "ambient"), ("float", "diffuse"), ("float", "specular"),
                ("uint32_t", "shininess_log2"), ("float", "background[3]"), ("float", "sky_top[3]"), ("float", "sky_bottom[3]")]
LOOK_FIELDS = [("float", "emission[3]"), ("uint32_t", "reflect_type")]
PARAM_SIZE, LOOK_SIZE = 68, 16  # 17 words; 4 words
FUNCTIONS = ["pt_ctx_solid", "pt_solid_defaults", "pt_solid_look_of", "pt_solid_pixel_host"]
CONSTANTS = {"PT_SOLID_HEADLIGHT": 1, "PT_SOLID_REFLECT_SKY": 2, "PT_SOLID_MAX_SHININESS_LOG2": 10}

ABOVE = dict(position=(0.5, 3.0, 4.0), direction=(-0.1, -0.6, -0.79), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
LEVEL = dict(position=(1.0, 0.25, 6.0), direction=(-0.15, 0.0, -0.98), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
DOWN = dict(position=(0.0, 5.0, 0.0), direction=(0.0, -1.0, 0.0), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "ptrace_solid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


@pytest.fixture(scope="module")
def L():
    return ptlib.product()


# ---------------------------------------------------------------------------------------------------------- the ABI
def _fields(h, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, flags=re.S).group(1)
    return [(t, n.strip()) for t, names in re.findall(r"\b(uint32_t|int32_t|float)\s+([\w\s,\[\]]+);", body) for n in names.split(",")]


def test_header_declares_them():
    h = _header()
    assert _fields(h, "pt_solid_params") == PARAM_FIELDS and _fields(h, "pt_solid_look") == LOOK_FIELDS
    assert [n for n, _ in PtSolidParams._fields_] == [n.split("[")[0] for _, n in PARAM_FIELDS]
    assert [n for n, _ in PtSolidLook._fields_] == [n.split("[")[0] for _, n in LOOK_FIELDS]
    assert C.sizeof(PtSolidParams) == PARAM_SIZE and C.sizeof(PtSolidLook) == LOOK_SIZE
    m = re.search(r"\bint pt_ctx_solid\((.*?)\);", h, flags=re.S)
    names = [q.split()[-1].lstrip("*") for q in m.group(1).split(",")]
    assert names == ["ctx", "width", "height", "params", "cam", "d_albedo", "d_normal", "d_depth", "d_object_id", "looks", "n_looks",
                     "d_out", "hip_stream"]
    assert "".join("p" if "*" in q else "i" for q in m.group(1).split(",")) == "piipppppppipp"
    assert re.search(r"void \*hip_stream\s*$", m.group(1))  # the stream is the last parameter, under ptrace.h's name
    assert re.search(r"\bint pt_solid_defaults\(\s*pt_solid_params \*\w+\);", h)
    assert re.search(r"\bint pt_solid_look_of\(\s*const pt_object \*\w+\s*,\s*pt_solid_look \*\w+\);", h)
    m = re.search(r"\bint pt_solid_pixel_host\((.*?)\);", h, flags=re.S)
    assert [q.split()[-1].lstrip("*").split("[")[0] for q in m.group(1).split(",")] == [
        "cam", "width", "height", "params", "idx", "object_id", "depth", "albedo", "normal", "look", "rgb_out"]
    for name, val in CONSTANTS.items():
        assert int(re.search(r"#define %s\s+(\d+)u" % name, h).group(1)) == val
        assert getattr(ref.solid_abi, name) == val
    assert '#include "ptrace.h"' in h  # a header of its own, on top of ptrace.h


def test_the_other_headers_do_not_know_it():
    main = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    overlay = open(os.path.join(ROOT, "include", "ptrace_overlay.h")).read()
    assert re.search(r"#define PT_ABI_VERSION 5\b", main)  # symbols were added, nothing changed
    assert "pt_solid" not in main and "pt_solid" not in overlay and "PT_SOLID" not in main and "PT_SOLID" not in overlay


def test_solid_abi_py_is_the_header_as_the_compiler_sees_it(tmp_path):
    """solid_abi.py against include/ptrace_solid.h as tests/test_abi.py holds abi.py to ptrace.h: one table entry per declared
    function with as many parameters, and sizeof, every offsetof and every PT_SOLID_* value from a C program"""
    sa = ref.solid_abi
    protos = dict(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(((?:[^()])*)\)\s*;", _header()))
    assert sorted(protos) == sorted(sa.SIGNATURES) == FUNCTIONS
    L = ptlib.product()
    for name, params in protos.items():
        restype, argtypes = sa.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params.split(",")), name
        kinds = "".join("p" if "*" in q or "[" in q else ("f" if q.split()[0] == "float" else "i") for q in params.split(","))
        got = "".join("f" if t is C.c_float else ("i" if t in (C.c_int, C.c_int32, C.c_uint32) else "p") for t in argtypes)
        assert kinds == got, name
        assert getattr(L, name).argtypes == argtypes  # abi.load() declared it with the rest
    consts = {n: v for n, v in vars(sa).items() if n.startswith("PT_") and isinstance(v, int)}
    assert consts == CONSTANTS
    want, prog = [], ["#include <stdio.h>", "#include <stddef.h>", '#include "ptrace_solid.h"', "int main(void) {"]
    for cname, ctype in (("pt_solid_params", PtSolidParams), ("pt_solid_look", PtSolidLook)):
        prog.append('printf("size %%zu\\n", sizeof(%s));' % cname)
        want.append("size %d" % C.sizeof(ctype))
        for field, _ in ctype._fields_:
            prog.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (field, cname, field))
            want.append("%s %d" % (field, getattr(ctype, field).offset))
    for n, v in sorted(consts.items()):
        prog.append('printf("%s %%lld\\n", (long long)(%s));' % (n, n))
        want.append("%s %d" % (n, v))
    prog.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(prog) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe])
    got = subprocess.check_output([exe]).decode().split("\n")[:-1]
    assert got == want
    assert got[0] == "size 68" and "size 16" in got


def test_header_states_the_contract():
    def norm(t):
        return " ".join(t.replace("*", " ").split())

    text = _header(strip=False)
    at = text.index("pt_ctx_solid shades")
    doc = norm(text[at:text.index("#define PT_SOLID_HEADLIGHT", at)])
    for phrase in ("THE ARITHMETIC", "dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z", "pos(v) = v > 0 ? v : 0", "mix(a, b, t) = a + (b - a) * t",
                   "clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v)", "out[idx][c] = background[c]", "no other plane of this pixel is read",
                   "exactly as step 1 of pt_ctx_overlay", "P[a] = L[a] + d[a] * depth[idx]", "v = -d", "(0, 0, 0) when the length is not > 0",
                   "Q = L with PT_SOLID_HEADLIGHT", "lv = Q - P", "ll = sqrt(dot(lv, lv))", "ld = ll > 0 ? lv * (1 / ll) : (0, 0, 0)",
                   "ndl = dot(N, ld)", "dif = pos(ndl)", "r[a] = N[a] * (2 * ndl) - ld[a]", "s = ndl > 0 ? pos(dot(v, r)) : 0",
                   "s = s * s, shininess_log2 times", "k = (ambient + diffuse * dif) + specular * s", "b[c] = A[c] * k",
                   "(uint32)id < n_looks ? looks[id] : {0, 0, 0, PT_DIFFUSE}", "dn = dot(N, d)", "m_y = d.y - N.y * (2 * dn)",
                   "t = clamp(m_y * 0.5 + 0.5)", "b[c] = A[c] * mix(sky_bottom[c], sky_top[c], t) + specular * s",
                   "PT_REFRACT is shaded as PT_DIFFUSE", "out[idx][c] = clamp(b[c] + rec.emission[c])", "d_out may be d_albedo or d_normal",
                   "NULL is the context's own stream", "ordered on that stream", "complete when the call returns", "HOST array",
                   "16 B per record", "grown on demand", "freed by pt_ctx_destroy", "never a read outside it", "no \"0 = default\"",
                   "checked in this order", "ambient 0.1, diffuse 1, specular 0.5, shininess_log2 5"):
        assert norm(phrase) in doc, phrase
    order = ["unknown flag bits", "shininess_log2 above", "an ambient, diffuse or specular", "without PT_SOLID_HEADLIGHT a light component",
             "a background, sky_top or sky_bottom component", "width or height 0", "above 2^28", "NULL cam", "lens centre is not finite",
             "NULL d_normal, d_depth, d_object_id or d_out", "n_looks above 2^20", "NULL looks with n_looks != 0", "reflect_type is above PT_REFRACT",
             "NULL ctx"]
    where = [doc.index(norm(p)) for p in order]
    assert where == sorted(where)


def test_library_exports_them_and_the_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(FUNCTIONS) <= exported
    assert L.pt_abi_version() == 5


def test_rust_shim_mirrors_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    want = {"uint32_t": "u32", "int32_t": "i32", "float": "f32"}
    for rname, fields, size in (("PtSolidParams", PARAM_FIELDS, PARAM_SIZE), ("PtSolidLook", LOOK_FIELDS, LOOK_SIZE)):
        body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s \{(.*?)\n\}" % rname, rust, flags=re.S).group(1)
        got = re.findall(r"pub (\w+): ([\w\[\]; ]+),", body)
        exp = []
        for t, n in fields:
            m = re.match(r"(\w+)\[(\d+)\]", n)
            exp.append((m.group(1), "[%s; %s]" % (want[t], m.group(2))) if m else (n, want[t]))
        assert got == exp
        words = sum(int(re.search(r"; (\d+)\]", t).group(1)) if "[" in t else 1 for _, t in got)
        assert words * 4 == size
    for name, val in (("PT_SOLID_HEADLIGHT", 1), ("PT_SOLID_REFLECT_SKY", 2), ("PT_SOLID_MAX_SHININESS_LOG2", 10)):
        assert re.search(r"pub const %s: u32 = %d;" % (name, val), rust)
    (ext,) = [b for b in re.findall(r'extern "C" \{(.*?)\n\}', rust, flags=re.S) if "pt_ctx_solid" in b]  # the header's own block
    assert "pt_ctx_overlay" not in ext and "pt_ctx_render" not in ext
    m = re.search(r"pub fn pt_ctx_solid\((.*?)\)\s*->\s*i32;", ext, flags=re.S)
    types = [q.split(":", 1)[1].strip() for q in m.group(1).split(",") if ":" in q]
    assert "".join("p" if t.startswith("*") else "i" for t in types) == "piipppppppipp"
    assert types[3] == "*const PtSolidParams" and types[4] == "*const PtCamera" and types[9] == "*const PtSolidLook"
    assert re.search(r"pub fn pt_solid_defaults\(\s*out: \*mut PtSolidParams\s*\)\s*->\s*i32;", ext)
    assert re.search(r"pub fn pt_solid_look_of\(\s*obj: \*const PtObject,\s*out: \*mut PtSolidLook\s*\)\s*->\s*i32;", ext)
    assert re.search(r"pub fn pt_solid_pixel_host\(", ext)


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    assert pkg.pt_solid_params is ref.solid_abi.pt_solid_params and pkg.pt_solid_look is ref.solid_abi.pt_solid_look
    assert (pkg.PT_SOLID_HEADLIGHT, pkg.PT_SOLID_REFLECT_SKY, pkg.PT_SOLID_MAX_SHININESS_LOG2) == (1, 2, 10)
    assert callable(pkg.Context.solid)
    p = pkg.solid_defaults()
    assert p.flags == 1 and p.shininess_log2 == 5 and p.diffuse == 1.0
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    looks = pkg.solid_looks([sc.objs[i] for i in range(sc.n_objs)])
    assert len(looks) == sc.n_objs and C.sizeof(looks) == 16 * sc.n_objs
    for i in range(sc.n_objs):
        assert tuple(looks[i].emission) == tuple(sc.objs[i].emission) and looks[i].reflect_type == sc.objs[i].reflect_type
    assert any(max(lk.emission) > 0 for lk in looks) and {lk.reflect_type for lk in looks} == {0, 1, 2}  # a lamp, a mirror, a glass


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_in_order_without_a_device(L):
    """Each call breaks one rule and every rule checked AFTER it: the message names the first.  The context is NULL throughout."""
    alb, nrm, z, ids, out = (C.c_void_p(0x1000 * k) for k in range(1, 6))  # never dereferenced
    BIG = 1 << 15
    nan, inf = float("nan"), float("inf")
    good_cam = ref.pt_camera(ABOVE)
    bad_cam = ref.pt_camera(dict(ABOVE, position=(inf, 0.0, 0.0)))
    ok_looks = ref.looks_array([((0.0, 0.0, 0.0), 0), ((2.0, 2.0, 2.0), 2)])
    bad_type = ref.looks_array([((0.0, 0.0, 0.0), 0), ((0.0, 0.0, 0.0), 3)])
    bad_emission = [ref.looks_array([((0.0, e, 0.0), 1)]) for e in (-1.0, nan, inf)]

    def P(**kw):
        return ref.struct(ref.params(**kw))

    def call(p, w=0, h=0, cam=None, d_n=None, d_z=None, d_id=None, d_out=None, looks=None, n_looks=(1 << 20) + 1, d_alb=None):
        rc = L.pt_ctx_solid(None, w, h, C.byref(p) if p is not None else None, C.byref(cam) if cam is not None else None, d_alb, d_n, d_z,
                            d_id, looks, n_looks, d_out, None)
        return rc, L.pt_last_error().decode()

    # what comes later in the order, broken as well: by default every call has a frame of 0 x 0, no camera, no plane, no table
    # and 2^20 + 1 records
    later = dict(shininess_log2=11, ambient=-1.0, light=(nan, 0.0, 0.0), background=(-1.0, 0.0, 0.0))
    planes = dict(d_n=nrm, d_z=z, d_id=ids, d_out=out)
    cases = [
        (call(P(flags=4, **later)), "flags"),
        (call(P(flags=0x80000001, **later)), "flags"),
        (call(P(flags=2, **later)), "shininess_log2"),
        (call(P(flags=2, **dict(later, shininess_log2=10))), "ambient, diffuse or specular"),
        (call(P(flags=2, diffuse=nan, light=(nan, 0.0, 0.0), background=(-1.0, 0.0, 0.0))), "ambient, diffuse or specular"),
        (call(P(flags=2, specular=inf, light=(nan, 0.0, 0.0), background=(-1.0, 0.0, 0.0))), "ambient, diffuse or specular"),
        (call(P(flags=2, light=(0.0, 0.0, inf), background=(-1.0, 0.0, 0.0))), "light"),
        (call(P(flags=0, light=(0.0, nan, 0.0), background=(-1.0, 0.0, 0.0))), "light"),
        (call(P(flags=3, light=(nan, nan, nan), background=(0.0, -1.0, 0.0))), "colour"),  # a headlight: the light is not read
        (call(P(sky_top=(0.0, 0.0, inf))), "colour"),
        (call(P(sky_bottom=(nan, 0.0, 0.0))), "colour"),
        (call(P(), 0, 5), "width and height"),
        (call(None, 5, 0), "width and height"),
        (call(None, BIG, BIG), "2^28"),
        (call(None, 4, 4), "cam is NULL"),
        (call(None, 4, 4, bad_cam), "lens centre"),
        (call(None, 4, 4, good_cam, None, z, ids, out), "d_normal"),
        (call(None, 4, 4, good_cam, nrm, None, ids, out), "d_depth"),
        (call(None, 4, 4, good_cam, nrm, z, None, out), "d_object_id"),
        (call(None, 4, 4, good_cam, nrm, z, ids, None), "d_out"),
        (call(None, 4, 4, good_cam, **planes), "2^20"),
        (call(None, 4, 4, good_cam, n_looks=1 << 20, **planes), "looks is NULL"),
        (call(None, 4, 4, good_cam, looks=bad_type, n_looks=2, **planes), "reflect_type"),
        (call(None, 4, 4, good_cam, looks=bad_emission[0], n_looks=1, **planes), "emission"),
        (call(None, 4, 4, good_cam, looks=bad_emission[1], n_looks=1, **planes), "emission"),
        (call(None, 4, 4, good_cam, looks=bad_emission[2], n_looks=1, **planes), "emission"),
        (call(None, 4, 4, good_cam, looks=ok_looks, n_looks=2, **planes), "ctx"),
        (call(None, 4, 4, good_cam, looks=bad_type, n_looks=1, **planes), "ctx"),  # the bad record lies beyond n_looks
        (call(None, 4, 4, good_cam, looks=ok_looks, n_looks=0, **planes), "ctx"),
        (call(None, 4, 4, good_cam, looks=None, n_looks=0, **planes), "ctx"),  # no albedo: a clay view
        (call(P(flags=0, shininess_log2=0, ambient=0.0, diffuse=0.0, specular=0.0), 1 << 14, 1 << 14, good_cam, nrm, z, ids, nrm, None, 0,
              d_alb=alb), "ctx"),  # 2^28 pixels exactly, in place on the normals
        (call(P(flags=3, shininess_log2=10), 4, 4, good_cam, nrm, z, ids, alb, None, 0, d_alb=alb), "ctx"),
    ]
    for i, ((rc, msg), word) in enumerate(cases):
        assert rc == PT_ERR_INVALID and word in msg, (i, rc, msg, word)


# -------------------------------------------------------------------------------------------------------- defaults
def test_defaults_and_look_of(L):
    s = PtSolidParams()
    assert L.pt_solid_defaults(None) == PT_ERR_INVALID
    assert L.pt_solid_defaults(C.byref(s)) == 0
    d = ref.from_struct(s)
    want = ref.params()
    assert d["flags"] == HEADLIGHT == want["flags"] and d["shininess_log2"] == 5
    for k in ref.VECTORS:
        assert tuple(F32(c) for c in d[k]) == tuple(F32(c) for c in want[k]), k
    for k in ref.SCALARS:
        assert F32(d[k]) == F32(want[k]), k
    o = overlay_ref.defaults(L)  # the sky is pt_overlay_defaults'
    assert d["sky_top"] == o["sky_top"] and d["sky_bottom"] == o["sky_bottom"]
    # what it writes passes the validator
    cam = ref.pt_camera(ABOVE)
    p16 = C.c_void_p(16)
    assert L.pt_ctx_solid(None, 4, 4, C.byref(s), C.byref(cam), None, p16, p16, p16, None, 0, p16, None) == PT_ERR_INVALID
    assert "ctx" in L.pt_last_error().decode()
    obj = ptlib.make_sphere((1.0, 2.0, 3.0), 0.5, (0.25, 0.5, 0.75), (2.0, 0.0, 0.125), ptlib.REFLECT["Refract"])
    look = PtSolidLook()
    assert L.pt_solid_look_of(C.byref(obj), C.byref(look)) == 0
    assert tuple(look.emission) == (2.0, 0.0, 0.125) and look.reflect_type == 2
    assert L.pt_solid_look_of(None, C.byref(look)) == PT_ERR_INVALID and L.pt_solid_look_of(C.byref(obj), None) == PT_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the pixel on the host
LOOKS = [((0.0, 0.0, 0.0), 0), ((0.0, 0.0, 0.0), 1), ((0.0, 0.0, 0.0), 2), ((2.0, 1.5, 0.25), 0), ((0.125, 0.0, 0.5), 1)]
SPECIAL_BITS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], dtype=np.uint32)


def host_pixels(L, cam, W, H, p, idx, oid, depth, albedo, normal, looks):
    s = ref.struct(p) if p is not None else None
    c = ref.pt_camera(cam)
    arr = ref.looks_array(looks)
    normal = np.ascontiguousarray(normal, dtype=F32)
    albedo = None if albedo is None else np.ascontiguousarray(albedo, dtype=F32)
    out = np.zeros((len(idx), 3), dtype=F32)
    fp = C.POINTER(C.c_float)
    for i in range(len(idx)):
        look = C.byref(arr[int(oid[i])]) if 0 <= oid[i] < len(looks) else None  # beyond the table: the default record
        rc = L.pt_solid_pixel_host(C.byref(c), W, H, C.byref(s) if p is not None else None, int(idx[i]), int(oid[i]), float(depth[i]),
                                   albedo[i].ctypes.data_as(fp) if albedo is not None else None, normal[i].ctypes.data_as(fp), look,
                                   out[i].ctypes.data_as(fp))
        assert rc == 0, (rc, L.pt_last_error())
    return out


def random_pixels(rng, n, W, H):
    idx = rng.integers(0, W * H, size=n)
    oid = rng.integers(-1, len(LOOKS) + 3, size=n).astype(np.int32)  # misses, the table, and ids beyond it
    oid[rng.random(n) < 0.05] = 1 << 30
    depth = (0.5 + rng.random(n) * 12).astype(F32)
    depth[rng.random(n) < 0.05] = np.inf
    depth[rng.random(n) < 0.03] = 0.0
    albedo = rng.random((n, 3)).astype(F32)
    normal = (rng.random((n, 3)) - 0.5).astype(F32)
    normal[rng.random(n) < 0.1] = 0.0
    for plane in (albedo, normal):  # NaN payloads, -0, denormals, infinities
        special = rng.random((n, 3)) < 0.1
        plane.view(np.uint32)[special] = rng.choice(SPECIAL_BITS, size=int(special.sum()))
    return idx, oid, depth, albedo, normal


@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("flags", [0, HEADLIGHT, REFLECT_SKY, HEADLIGHT | REFLECT_SKY])
def test_pixel_host_is_the_restatement(L, flags, with_albedo):
    W, H, n = 48, 32, 1000
    seen = dict(miss=0, beyond=0, mirror=0, lit=0, unlit=0, zero_normal=0, saturated=0, nan_out=0)
    for k, (cam, shin) in enumerate(((ABOVE, 5), (LEVEL, 0), (DOWN, 10))):
        rng = np.random.default_rng(flags * 100 + with_albedo * 10 + k)
        p = ref.params(flags=flags, light=(1.5, 4.0, 2.0), ambient=0.125, diffuse=0.75, specular=0.5, shininess_log2=shin,
                       background=(0.0, 0.25, 0.5), sky_top=(0.25, 0.5, 0.75), sky_bottom=(0.75, 0.75, 0.7))
        idx, oid, depth, albedo, normal = random_pixels(rng, n, W, H)
        alb = albedo if with_albedo else None
        want = ref.shade(cam, W, H, p, idx, oid, depth, alb, normal, LOOKS)
        got = host_pixels(L, cam, W, H, p, idx, oid, depth, alb, normal, LOOKS)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
        hit = oid >= 0
        seen["miss"] += int((~hit).sum())
        seen["beyond"] += int((oid >= len(LOOKS)).sum())
        seen["mirror"] += int(np.isin(oid, (1, 4)).sum())
        seen["zero_normal"] += int((hit & (normal == 0).all(axis=1)).sum())
        seen["saturated"] += int((hit[:, None] & (want == 1.0)).sum())
        seen["nan_out"] += int(np.isnan(want).sum())
        grey = ref.shade(cam, W, H, dict(p, ambient=0.0, specular=0.0, diffuse=1.0), idx, oid, depth, None, normal, None)
        seen["lit"] += int((hit & (grey[:, 0] > 0)).sum())
        seen["unlit"] += int((hit & (grey[:, 0] == 0)).sum())
        assert (want[~hit] == np.array(p["background"], dtype=F32)).all()
    assert all(v > 0 for k, v in seen.items() if k != "nan_out" or with_albedo), seen
    # the defaults: NULL params is pt_solid_defaults
    idx, oid, depth, albedo, normal = random_pixels(np.random.default_rng(7), 200, W, H)
    want = ref.shade(ABOVE, W, H, ref.params(), idx, oid, depth, albedo, normal, LOOKS)
    assert host_pixels(L, ABOVE, W, H, None, idx, oid, depth, albedo, normal, LOOKS).view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_pixel_host_refusals(L):
    fp = C.POINTER(C.c_float)
    v = np.array([0.0, 1.0, 0.0], dtype=F32)
    a = v.ctypes.data_as(fp)
    o = np.zeros(3, dtype=F32).ctypes.data_as(fp)
    cam = ref.pt_camera(ABOVE)
    far = ref.pt_camera(dict(ABOVE, position=(float("inf"), 0.0, 0.0)))
    bad = ref.struct(ref.params(shininess_log2=11))
    bad_look = PtSolidLook(ptlib.f3(0.0, 0.0, 0.0), 3)
    dim_look = PtSolidLook(ptlib.f3(-1.0, 0.0, 0.0), 0)
    f = L.pt_solid_pixel_host
    assert f(C.byref(cam), 4, 4, None, 0, 0, 1.0, None, a, None, o) == 0  # NULL params, albedo and look
    assert f(C.byref(cam), 4, 4, None, 15, -1, 1.0, a, a, None, o) == 0
    assert f(C.byref(cam), 4, 4, C.byref(bad), 0, 0, 1.0, a, a, None, o) == PT_ERR_INVALID
    assert f(None, 4, 4, None, 0, 0, 1.0, a, a, None, o) == PT_ERR_INVALID
    assert f(C.byref(far), 4, 4, None, 0, 0, 1.0, a, a, None, o) == PT_ERR_INVALID
    assert f(C.byref(cam), 0, 4, None, 0, 0, 1.0, a, a, None, o) == PT_ERR_INVALID
    assert f(C.byref(cam), 1 << 15, 1 << 15, None, 0, 0, 1.0, a, a, None, o) == PT_ERR_INVALID
    assert f(C.byref(cam), 4, 4, None, 16, 0, 1.0, a, a, None, o) == PT_ERR_INVALID
    assert f(C.byref(cam), 4, 4, None, 0, 0, 1.0, a, None, None, o) == PT_ERR_INVALID
    assert f(C.byref(cam), 4, 4, None, 0, 0, 1.0, a, a, None, None) == PT_ERR_INVALID
    assert f(C.byref(cam), 4, 4, None, 0, 0, 1.0, a, a, C.byref(bad_look), o) == PT_ERR_INVALID
    assert f(C.byref(cam), 4, 4, None, 0, 0, 1.0, a, a, C.byref(dim_look), o) == PT_ERR_INVALID


# ---------------------------------------------------------------------------------------------- the host check program
def test_solid_check_program():
    ptlib.host_check("solid")
    mk = open(os.path.join(ptlib.PKG, "Makefile")).read()
    assert "pt_solid" in re.search(r"^UNITS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "pt_solid" not in re.search(r"^TUNED\s*=(.*)$", mk, flags=re.M).group(1).split()  # COMMON alone
    assert "solid" in re.search(r"^CHECKS\s*=(.*)$", mk, flags=re.M).group(1).split()
