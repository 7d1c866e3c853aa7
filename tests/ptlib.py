"""ctypes views of the C ABI (include/ptrace.h) and of the oracle (oracle/pt_oracle.h) for the tests.

The scene loader in this file is an independent Python reading of the reference's JSON/OFF formats
(src/render/mod.rs:85-90,236-241,297-324; src/render/load_off.rs:8-85) used to cross-check the
product's C++ loader; it is test code only.
"""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "path-tracer-rust_amd")
ORACLE_SO = os.path.join(ROOT, "oracle", "libpt_oracle.so")
PRODUCT_SO = os.path.join(PKG, "libptrace_hip.so")

if ROOT not in sys.path:  # the tools import this module without the tests' conftest
    sys.path.insert(0, ROOT)
abi = importlib.import_module("path-tracer-rust_amd.abi")  # include/ptrace.h as ctypes: structs, constants, signatures

f3 = abi.f3
# the names the tests use for the structs of ptrace.h (this is the only file that holds such aliases)
PtCamera, PtTriangle, PtObject, PtConfig, PtStats = abi.pt_camera, abi.pt_triangle, abi.pt_object, abi.pt_config, abi.pt_stats
PtScatterItem, PtScatterSurface, PtScatterOut = abi.pt_scatter_item, abi.pt_scatter_surface, abi.pt_scatter_out
PtNoiseStats, PtNoiseTarget = abi.pt_noise_stats, abi.pt_noise_target
PtAdaptiveParams, PtAdaptiveStats, PtAdaptiveInfo = abi.pt_adaptive_params, abi.pt_adaptive_stats, abi.pt_adaptive_info
PtAovParams, PtDenoiseParams, PtDenoiseVarParams = abi.pt_aov_params, abi.pt_denoise_params, abi.pt_denoise_var_params
PtPresentParams, PtUpsampleParams, PtSelectParams = abi.pt_present_params, abi.pt_upsample_params, abi.pt_select_params
PtReprojectParams, PtReprojectVarParams = abi.pt_reproject_params, abi.pt_reproject_var_params
PtObjectMotion = abi.pt_object_motion


class PtoScene(C.Structure):
    _fields_ = [("camera", PtCamera), ("objs", C.POINTER(PtObject)), ("n_objs", C.c_uint32),
                ("tris", C.POINTER(PtTriangle)), ("n_tris", C.c_uint32)]


class PtoConfig(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("_pad", C.c_uint32),
                ("seed", C.c_uint64)]


class PtoCounters(C.Structure):
    _fields_ = [("ray_bounces", C.c_uint64), ("misses", C.c_uint64), ("splits", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("triangle_tests", C.c_uint64)]


PT_SPHERE, PT_MESH = abi.PT_SPHERE, abi.PT_MESH
REFLECT = {"Diffuse": abi.PT_DIFFUSE, "Specular": abi.PT_SPECULAR, "Refract": abi.PT_REFRACT}
BACKEND_WAVEFRONT, BACKEND_MEGAKERNEL = abi.PT_BACKEND_WAVEFRONT, abi.PT_BACKEND_MEGAKERNEL
FLAG_NO_BVH = abi.PT_FLAG_NO_BVH
PROGRESS_EVERY_PASS = abi.PT_PROGRESS_EVERY_PASS
PT_CANCELLED = abi.PT_CANCELLED

fp = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)


def _np_f(a):
    return a.ctypes.data_as(fp)


_oracle = None


def oracle():
    """Load (building if needed) the CPU restatement."""
    global _oracle
    if _oracle is not None:
        return _oracle
    if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(
            os.path.join(ROOT, "oracle", "pt_oracle.c")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    L = C.CDLL(ORACLE_SO)
    L.pto_vec_ops.argtypes = [fp, fp, C.c_float, fp]
    L.pto_sinf.argtypes = [C.c_float]
    L.pto_sinf.restype = C.c_float
    L.pto_cosf.argtypes = [C.c_float]
    L.pto_cosf.restype = C.c_float
    L.pto_sincos_vs_libm.argtypes = [C.c_uint32, C.c_uint32, u64p, u64p]
    L.pto_philox4x32_10.argtypes = [u32p, u32p, u32p]
    L.pto_philox4x32_7.argtypes = [u32p, u32p, u32p]
    L.pto_u32_to_unit.argtypes = [C.c_uint32]
    L.pto_u32_to_unit.restype = C.c_float
    L.pto_draw4.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, fp]
    L.pto_gamma_correction.argtypes = [C.c_float]
    L.pto_gamma_correction.restype = C.c_float
    L.pto_to_int_with_gamma_correction.argtypes = [C.c_float]
    L.pto_to_int_with_gamma_correction.restype = C.c_uint32
    L.pto_camera_basis.argtypes = [C.POINTER(PtCamera), fp, fp, fp]
    L.pto_mesh_bounding_sphere.argtypes = [C.POINTER(PtTriangle), C.c_uint32, fp, fp]
    L.pto_intersect_sphere.argtypes = [fp, C.c_float, fp, fp, fp, fp, fp]
    L.pto_intersect_sphere.restype = C.c_int
    L.pto_intersect_batch.argtypes = [C.POINTER(PtoScene), fp, fp, C.c_uint32, fp, i32p, i32p, fp, fp]
    L.pto_radiance_mean.argtypes = [C.POINTER(PtoScene), fp, fp, C.c_uint64, C.c_uint32, C.c_uint32, fp,
                                    C.POINTER(PtoCounters)]
    L.pto_radiance_mean_at.argtypes = [C.POINTER(PtoScene), fp, fp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, fp,
                                       C.POINTER(PtoCounters)]
    L.pto_primary_ray.argtypes = [C.POINTER(PtCamera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_uint64, fp, fp]
    L.pto_render_pixel.argtypes = [C.POINTER(PtoScene), C.POINTER(PtoConfig), C.c_uint32, fp,
                                   C.POINTER(PtoCounters)]
    L.pto_dump_rays.argtypes = [C.POINTER(PtoScene), C.POINTER(PtoConfig), C.c_uint32, C.c_uint32, fp,
                                C.c_uint64]
    L.pto_dump_rays.restype = C.c_uint64
    L.pto_dump_paths.argtypes = [C.POINTER(PtoScene), C.POINTER(PtoConfig), C.c_uint32, C.c_uint32, fp, u32p, C.c_uint64]
    L.pto_dump_paths.restype = C.c_uint64
    L.pto_render.argtypes = [C.POINTER(PtoScene), C.POINTER(PtoConfig), C.c_uint32, C.c_uint32, fp, C.c_int,
                             C.POINTER(PtoCounters), C.POINTER(C.c_double)]
    L.pto_render.restype = C.c_int
    L.pto_max_threads.restype = C.c_int
    L.pto_render_mock.argtypes = [C.POINTER(PtoScene), C.POINTER(PtoConfig), fp, C.POINTER(PtoCounters), u64p]
    L.pto_render_mock.restype = C.c_int
    L.pto_mesh_bounding_box.argtypes = [C.POINTER(PtTriangle), C.c_uint32, C.POINTER(PtTriangle)]
    L.pto_mesh_bounding_box.restype = None
    L.pto_intersect_bounds_batch.argtypes = [C.POINTER(PtoScene), C.POINTER(PtTriangle), C.c_uint32, fp, fp, C.c_uint32,
                                             i32p, fp, fp, fp]
    L.pto_intersect_bounds_batch.restype = None
    L.pto_orbit_point_batch.argtypes = [C.POINTER(PtoScene), C.POINTER(PtTriangle), fp, fp, C.c_uint32, i32p, fp, i32p, fp]
    L.pto_orbit_point_batch.restype = None
    L.pto_format_ppm.argtypes = [fp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_char_p,
                                 C.c_size_t]
    L.pto_format_ppm.restype = C.c_size_t
    L.pto_siphash13.argtypes = [C.c_char_p, C.c_size_t]
    L.pto_siphash13.restype = C.c_uint64
    L.pto_image_hash.argtypes = [fp, C.c_size_t]
    L.pto_image_hash.restype = C.c_uint64
    _oracle = L
    return L


def _make(*words):
    """make -C PKG <words>; a failure shows the tail of make's output.  Returns the output."""
    r = subprocess.run(["make", "-C", PKG, "-j4"] + list(words), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, "make %s failed:\n%s" % (" ".join(words), r.stdout[-6000:])
    return r.stdout


def _sanitized(exe):
    """the program was linked with the AddressSanitizer and UBSan runtimes (make says which flags only when it has to build)"""
    image = open(exe, "rb").read()
    return b"__asan_init" in image and b"__ubsan_handle" in image


_host_programs = {}


def host_program(name, sanitize=True):
    """host/<name>.cpp built by the Makefile's rule for host programs - at most once per process - under AddressSanitizer and
    UBSan, or plain (sanitize=False: the two table generators that GPU tests reach, nothing else): tool(*args, input=None) ->
    what the program writes to stdout; a non-zero exit status raises."""
    if (name, sanitize) not in _host_programs:
        _make("host-program", "P=" + name, *([] if sanitize else ["SAN="]))
        exe = os.path.join(PKG, "build", "host-san" if sanitize else "host-plain", name)
        assert _sanitized(exe) == sanitize, exe
        _host_programs[name, sanitize] = exe
    exe = _host_programs[name, sanitize]
    return lambda *args, input=None: subprocess.check_output([exe] + [str(a) for a in args], input=input).decode()


def host_check(name):
    """`make <name>-check`: host/<name>_check.cpp (- for _) built under the sanitizers and run; it must exit 0 and close with
    "<name>_check: ok" (some add counts in brackets).  Returns what make and the program wrote."""
    prog = name.replace("-", "_") + "_check"
    out = _make("--no-print-directory", name + "-check")
    assert (out.splitlines()[-1] + " ").startswith(prog + ": ok "), out[-6000:]
    assert _sanitized(os.path.join(PKG, "build", "host-san", prog))
    return out


PROGRESS_FN = abi.pt_progress_fn

_product = None


def product():
    """Load libptrace_hip.so (the product) with every prototype of ptrace.h declared.  Never falls back to anything."""
    global _product
    if _product is None:
        if not os.path.exists(PRODUCT_SO):
            raise RuntimeError("libptrace_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _product = abi.load(PRODUCT_SO)
    return _product


# ---------------------------------------------------------------------------- python scene reader
def _v3(v):
    return f3(*[float(np.float32(x)) for x in v])


def load_off_py(path, scale, triangulate=False):
    """load_off.rs:8-85 in Python (f32 arithmetic through numpy); triangulate=True: fan over polygon faces."""
    lines = []
    for l in open(path):
        l = l.strip()
        if l and not l.startswith("#"):
            lines.append(l)
    assert lines[0] == "OFF"
    nv, nf, _ = [int(t) for t in lines[1].split()]
    sc = np.float32(scale)
    verts = [np.array([np.float32(t) for t in l.split()], dtype=np.float32) * sc for l in lines[2:2 + nv]]
    tris = []
    for l in lines[2 + nv:2 + nv + nf]:
        t = l.split()
        k = int(t[0])
        assert k == 3 or (triangulate and k > 3)
        for j in range(2, k):
            tris.append((verts[int(t[1])], verts[int(t[j])], verts[int(t[j + 1])]))
    return tris


class Scene:
    """Flattened scene: pt_camera + pt_object[] + pt_triangle[] (kept alive by this object)."""

    def __init__(self, sid, cam, objs, tris):
        self.id = sid
        self.cam = cam
        self.n_objs = len(objs)
        self.n_tris = len(tris)
        self.objs = (PtObject * max(1, len(objs)))(*objs)
        self.tris = (PtTriangle * max(1, len(tris)))(*tris)

    def pto(self):
        s = PtoScene()
        s.camera = self.cam
        s.objs = C.cast(self.objs, C.POINTER(PtObject))
        s.n_objs = self.n_objs
        s.tris = C.cast(self.tris, C.POINTER(PtTriangle))
        s.n_tris = self.n_tris
        return s


def make_camera(position, direction, focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5):
    cam = PtCamera()
    cam.position = _v3(position)
    cam.direction = _v3(direction)
    cam.focal_length = float(np.float32(focal_length))
    cam.sensor_width = float(np.float32(sensor_width))
    cam.aspect_ratio = float(np.float32(aspect_ratio))
    return cam


def make_sphere(position, radius, color, emission, reflect):
    o = PtObject()
    o.kind = PT_SPHERE
    o.position = _v3(position)
    o.radius = float(np.float32(radius))
    o.color = _v3(color)
    o.emission = _v3(emission)
    o.reflect_type = REFLECT[reflect] if isinstance(reflect, str) else reflect
    return o


def make_mesh(position, color, emission, reflect, tri_offset, tri_count, bs_center, bs_radius):
    o = PtObject()
    o.kind = PT_MESH
    o.position = _v3(position)
    o.color = _v3(color)
    o.emission = _v3(emission)
    o.reflect_type = REFLECT[reflect] if isinstance(reflect, str) else reflect
    o.tri_offset = tri_offset
    o.tri_count = tri_count
    o.bs_center = _v3(bs_center)
    o.bs_radius = float(np.float32(bs_radius))
    return o


def make_tri(a, b, c):
    t = PtTriangle()
    t.a = _v3(a)
    t.b = _v3(b)
    t.c = _v3(c)
    return t


def load_scene_py(path, base_dir=None, triangulate=False):
    """SceneDescriptor::load + to_data (mod.rs:92-110,304-318) in Python."""
    base_dir = base_dir or os.path.dirname(os.path.dirname(os.path.abspath(path)))
    d = json.load(open(path))
    c = d["camera"]
    cam = make_camera(c["position"], c["direction"], c["focal_length"], c["sensor_width"], c["aspect_ratio"])
    objs, tris = [], []
    for od in d["objects"]:
        m = od["material"]
        ty = od["type_"]
        (kind, val), = ty.items()
        if kind == "Sphere":
            objs.append(make_sphere(od["position"], val["radius"], m["color"], m["emmission"], m["reflect_type"]))
            continue
        if kind == "MeshFile":
            tl = load_off_py(os.path.join(base_dir, val["path"]), val["scale"], triangulate)
            tlist = [make_tri(a, b, c_) for a, b, c_ in tl]
            arr = (PtTriangle * len(tlist))(*tlist)
            ctr = (C.c_float * 3)()
            rad = C.c_float()
            oracle().pto_mesh_bounding_sphere(arr, len(tlist), ctr, C.byref(rad))
            bs_c, bs_r = list(ctr), rad.value
        else:
            tlist = [make_tri(t["a"], t["b"], t["c"]) for t in val["triangles"]]
            bs_c, bs_r = val["bounding_sphere"]["position"], val["bounding_sphere"]["radius"]
        objs.append(make_mesh(od["position"], m["color"], m["emmission"], m["reflect_type"], len(tris),
                              len(tlist), bs_c, bs_r))
        tris.extend(tlist)
    return Scene(d["id"], cam, objs, tris)


def oracle_boxes(scene):
    """Mesh.bounding_box of every object as Mesh::new computes it (12 object-local triangles per object; zeros for
    spheres): the `boxes` argument of pto_intersect_bounds_batch / pto_orbit_point_batch."""
    L = oracle()
    boxes = (PtTriangle * (12 * max(1, scene.n_objs)))()
    for i in range(scene.n_objs):
        o = scene.objs[i]
        if o.kind != PT_MESH:
            continue
        arr = (PtTriangle * o.tri_count)(*[scene.tris[o.tri_offset + k] for k in range(o.tri_count)])
        out = (PtTriangle * 12)()
        L.pto_mesh_bounding_box(arr, o.tri_count, out)
        for k in range(12):
            boxes[12 * i + k] = out[k]
    return boxes


def oracle_render_mock(scene, width, height, spp):
    """The reference's frame with MOCK_RANDOM = true (mod.rs:31-51): image, counters, number of rand01() calls."""
    L = oracle()
    cfg = PtoConfig(width, height, spp, 0, 0)
    out = np.zeros((width * height, 3), dtype=np.float32)
    cnt = PtoCounters()
    draws = C.c_uint64()
    ps = scene.pto()
    assert L.pto_render_mock(C.byref(ps), C.byref(cfg), _np_f(out), C.byref(cnt), C.byref(draws)) == 0
    return out, cnt, draws.value


def oracle_intersect(scene, o, d):
    """intersect_scene ray by ray: (t, object_id, tri_id, x, n) arrays."""
    L = oracle()
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    m = len(o)
    t, oid, tid = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    x, nr = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
    ps = scene.pto()
    L.pto_intersect_batch(C.byref(ps), _np_f(o), _np_f(d), m, _np_f(t), oid.ctypes.data_as(i32p),
                          tid.ctypes.data_as(i32p), _np_f(x), _np_f(nr))
    return t, oid, tid, x, nr


def oracle_radiance(scene, o, d, depth, n, seed, pixel):
    """radiance(&ray, depth, scene) averaged over n samples keyed (seed; pixel, i): (mean rgb, counters)."""
    L = oracle()
    o = np.ascontiguousarray(o, dtype=np.float32)
    d = np.ascontiguousarray(d, dtype=np.float32)
    out = np.zeros(3, np.float32)
    cnt = PtoCounters()
    ps = scene.pto()
    L.pto_radiance_mean_at(C.byref(ps), _np_f(o), _np_f(d), depth, seed, pixel, n, _np_f(out), C.byref(cnt))
    return out, cnt


def scene_path(sid):
    return os.path.join(ROOT, "scenes", sid + ".json")


def oracle_render(scene, width, height, spp, seed, idx_begin=0, idx_end=None, threads=0):
    L = oracle()
    cfg = PtoConfig(width, height, spp, 0, seed)
    idx_end = width * height if idx_end is None else idx_end
    out = np.zeros((width * height, 3), dtype=np.float32)
    cnt = PtoCounters()
    secs = C.c_double()
    ps = scene.pto()
    rc = L.pto_render(C.byref(ps), C.byref(cfg), idx_begin, idx_end, _np_f(out), threads, C.byref(cnt),
                      C.byref(secs))
    assert rc == 0
    return out, cnt, secs.value
