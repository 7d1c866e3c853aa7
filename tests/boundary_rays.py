"""Scenes and ray sets that sit on the boundaries the device's conservative tests rest on (CPU only, no GPU calls).

The intersect kernels do not evaluate the reference's arithmetic everywhere: the flat candidate filters (filter_flat) and
the BVH box tests (bvh_closest*, bvh_wants) first run conservative tests whose error bounds are argued in comments
(csrc/pt_host.cpp: FlatPairRec.hb / hc / tpad, the BVH box pads), and ties are settled by (distance, rank) keys.  A bound
that is too tight drops a true hit or lets a later primitive win, and only for rays near a boundary.  This module builds
such rays from a seed:

* scene families, one per bound: axis-perpendicular walls (sign_exact) next to walls tilted by 1e-7 / 1e-5 / 1e-3 rad and
  slivers; triangles near the |det| < 1e-4 rejection; scales 1e-2, 1 and 1e3 and a mesh far from the origin; BVH meshes of
  16, 17, 64, 500 and 5 000 triangles (soups and closed surfaces; the largest keeps its nodes in global memory); exact
  ties; spheres (tangent rays, origins inside and 1e-4 from the surface);
* ray families aimed at vertices, edges (f32 lerp) and centroids; at the corners and faces of the padded BVH boxes and
  the edges of the flat filter records READ FROM THE PRODUCT'S OWN TABLES (host::flatten_scene, dumped by
  host/tables_dump.cpp over the library's host code - the padding formulas are not restated here); directions with exact +-0
  components and components of 1e-19 .. 1e-38 and subnormal (the +-1e18 clamp and v_rcp_f32's sign decide); origins on
  the surfaces, taken from the oracle's own hit points as the path tracer's bounce rays are.

Every target also gets the same ray with one origin component and one direction component moved by -2, -1, +1, +2 ulp
(binary32).  All ray arithmetic is binary32; directions are normalised in f32 (unit within a few ulp) and origins lie in
the bounding box of the scene's objects and camera - the header's contract for pt_ctx_intersect / _streams.
"""
import atexit
import ctypes as C
import os
import shutil
import tempfile

import numpy as np

import ptlib
from ptlib import make_camera, make_mesh, make_sphere, make_tri, Scene

F = np.float32
ULP_STEPS = (-2, -1, 1, 2)
VARIANTS = 1 + 2 * len(ULP_STEPS)  # the target ray, then origin +-1/2 ulp, then direction +-1/2 ulp
RAY_KINDS = ["vertex", "edge", "centroid", "box", "flat_edge", "zero_dir", "tiny_dir", "surface", "sphere", "tie"]

# ---------------------------------------------------------------------------------------------------------- tables
_f2 = (np.float32, (2,))
_u2 = (np.uint32, (2,))
OBJ_DT = np.dtype([("c", np.float32, (3,)), ("rr", np.float32), ("kind", np.uint32), ("tri_begin", np.uint32),
                   ("tri_count", np.uint32), ("pair_begin", np.uint32), ("pair_count", np.uint32), ("bvh_root", np.int32),
                   ("rr_in", np.float32), ("pad1", np.uint32)])
PAIR_DT = np.dtype([(k, *_f2) for k in ("ax", "ay", "az", "e1x", "e1y", "e1z", "e2x", "e2y", "e2z")] + [("id", *_u2)])
NODE_DT = np.dtype([(k, *_f2) for k in ("lox", "loy", "loz", "hix", "hiy", "hiz")] + [("c", np.int32, (2,)), ("pad", *_u2)])
NODE4_DT = np.dtype([(k, np.float32, (4,)) for k in ("lox", "loy", "loz", "hix", "hiy", "hiz")] +
                    [("c", np.int32, (4,)), ("pad", np.uint32, (4,))])
FLAT_DT = np.dtype([(k, *_f2) for k in ("pc", "cb", "hb", "cc", "hc", "tpad")] + [("pair", *_u2), ("axis", np.uint32),
                                                                                   ("sign_exact", np.uint32)])
CAND_DT = np.dtype([(k, *_f2) for k in ("ax", "ay", "az", "e1x", "e1y", "e1z", "e2x", "e2y", "e2z")] +
                   [("id", *_u2), ("g", np.float32, (4,)), ("grr_in", np.float32), ("pad", np.uint32, (3,))])
MESH_DT = np.dtype([("c", np.float32, (3,)), ("rr", np.float32), ("root", np.int32), ("root4", np.int32), ("pad", *_u2)])
NO_PAIR = 0xffffffff
NO_TRI = 0x7fffffff

_work = None


def workdir():
    """this process's directory for the files the two table generators (host/tables_dump.cpp, host/layout_dump.cpp) read and write"""
    global _work
    if _work is None:
        _work = tempfile.mkdtemp(prefix="pt_tables_")
        atexit.register(shutil.rmtree, _work, True)
    return _work


def write_scene(sc, path):
    """The scene file of the two generators: u32 n_objs, u32 n_tris, pt_camera, pt_object[n_objs], pt_triangle[n_tris]."""
    with open(path, "wb") as f:
        f.write(np.array([sc.n_objs, sc.n_tris], np.uint32).tobytes())
        f.write(bytes(sc.cam))
        f.write(bytes(sc.objs)[:sc.n_objs * C.sizeof(ptlib.PtObject)])
        f.write(bytes(sc.tris)[:sc.n_tris * C.sizeof(ptlib.PtTriangle)])
    return path


def scene_tables(sc):
    """host::flatten_scene's tables of a scene (the records pt_ctx_set_scene uploads), as numpy record arrays.  The generator is the
    PLAIN build of host/tables_dump.cpp: GPU tests come through here, and no sanitizer build runs on a GPU machine
    (tests/test_boundary_rays.py holds the sanitized build to the same bytes)."""
    path_in, path_out = write_scene(sc, os.path.join(workdir(), "scene.bin")), os.path.join(workdir(), "tables.bin")
    out = ptlib.host_program("tables_dump", sanitize=False)(path_in, path_out).split()
    sizes = [int(v) for v in out[1:]]
    assert out[0] == "OK" and sizes == [t.itemsize for t in (OBJ_DT, PAIR_DT, NODE_DT, NODE4_DT, FLAT_DT, CAND_DT, MESH_DT)], out
    raw = open(path_out, "rb").read()
    h = np.frombuffer(raw[:64], np.uint32)
    pos = 64
    tabs = {"n_flat_exact": int(h[7]), "n_other_pairs": int(h[8]), "cand_ok": bool(h[11]), "bvh_stack": int(h[12])}
    for name, dt, cnt in (("objs", OBJ_DT, h[0]), ("tri_pairs", PAIR_DT, h[1]), ("bvh_nodes", NODE_DT, h[2]),
                          ("bvh_nodes4", NODE4_DT, h[3]), ("flat_pairs", FLAT_DT, h[4]), ("cand_pairs", CAND_DT, h[5]),
                          ("bvh_meshes", MESH_DT, h[6]), ("tri_rank", np.dtype(np.uint32), h[9]),
                          ("rank_id", np.dtype(np.uint32), h[10])):
        n = int(cnt) * dt.itemsize
        tabs[name] = np.frombuffer(raw[pos:pos + n], dt).copy()
        pos += n
    assert pos == len(raw)
    return tabs


def flat_record_triangles(sc, tabs, k, hf):
    """Flattened triangle indices of half `hf` of flat filter record k (via its candidate record's visiting ranks)."""
    p = int(tabs["flat_pairs"]["pair"][k][hf])
    if p == NO_PAIR:
        return []
    ids = tabs["cand_pairs"]["id"][p]
    return [int(tabs["rank_id"][r]) - sc.n_objs for r in ids if r != NO_TRI]


# ---------------------------------------------------------------------------------------------------------- scenes
def _mesh_obj(tris_local, tri_offset, position=(0, 0, 0), color=(0.7, 0.7, 0.7), emission=(0, 0, 0), reflect="Diffuse"):
    tl = [make_tri(*t) for t in tris_local]
    arr = (ptlib.PtTriangle * len(tl))(*tl)
    c, r = (C.c_float * 3)(), C.c_float()
    ptlib.oracle().pto_mesh_bounding_sphere(arr, len(tl), c, C.byref(r))
    return make_mesh(position, color, emission, reflect, tri_offset, len(tl), list(c), r.value), tl


class _Builder:
    def __init__(self):
        self.objs, self.tris = [], []

    def mesh(self, tris_local, position=(0, 0, 0), **kw):
        o, tl = _mesh_obj(tris_local, len(self.tris), position, **kw)
        self.objs.append(o)
        self.tris.extend(tl)

    def sphere(self, pos, r, color=(0.7, 0.7, 0.7), emission=(0, 0, 0), reflect="Diffuse"):
        self.objs.append(make_sphere(pos, r, color, emission, reflect))

    def scene(self, name, cam_pos, cam_dir=(0, 0, -1)):
        return Scene(name, make_camera(cam_pos, cam_dir), self.objs, self.tris)


def _quad(axis, coord, lo, hi, tilt=0.0):
    """Two triangles of the rectangle [lo, hi]^2 in the plane x_axis = coord; tilt (rad) turns it about axis+1."""
    b, c = (axis + 1) % 3, (axis + 2) % 3
    pts = []
    for (u, v) in ((lo, lo), (hi, lo), (hi, hi), (lo, hi)):
        p = np.zeros(3)
        p[axis] = coord + np.tan(tilt) * v
        p[b], p[c] = u, v
        pts.append(tuple(float(F(x)) for x in p))
    return [(pts[0], pts[1], pts[2]), (pts[0], pts[2], pts[3])]


def _soup(rng, n, centre, spread, size):
    out = []
    for _ in range(n):
        a = np.asarray(centre) + rng.uniform(-spread, spread, 3)
        out.append((tuple(a), tuple(a + rng.normal(0, size, 3)), tuple(a + rng.normal(0, size, 3))))
    return out


def _sphere_mesh(n_lat, n_lon, r=1.0, centre=(0, 0, 0), wobble=0.0):
    """A closed tessellated sphere (shared edges and vertices): 2 n_lon (n_lat - 1) triangles."""
    def P(i, j):
        t, p = np.pi * i / n_lat, 2 * np.pi * j / n_lon
        rr = r * (1.0 + wobble * np.sin(5 * t) * np.cos(3 * p))
        return tuple(float(F(v)) for v in (centre[0] + rr * np.sin(t) * np.cos(p), centre[1] + rr * np.cos(t),
                                           centre[2] + rr * np.sin(t) * np.sin(p)))
    out = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1)
            if i != 0:
                out.append((a, b, d))
            if i != n_lat - 1:
                out.append((b, c, d))
    return out


def _box_mesh(lo, hi, split):
    """A closed axis-aligned box, every face a grid of split x split quads (axis-perpendicular triangles)."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    out = []
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for side in (lo[axis], hi[axis]):
            g = [[None] * (split + 1) for _ in range(split + 1)]
            for i in range(split + 1):
                for j in range(split + 1):
                    p = np.zeros(3)
                    p[axis], p[b], p[c] = side, lo[b] + (hi[b] - lo[b]) * i / split, lo[c] + (hi[c] - lo[c]) * j / split
                    g[i][j] = tuple(float(F(v)) for v in p)
            for i in range(split):
                for j in range(split):
                    out.append((g[i][j], g[i + 1][j], g[i + 1][j + 1]))
                    out.append((g[i][j], g[i + 1][j + 1], g[i][j + 1]))
    return out


def _scaled(tris, s, shift=(0, 0, 0)):
    return [tuple(tuple(float(F(F(v) * F(s) + F(sh))) for v, sh in zip(p, shift)) for p in t) for t in tris]


def build_scenes(seed):
    """[(family, Scene)] for one seed."""
    rng = np.random.default_rng(seed)
    out = []
    # -- walls: axis-perpendicular (sign_exact), tilted by 1e-7 / 1e-5 / 1e-3 rad (not flat or not sign_exact), a sliver
    b = _Builder()
    for axis, coord in ((0, -2.0), (1, -1.5), (2, -3.0), (2, 1.0)):
        b.mesh(_quad(axis, coord, -1.5, 1.5))
    for k, tilt in enumerate((1e-7, 1e-5, 1e-3)):
        b.mesh(_quad(2, -1.0 - 0.5 * k, -1.0 + 0.3 * k, 0.8 + 0.3 * k, tilt))
    b.mesh([((0.0, 0.0, 0.5), (1.0, 1.0, 0.5), (1.0, 1.0005, 0.5)), ((-1.0, 0.0, 0.5), (-0.5, 0.0, 0.5), (-1.0, 0.5, 0.5))])
    out.append(("walls", b.scene("walls", (0.3, 0.2, 3.0))))
    # -- triangles near the |det| < 1e-4 rejection for unit rays: edges around 1e-2 (a BVH mesh and loose pairs)
    b = _Builder()
    b.mesh(_soup(rng, 40, (0, 0, 0), 0.6, 0.008))
    for k in range(6):
        e = float(F(0.008 + 0.002 * k))
        b.mesh([((0.1 * k, -0.5, -0.2), (0.1 * k + e, -0.5, -0.2), (0.1 * k, -0.5 + e, -0.2)),
                ((0.1 * k, 0.5, 0.1), (0.1 * k + e, 0.5, 0.1 + 0.3 * e), (0.1 * k, 0.5 + e, 0.1))])
    out.append(("near_det", b.scene("near_det", (0.0, 0.0, 1.5))))
    # -- scale: the same room at 1e-2, 1 and 1e3, and a mesh far from the coordinate origin
    room = _box_mesh((-1, -1, -1), (1, 1, 1), 2)
    inner = _sphere_mesh(6, 8, 0.35, (0.2, -0.1, 0.0), 0.05)
    soup = _soup(rng, 24, (-0.3, 0.3, 0.2), 0.3, 0.15)
    for s in (1e-2, 1.0, 1e3):
        b = _Builder()
        b.mesh(_scaled(room, s))
        b.mesh(_scaled(inner, s))
        b.mesh(_scaled(soup, s))
        b.mesh(_scaled(_quad(1, -0.6, -0.5, 0.5), s))
        b.sphere((0.5 * s, 0.5 * s, -0.4 * s), 0.2 * s)
        out.append(("scale", b.scene("scale%g" % s, (0.1 * s, 0.2 * s, 0.9 * s))))
    b = _Builder()
    far = (3000.0, -2000.0, 1000.0)
    b.mesh(_sphere_mesh(8, 10, 1.0, (0, 0, 0), 0.08), position=far)
    b.mesh(_quad(2, -1.5, -2.0, 2.0), position=far)
    b.mesh(_box_mesh((-0.5, -0.5, 1.2), (0.5, 0.5, 1.4), 2), position=far)
    out.append(("scale", b.scene("far", (far[0] + 0.2, far[1] + 0.1, far[2] + 2.5))))
    # -- BVH meshes of 16 (kBvhMinTris), 17, 64, 500 and 5 000 triangles: soups and closed surfaces
    b = _Builder()
    b.mesh(_soup(rng, 16, (-1.2, 0, 0), 0.5, 0.3))
    b.mesh(_soup(rng, 17, (1.2, 0, 0), 0.5, 0.3))
    b.mesh(_sphere_mesh(5, 8, 0.6, (0, 1.2, 0)))  # 64 triangles
    b.mesh(_box_mesh((-0.4, -1.6, -0.4), (0.4, -0.8, 0.4), 1) + _soup(rng, 52, (0, -1.2, 0), 0.3, 0.1))
    out.append(("bvh", b.scene("bvh_small", (0.0, 0.0, 3.0))))
    b = _Builder()
    b.mesh(_sphere_mesh(16, 16, 1.0, (0, 0, 0), 0.06))  # 480 triangles
    b.mesh(_soup(rng, 500, (0, 0, 0), 1.6, 0.12))
    out.append(("bvh", b.scene("bvh_500", (0.3, 0.2, 3.2))))
    b = _Builder()
    b.mesh(_sphere_mesh(50, 51, 1.0, (0, 0, 0), 0.05))  # 5 049 triangles: more than kBvhMaxLdsNodes nodes
    b.mesh(_quad(1, -1.2, -2.0, 2.0))
    out.append(("bvh", b.scene("bvh_5000", (0.2, 0.3, 2.8))))
    # -- exact ties: the reference keeps the first in scan order (objects from the last to the first)
    b = _Builder()
    base = _sphere_mesh(4, 6, 0.5, (0, 0, 0))  # 36 triangles
    dup = list(base)
    dup[3:3] = [base[5]] * 3                   # copies next to each other: the same leaf
    dup += [base[5], base[10], base[10]]       # and at the end of the list: other leaves
    b.mesh(dup, position=(-1.0, 0.0, 0.0))
    b.mesh(base, position=(1.0, 0.0, 0.0))     # two coincident BVH meshes: ties across walks
    b.mesh(base, position=(1.0, 0.0, 0.0))
    b.mesh([((-0.5, -1.5, 0.0), (0.5, -1.5, 0.0), (0.5, -0.5, 0.0)), ((-0.5, -1.5, 0.0), (0.5, -0.5, 0.0), (-0.5, -0.5, 0.0)),
            ((-0.25, -1.25, 0.0), (0.75, -1.25, 0.0), (0.25, -0.75, 0.0))])  # coplanar overlapping triangles
    b.sphere((0.0, 1.2, 0.0), 0.4)             # coincident spheres
    b.sphere((0.0, 1.2, 0.0), 0.4)
    b.mesh(_quad(2, 0.0, -0.25, 0.25), position=(-1.0, -1.5, 0.5))  # a sphere tangent to a wall: equal distances
    b.sphere((-1.0, -1.5, -0.5), 1.0)
    b.mesh(_box_mesh((-0.25, -0.25, 0.0), (0.25, 0.25, 0.5), 2), position=(1.5, -1.5, -1.5))  # a BVH box with a tangent sphere
    b.sphere((1.5, -1.5, -2.5), 1.0)
    # the same two kinds of tie with the triangles visited FIRST (the higher object index), so that they must win: a flat
    # record's wall, and a BVH mesh of edges 1/64 whose boxes carry a pad of about 1e-4 - a walk the bound of bvh_wants admits
    # only if that bound is not too tight
    b.sphere((-2.0, 1.5, -1.0), 0.5)
    b.mesh(_quad(2, 0.0, -0.25, 0.25), position=(-2.0, 1.5, -0.5))
    b.sphere((2.0, 1.5, -1.0), 0.5)
    b.mesh(_box_mesh((-1 / 64, -1 / 64, 0.0), (1 / 64, 1 / 64, 1 / 32), 2), position=(2.0, 1.5, -0.5))
    sc = b.scene("ties", (0.0, 0.0, 3.0))
    # axis-parallel rays through the tangent points: sphere and triangle at exactly the same distance (from outside the
    # sphere: the near root; from inside it: the far root)
    z_out = [0.75 + 0.25 * k for k in range(10)]
    z_in = [-3.0, -2.75, -2.5, -2.25, -2.0, -1.75]
    z_wall = [0.125 * k for k in range(14)]
    z_small = [-1.375 + 0.125 * k for k in range(7)]
    sc.tie_rays = (np.array([(-1.0, -1.5, z) for z in z_out] + [(1.5, -1.5, z) for z in z_in] +
                            [(-2.0, 1.5, z) for z in z_wall] + [(2.0, 1.5, z) for z in z_small], F),
                   np.array([(0.0, 0.0, -1.0)] * len(z_out) + [(0.0, 0.0, 1.0)] * len(z_in) +
                            [(0.0, 0.0, -1.0)] * len(z_wall) + [(0.0, 0.0, 1.0)] * len(z_small), F))
    out.append(("ties", sc))
    # -- spheres: tangent rays, origins inside and about 1e-4 from the surface
    b = _Builder()
    for k in range(5):
        b.sphere((float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1.5, 0.5))),
                 float(rng.choice([0.05, 0.3, 1.0])))
    b.sphere((0.0, 0.0, 0.0), 2.5, reflect="Refract")
    b.mesh(_quad(1, -2.0, -2.0, 2.0))
    out.append(("spheres", b.scene("spheres", (0.0, 0.5, 2.0))))
    return out


# ---------------------------------------------------------------------------------------------------------- rays
def scene_box(sc):
    """Bounding box of the scene's objects and camera (the origins' domain)."""
    pts = [np.array(list(sc.cam.position), F)]
    for i in range(sc.n_objs):
        o = sc.objs[i]
        p = np.array(list(o.position), F)
        if o.kind == ptlib.PT_SPHERE:
            pts += [p - F(o.radius), p + F(o.radius)]
        else:
            for k in range(o.tri_offset, o.tri_offset + o.tri_count):
                t = sc.tris[k]
                pts += [np.array(list(t.a), F) + p, np.array(list(t.b), F) + p, np.array(list(t.c), F) + p]
    pts = np.array(pts, F)
    return pts.min(0), pts.max(0)


def _normalise(v):
    v = np.asarray(v, F)
    n = np.sqrt(np.sum(v * v, axis=-1, keepdims=True, dtype=F)).astype(F)
    return (v / np.where(n > 0, n, F(1))).astype(F)


def _world_tris(sc):
    """(n_tris, 3, 3) world-space vertices as Triangle::transformed makes them (f32 adds)."""
    v = np.zeros((sc.n_tris, 3, 3), F)
    for i in range(sc.n_objs):
        o = sc.objs[i]
        if o.kind != ptlib.PT_MESH:
            continue
        p = np.array(list(o.position), F)
        for k in range(o.tri_offset, o.tri_offset + o.tri_count):
            t = sc.tris[k]
            v[k] = np.array([list(t.a), list(t.b), list(t.c)], F) + p
    return v


def _step(x, k):
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf)).astype(F)
    return x


def _variants(o, d, rng):
    """Each target ray, then its origin moved along one axis and its direction along one axis by -2, -1, +1, +2 ulp."""
    n = len(o)
    oa, da = rng.integers(0, 3, n), rng.integers(0, 3, n)
    oo, dd = [o], [d]
    for k in ULP_STEPS:
        x = o.copy()
        x[np.arange(n), oa] = _step(o[np.arange(n), oa], k)
        oo.append(x)
        dd.append(d)
    for k in ULP_STEPS:
        x = d.copy()
        x[np.arange(n), da] = _step(d[np.arange(n), da], k)
        oo.append(o)
        dd.append(x)
    # ray-major: target i's variants are rays [i * VARIANTS, (i + 1) * VARIANTS)
    return np.stack(oo, 1).reshape(-1, 3), np.stack(dd, 1).reshape(-1, 3)


def _aim(rng, lo, hi, tgt):
    """Origins uniform in [lo, hi], directions towards the targets (f32, unit); targets equal to their origin dropped."""
    o = rng.uniform(lo, hi, size=(len(tgt), 3)).astype(F)
    d = (np.asarray(tgt, F) - o).astype(F)
    ok = np.sum(d * d, 1) > F(1e-12) * F(1.0 + float(np.max(np.abs(hi - lo))) ** 2)
    return o[ok], _normalise(d[ok])


def _clip_origins(o, lo, hi):
    return np.minimum(np.maximum(o, lo), hi).astype(F)


def build_rays(sc, tabs, rng, per_kind=160):
    """(o, d, kind) of the scene: targets of every ray family, each followed by its VARIANTS - 1 ulp variants."""
    lo, hi = scene_box(sc)
    ext = (hi - lo).astype(F)
    W = _world_tris(sc)
    groups = []  # (kind index, o, d) of target rays

    def add(kind, o, d):
        if len(o):
            o = _clip_origins(np.asarray(o, F), lo, hi)
            groups.append((RAY_KINDS.index(kind), o.astype(F), _normalise(d)))

    if sc.n_tris:
        pick = rng.integers(0, sc.n_tris, per_kind)
        add("vertex", *_aim(rng, lo, hi, W[pick, rng.integers(0, 3, per_kind)]))
        pick = rng.integers(0, sc.n_tris, per_kind)
        e0 = rng.integers(0, 3, per_kind)
        a, bb = W[pick, e0], W[pick, (e0 + 1) % 3]
        s = rng.uniform(size=(per_kind, 1)).astype(F)
        add("edge", *_aim(rng, lo, hi, (a + (bb - a) * s).astype(F)))  # f32 lerp
        pick = rng.integers(0, sc.n_tris, per_kind)
        add("centroid", *_aim(rng, lo, hi, ((W[pick, 0] + W[pick, 1] + W[pick, 2]) / F(3)).astype(F)))
    # corners and face points of the padded BVH boxes (binary tree: the boxes every walker tests)
    nodes = tabs["bvh_nodes"]
    if len(nodes):
        k = rng.integers(0, len(nodes), per_kind)
        h = rng.integers(0, 2, per_kind)
        blo = np.stack([nodes["lox"][k, h], nodes["loy"][k, h], nodes["loz"][k, h]], 1)
        bhi = np.stack([nodes["hix"][k, h], nodes["hiy"][k, h], nodes["hiz"][k, h]], 1)
        corner = np.where(rng.integers(0, 2, (per_kind, 3)) == 1, bhi, blo).astype(F)
        face = (blo + (bhi - blo) * rng.uniform(size=(per_kind, 3)).astype(F)).astype(F)
        ax = rng.integers(0, 3, per_kind)
        ar = np.arange(per_kind)
        face[ar, ax] = np.where(rng.integers(0, 2, per_kind) == 1, bhi[ar, ax], blo[ar, ax])
        tgt = np.where((np.arange(per_kind) % 2 == 0)[:, None], corner, face)
        o, d = _aim(rng, lo, hi, tgt)
        add("box", o, d)
        # origins ON a box face with the direction component across it exactly +-0 or tiny: the slab test's 0 * inf and
        # the +-1e18 clamp decide
        o = face.copy()
        d = _normalise(rng.normal(size=(per_kind, 3)))
        tiny = rng.choice([0.0, -0.0, 1e-19, -1e-19, 1e-30, -1e-38, 1e-40, -1e-44], per_kind).astype(F)
        d[np.arange(per_kind), ax] = 0.0
        d = _normalise(d)
        d[np.arange(per_kind), ax] = tiny
        add("tiny_dir", o, d)
    # the edges of the flat filter records' padded rectangles
    fl = tabs["flat_pairs"]
    if len(fl):
        rec = []
        for k in range(len(fl)):
            for hf in range(2):
                if fl["pair"][k][hf] != NO_PAIR:
                    rec.append((k, hf))
        pick = rng.integers(0, len(rec), per_kind)
        tgt = np.zeros((per_kind, 3), F)
        for i, p in enumerate(pick):
            k, hf = rec[p]
            a = int(fl["axis"][k])
            bx, cx = (a + 1) % 3, (a + 2) % 3
            cb, hb, cc, hc = (F(fl[f][k][hf]) for f in ("cb", "hb", "cc", "hc"))
            ub, uc = F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1))
            if i % 2 == 0:
                ub = F(1) if rng.random() < 0.5 else F(-1)
            else:
                uc = F(1) if rng.random() < 0.5 else F(-1)
            tgt[i, a] = fl["pc"][k][hf]
            tgt[i, bx] = cb + hb * ub
            tgt[i, cx] = cc + hc * uc
        add("flat_edge", *_aim(rng, lo, hi, tgt))
    # directions with exact +-0 components, aimed at vertices (the rays lie in planes through the vertex)
    if sc.n_tris:
        pick = rng.integers(0, sc.n_tris, per_kind)
        tgt = W[pick, rng.integers(0, 3, per_kind)]
        d = _normalise(rng.normal(size=(per_kind, 3)))
        for i in range(per_kind):
            for axz in rng.choice(3, int(rng.integers(1, 3)), replace=False):
                d[i, axz] = F(0.0) if rng.random() < 0.5 else F(-0.0)
        d = _normalise(d)
        o = (tgt - d * F(rng.uniform(0.2, 1.0)) * F(np.max(ext))).astype(F)
        keep = np.all((o >= lo) & (o <= hi), 1) & (np.abs(d).sum(1) > 0)
        add("zero_dir", o[keep], d[keep])
        # components of magnitude 1e-19 .. 1e-38 and subnormal, origins level with a vertex along that axis
        d = _normalise(rng.normal(size=(per_kind, 3)))
        axz = rng.integers(0, 3, per_kind)
        d[np.arange(per_kind), axz] = 0.0
        d = _normalise(d)
        d[np.arange(per_kind), axz] = rng.choice([1e-19, -1e-19, 1e-25, -1e-30, 1e-38, -1e-38, 3e-41, -1e-45], per_kind).astype(F)
        tgt = W[rng.integers(0, sc.n_tris, per_kind), rng.integers(0, 3, per_kind)]
        o = (tgt - d * F(0.5) * F(np.max(ext))).astype(F)
        o[np.arange(per_kind), axz] = tgt[np.arange(per_kind), axz]
        keep = np.all((o >= lo) & (o <= hi), 1)
        add("tiny_dir", o[keep], d[keep])
    if getattr(sc, "tie_rays", None) is not None:
        add("tie", *sc.tie_rays)
    # spheres: tangent rays, origins inside, origins about 1e-4 from the surface
    sph = [i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_SPHERE]
    if sph:
        n = per_kind
        idx = rng.integers(0, len(sph), n)
        c = np.array([list(sc.objs[sph[j]].position) for j in idx], F)
        r = np.array([sc.objs[sph[j]].radius for j in idx], F)[:, None]
        u = _normalise(rng.normal(size=(n, 3)))
        w = _normalise(np.cross(u, rng.normal(size=(n, 3))).astype(F))
        mode = np.arange(n) % 3
        tangent_o = (c + u * r - w * F(0.5) * r * F(4)).astype(F)  # towards the point c + u r along w: tangent
        tangent_d = w
        inside_o = (c + u * r * F(0.5)).astype(F)
        inside_d = _normalise(rng.normal(size=(n, 3)))
        off = rng.choice([1e-4, -1e-4, 1.5e-4, -0.5e-4, 0.0], n).astype(F)[:, None]
        near_o = (c + u * (r + off)).astype(F)
        near_d = _normalise(np.where(rng.random((n, 1)) < 0.5, u, -u) + rng.normal(0, 0.3, (n, 3)).astype(F))
        o = np.where((mode == 0)[:, None], tangent_o, np.where((mode == 1)[:, None], inside_o, near_o))
        d = np.where((mode == 0)[:, None], tangent_d, np.where((mode == 1)[:, None], inside_d, near_d))
        add("sphere", o, d)
    # origins on the surfaces: the oracle's own hit points of the rays so far, sent off as bounce rays
    o_all = np.concatenate([g[1] for g in groups])
    d_all = np.concatenate([g[2] for g in groups])
    pick = rng.permutation(len(o_all))[:4 * per_kind]
    t, oid, tid, x, nr = ptlib.oracle_intersect(sc, o_all[pick], d_all[pick])
    hit = oid >= 0
    x, nr, din = x[hit], nr[hit], d_all[pick][hit]
    if len(x):
        m = min(len(x), 2 * per_kind)
        x, nr, din = x[:m], nr[:m], din[:m]
        side = np.where(np.sum(nr * din, 1, keepdims=True) < 0, nr, -nr).astype(F)  # normal_towards_ray
        hemi = _normalise(rng.normal(size=(m, 3)))
        hemi = np.where(np.sum(hemi * side, 1, keepdims=True) < 0, -hemi, hemi).astype(F)
        refl = _normalise(din - nr * F(2) * np.sum(nr * din, 1, keepdims=True).astype(F))
        back = rng.random(m) < 0.15  # some leave through the surface (refraction)
        d = np.where((np.arange(m) % 2 == 0)[:, None], hemi, refl)
        d = np.where(back[:, None], -d, d)
        add("surface", x, d)
    kinds, os_, ds_ = [], [], []
    for kind, o, d in groups:
        vo, vd = _variants(o, d, rng)
        os_.append(vo)
        ds_.append(vd)
        kinds.append(np.full(len(vo), kind, np.int8))
    o = _clip_origins(np.concatenate(os_), lo, hi)
    return np.ascontiguousarray(o, F), np.ascontiguousarray(np.concatenate(ds_), F), np.concatenate(kinds)


class RaySet:
    """One scene of a family, its product tables and its boundary rays (o, d, kind per ray; VARIANTS rays per target)."""

    def __init__(self, family, sc, tabs, o, d, kind):
        self.family, self.scene, self.tables = family, sc, tabs
        self.o, self.d, self.kind = o, d, kind

    @property
    def n(self):
        return len(self.o)


def build(seed=20261016, per_kind=160):
    """Every family's scenes and ray sets for a seed: [RaySet]."""
    out = []
    for k, (family, sc) in enumerate(build_scenes(seed)):
        tabs = scene_tables(sc)
        rng = np.random.default_rng([seed, k])
        o, d, kind = build_rays(sc, tabs, rng, per_kind)
        out.append(RaySet(family, sc, tabs, o, d, kind))
    return out


def verdict_flips(ids):
    """Targets whose oracle verdict (hit or miss, object, triangle: one id per ray) is not the same on all their variants."""
    g = np.asarray(ids).reshape(-1, VARIANTS)
    return np.any(g != g[:, :1], axis=1)


def first_hit_variant(sc, keep_color=False):
    """The scene with a distinct emission per object and every object black (roulette always stops: max_reflection = 0, so
    radiance at depth 5 is exactly the emission of the first object hit, or zero on a miss) - or, keep_color=True, with
    the colours kept (paths go on, and what the first hit was changes the rest of the path)."""
    objs = []
    for i in range(sc.n_objs):
        o = sc.objs[i]
        em = (float(i + 1), 0.5 * float(2 * i + 1), 1.0 / float(i + 1))
        col = list(o.color) if keep_color else (0, 0, 0)
        if o.kind == ptlib.PT_SPHERE:
            objs.append(make_sphere(list(o.position), o.radius, col, em, o.reflect_type))
        else:
            objs.append(make_mesh(list(o.position), col, em, o.reflect_type, o.tri_offset, o.tri_count,
                                  list(o.bs_center), o.bs_radius))
    return Scene(sc.id + ("_shaded" if keep_color else "_first_hit"), sc.cam, objs, [sc.tris[k] for k in range(sc.n_tris)])
