"""pt_ctx_set_object on the device: replacing one object of a context's scene gives, bit for bit, what a FRESH context gives
after pt_ctx_set_scene with the edited objects - on the MATERIAL path, on the MOVE path inside the scene's reach (a sphere, a
listed mesh, a mesh with a BVH refit by the kernels of pt_refit.hip) and out of reach (the tables rebuilt) - and every case
asserts the `rebuilt` flag it expects.  The edited context is never compared against itself.

Scenes, the smallest that reach each branch: cornell.json (spheres; wall meshes below 16 triangles with flat filters);
mesh.json (810 triangles); generated terrains of 16 (the smallest BVH), 17 (a half-filled record) and 19 triangles (the cnt == 3
split), one of 64 with a zero-length edge and a zero-area triangle, one of 5 000 (the leaf kernel spans many workgroups, the
tree has a dozen heights), and a scene of two meshes with a BVH.  The terrains are EXACT fixtures: every coordinate a
multiple of 1/8, so that after a move by multiples of 1/8 the SAH tree is the original's and the refit must reproduce a fresh
build's tables to the bit (pt_ctx_table_hashes).  Frames are 64x48 at 2 to 8 samples per pixel."""
import ctypes as C
import os

import numpy as np
import pytest

import gpudev
import ptlib
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtObject, PtTriangle

pytestmark = pytest.mark.gpu

PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
NO_BVH, SEPARATE = ptlib.abi.PT_FLAG_NO_BVH, ptlib.abi.PT_FLAG_SEPARATE_KERNELS
W, H, SEED = 64, 48, 23
F32 = np.float32
fp = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
TABLES = ("objs", "obj_pairs", "tri_pairs", "mats", "tri_shade", "bvh_nodes", "bvh_nodes4", "sph_pairs", "flat_pairs", "cand_pairs",
          "rank_id", "surf", "tri_rank", "bvh_meshes")
INEXACT = (0.1, -1.0 / 3.0, 0.07)


# ------------------------------------------------------------------------------------------------------- scenes
def lcg(s):
    return (s * 1664525 + 1013904223) & 0xffffffff


def terrain(q, n, seed):
    """host/object_check.cpp's terrain: q x q quads, two triangles each, the first n; every coordinate a multiple of 1/8"""
    h, s = [], seed
    for _ in range((q + 1) * (q + 1)):
        s = lcg(s)
        h.append((s >> 26) * 0.125)
    vert = lambda i, j: (i * 0.375 - 1.0, h[i * (q + 1) + j], j * 0.625 - 2.0)
    out = []
    for i in range(q):
        for j in range(q):
            out.append((vert(i, j), vert(i + 1, j), vert(i + 1, j + 1)))
            out.append((vert(i, j), vert(i + 1, j + 1), vert(i, j + 1)))
    assert len(out) >= n
    return out[:n]


def mesh_of(L, tris, offset, position, color=(0.75, 0.5, 0.25), reflect=0):
    arr = (PtTriangle * len(tris))(*[ptlib.make_tri(*t) for t in tris])
    ctr, rad = (C.c_float * 3)(), C.c_float()
    assert L.pt_mesh_bounding_sphere(arr, len(tris), ctr, C.byref(rad)) == 0
    return ptlib.make_mesh(position, color, (0, 0, 0), reflect, offset, len(tris), list(ctr), rad.value)


def terrain_scene(L, sid, parts):
    """a floor sphere, a light and the terrains `parts` = [(triangles, position)]: exact coordinates throughout; the floor's
    box holds every move the tests make, so the scene's reach does too"""
    objs = [ptlib.make_sphere((0, -64, 0), 62.0, (0.75, 0.75, 0.75), (0, 0, 0), 0)]
    tris = []
    for t, pos in parts:
        objs.append(mesh_of(L, t, len(tris), pos))
        tris += t
    objs.append(ptlib.make_sphere((2, 14, -1), 3.0, (0, 0, 0), (12, 12, 12), 0))
    cam = ptlib.make_camera((0.5, 7.0, -14.0), (0.0, -0.3125, 1.0))
    return ptlib.Scene(sid, cam, objs, [ptlib.make_tri(*t) for t in tris])


_scenes = {}


def scene(L, sid):
    """-> (scene, index of the object the tests edit)"""
    if sid in _scenes:
        return _scenes[sid]
    if sid in ("cornell-sphere", "cornell-wall"):
        sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
        kind = ptlib.PT_SPHERE if sid == "cornell-sphere" else ptlib.PT_MESH
        index = [i for i in range(sc.n_objs) if sc.objs[i].kind == kind and not any(sc.objs[i].emission)][0]
    elif sid == "mesh":
        sc = ptlib.load_scene_py(ptlib.scene_path("mesh"))
        index = max(range(sc.n_objs), key=lambda i: sc.objs[i].tri_count)
        assert sc.objs[index].tri_count == 810
    elif sid == "two-meshes":
        sc, index = terrain_scene(L, sid, [(terrain(6, 40, 21), (-3, 0, 0)), (terrain(6, 33, 22), (3, 0, 0))]), 2
    else:
        n = int(sid[3:])
        t = terrain(50 if n > 1000 else 6, n, 7 + n)
        if sid == "bvh64":  # a zero-length edge (the normal is NaN) and a zero-area triangle
            t[5] = (t[5][0], t[5][0], t[5][2])
            t[9] = (t[9][0], t[9][1], t[9][1])
        sc, index = terrain_scene(L, sid, [(t, (0, 0, 0))]), 1
    _scenes[sid] = (sc, index)
    return _scenes[sid]


BVH_SCENES = ("bvh16", "bvh17", "bvh19", "bvh64", "bvh5000", "two-meshes")
ALL_SCENES = ("cornell-sphere", "cornell-wall", "mesh") + BVH_SCENES


def edited(sc, index, **changes):
    """a copy of the scene's objects with object `index` changed: position=, move=, color=, emission=, reflect_type=, radius="""
    objs = [PtObject.from_buffer_copy(sc.objs[i]) for i in range(sc.n_objs)]
    o = objs[index]
    if "move" in changes:
        o.position = ptlib.f3(*[float(F32(F32(p) + F32(d))) for p, d in zip(o.position, changes.pop("move"))])
    for k, v in changes.items():
        setattr(o, k, ptlib.f3(*[float(F32(x)) for x in v]) if isinstance(v, tuple) else v)
    out = ptlib.Scene(sc.id, sc.cam, objs, [])
    out.tris, out.n_tris = sc.tris, sc.n_tris
    return out


# ------------------------------------------------------------------------------------------------------- the device
class Dev(gpudev.Device):
    """a context with one frame buffer and four AOV planes of W*H pixels"""

    def __init__(self, L, sc):
        super().__init__(L, sc)
        self.bufs = [self.alloc(W * H * k * 4) for k in (3, 3, 3, 1, 1)]

    def set_object(self, index, obj, expect=None):
        rebuilt = C.c_int(-7)
        assert self.L.pt_ctx_set_object(self.ctx, index, C.byref(obj), C.byref(rebuilt)) == 0, self.L.pt_last_error()
        assert rebuilt.value in (0, 1)
        if expect is not None:
            assert rebuilt.value == expect, "rebuilt = %d, the case expects %d" % (rebuilt.value, expect)
        return rebuilt.value

    def reach(self):
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        assert self.L.pt_ctx_camera_reach(self.ctx, lo, hi) == 0, self.L.pt_last_error()
        return np.array(list(lo), F32), np.array(list(hi), F32)

    def reserve(self, lo, hi):
        rebuilt = C.c_int(-7)
        assert self.L.pt_ctx_reserve_camera_reach(self.ctx, ptlib.f3(*[float(x) for x in lo]), ptlib.f3(*[float(x) for x in hi]),
                                                  C.byref(rebuilt)) == 0, self.L.pt_last_error()
        return rebuilt.value

    def hashes(self):
        out = (C.c_uint64 * len(TABLES))()
        assert self.L.pt_ctx_table_hashes(self.ctx, out) == 0, self.L.pt_last_error()
        return dict(zip(TABLES, out))

    def fetch(self, i, n, dt=F32):
        return self.download(self.bufs[i], n, dt)

    def render(self, cfg, accumulate=False):
        img, st = super().render(cfg, self.bufs[0], accumulate)
        return img.tobytes(), st

    def aov(self, cfg):
        assert self.L.pt_ctx_render_aov(self.ctx, C.byref(cfg), self.bufs[1], self.bufs[2], self.bufs[3], self.bufs[4], None) == 0, \
            self.L.pt_last_error()
        n = cfg.width * cfg.height
        return [self.fetch(1, n * 3).tobytes(), self.fetch(2, n * 3).tobytes(), self.fetch(3, n).tobytes(), self.fetch(4, n, np.int32).tobytes()]

    def primary_rays(self):
        n = W * H
        pixel = np.arange(n, dtype=np.uint32)
        sample = (pixel % 4).astype(np.uint32)
        o, d = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        assert self.L.pt_ctx_primary_rays(self.ctx, W, H, SEED, pixel.ctypes.data_as(u32p), sample.ctypes.data_as(u32p), n, 0,
                                          o.ctypes.data_as(fp), d.ctypes.data_as(fp)) == 0, self.L.pt_last_error()
        return o, d

    def intersect(self, o, d):
        n = len(o)
        t, oid, tid, x, nr = np.zeros(n, F32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        assert self.L.pt_ctx_intersect(self.ctx, o.ctypes.data_as(fp), d.ctypes.data_as(fp), n, t.ctypes.data_as(fp), oid.ctypes.data_as(i32p),
                                       tid.ctypes.data_as(i32p), x.ctypes.data_as(fp), nr.ctypes.data_as(fp)) == 0, self.L.pt_last_error()
        return [a.tobytes() for a in (t, oid, tid, x, nr)], oid

    def intersect_streams(self, o, d, flags):
        n = len(o)
        t, ids = np.zeros(n, F32), np.zeros(n, np.int32)
        assert self.L.pt_ctx_intersect_streams(self.ctx, o.ctypes.data_as(fp), d.ctypes.data_as(fp), n, flags, t.ctypes.data_as(fp),
                                               ids.ctypes.data_as(i32p)) == 0, self.L.pt_last_error()
        return t.tobytes() + ids.tobytes()

    def bounds(self, obj, o, d):
        n = len(o)
        hit, t = np.zeros(n, np.int32), np.zeros(n, F32)
        assert self.L.pt_ctx_intersect_bounds(self.ctx, obj, o.ctypes.data_as(fp), d.ctypes.data_as(fp), n, hit.ctypes.data_as(i32p),
                                              t.ctypes.data_as(fp), None, None) == 0, self.L.pt_last_error()
        return hit, t

    def accum_info(self, cfg):
        lo, hi = C.c_uint32(), C.c_uint32()
        assert self.L.pt_ctx_accum_info(self.ctx, C.byref(cfg), C.byref(lo), C.byref(hi)) == 0
        return lo.value, hi.value


def cfg_of(spp, flags=0, backend=0):
    return gpudev.config(W, H, spp, backend=backend, seed=SEED, flags=flags)


def surface_rays(sc, index):
    """rays that start ON the triangles of mesh `index` as the scene places it: up to 512 centroids, directions from a generator"""
    o = sc.objs[index]
    if o.kind != ptlib.PT_MESH:
        return np.zeros((0, 3), F32), np.zeros((0, 3), F32)
    n = min(o.tri_count, 512)
    tri = np.array([[list(getattr(sc.tris[o.tri_offset + k], v)) for v in "abc"] for k in range(n)], F32)
    org = (tri.sum(axis=1, dtype=F32) / F32(3.0) + np.array(list(o.position), F32)).astype(F32)
    rng = np.random.default_rng(5)
    d = rng.standard_normal((n, 3)).astype(F32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return org, d


def everything(dev, sc, index, frames=True):
    """every result of a context that the scene decides, as named byte strings"""
    out = {}
    if frames:
        for name, cfg in (("wavefront", cfg_of(4)), ("megakernel", cfg_of(4, backend=1)), ("no-bvh", cfg_of(2, flags=NO_BVH)),
                          ("separate", cfg_of(2, flags=SEPARATE))):
            img, st = dev.render(cfg)
            out[name] = img
            out[name + " ray_bounces"] = st.ray_bounces
            assert st.ray_bounces >= W * H * cfg.spp
        for name, plane in zip(("albedo", "normal", "depth", "object_id"), dev.aov(cfg_of(4))):
            out["aov " + name] = plane
    po, pd = dev.primary_rays()
    so, sd = surface_rays(sc, index)
    o, d = np.ascontiguousarray(np.vstack([po, so])), np.ascontiguousarray(np.vstack([pd, sd]))
    out["rays"] = po.tobytes() + pd.tobytes()
    hits, oid = dev.intersect(o, d)
    for name, a in zip(("t", "object_id", "tri_id", "x", "normal"), hits):
        out["intersect " + name] = a
    out["intersect_streams"] = dev.intersect_streams(o, d, 0)
    out["intersect_streams no-bvh"] = dev.intersect_streams(o, d, NO_BVH)
    return out, float((oid == index).mean())


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], "%s: %s differs" % (what, k)


def room_to_move(dev):
    """cornell's walls and mesh.json's room ARE the scene's box: reserve one unit around it, so that a move stays in reach"""
    lo, hi = dev.reach()
    dev.reserve(lo - F32(1.0), hi + F32(1.0))


# ------------------------------------------------------------------------------------------------------- 1. MOVE in reach
@pytest.mark.parametrize("sid", ALL_SCENES)
def test_move_in_reach_equals_a_fresh_context(L, sid):
    sc, index = scene(L, sid)
    moved = edited(sc, index, move=INEXACT)
    dev, fresh = Dev(L, sc), Dev(L, moved)
    try:
        room_to_move(dev)
        before, _ = everything(dev, sc, index)
        dev.set_object(index, moved.objs[index], expect=0)
        got, on_it = everything(dev, moved, index)
        want, _ = everything(fresh, moved, index)
        assert on_it > 0.0, "no ray reaches the moved object"
        assert_same(got, want, sid + " moved")
        assert got["wavefront"] != before["wavefront"] and got["intersect t"] != before["intersect t"]
        # back: the original frames return
        dev.set_object(index, sc.objs[index], expect=0)
        again, _ = everything(dev, sc, index)
        assert_same(again, before, sid + " moved back")
    finally:
        dev.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------------- 2. exact moves: the tables
@pytest.mark.parametrize("sid", ("cornell-sphere", "cornell-wall") + BVH_SCENES)
def test_tables_equal_a_fresh_builds(L, sid):
    """Spheres and listed meshes: any move (no tree is involved).  Meshes with a BVH: moves by multiples of 1/8 on the exact
    fixtures, where a fresh build chooses the tree the refit kept.  Both contexts hold the same box B."""
    sc, index = scene(L, sid)
    moves = (INEXACT, (0.125, -0.25, 0.5)) if sid.startswith("cornell") else ((0.125, -0.5, 1.0), (-2.25, 0.375, -0.125), (0.0, 0.0, 0.0))
    with Dev(L, sc) as dev:
        room_to_move(dev)
        lo, hi = dev.reach()
        for mv in moves:
            to = edited(sc, index, position=tuple(float(F32(p) + F32(d)) for p, d in zip(sc.objs[index].position, mv)))
            if mv[0] < 0.0:
                to = edited(to, index, color=(0.125, 0.5, 1.0), reflect_type=1)  # the material with the move
            dev.set_object(index, to.objs[index], expect=0)
            with Dev(L, to) as fresh:
                fresh.reserve(lo, hi)
                flo, fhi = fresh.reach()
                assert flo.tobytes() == lo.tobytes() and fhi.tobytes() == hi.tobytes()
                got, want = dev.hashes(), fresh.hashes()
                assert got == want, (sid, mv, [k for k in TABLES if got[k] != want[k]])


# ------------------------------------------------------------------------------------------------------- 3. MATERIAL edits
GEOMETRY = tuple(t for t in TABLES if t not in ("mats", "surf"))


@pytest.mark.parametrize("sid", ("cornell-sphere", "bvh5000"))
def test_material_edits(L, sid, monkeypatch):
    """colour, emission, diffuse -> refract -> specular: the frames of a fresh context, no geometry table touched.  With the glass
    deferral switched on (PT_GLASS_DEFER=1, read when a context is made) the switch to and from glass toggles it as a fresh
    context does: equal frames and bounce counts on the pass kernel that defers."""
    monkeypatch.setenv("PT_GLASS_DEFER", "1")
    sc, index = scene(L, sid)
    with Dev(L, sc) as dev:
        geometry = {k: v for k, v in dev.hashes().items() if k in GEOMETRY}
        cur = sc
        for change in (dict(color=(0.25, 0.875, 0.5)), dict(emission=(0.5, 0.25, 2.0)), dict(reflect_type=2), dict(reflect_type=1),
                       dict(reflect_type=0, color=(0.5, 0.5, 0.5), emission=(0.0, 0.0, 0.0))):
            cur = edited(cur, index, **change)
            dev.set_object(index, cur.objs[index], expect=0)
            now = dev.hashes()
            assert {k: v for k, v in now.items() if k in GEOMETRY} == geometry, [k for k in GEOMETRY if now[k] != geometry[k]]
            with Dev(L, cur) as fresh:
                for cfg in (cfg_of(8), cfg_of(4, backend=1), cfg_of(2, flags=SEPARATE)):
                    got, gst = dev.render(cfg)
                    want, wst = fresh.render(cfg)
                    assert got == want and gst.ray_bounces == wst.ray_bounces, (sid, change, cfg.backend, cfg.flags)
                assert [a for a in dev.aov(cfg_of(4))] == [a for a in fresh.aov(cfg_of(4))]
                lo, hi = dev.reach()
                fresh.reserve(lo, hi)
                assert dev.hashes() == fresh.hashes()


# ------------------------------------------------------------------------------------------------------- 4. OUT OF REACH
def grow(lo, hi, blo, bhi):
    """the growth rule in numpy binary32, applied to the bounds the object's box violates"""
    lo, hi = lo.copy(), hi.copy()
    for a in range(3):
        if blo[a] < lo[a]:
            lo[a] = F32(blo[a] - F32(lo[a] - blo[a]))
        if bhi[a] > hi[a]:
            hi[a] = F32(bhi[a] + F32(bhi[a] - hi[a]))
    return lo, hi


def bounds_of(sc, index):
    o = sc.objs[index]
    pos = np.array(list(o.position), F32)
    if o.kind == ptlib.PT_SPHERE:
        r = np.abs(F32(o.radius))
        return pos - r, pos + r
    v = np.array([list(getattr(sc.tris[k], n)) for k in range(o.tri_offset, o.tri_offset + o.tri_count) for n in "abc"], F32)
    return np.fmin.reduce(v + pos, axis=0), np.fmax.reduce(v + pos, axis=0)


@pytest.mark.parametrize("sid", ("cornell-sphere", "cornell-wall", "mesh"))
def test_out_of_reach_rebuilds_and_grows_by_the_rule(L, sid):
    sc, index = scene(L, sid)
    with Dev(L, sc) as dev:
        lo, hi = dev.reach()
        ext = hi - lo
        far = edited(sc, index, move=(float(ext[0]), 0.0, float(-0.5 * ext[2])))
        blo, bhi = bounds_of(far, index)
        assert not (((lo <= blo) & (bhi <= hi)).all())
        dev.set_object(index, far.objs[index], expect=1)
        glo, ghi = dev.reach()
        wlo, whi = grow(lo, hi, blo, bhi)
        assert glo.tobytes() == wlo.tobytes() and ghi.tobytes() == whi.tobytes(), (glo, wlo, ghi, whi)
        with Dev(L, far) as fresh:
            assert_same(everything(dev, far, index)[0], everything(fresh, far, index)[0], sid + " out of reach")
        # a second, smaller push stays inside what the first one reserved (the overshoot doubled): the plans were dropped with the
        # rebuild, so a mesh with a BVH is refit from a new one
        room = ghi[0] - bhi[0]
        assert room > 0
        further = edited(far, index, move=(float(F32(0.5) * room), 0.0, 0.0))
        flo, fhi = bounds_of(further, index)
        assert ((glo <= flo) & (fhi <= ghi)).all() and fhi[0] > bhi[0]
        dev.set_object(index, further.objs[index], expect=0)
        assert dev.reach()[0].tobytes() == glo.tobytes() and dev.reach()[1].tobytes() == ghi.tobytes()
        with Dev(L, further) as fresh:
            assert_same(everything(dev, further, index)[0], everything(fresh, further, index)[0], sid + " second push")


# ------------------------------------------------------------------------------------------------------- 5. state
def test_refusals_in_order_leave_everything(L):
    sc, index = scene(L, "bvh19")
    dev = Dev(L, sc)
    empty = gpudev.new_ctx(L)
    try:
        cfg = cfg_of(4)
        before, _ = dev.render(cfg, accumulate=True)
        tables = dev.hashes()
        bad = edited(sc, index, reflect_type=7, position=(float("nan"), 0.0, 0.0)).objs[index]
        bad.tri_count = 18
        rebuilt = C.c_int(-7)
        for args, word in (((None, 9, None), b"ctx is NULL"), ((dev.ctx, 9, None), b"obj is NULL"), ((empty, 9, C.byref(bad)), b"no scene"),
                           ((dev.ctx, sc.n_objs, C.byref(bad)), b"index"), ((dev.ctx, index, C.byref(bad)), b"topology")):
            assert L.pt_ctx_set_object(*args, C.byref(rebuilt)) == PT_ERR_INVALID and word in L.pt_last_error(), word
        bad.tri_count = 19
        assert L.pt_ctx_set_object(dev.ctx, index, C.byref(bad), C.byref(rebuilt)) == PT_ERR_INVALID and b"reflect_type" in L.pt_last_error()
        bad.reflect_type = 2
        assert L.pt_ctx_set_object(dev.ctx, index, C.byref(bad), C.byref(rebuilt)) == PT_ERR_INVALID and b"not finite" in L.pt_last_error()
        assert rebuilt.value == -7
        assert dev.accum_info(cfg) == (4, 4) and dev.hashes() == tables
        assert dev.render(cfg_of(4))[0] == before
        assert L.pt_ctx_set_object(dev.ctx, index, C.byref(sc.objs[index]), None) == 0  # rebuilt may be NULL
    finally:
        L.pt_ctx_destroy(empty)
        dev.close()


def test_held_frame_fingerprint_and_bounds_follow_the_edit(L, tmp_path):
    sc, index = scene(L, "mesh")
    moved = edited(sc, index, move=INEXACT)
    dev, fresh = Dev(L, sc), Dev(L, moved)
    try:
        room_to_move(dev)
        cfg = cfg_of(4)
        dev.render(cfg, accumulate=True)
        assert dev.accum_info(cfg) == (4, 4)
        dev.set_object(index, sc.objs[index], expect=0)  # SAME keeps the held frame
        assert dev.accum_info(cfg) == (4, 4)
        dev.set_object(index, moved.objs[index], expect=0)
        assert dev.accum_info(cfg) == (0, 0)
        # the checkpoint a fresh context writes: same frame, same fingerprint, same bytes
        got, _ = dev.render(cfg, accumulate=True)
        want, _ = fresh.render(cfg, accumulate=True)
        assert got == want
        a, b = str(tmp_path / "edited.ckpt").encode(), str(tmp_path / "fresh.ckpt").encode()
        assert L.pt_ctx_accum_save(dev.ctx, a) == 0 and L.pt_ctx_accum_save(fresh.ctx, b) == 0, L.pt_last_error()
        assert open(a, "rb").read() == open(b, "rb").read()
        # the bounding-box queries follow the moved mesh, with Mesh::new's boxes and with given ones
        o, d = dev.primary_rays()
        same = lambda x, y: x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
        assert same(dev.bounds(index, o, d), fresh.bounds(index, o, d))
        box = (PtTriangle * 12)()
        first = C.cast(C.addressof(sc.tris) + sc.objs[index].tri_offset * C.sizeof(PtTriangle), C.POINTER(PtTriangle))
        assert L.pt_mesh_bounding_box(first, 100, box) == 0
        for x in (dev, fresh):
            assert L.pt_ctx_set_mesh_bounds(x.ctx, index, box) == 0
        hit = dev.bounds(index, o, d)
        assert hit[0].any() and same(hit, fresh.bounds(index, o, d))
        dev.set_object(index, sc.objs[index], expect=0)
        assert not same(dev.bounds(index, o, d), hit)  # (the box moved back with the mesh)
    finally:
        dev.close()
        fresh.close()


def test_set_camera_and_set_object_interleave(L):
    sc, index = scene(L, "bvh64")
    moved = edited(sc, index, move=INEXACT)
    cam = ptlib.make_camera((-3.0, 8.0, -13.0), (0.25, -0.375, 1.0))
    target = ptlib.Scene(sc.id, cam, [moved.objs[i] for i in range(sc.n_objs)], [])
    target.tris, target.n_tris = sc.tris, sc.n_tris
    a, b, fresh = Dev(L, sc), Dev(L, sc), Dev(L, target)
    try:
        rebuilt = C.c_int()
        assert L.pt_ctx_set_camera(a.ctx, C.byref(cam), C.byref(rebuilt)) == 0 and rebuilt.value == 0
        a.set_object(index, moved.objs[index], expect=0)
        b.set_object(index, moved.objs[index], expect=0)
        assert L.pt_ctx_set_camera(b.ctx, C.byref(cam), C.byref(rebuilt)) == 0 and rebuilt.value == 0
        want, _ = everything(fresh, target, index)
        assert_same(everything(a, target, index)[0], want, "camera then object")
        assert_same(everything(b, target, index)[0], want, "object then camera")
    finally:
        a.close()
        b.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------------- 6. sequences
def test_twenty_moves_do_not_drift(L):
    sc, index = scene(L, "mesh")
    with Dev(L, sc) as dev:
        room_to_move(dev)
        cur = sc
        for k in range(20):
            cur = edited(cur, index, move=(0.013 * (1 + k % 3), -0.007, 0.011 if k % 2 else -0.017))
            dev.set_object(index, cur.objs[index], expect=0)
        with Dev(L, cur) as fresh:
            assert_same(everything(dev, cur, index)[0], everything(fresh, cur, index)[0], "after twenty moves")
