"""A ladder of scenes and stream lengths on both sides of every LDS-layout cliff of the kernels that stage scene records (CPU only).

Each launch of k_pass_cand, k_pass, k_intersect_cand and the megakernel lays out its workgroup's LDS by lds_layout
(csrc/pt_layout.h): which template instance runs, whether the candidate and shading records are copied to LDS, how many leading
ranks of the shading table are, where the megakernel's spare rays and staged table start.  Every decision sits on a size cliff -
one candidate pair record, one shading record, one BVH node or one pixel per stream more selects another layout - and a wrong
offset at a cliff reads records that were never written, silently, for the objects at the end of the staged table only.

This module builds, from a seed and in binary32, a pair of scenes (or of stream lengths m, set through PT_STREAMS) for every
cliff: one just inside and one just outside, one step of its knob apart.  The layouts are never restated here:
host/layout_dump.cpp compiles pt_layout.h with the host compiler, fills the DevScene counts from host::flatten_scene (the tables
pt_ctx_set_scene uploads) and prints lds_layout's answer and the line the library itself writes to stderr under PT_LDS_PAD.
The knob of a pair is found by bisection over what that program says.
"""
import os

import numpy as np

import boundary_rays as br
import ptlib

F = np.float32
# tuning switches of a query (bits): the environment variables a GPU context runs with
SW_NO_CAND = 1      # PT_CAND_SCAN=0
SW_NO_CAND_BVH = 2  # PT_CAND_BVH=0
SW_DEFER = 4        # PT_GLASS_DEFER=1
SW_NO_NODES = 8     # PT_NODES_LDS=0
SW_ENV = {SW_NO_CAND: ("PT_CAND_SCAN", "0"), SW_NO_CAND_BVH: ("PT_CAND_BVH", "0"), SW_DEFER: ("PT_GLASS_DEFER", "1"),
          SW_NO_NODES: ("PT_NODES_LDS", "0")}
Q_FIELDS = ("n_objs", "n_tris", "n_cand_pairs", "n_bvh_nodes", "n_bvh_nodes4", "bvh_stack", "cand_scan", "pass", "m", "bvh_in_lds",
            "staged", "defer", "nodes_lds", "surf_staged", "surf_head", "pass_lds", "isect_staged", "isect_lds", "mega_cand",
            "mega_depth", "mega_spare_off", "mega_surf_off", "mega_lds")
PASS_PLAIN, PASS_DEFER, PASS_CAND, PASS_CAND_BVH = 0, 1, 2, 3


def layouts(sc, queries):
    """lds_layout for scene sc at each (m, switches) of queries: [(dict of the fields, [the three stderr lines])].  The generator
    is the PLAIN build of host/layout_dump.cpp: GPU tests come through here, and no sanitizer build runs on a GPU machine
    (tests/test_lds_layouts.py holds the sanitized build to the same bytes)."""
    path = br.write_scene(sc, os.path.join(br.workdir(), "layout_scene.bin"))
    out = ptlib.host_program("layout_dump", sanitize=False)(path, *["%d,%d" % q for q in queries]).splitlines()
    assert len(out) == 4 * len(queries), out[:3]
    res = []
    for k in range(len(queries)):
        q = out[4 * k].split()
        assert q[0] == "Q", out[4 * k]
        lines = [out[4 * k + 1 + w][3:] for w in range(3)]
        res.append((dict(zip(Q_FIELDS, (int(v) for v in q[1:]))), lines))
    return res


def layout(sc, m=1, sw=0):
    return layouts(sc, [(m, sw)])[0]


# ------------------------------------------------------------------------------------------------------------ scenes
class _Grid:
    """Objects in the cells of a grid in the plane z = 0, all in view of a camera on +z: every object can be aimed at."""

    def __init__(self, rng, cols=24):
        self.rng, self.cols, self.k = rng, cols, 0
        self.b = br._Builder()

    def cell(self):
        i, j = self.k % self.cols, self.k // self.cols
        self.k += 1
        return np.array([i - (self.cols - 1) / 2.0, j - (self.cols - 1) / 2.0, 0.0])

    def spheres(self, n, glass_every=0):
        for k in range(n):
            c = self.cell()
            col = tuple(float(F(v)) for v in self.rng.uniform(0.2, 0.9, 3))
            em = (2.0, 2.0, 2.0) if k % 17 == 5 else (0, 0, 0)
            refl = "Refract" if glass_every and k % glass_every == 0 else ("Specular" if k % 7 == 3 else "Diffuse")
            self.b.sphere(tuple(float(F(v)) for v in c + self.rng.uniform(-0.05, 0.05, 3)), float(F(0.3 + 0.1 * self.rng.random())),
                          col, em, refl)

    def meshes(self, sizes):
        """One small mesh (no BVH: under 16 triangles) per entry, that many triangles, in a cell of its own."""
        for t in sizes:
            c = self.cell()
            tl = []
            for q in range(t):
                a = c + np.array([0.35 * np.cos(2 * np.pi * q / t), 0.35 * np.sin(2 * np.pi * q / t), 0.02 * q])
                tl.append(tuple(tuple(float(F(v)) for v in p) for p in (c + [0, 0, 0.1], a, a + self.rng.uniform(-0.15, 0.15, 3))))
            self.b.mesh(tl, color=tuple(float(F(v)) for v in self.rng.uniform(0.2, 0.9, 3)))

    def bvh_mesh(self, n_tris):
        """A tessellated sphere of about n_tris triangles (a BVH mesh: 16 or more), in front of the grid."""
        n_lon = max(4, int(np.ceil(np.sqrt(n_tris / 2.0))))
        n_lat = int(np.ceil(n_tris / (2.0 * n_lon))) + 1
        tl = br._sphere_mesh(n_lat, n_lon, r=1.5, centre=(0.0, 0.0, 2.0))
        rng = np.random.default_rng(n_tris)
        keep = np.sort(rng.permutation(len(tl))[:n_tris]) if len(tl) > n_tris else np.arange(len(tl))
        self.b.mesh([tl[k] for k in keep], color=(0.8, 0.8, 0.8))

    def scene(self, name):
        return self.b.scene(name, (0.0, 0.0, 1.2 * self.cols + 4.0))


def _cornell():
    return ptlib.load_scene_py(ptlib.scene_path("cornell"))


# scene makers (seed, knob) -> Scene
def _flat_spheres(seed, n, glass=0):
    g = _Grid(np.random.default_rng(seed))
    g.spheres(n, glass)
    return g.scene("spheres%d" % n)


def _flat_meshes(seed, n, big=False):
    rng = np.random.default_rng(seed)
    g = _Grid(np.random.default_rng(seed + 1))
    g.meshes([15 if big else int(v) for v in rng.integers(1, 16, n)])
    return g.scene("meshes%d" % n)


def _pairs(seed, n):
    """n meshes of two triangles: one candidate pair record each."""
    g = _Grid(np.random.default_rng(seed))
    g.meshes([2] * n)
    return g.scene("pairs%d" % n)


def _mega_depth2_spheres(seed, n):
    g = _Grid(np.random.default_rng(seed))
    g.meshes([15] * 7)  # 7 x 8 pair records: past the room of four spare rays per lane, inside that of two
    g.spheres(n)
    return g.scene("mega2_spheres%d" % n)


def _bvh_tris(seed, t):
    g = _Grid(np.random.default_rng(seed))
    g.bvh_mesh(t)
    g.spheres(3)
    return g.scene("bvh_tris%d" % t)


def _bvh_spheres(seed, n, bvh_tris=40):
    g = _Grid(np.random.default_rng(seed))
    g.bvh_mesh(bvh_tris)
    g.spheres(n)
    return g.scene("bvh_spheres%d" % n)


def _bvh_pairs(seed, n, bvh_tris=150):
    g = _Grid(np.random.default_rng(seed))
    g.bvh_mesh(bvh_tris)
    g.spheres(4)
    g.meshes([2] * n)
    return g.scene("bvh_pairs%d" % n)


def _is_pass(kind):
    return lambda L: L["pass"] == kind


# The cliffs.  knob: the range bisected over; make: (seed, knob) -> Scene, or None when the knob is m (then `scene` gives the
# scene); sw: tuning switches; decide: what the cliff is about (it flips between the two sides); pre: the layout both sides must
# have; differs: the layout fields that change across the pair besides those in DERIVED - nothing else may.
CLIFFS = [
    # k_pass_cand without walks: candidate and shading records staged whole, or read from global memory
    dict(name="cand_staged_spheres", differs={"staged", "surf_staged"},
         knob=(1, 600), make=_flat_spheres, sw=0, decide=lambda L: L["staged"],
         pre=_is_pass(PASS_CAND)),
    dict(name="cand_staged_meshes", differs={"staged", "surf_staged"},
         knob=(1, 300), make=_flat_meshes, sw=0, decide=lambda L: L["staged"], pre=_is_pass(PASS_CAND)),
    dict(name="cand_staged_m", differs={"staged", "surf_staged"},
         knob=(1, 1024), make=None, scene=_cornell, sw=0, decide=lambda L: L["staged"],
         pre=_is_pass(PASS_CAND)),
    dict(name="cand_defer_staged", differs={"staged", "surf_staged"},
         knob=(1, 600), make=lambda s, n: _flat_spheres(s, n, glass=4), sw=SW_DEFER,
         decide=lambda L: L["staged"], pre=lambda L: L["pass"] == PASS_CAND and L["defer"] == 1),
    # k_pass (PT_CAND_SCAN=0): the deferral buffers while they fit 32 KiB with the stream's accumulators
    dict(name="pass_defer_m", differs={"pass", "defer"},
         knob=(1, 1024), make=None, scene=_cornell, sw=SW_NO_CAND, decide=lambda L: L["pass"],
         pre=lambda L: L["pass"] in (PASS_PLAIN, PASS_DEFER)),
    # the separate intersect step: k_intersect_cand<true> / <false>
    dict(name="isect_staged", differs={"isect_staged"},
         knob=(1, 400), make=_pairs, sw=0, decide=lambda L: L["isect_staged"], pre=_is_pass(PASS_CAND)),
    # the megakernel: k_mega_cand or k_mega; four spare rays per lane or two; the shading records staged or not
    dict(name="mega_cand", differs={"mega_cand", "mega_depth"},
         knob=(1, 400), make=_pairs, sw=0, decide=lambda L: L["mega_cand"], pre=_is_pass(PASS_CAND)),
    dict(name="mega_depth", differs={"mega_depth"},
         knob=(1, 120), make=_pairs, sw=0, decide=lambda L: L["mega_depth"], pre=lambda L: L["mega_cand"] == 1),
    dict(name="mega_surf_depth4", differs=set(),
         knob=(1, 400), make=_flat_spheres, sw=0, decide=lambda L: L["mega_surf_off"] != 0,
         pre=lambda L: L["mega_depth"] == 4),
    dict(name="mega_surf_depth2", differs=set(),
         knob=(0, 300), make=_mega_depth2_spheres, sw=0, decide=lambda L: L["mega_surf_off"] != 0,
         pre=lambda L: L["mega_depth"] == 2),
    # k_pass_cand with walks: the nodes in LDS; the whole shading table, all ranks but one, some or none; records or nothing
    dict(name="bvh_nodes_lds", differs={"nodes_lds"}, knob=(16, 3000), make=_bvh_tris, sw=0, decide=lambda L: L["nodes_lds"],
         pre=lambda L: L["pass"] == PASS_CAND_BVH and L["staged"] == 1),
    dict(name="bvh_surf_all", differs={"surf_staged"},
         knob=(0, 400), make=_bvh_spheres, sw=0, decide=lambda L: L["surf_staged"],
         pre=lambda L: L["pass"] == PASS_CAND_BVH and L["staged"] == 1),
    dict(name="bvh_surf_all_nodes_global", differs={"surf_staged"},
         knob=(0, 400), make=_bvh_spheres, sw=SW_NO_NODES, decide=lambda L: L["surf_staged"],
         pre=lambda L: L["pass"] == PASS_CAND_BVH and L["staged"] == 1 and L["nodes_lds"] == 0),
    dict(name="bvh_surf_head_none", differs=set(),
         knob=(0, 200), make=_bvh_pairs, sw=SW_NO_NODES, decide=lambda L: L["surf_head"] == 0,
         pre=lambda L: L["pass"] == PASS_CAND_BVH and L["staged"] == 1 and L["surf_staged"] == 0),
    dict(name="bvh_staged", differs={"staged"}, knob=(60, 300), make=_bvh_pairs, sw=SW_NO_NODES, decide=lambda L: L["staged"],
         pre=lambda L: L["pass"] == PASS_CAND_BVH and L["surf_head"] == 0 and L["surf_staged"] == 0),
]
# the layout fields every pair may differ in: what follows from its knob and decision (counts, bytes, offsets); a cliff's
# `differs` names the decisions that flip across it
DERIVED = {"n_objs", "n_tris", "n_cand_pairs", "n_bvh_nodes", "n_bvh_nodes4", "m", "pass_lds", "isect_lds", "mega_lds",
           "mega_spare_off", "mega_surf_off", "surf_head", "bvh_stack", "bvh_in_lds"}


class Rung:
    """One side of a cliff: the scene, m (PT_STREAMS makes a frame of m x 4 pixels with 4 streams: m per stream), switches, the
    layout lds_layout gives it and the three lines the library says under PT_LDS_PAD."""

    def __init__(self, cliff, side, knob, sc, m, sw, L, lines):
        self.cliff, self.side, self.knob, self.scene, self.m, self.sw, self.L, self.lines = cliff, side, knob, sc, m, sw, L, lines

    @property
    def env(self):
        e = {SW_ENV[b][0]: SW_ENV[b][1] for b in SW_ENV if self.sw & b}
        return e


def _eval(cl, seed, k):
    if cl["make"] is None:
        sc = cl["scene"]()
        return sc, k, layout(sc, k, cl["sw"])
    sc = cl["make"](seed, k)
    return sc, 1, layout(sc, 1, cl["sw"])


def build(seed):
    """[(cliff name, inside Rung, outside Rung)] for one seed: the knob value just before the decision flips and the next one."""
    out = []
    for cl in CLIFFS:
        lo, hi = cl["knob"]
        e_lo, e_hi = _eval(cl, seed, lo), _eval(cl, seed, hi)
        d_lo = cl["decide"](e_lo[2][0])
        assert cl["decide"](e_hi[2][0]) != d_lo, (cl["name"], lo, hi, e_lo[2][0], e_hi[2][0])
        cache = {lo: e_lo, hi: e_hi}
        while hi - lo > 1:
            mid = (lo + hi) // 2
            cache[mid] = _eval(cl, seed, mid)
            if cl["decide"](cache[mid][2][0]) == d_lo:
                lo = mid
            else:
                hi = mid
        rungs = []
        for side, k in (("inside", lo), ("outside", hi)):
            sc, m, (L, lines) = cache[k]
            rungs.append(Rung(cl["name"], side, k, sc, m, cl["sw"], L, lines))
        out.append((cl["name"], rungs[0], rungs[1]))
    return out


# --------------------------------------------------------------------------------------------------- edge-of-table rays
def edge_targets(rung, tabs):
    """Ranks a probe ray should hit for this rung's layout: the last and first of the staged shading table region (surf_head - 1,
    surf_head), the highest rank and rank 0, and the ranks of the triangles of the last candidate record (the end of the staged
    record region) - as (rank, object index, triangle index within the object or -1)."""
    sc, L = rung.scene, rung.L
    n_ranks = sc.n_objs + sc.n_tris
    ranks = {0, n_ranks - 1}
    if L["surf_head"]:
        ranks |= {L["surf_head"] - 1, min(L["surf_head"], n_ranks - 1)}
    if len(tabs["cand_pairs"]):
        ranks |= {int(r) for r in tabs["cand_pairs"]["id"][-1] if r != br.NO_TRI}
        ranks |= {int(r) for r in tabs["cand_pairs"]["id"][0] if r != br.NO_TRI}
    out = []
    offs = [sc.objs[i].tri_offset for i in range(sc.n_objs)]
    for r in sorted(ranks):
        hid = int(tabs["rank_id"][r])
        if hid < sc.n_objs:  # a sphere, or a mesh object's own rank (never a hit): its first triangle
            out.append((r, hid, -1 if sc.objs[hid].kind == ptlib.PT_SPHERE else 0))
        else:
            t = hid - sc.n_objs
            obj = max(i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_MESH and offs[i] <= t)
            out.append((r, obj, t - offs[obj]))
    return out


def aim(sc, obj, tri):
    """A ray whose first hit by the oracle's intersect_scene is the given sphere (tri < 0) or triangle of a mesh, or None.  It starts
    a short way off the surface - outside the sphere on the camera's side, or off either face of the triangle along its normal, at
    0.02 and then 0.002 - and points back at the centre / centroid (binary32, unit direction): a camera ray at a back-facing or
    hidden triangle of a closed mesh would hit another one first."""
    pos = np.array(list(sc.objs[obj].position), np.float64)
    if tri < 0:
        u = np.array(list(sc.cam.position), np.float64) - pos
        u /= np.linalg.norm(u)
        starts = [(pos + (sc.objs[obj].radius + h) * u, pos) for h in (0.02, 0.002)]
    else:
        t = sc.tris[sc.objs[obj].tri_offset + tri]
        p = [np.array(list(getattr(t, k)), np.float64) + pos for k in ("a", "b", "c")]
        c = (p[0] + p[1] + p[2]) / 3.0
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        if not np.linalg.norm(nrm) > 0:
            return None
        nrm /= np.linalg.norm(nrm)
        starts = [(c + side * h * nrm, c) for h in (0.02, 0.002) for side in (1.0, -1.0)]
    for o, tgt in starts:
        o = o.astype(F)
        d = tgt - o.astype(np.float64)
        d = (d / np.linalg.norm(d)).astype(F)
        _, oid, tid, _, _ = ptlib.oracle_intersect(sc, o, d)
        if int(oid[0]) == obj and int(tid[0]) == tri:
            return o, d
    return None


def probe_rays(rung, tabs):
    """edge_targets with their rays: [(rank, object, triangle, o, d)], each ray's first hit (by the oracle) being its target."""
    out = []
    for r, obj, tri in edge_targets(rung, tabs):
        ray = aim(rung.scene, obj, tri)
        assert ray is not None, (rung.cliff, rung.side, r, obj, tri)
        out.append((r, obj, tri) + ray)
    return out


def kinds(L):
    """The layouts a scene reaches at one m: names of the (kernel, layout) cases the ladder covers."""
    out = set()
    if L["pass"] == PASS_CAND:
        out.add("k_pass_cand%s %s" % ("<DEFER>" if L["defer"] else "", "staged" if L["staged"] else "unstaged"))
        out.add("k_intersect_cand<%s>" % ("true" if L["isect_staged"] else "false"))
    elif L["pass"] == PASS_CAND_BVH:
        if not L["staged"]:
            out.add("k_pass_cand<BVH> nothing staged")
        else:
            if L["nodes_lds"]:
                out.add("k_pass_cand<BVH> nodes_lds")
            n_ranks = L["n_objs"] + L["n_tris"]
            out.add("k_pass_cand<BVH> " + ("surf_staged" if L["surf_staged"] else "surf_head none" if L["surf_head"] == 0 else
                                          "surf_head all but one" if L["surf_head"] == n_ranks - 1 else "surf_head some"))
    elif L["pass"] == PASS_DEFER and L["cand_scan"] == 0 and L["n_bvh_nodes"] == 0:
        out.add("k_pass<DEFER>")
    elif L["cand_scan"] == 0 and L["n_bvh_nodes"] == 0:
        out.add("k_pass plain")
    if L["mega_cand"]:
        out.add("k_mega_cand depth %d %s" % (L["mega_depth"], "surf_off" if L["mega_surf_off"] else "no surf_off"))
    elif L["cand_scan"]:
        out.add("k_mega fallback (candidate scene)")
    return out


LADDER_KINDS = ["k_pass_cand staged", "k_pass_cand unstaged", "k_pass_cand<DEFER> staged", "k_pass_cand<DEFER> unstaged",
                "k_pass<DEFER>", "k_pass plain", "k_intersect_cand<true>", "k_intersect_cand<false>",
                "k_mega_cand depth 4 surf_off", "k_mega_cand depth 4 no surf_off", "k_mega_cand depth 2 surf_off",
                "k_mega_cand depth 2 no surf_off", "k_mega fallback (candidate scene)", "k_pass_cand<BVH> nodes_lds",
                "k_pass_cand<BVH> surf_staged", "k_pass_cand<BVH> surf_head all but one", "k_pass_cand<BVH> surf_head some",
                "k_pass_cand<BVH> surf_head none", "k_pass_cand<BVH> nothing staged"]
