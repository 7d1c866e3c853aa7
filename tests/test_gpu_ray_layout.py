"""k_pass_cand holds a ray in the rows it is stored in, reloads a valid lane's ray into the lanes past a partial chunk, and runs one
filter loop per axis over the records with the sign rule.  Every check here is bit for bit against code that shares none of that.
-m gpu.

The yardsticks: the pass kernel WITHOUT the candidate scan (PT_FLAG_NO_BVH -> k_pass: every ray against every triangle, rays as
two vec3, masked loads), and for the frames tests/frame_sums.py walks the oracle's own integer sums.

The shapes are the smallest at which the new code can go wrong:
- cornell 9x7 @1: 63 primary rays - every chunk of the frame is partial;
- cornell 13x5 @1: 65 - one full chunk and a chunk of ONE ray (lanes 1..63 repeat lane 0's);
- cornell 5x3 @3; cornell 16x12 @8: a wave's fading last trips pop cnt < 64 from its stack;
- three-spheres 16x12 @8: no filter record at all (all six per-axis counts are 0);
- mesh.json 12x8 @4: the BVH instance of the kernel (rays parked for a walk are read back from the chunk's LDS slot);
- cornell without its two z walls: records on two axes only, one per-axis loop runs zero times between two that run;
- cornell with two slivers and a tilted triangle added: filter records WITHOUT the sign rule on the x and z axes only (the loops of the
  second group, its y loop empty) and a record without a filter;
- single rays (pt_ctx_radiance, 65 samples: a full chunk and a chunk of one) along each axis - two direction components are zero,
  their reciprocals +-inf in the (inv.x, inv.y), (inv.z, bound) pairs - with one zero component, and with |d_a| one ulp step below
  and above the filters' grazing limit 1/64 on each axis."""
import ctypes as C
import json

import numpy as np
import pytest

import boundary_rays as br
import frame_sums as fs
import gpudev
import ptlib
import scatter_walk
from gpudev import L, same_bytes  # noqa: F401  (L: fixture)
from ptlib import PtConfig, PtStats, _np_f
from test_gpu_frame_sums import _saved, assert_planes

pytestmark = pytest.mark.gpu

SEED = scatter_walk.SEED
# (scene, width, height, samples); the last three are frame_sums' walked frames
FRAMES = [("cornell", 9, 7, 1), ("cornell", 13, 5, 1), ("cornell", 5, 3, 3)] + list(scatter_walk.FRAMES)
FRAME_IDS = ["%s-%dx%d@%d" % f for f in FRAMES]
KERNEL = {"cornell": "k_pass_cand", "three-spheres": "k_pass_cand", "mesh": "k_pass_cand_bvh", "cornell_xy": "k_pass_cand",
          "cornell_odd": "k_pass_cand"}


@pytest.fixture(scope="module")
def dev(L):
    with gpudev.Device(L) as dev:
        yield dev


def _set_scene(L, dev, sc):
    """the scene set; the default form runs the candidate scan on it and PT_FLAG_NO_BVH the scan of every triangle"""
    gpudev.set_scene(L, dev.ctx, sc)
    assert L.pt_ctx_pass_kernel(dev.ctx, 0).decode() == KERNEL[sc.id], sc.id
    assert L.pt_ctx_pass_kernel(dev.ctx, ptlib.FLAG_NO_BVH).decode() == "k_pass", sc.id


def _both(L, dev, out, w, h, spp, what):
    """the frame through the candidate scan and through k_pass: the same floats and the same bounce count"""
    got, st = dev.render(PtConfig(w, h, spp, 0, SEED, 0, 0, 0, 0), out)
    want, st_ref = dev.render(PtConfig(w, h, spp, 0, SEED, 0, 0, 0, ptlib.FLAG_NO_BVH), out)
    assert st.ray_bounces == st_ref.ray_bounces and st.ray_bounces >= w * h * spp, (what, st.ray_bounces, st_ref.ray_bounces)
    same_bytes(got, want, what + " against k_pass")
    assert np.isfinite(got).all() and got.max() > 0.0, what
    return got, st.ray_bounces


@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
def test_frame_is_the_scan_of_every_triangle(L, dev, frame):
    sid, w, h, spp = frame
    sc = scatter_walk._scene(sid)
    out = dev.alloc(w * h * 12)
    try:
        _set_scene(L, dev, sc)
        _both(L, dev, out, w, h, spp, FRAME_IDS[FRAMES.index(frame)])
    finally:
        dev.free(out)


@pytest.mark.parametrize("frame", scatter_walk.FRAMES, ids=FRAME_IDS[3:])
def test_walked_frame_holds_the_oracle_sums(L, dev, frame, tmp_path):
    """the raw 32.32 sums of the default form are the integers frame_sums chains down the oracle's paths, and the megakernel's
    frame of cornell is the wavefront's"""
    sid, w, h, spp = frame
    W, sums = fs.frame(sid, w, h, spp, SEED)
    total = fs.total_over(sums, range(spp))
    out = dev.alloc(w * h * 12)
    try:
        _set_scene(L, dev, W.scene)
        cfg = PtConfig(w, h, spp, 0, SEED, 0, 0, 0, 0)
        img, st = dev.render(cfg, out, accumulate=True)
        assert st.ray_bounces == W.n, (sid, st.ray_bounces, W.n)
        assert_planes(_saved(L, dev.ctx, tmp_path / "frame.ptacc")["sums"], fs.planes(total), sid)
        same_bytes(img, fs.resolved(total, spp, clamp=True), sid)
        if sid == "cornell":
            mega, st_m = dev.render(PtConfig(w, h, spp, ptlib.BACKEND_MEGAKERNEL, SEED, 0, 0, 0, 0), out)
            assert st_m.ray_bounces == W.n
            same_bytes(mega, img, "megakernel against wavefront")
    finally:
        dev.free(out)


@pytest.fixture(scope="module")
def cornell_xy(tmp_path_factory):
    """cornell.json without the two walls that lie in z planes: flat records on the x and y axes only"""
    d = json.load(open(ptlib.scene_path("cornell")))
    keep = [o for o in d["objects"] if not ("Mesh" in o["type_"] and abs(o["position"][2]) == 8.8)]
    assert len(keep) == len(d["objects"]) - 2
    d["objects"], d["id"] = keep, "cornell_xy"
    path = tmp_path_factory.mktemp("ray_layout") / "cornell_xy.json"
    path.write_text(json.dumps(d))
    return ptlib.load_scene_py(str(path), base_dir=ptlib.ROOT)


def _mesh(tris, color):
    return {"position": [0.0, 0.0, 0.0], "material": {"color": color, "emmission": [0.0, 0.0, 0.0], "reflect_type": "Diffuse"},
            "type_": {"Mesh": {"triangles": [dict(zip("abc", t)) for t in tris],
                               "bounding_sphere": {"position": [0.0, 0.0, 0.0], "radius": 100.0}}}}


@pytest.fixture(scope="module")
def cornell_odd(tmp_path_factory):
    """cornell.json and three small meshes inside the room: in the plane x = 0.9 and in the plane z = 2.5 a well-shaped triangle
    beside a sliver (edges (1, 1) and (1, 1.0005) in the plane: tests/test_host_logic.py's, no sign rule for its record), and one
    tilted triangle (no filter at all)"""
    d = json.load(open(ptlib.scene_path("cornell")))
    d["objects"] += [
        _mesh([([0.9, -1.0, 3.0], [0.9, 0.0, 3.0], [0.9, -1.0, 4.0]), ([0.9, -1.0, 3.0], [0.9, 0.0, 4.0], [0.9, 0.0, 4.0005])], [0.9, 0.2, 0.2]),
        _mesh([([-2.0, 0.0, 2.5], [-1.0, 0.0, 2.5], [-2.0, 1.0, 2.5]), ([-2.0, 0.0, 2.5], [-1.0, 1.0, 2.5], [-1.0, 1.0005, 2.5])], [0.2, 0.9, 0.2]),
        _mesh([([1.5, -2.0, 5.0], [2.5, -2.0, 5.0], [2.0, -1.0, 5.3])], [0.2, 0.2, 0.9])]
    d["id"] = "cornell_odd"
    path = tmp_path_factory.mktemp("ray_layout_odd") / "cornell_odd.json"
    path.write_text(json.dumps(d))
    return ptlib.load_scene_py(str(path), base_dir=ptlib.ROOT)


def _check_table_order(tabs):
    """what the kernel's loops assume of the table: the records with the sign rule first, each group sorted by axis"""
    flat, ne = tabs["flat_pairs"], tabs["n_flat_exact"]
    assert (flat["sign_exact"][:ne] == 1).all() and (flat["sign_exact"][ne:] == 0).all()
    for part in (flat["axis"][:ne], flat["axis"][ne:]):
        assert (np.diff(part.astype(np.int64)) >= 0).all()
    return flat["axis"][:ne].tolist(), flat["axis"][ne:].tolist()


def test_second_group_and_unfiltered_records(L, dev, cornell_odd):
    tabs = br.scene_tables(cornell_odd)
    assert _check_table_order(tabs) == ([0, 1, 1, 2], [0, 2]) and tabs["n_other_pairs"] == 1
    out = dev.alloc(16 * 12 * 12)
    try:
        _set_scene(L, dev, cornell_odd)
        _both(L, dev, out, 16, 12, 8, "cornell_odd")
    finally:
        dev.free(out)


def test_two_axes_only(L, dev, cornell_xy):
    tabs = br.scene_tables(cornell_xy)
    assert _check_table_order(tabs) == ([0, 1, 1], []) and tabs["n_other_pairs"] == 0
    out = dev.alloc(16 * 12 * 12)
    try:
        _set_scene(L, dev, cornell_xy)
        _, bounces = _both(L, dev, out, 16, 12, 8, "cornell_xy")
        assert bounces > 16 * 12 * 8  # (paths go on past the first hit)
    finally:
        dev.free(out)


GRAZE = np.float32(1.0 / 64.0)
PROBE_O = (0.3, 0.4, 2.0)  # inside the room, on no plane of it, clear of the spheres along all three axes


def _probe_dirs():
    """(name, direction): unit to rounding; both forms get the same floats"""
    out = []
    for a in range(3):
        for s in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[a] = s
            out.append(("axis%d%+d" % (a, s), d))
            neg = [-0.0, -0.0, -0.0]  # the other two components -0: reciprocals -inf
            neg[a] = s
            out.append(("axis%d%+d_negzero" % (a, s), neg))
        z = [0.0, 0.0, 0.0]
        z[(a + 1) % 3], z[(a + 2) % 3] = 0.6, -0.8
        out.append(("zero%d" % a, z))
        for name, v in (("below", np.nextafter(GRAZE, np.float32(0))), ("at", GRAZE), ("above", np.nextafter(GRAZE, np.float32(1)))):
            for s in (1.0, -1.0):
                g = [0.0, 0.0, 0.0]
                g[a] = s * float(v)
                rest = np.sqrt(np.float32(1) - v * v, dtype=np.float32)
                g[(a + 1) % 3], g[(a + 2) % 3] = float(np.float32(0.6) * rest), float(np.float32(-0.8) * rest)
                out.append(("graze%d_%s%+d" % (a, name, s), g))
    return out


@pytest.mark.parametrize("sid", ["cornell", "cornell_xy", "cornell_odd"])
def test_single_rays_at_the_filters_edges(L, dev, sid, cornell_xy, cornell_odd):
    sc = {"cornell_xy": cornell_xy, "cornell_odd": cornell_odd}.get(sid) or scatter_walk._scene(sid)
    _set_scene(L, dev, sc)
    o = np.array(PROBE_O, np.float32)
    dirs = _probe_dirs()
    assert len(dirs) == 3 * (4 + 1 + 6)
    hits = 0
    for k, (name, d) in enumerate(dirs):
        d = np.array(d, np.float32)
        res = []
        for flags in (0, ptlib.FLAG_NO_BVH):
            out, st = np.zeros(3, np.float32), PtStats()
            rc = L.pt_ctx_radiance(dev.ctx, _np_f(o), _np_f(d), 0, 65, SEED, k, 0, flags, _np_f(out), C.byref(st))
            assert rc == 0, L.pt_last_error()
            res.append((out.view(np.uint32).tolist(), st.ray_bounces))
        assert res[0] == res[1], (sid, name, d.tolist(), res)
        assert res[0][1] >= 65
        hits += res[0][1] > 65
    assert hits >= len(dirs) // 2, "most probes hit a wall and go on"
