"""pt_ctx_reproject_moved and pt_ctx_reproject_var_moved on the GPU against tests/reproject_moved_ref.py, the restatement of the
contract in include/ptrace.h in numpy binary32.  Every comparison is of bytes, for equality, and every output has guard floats
behind it.  The frames are tests/test_gpu_reproject.py's - one pixel, 7x5, 257x3 (two workgroups with a one-lane tail, taps that
leave the frame above and below) and 33x25 - and the planes tests/test_gpu_reproject_var.py's, with the object ids spread over
0..5 against a table of FOUR records: IDENTITY, a translation, a scale with a translation, and the marker, so that ids 4 and 5
lie beyond the table.  The cameras: identical (a wave then mixes step 2's single tap with four-tap lanes), translated, orbited."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpudev
import ptlib
import reproject_moved_ref as mref
import reproject_ref as ref
import reproject_var_ref as rv
import test_gpu_reproject as base
import test_gpu_reproject_var as vbase
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtConfig, PtObjectMotion, PtReprojectParams, PtReprojectVarParams
from reproject_moved_ref import IDENTITY, MARKER
from reproject_ref import F32, I32

pytestmark = pytest.mark.gpu

FRAMES = base.FRAMES
CUR = base.CUR
CAMERAS = {
    "identical": base.CAMERAS["identical"],
    "translated": base.CAMERAS["translated"],
    "orbited": (ref.orbit(CUR, ref.ORBIT_DEGREES), CUR),
}
PARAMS = vbase.PARAMS
# a pixel at depth 6 is about 0.19 wide at 33 columns: the records move a point by a fraction of a pixel to about a pixel
MOTION = (IDENTITY, (0.11, -0.05, 0.02, 1.0), (0.02, 0.01, -0.03, 0.98), MARKER)
CLI = os.path.join(ptlib.PKG, "ptrace")


class Dev(vbase.Dev):
    """tests/test_gpu_reproject_var.py's planes and guards, and the two moved calls"""

    def reproject_var_moved(self, w, h, cam, hist_cam, motion, n_motion=None, normal=True, in_place=False, stream=None, params=PARAMS):
        n = w * h
        self._guards(n, in_place)
        p = PtReprojectVarParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"],
                                 params["min_frames"], params["radius"], 0)
        a, b = ref.pt_camera(cam), ref.pt_camera(hist_cam)
        P = self.p
        t = mref.table(motion) if motion is not None else None
        rc = self.L.pt_ctx_reproject_var_moved(self.ctx, w, h, C.byref(p), C.byref(a), P["color"], P["depth"], P["oid"],
                                               P["normal"] if normal else None, C.byref(b), P["hcolor"], P["hlen"], P["hmom"],
                                               P["hdepth"], P["hoid"], P["hnormal"] if normal else None,
                                               P["color" if in_place else "out"], P["len"], P["mom"], P["err"], t,
                                               len(motion) if n_motion is None else n_motion, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        return self._collect(n, in_place)

    def reproject_moved(self, w, h, cam, hist_cam, motion, n_motion=None, normal=True, in_place=False, stream=None, params=PARAMS):
        n = w * h
        out = "color" if in_place else "out"
        self.fill_guarded(out, n * 3, base.GUARD, -3.0, tail_only=in_place)
        self.fill_guarded("len", n, base.GUARD, -3.0)
        p = PtReprojectParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"], 0)
        a, b = ref.pt_camera(cam), ref.pt_camera(hist_cam)
        P = self.p
        t = mref.table(motion) if motion is not None else None
        rc = self.L.pt_ctx_reproject_moved(self.ctx, w, h, C.byref(p), C.byref(a), P["color"], P["depth"], P["oid"],
                                           P["normal"] if normal else None, C.byref(b), P["hcolor"], P["hlen"], P["hdepth"], P["hoid"],
                                           P["hnormal"] if normal else None, P["color" if in_place else "out"], P["len"], t,
                                           len(motion) if n_motion is None else n_motion, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.read_guarded(out, n * 3, base.GUARD, -3.0, "the colour output")
        return got.reshape(n, 3), self.read_guarded("len", n, base.GUARD, -3.0, "the length output")

    def plain(self, w, h, cam, hist_cam, normal=True):
        """pt_ctx_reproject's two outputs on the planes as they are"""
        n = w * h
        p = PtReprojectParams(PARAMS["weight"], PARAMS["max_history"], PARAMS["depth_tol"], PARAMS["normal_min"], 0)
        a, b = ref.pt_camera(cam), ref.pt_camera(hist_cam)
        P = self.p
        rc = self.L.pt_ctx_reproject(self.ctx, w, h, C.byref(p), C.byref(a), P["color"], P["depth"], P["oid"], P["normal"] if normal else None,
                                     C.byref(b), P["hcolor"], P["hlen"], P["hdepth"], P["hoid"], P["hnormal"] if normal else None,
                                     P["out"], P["len"], None)
        assert rc == 0, (rc, self.L.pt_last_error())
        return self.download("out", n * 3).reshape(n, 3), self.download("len", n)


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


# ------------------------------------------------------------------------------------------------------ the inputs
_cache = {}


def synthetic(w, h):
    """tests/test_gpu_reproject_var.py's frames with the ids 0..2 spread over 0..5 - the same way in the frame and in its history,
    so that what matched still matches - and -1 left alone"""
    if (w, h) not in _cache:
        cur, hist = vbase.synthetic(w, h)
        cur, hist = {k: v.copy() for k, v in cur.items()}, {k: v.copy() for k, v in hist.items()}
        i = np.arange(w * h)
        up = (((i % w) // 2 + (i // w)) % 2 * 3).astype(I32)
        for f in (cur, hist):
            f["oid"] = np.where(f["oid"] >= 0, f["oid"] + up, f["oid"]).astype(I32)
        _cache[(w, h)] = (cur, hist)
    return _cache[(w, h)]


def hist_kw(hist_cam, hist, normal=True, var=True):
    kw = dict(hist_cam=hist_cam, hist_color=hist["color"], hist_len=hist["len"], hist_depth=hist["depth"], hist_object_id=hist["oid"],
              hist_normal=hist["normal"] if normal else None)
    if var:
        kw["hist_moments"] = hist["mom"]
    return kw


PLAIN_KEYS = ("weight", "max_history", "depth_tol", "normal_min")
_want = {}


def want_var(w, h, camera, normal=True, motion=MOTION):
    key = ("var", w, h, camera, normal, motion)
    if key not in _want:
        cam, hist_cam = CAMERAS[camera]
        cur, hist = synthetic(w, h)
        _want[key] = mref.reproject_var_moved(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"] if normal else None,
                                              motion=motion, **hist_kw(hist_cam, hist, normal), **PARAMS)
    return _want[key]


def want_plain(w, h, camera, normal=True, motion=MOTION):
    key = ("plain", w, h, camera, normal, motion)
    if key not in _want:
        cam, hist_cam = CAMERAS[camera]
        cur, hist = synthetic(w, h)
        _want[key] = mref.reproject_moved(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"] if normal else None,
                                          motion=motion, **hist_kw(hist_cam, hist, normal, var=False),
                                          **{k: PARAMS[k] for k in PLAIN_KEYS})
    return _want[key]


def same2(got, exp, what):
    base.same_bytes(got, exp, what)


# --------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % s for s in FRAMES])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_is_the_restatement(dev, size, camera):
    w, h = size
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    with dev.stream() as st:
        for normal in (True, False):
            dev.put(cur, hist)
            vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, MOTION, normal=normal), want_var(w, h, camera, normal),
                             (camera, "var", normal))
            same2(dev.reproject_moved(w, h, cam, hist_cam, MOTION, normal=normal), want_plain(w, h, camera, normal),
                  (camera, "plain", normal))
            vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, MOTION, normal=normal, stream=st), want_var(w, h, camera, normal),
                             (camera, "var on a stream", normal))
            same2(dev.reproject_moved(w, h, cam, hist_cam, MOTION, normal=normal, stream=st), want_plain(w, h, camera, normal),
                  (camera, "plain on a stream", normal))
            # in place: d_out_color == d_color
            vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, MOTION, normal=normal, in_place=True, stream=st),
                             want_var(w, h, camera, normal), (camera, "var in place", normal))
            dev.put(cur, hist)
            same2(dev.reproject_moved(w, h, cam, hist_cam, MOTION, normal=normal, in_place=True), want_plain(w, h, camera, normal),
                  (camera, "plain in place", normal))
    # the inputs reach what they are there for: on the larger frames every kind of record has pixels, and moved pixels blend
    if w * h > 35:
        ids = cur["oid"]
        assert all((ids == k).any() for k in range(6))
        ln = want_var(w, h, camera)[1]
        assert (ln[(ids == 1) | (ids == 2)] > PARAMS["weight"]).any(), camera


# ------------------------------------------------------------------------------------- thin, long and full-size frames
# tests/test_gpu_reproject.py's LARGE (it says what each shape crosses) through both moved calls with ONE moving object: a table
# of two records, IDENTITY and a translation, so object 1 moves and ids 2..5 lie beyond the table.  The camera stands still - the
# drag loop - so a wave mixes step 2's single tap with four-tap lanes.  The spatial window is the smallest (radius 1): the window
# does not read the table, and tests/test_gpu_reproject_var.py runs it at every radius on these shapes.
ONE_MOVING = (IDENTITY, (0.11, -0.05, 0.02, 1.0))
LARGE_PARAMS = dict(PARAMS, radius=1)


@pytest.fixture(scope="module")
def bigdev(L):
    with Dev(L, base.MAXPIX_LARGE) as d:
        yield d


@pytest.mark.parametrize("size", base.LARGE, ids=base.LARGE_IDS)
def test_large_frames_with_one_moving_object(bigdev, size):
    w, h = size
    cam, hist_cam = CAMERAS["identical"]
    cur, hist = synthetic(w, h)
    bigdev.put(cur, hist)
    exp = mref.reproject_var_moved(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"], motion=ONE_MOVING,
                                   **hist_kw(hist_cam, hist), **LARGE_PARAMS)
    got = bigdev.reproject_var_moved(w, h, cam, hist_cam, ONE_MOVING, params=LARGE_PARAMS)
    vbase.same_bytes(got, exp, (size, "var"))
    vbase.no_fill_left(got)
    exp2 = mref.reproject_moved(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"], motion=ONE_MOVING,
                                **hist_kw(hist_cam, hist, var=False), **{k: PARAMS[k] for k in PLAIN_KEYS})
    got2 = bigdev.reproject_moved(w, h, cam, hist_cam, ONE_MOVING, params=LARGE_PARAMS)
    same2(got2, exp2, (size, "plain"))
    vbase.no_fill_left(got2)
    assert exp2[0].tobytes() == exp[0].tobytes() and exp2[1].tobytes() == exp[1].tobytes()  # "colour and length are the moved call's"
    moving = cur["oid"] == 1
    print("%dx%d: %d pixels of the moving object, %d of them blend" % (w, h, moving.sum(), (exp[1][moving] > PARAMS["weight"]).sum()))
    assert moving.any() and (cur["oid"] >= 2).any() and (exp[1][~moving] > PARAMS["weight"]).any()


@pytest.mark.parametrize("camera", list(CAMERAS))
def test_delegation(dev, camera):
    """motion NULL, n_motion 0 and an all-IDENTITY table each give the plain calls' bytes on the same inputs"""
    w, h = 33, 25
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    plain_var = dev.reproject_var(w, h, cam, hist_cam)
    plain = dev.plain(w, h, cam, hist_cam)
    for what, motion, n_motion in (("NULL", None, 0), ("n_motion 0", MOTION, 0), ("all IDENTITY", (IDENTITY,) * 6, 6)):
        vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, motion, n_motion), plain_var, what)
        same2(dev.reproject_moved(w, h, cam, hist_cam, motion, n_motion), plain, what)


@pytest.mark.parametrize("size", FRAMES[1:], ids=["%dx%d" % s for s in FRAMES[1:]])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_exact_properties(dev, size, camera):
    w, h = size
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    plain_var = dev.reproject_var(w, h, cam, hist_cam)
    got = dev.reproject_var_moved(w, h, cam, hist_cam, MOTION)
    got2 = dev.reproject_moved(w, h, cam, hist_cam, MOTION)
    ids = cur["oid"]
    # the marker: (color, wt), and the moments of a pixel without history
    mk = ids == 3
    s = rv.s_of(cur["color"])
    for colour, ln in ((got[0], got[1]), got2):
        assert colour[mk].tobytes() == cur["color"][mk].tobytes() and (ln[mk] == PARAMS["weight"]).all()
    assert got[2][mk].tobytes() == np.stack([s, s * s], axis=1)[mk].tobytes()
    # IDENTITY, beyond the table, and no hit at all: the plain call's bytes in every output
    same = (ids <= 0) | (ids >= 4)
    for a, b in zip(got, plain_var):
        assert np.ascontiguousarray(a[same]).tobytes() == np.ascontiguousarray(b[same]).tobytes()
    for a, b in zip(got2, plain_var[:2]):
        assert np.ascontiguousarray(a[same]).tobytes() == np.ascontiguousarray(b[same]).tobytes()
    # under bitwise-equal cameras a moved pixel is not the one-tap running mean: where the plain call found its own history pixel
    # (one tap, b = 1: its length is the history pixel's + wt), the moved call gathered four taps at a shifted position
    # (a pixel of which a single tap survives the tests may still land on the same bytes, so this asks for one, not for all)
    if camera == "identical" and w * h > 35:
        mv = ((ids == 1) | (ids == 2)) & (plain_var[1] > PARAMS["weight"]) & (got[1] > PARAMS["weight"])
        differs = (got[0][mv] != plain_var[0][mv]).any(axis=1)
        print("moved pixels that blend in both calls: %d, of which %d differ from the one-tap mean" % (mv.sum(), differs.sum()))
        assert differs.any(), (differs.sum(), mv.sum())


def test_table_scratch_grows_and_is_reused(dev):
    """a table of 4 records, then one of 3000 (the scratch grows), then 4 again: each call gives the restatement's bytes"""
    w, h = 33, 25
    cam, hist_cam = CAMERAS["translated"]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    exp = want_var(w, h, "translated")
    big = MOTION + ((0.5, 0.5, 0.5, 2.0),) * 2996  # ids 4 and 5 now have records
    exp_big = mref.reproject_var_moved(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"], motion=big,
                                       **hist_kw(hist_cam, hist), **PARAMS)
    vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, MOTION), exp, "4")
    vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, big), exp_big, "3000")
    vbase.same_bytes(dev.reproject_var_moved(w, h, cam, hist_cam, MOTION), exp, "4 again")
    assert exp_big[1].tobytes() != exp[1].tobytes()


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_cornell(L):
    """Frame A rendered and reprojected as a first frame; the first sphere moved with pt_ctx_set_object, inside the room, nothing
    rebuilt; frame B and its guides rendered; pt_ctx_reproject_var_moved with the table pt_object_motion_between makes.
    (a) all four outputs are the restatement's on the downloaded buffers, bit for bit;
    (b) the context is left alone otherwise: the scene's device tables hash as before (pt_ctx_table_hashes), the frame
        pt_ctx_accumulate holds is still held with its samples, and the same render gives the same bytes after the call as
        before it (the measured pass rates have no accessor; a frame planned with them is what can be seen of them)."""
    w, h = ref.ORBIT_SIZE
    spp = ref.ORBIT_SPP
    n = w * h
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    cam = ref.cam_dict(sc.cam)
    index = [i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_SPHERE][0]
    d = Dev(L, n)
    params = dict(rv.defaults(L), weight=spp)
    try:
        d.set_scene(sc)

        def frame(seed):
            d.render(gpudev.config(w, h, spp, seed=seed), d.p["color"])
            cfg = PtConfig(w, h, spp, 0, seed, 0, 0, 0, 0)
            assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), None, d.p["normal"], d.p["depth"], d.p["oid"], None) == 0, L.pt_last_error()
            return dict(color=d.download("color", n * 3).reshape(n, 3), depth=d.download("depth", n), oid=d.download("oid", n, I32),
                        normal=d.download("normal", n * 3).reshape(n, 3))

        a = frame(11)
        first = d.reproject_var(w, h, cam, None, history=False, hist_normal=False, params=params)
        a.update(color=first[0], len=first[1], mom=first[2])
        before = ptlib.PtObject.from_buffer_copy(sc.objs[index])
        now = ptlib.PtObject.from_buffer_copy(sc.objs[index])
        for k, step in enumerate((0.1, 1.0 / 3.0, 0.07)):
            now.position[k] = float(F32(before.position[k]) + F32(step))
        rebuilt = C.c_int(-1)
        assert L.pt_ctx_set_object(d.ctx, index, C.byref(now), C.byref(rebuilt)) == 0, L.pt_last_error()
        assert rebuilt.value == 0
        b = frame(12)
        assert (b["oid"] == index).sum() > 20 and b["oid"].tobytes() != a["oid"].tobytes()  # the sphere is in view, and moved
        rec = PtObjectMotion()
        assert L.pt_object_motion_between(C.byref(now), C.byref(before), C.byref(rec)) == 0
        motion = [IDENTITY] * sc.n_objs
        motion[index] = (*rec.offset, rec.scale)
        assert motion[index] == mref.motion_between(mref.object_dict(now), mref.object_dict(before))
        assert not mref.is_identity(motion[index]) and not mref.is_marker(motion[index])
        d.put(b, a)
        held_cfg = PtConfig(w, h, 2, 0, 99, 0, 0, 0, 0)                                                    # a held frame of 2 samples
        assert L.pt_ctx_accumulate(d.ctx, C.byref(held_cfg), d.p["dn"], None, None, None, None, None) == 0, L.pt_last_error()
        hashes = (C.c_uint64 * 14)()
        assert L.pt_ctx_table_hashes(d.ctx, hashes) == 0, L.pt_last_error()
        got = d.reproject_var_moved(w, h, cam, cam, motion, params=params)
        after = (C.c_uint64 * 14)()
        assert L.pt_ctx_table_hashes(d.ctx, after) == 0 and list(after) == list(hashes)                    # (b)
        lo, hi = C.c_uint32(), C.c_uint32()
        assert L.pt_ctx_accum_info(d.ctx, C.byref(held_cfg), C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (2, 2)
        exp = mref.reproject_var_moved(w, h, cam, b["color"], b["depth"], b["oid"], b["normal"], motion=motion, **hist_kw(cam, a), **params)
        vbase.same_bytes(got, exp, "cornell")                                                              # (a)
        on = b["oid"] == index
        print("the moved sphere: %d pixels, %d with history" % (on.sum(), (got[1][on] > spp).sum()))
        assert (got[1][on] > spp).any()
        d.render(gpudev.config(w, h, spp, seed=12), d.p["dn"])                                                    # (b)
        assert d.download("dn", n * 3).tobytes() == b["color"].tobytes()
        for name, src in (("color", b["color"]), ("hcolor", a["color"]), ("hlen", a["len"]), ("hmom", a["mom"])):
            assert d.download(name, src.size).tobytes() == np.ascontiguousarray(src).tobytes(), name       # the inputs are read only
    finally:
        d.close()


# ----------------------------------------------------------------------------------------------------------- the CLI
def test_cli_move_history(tmp_path):
    def run(args):
        return subprocess.run([CLI, "2", "32", "cornell", "--root", ptlib.ROOT, "--seed", "5"] + args, cwd=str(tmp_path),
                              capture_output=True, text=True, timeout=120)

    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    index = [i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_SPHERE][0]
    drag = ["--orbit", "3", "--orbit-step", "0", "--move", "%d:0.1,0.3333333,0.07" % index]
    r = run(drag + ["--preview", str(tmp_path / "kept.ppm"), "--move-history"])
    assert r.returncode == 0, r.stdout + r.stderr
    r = run(drag + ["--preview", str(tmp_path / "dropped.ppm")])
    assert r.returncode == 0, r.stdout + r.stderr
    kept = [open(tmp_path / ("kept-%03d.ppm" % k), "rb").read() for k in range(3)]
    dropped = [open(tmp_path / ("dropped-%03d.ppm" % k), "rb").read() for k in range(3)]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("kept")) == ["kept-%03d.ppm" % k for k in range(3)]
    assert kept[0] == dropped[0]      # frame 0 has no history either way
    assert kept[2] != dropped[2]      # history was used
    r = run(["--orbit", "3", "--preview", str(tmp_path / "no.ppm"), "--move-history"])
    assert r.returncode == 1 and "--move-history" in r.stderr, (r.returncode, r.stderr)
    r = run(drag + ["--preview", str(tmp_path / "no.ppm"), "--move-history", "0.5"])
    assert r.returncode == 1 and "--move-history" in r.stderr, (r.returncode, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]
