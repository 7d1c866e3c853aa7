"""pt_ctx_reproject on the GPU against tests/reproject_ref.py, the restatement of the contract in include/ptrace.h in numpy
binary32.  Every comparison is of bytes, for equality.  The frames are the smallest that reach every path: one pixel, odd sizes,
a frame of three long rows (257 x 3: two workgroups with a one-lane tail, taps that leave the frame above and below), and 33 x 25
(four workgroups of 256 with a tail).  The cameras: identical (step 2's single tap), translated by less than a pixel to a few
pixels, rotated onto orthogonals()' other `up` vector (the history frame is turned), and one that puts part of the frame behind
the history lens and part outside the history frame."""
import ctypes as C

import numpy as np
import pytest

import gpudev
import kats_camera as kc
import ptlib
import reproject_ref as ref
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtConfig, PtReprojectParams
from reproject_ref import F32, I32

pytestmark = pytest.mark.gpu

GUARD = 64  # floats behind each output
FRAMES = ((1, 1), (7, 5), (257, 3), (33, 25))
MAXPIX = 96 * 64
CUR = kc.CORNELL_CAM
CAMERAS = {
    "identical": (CUR, dict(CUR)),
    "translated": (CUR, dict(CUR, position=(0.05, -0.18000005, 7.8))),
    "other-up": (dict(kc.TILT_CAM, direction=(0.35355338, -0.8660254, 0.35355338)), kc.TILT_CAM),
    "partly-behind": (CUR, dict(CUR, position=(3.0, -0.2, 3.0), direction=(-0.9578263, 0.0, -0.2873479))),
}
PARAMS = dict(weight=4, max_history=64.0, depth_tol=0.05, normal_min=0.5)


NAMES = ("color", "depth", "oid", "normal", "hcolor", "hlen", "hdepth", "hoid", "hnormal", "out", "len")
FLOATS = dict(color=3, depth=1, oid=1, normal=3, hcolor=3, hlen=1, hdepth=1, hoid=1, hnormal=3, out=3, len=1)


class Dev(gpudev.Device):
    """one context and the eleven planes of a call, the two outputs with guard floats behind whatever a call writes"""

    def __init__(self, L, max_pix=MAXPIX):
        super().__init__(L)
        for name in NAMES:
            self.alloc((max_pix * FLOATS[name] + GUARD) * 4, name)

    def put(self, cur, hist=None):
        for name, key in (("color", "color"), ("depth", "depth"), ("oid", "oid"), ("normal", "normal")):
            self.upload(name, cur[key])
        if hist is not None:
            for name, key in (("hcolor", "color"), ("hlen", "len"), ("hdepth", "depth"), ("hoid", "oid"), ("hnormal", "normal")):
                self.upload(name, hist[key])

    def reproject(self, w, h, cam, hist_cam=None, normal=True, hist_normal=True, history=True, in_place=False, stream=None,
                  params=PARAMS, default_params=False):
        """the two outputs of one call, (w*h, 3) and (w*h,); the guards behind them are checked on the way"""
        n = w * h
        out = "color" if in_place else "out"
        self.fill_guarded(out, n * 3, GUARD, -3.0, tail_only=in_place)  # (in place: behind the frame)
        self.fill_guarded("len", n, GUARD, -3.0)
        p = PtReprojectParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"], 0)
        a = ref.pt_camera(cam)
        b = ref.pt_camera(hist_cam) if hist_cam is not None else None
        P = self.p
        hist = [P["hcolor"], P["hlen"], P["hdepth"], P["hoid"]] if history else [None] * 4
        rc = self.L.pt_ctx_reproject(self.ctx, w, h, None if default_params else C.byref(p), C.byref(a), P["color"], P["depth"],
                                     P["oid"], P["normal"] if normal else None, C.byref(b) if b is not None else None, *hist,
                                     P["hnormal"] if hist_normal else None, P[out], P["len"], stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.read_guarded(out, n * 3, GUARD, -3.0, "the colour output")
        return got.reshape(n, 3), self.read_guarded("len", n, GUARD, -3.0, "the length output")


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


# ------------------------------------------------------------------------------------------------------ the inputs
def synthetic(w, h):
    """(cur, hist): random colours in [0, 1]; depths on a few planes, in blocks so that neighbours mostly share one, and +inf;
    ids in {-1, 0, 1, 2}; normals around one direction, a tenth of them zero; history lengths 0, 4, .. 16; the history's guides
    are the frame's own with a part disturbed.  Pixel 0 always has a history that passes (the one-pixel frame blends)."""
    rng = np.random.default_rng(w * 100 + h)
    n = w * h
    planes = np.array([2.0, 6.0, 6.25, 9.0, np.inf], dtype=F32)
    block = (np.arange(n) % w) // 3 + (np.arange(n) // w) // 2
    depth = np.where(rng.random(n) < 0.1, planes[rng.integers(0, 5, n)], planes[block % 4]).astype(F32)
    oid = np.where(rng.random(n) < 0.15, rng.integers(-1, 3, n), block % 3).astype(I32)
    normal = (np.array([0.2, 0.3, 1.0], dtype=F32) + (rng.random((n, 3)).astype(F32) - F32(0.5)) * F32(0.6)).astype(F32)
    normal[rng.random(n) < 0.1] = 0
    depth[0], oid[0], normal[0] = 6.0, 1, (0.0, 0.0, 1.0)
    cur = dict(color=rng.random((n, 3)).astype(F32), depth=depth, oid=oid, normal=normal)
    hnormal = normal.copy()
    flip = rng.random(n) < 0.1
    hnormal[flip] = -hnormal[flip]
    hist = dict(color=rng.random((n, 3)).astype(F32), len=(rng.integers(0, 5, n) * 4).astype(F32),
                depth=np.where(rng.random(n) < 0.15, depth * F32(1.2), depth).astype(F32),
                oid=np.where(rng.random(n) < 0.1, rng.integers(-1, 3, n), oid).astype(I32), normal=hnormal)
    hist["len"][0], hist["depth"][0], hist["oid"][0], hist["normal"][0] = 8.0, 6.0, 1, (0.0, 0.0, 1.0)
    return cur, hist


def want(w, h, cam, cur, hist_cam=None, hist=None, normal=True, hist_normal=True, params=PARAMS):
    kw = {}
    if hist is not None:
        kw = dict(hist_cam=hist_cam, hist_color=hist["color"], hist_len=hist["len"], hist_depth=hist["depth"],
                  hist_object_id=hist["oid"], hist_normal=hist["normal"] if hist_normal else None)
    return ref.reproject(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"] if normal else None, **kw, **params)


def same_bytes(got, exp, what):
    for name, a, b in (("colour", got[0], exp[0]), ("length", got[1], exp[1])):
        gpudev.same_bytes(a, b, "%s %s" % (what, name))


# --------------------------------------------------------------------------------------------------- synthetic frames
@pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % s for s in FRAMES])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_is_the_restatement(dev, size, camera):
    w, h = size
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    exp = want(w, h, cam, cur, hist_cam, hist)
    same_bytes(dev.reproject(w, h, cam, hist_cam), exp, camera)
    # the inputs reach what they are there for: some pixels blend, and under the last camera some have no position
    blended = exp[1] > PARAMS["weight"]
    if camera != "partly-behind" or w * h > 35:
        assert blended.any(), camera
    if w * h > 35:
        assert not blended.all()
    if camera == "partly-behind" and w * h > 35:
        ok = ref.project(cam, hist_cam, w, h, np.arange(w * h), np.full(w * h, 6.0, dtype=F32))[0]
        assert 0.1 < ok.mean() < 0.9


# ------------------------------------------------------------------------------------- thin, long and full-size frames
# A tuple of its own, so that the parametrisations over FRAMES keep their cost.  The calls of this family check only
# width * height <= 2^28: an axis may be longer than the 2^14 pt_ctx_upsample stops at.
# - 100 x 30: 4 x 4 tiles of kernel B (32 x 8), the first frame with a tile that has neighbours on all four sides (W >= 65, H >= 17);
# - 65536 x 4: a width of 2^16 > 2^14, 2048 tiles across and one down, a row of 1024 workgroups of 256;
# - 3 x 40 000: tiles_x = 1 with 5000 tile rows, a height above 2^14, every workgroup of 256 spans 85 rows;
# - 1 x 262 144: a height of 2^18, one column: every tap beside it is outside the frame;
# - 1024 x 768: the documented frame, 3072 workgroups, 32 x 96 tiles.
# synthetic() seeds from w * 100 + h: 10030, 6553604, 40300, 262244 and 103168 - none is the seed of another shape here.
LARGE = ((100, 30), (65536, 4), (3, 40000), (1, 262144), (1024, 768))
LARGE_IDS = ["%dx%d" % s for s in LARGE]
MAXPIX_LARGE = max(w * h for w, h in LARGE)
_seeds = [w * 100 + h for w, h in FRAMES + LARGE]
assert len(set(_seeds)) == len(_seeds)


def tiles_of(w, h):
    """kernel B's grid: (tiles_x, tiles_y) of 32 x 8"""
    return -(-w // 32), -(-h // 8)


@pytest.fixture(scope="module")
def bigdev(L):
    with Dev(L, MAXPIX_LARGE) as d:
        yield d


@pytest.mark.parametrize("size", LARGE, ids=LARGE_IDS)
@pytest.mark.parametrize("camera", ["identical", "translated"])
def test_large_frames_are_the_restatement(bigdev, size, camera):
    w, h = size
    assert w * h <= 1 << 28  # all the validator asks
    premise = {(100, 30): tiles_of(w, h) == (4, 4), (65536, 4): w > 1 << 14 and tiles_of(w, h) == (2048, 1),
               (3, 40000): h > 1 << 14 and tiles_of(w, h) == (1, 5000), (1, 262144): h == 1 << 18 and w == 1,
               (1024, 768): -(-w * h // 256) == 3072 and tiles_of(w, h) == (32, 96)}
    assert premise[size]
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    bigdev.put(cur, hist)
    exp = want(w, h, cam, cur, hist_cam, hist)
    got = bigdev.reproject(w, h, cam, hist_cam)
    same_bytes(got, exp, (size, camera))
    assert not (got[0] == -3.0).any() and not (got[1] == -3.0).any()  # no pixel still holds the fill pattern
    blended = exp[1] > PARAMS["weight"]
    print("%dx%d %s: %d of %d pixels blend" % (w, h, camera, blended.sum(), w * h))
    assert blended.any() and not blended.all()


@pytest.mark.parametrize("camera", ["identical", "translated"])
def test_optional_normals(dev, camera):
    w, h = 33, 25
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    both = dev.reproject(w, h, cam, hist_cam)
    results = []
    for normal, hist_normal in ((False, False), (False, True), (True, False)):
        got = dev.reproject(w, h, cam, hist_cam, normal=normal, hist_normal=hist_normal)
        same_bytes(got, want(w, h, cam, cur, hist_cam, hist, normal=normal, hist_normal=hist_normal), (camera, normal, hist_normal))
        results.append(got)
    # the normal test runs only when both are given: the three forms agree, and differ from the call with both
    assert all(r[0].tobytes() == results[0][0].tobytes() and r[1].tobytes() == results[0][1].tobytes() for r in results)
    assert both[1].tobytes() != results[0][1].tobytes()


def test_first_frame_form(L, dev):
    w, h = 33, 25
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    for params in (PARAMS, dict(PARAMS, weight=0)):
        got = dev.reproject(w, h, CUR, None, history=False, hist_normal=False, params=params)
        assert got[0].tobytes() == cur["color"].tobytes() and (got[1] == (params["weight"] or 1)).all()
    # hist_cam and a lone history normal are not read
    got = dev.reproject(w, h, CUR, None, history=False, hist_normal=True)
    assert got[0].tobytes() == cur["color"].tobytes() and (got[1] == 4).all()
    # a partial set is refused on the device's side too
    a = ref.pt_camera(CUR)
    P = dev.p
    rc = L.pt_ctx_reproject(dev.ctx, w, h, None, C.byref(a), P["color"], P["depth"], P["oid"], None, C.byref(a), P["hcolor"], None,
                            P["hdepth"], P["hoid"], None, P["out"], P["len"], None)
    assert rc == -1 and "history" in L.pt_last_error().decode()


def test_defaults_stand_for_zero(L, dev):
    w, h = 33, 25
    cam, hist_cam = CAMERAS["translated"]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    d = ref.defaults(L)
    exp = want(w, h, cam, cur, hist_cam, hist, params=d)
    same_bytes(dev.reproject(w, h, cam, hist_cam, default_params=True), exp, "NULL params")
    same_bytes(dev.reproject(w, h, cam, hist_cam, params=dict(weight=0, max_history=0.0, depth_tol=0.0, normal_min=0.0)), exp, "zeros")


@pytest.mark.parametrize("camera", ["identical", "translated"])
def test_in_place_and_on_a_stream(dev, camera):
    w, h = 33, 25
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    exp = want(w, h, cam, cur, hist_cam, hist)
    with dev.stream() as st:
        same_bytes(dev.reproject(w, h, cam, hist_cam, stream=st), exp, "stream")
        same_bytes(dev.reproject(w, h, cam, hist_cam), exp, "again")
        same_bytes(dev.reproject(w, h, cam, hist_cam, in_place=True, stream=st), exp, "in place")  # d_out_color == d_color


def test_still_camera_accumulates_a_running_mean(dev):
    """three calls with one camera, the outputs swapped in as the history: lengths 4, 8, 12 and the mean of the three colours"""
    w, h = 7, 5
    n = w * h
    rng = np.random.default_rng(9)
    guides = dict(depth=np.full(n, 6.0, dtype=F32), oid=np.ones(n, dtype=I32), normal=np.tile(np.array([0, 0, 1], dtype=F32), (n, 1)))
    colors = [rng.random((n, 3)).astype(F32) for _ in range(3)]
    hist = None
    for k, c in enumerate(colors):
        cur = dict(guides, color=c)
        dev.put(cur, hist)
        got = dev.reproject(w, h, CUR, CUR, history=hist is not None, hist_normal=hist is not None)
        same_bytes(got, want(w, h, CUR, cur, CUR, hist), k)
        hist = dict(guides, color=got[0], len=got[1])
    assert (hist["len"] == 12).all()
    assert np.abs(hist["color"] - np.mean(colors, axis=0)).max() < 1e-6


# ---------------------------------------------------------------------------------------------------- no state touched
def test_leaves_the_context_alone(L):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    w, h = 33, 25
    with Dev(L, w * h) as d:
        d.set_scene(sc)
        d.render(gpudev.config(w, h, 4, seed=3), d.p["hcolor"])
        before = d.download("hcolor", w * h * 3)
        cur, hist = synthetic(w, h)
        d.put(cur, hist)
        cam, hist_cam = CAMERAS["translated"]
        same_bytes(d.reproject(w, h, cam, hist_cam), want(w, h, cam, cur, hist_cam, hist), "with a scene")
        for name, key in (("color", "color"), ("depth", "depth"), ("normal", "normal"), ("hcolor", "color"), ("hlen", "len")):
            src = cur if not name.startswith("h") else hist
            assert d.download(name, src[key].size).tobytes() == src[key].tobytes(), name  # the inputs are read only
        d.render(gpudev.config(w, h, 4, seed=3), d.p["hcolor"])
        assert d.download("hcolor", w * h * 3).tobytes() == before.tobytes()


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_cornell(L):
    """Frame A with the scene's camera, frame B one step of the study's orbit on (reproject_ref.ORBIT_DEGREES), each at the study's
    samples per pixel with its first-hit guides; the history starts at A and is reprojected onto B.
    (a) the outputs are the restatement's on the downloaded inputs, bit for bit;
    (b) at least 3/4 of B's hit pixels end with len_out > wt;
    (c) over those pixels the mean absolute error against B's truth (4096 samples on the device) is below that of B's own colour.
    The study (profiles/reproject_cpu_study.json, "end_to_end") shows (b) and (c) on oracle inputs, for the whole frame: share
    0.983, errors 0.0822 with history against 0.1280 without."""
    w, h = ref.ORBIT_SIZE
    spp = ref.ORBIT_SPP
    n = w * h
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    cam_a = ref.cam_dict(sc.cam)
    cam_b = ref.orbit(cam_a, ref.ORBIT_DEGREES)
    with Dev(L, n) as d:
        d_truth = d.alloc(n * 12)
        frames = {}
        for name, cam, seed in (("a", cam_a, 11), ("b", cam_b, 12)):
            c = ref.pt_camera(cam)
            d.set_scene(sc, c)
            d.render(gpudev.config(w, h, spp, seed=seed), d.p["color"])
            cfg = PtConfig(w, h, spp, 0, seed, 0, 0, 0, 0)
            assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), None, d.p["normal"], d.p["depth"], d.p["oid"], None) == 0, L.pt_last_error()
            frames[name] = dict(color=d.download("color", n * 3).reshape(n, 3), depth=d.download("depth", n),
                                oid=d.download("oid", n, I32), normal=d.download("normal", n * 3).reshape(n, 3))
            if name == "a":  # the history starts here: the first-frame form, in place
                first = d.reproject(w, h, cam, None, history=False, hist_normal=False, in_place=True, params=dict(PARAMS, weight=spp))
                assert first[0].tobytes() == frames["a"]["color"].tobytes() and (first[1] == spp).all()
                frames["a"]["len"] = first[1]
            else:
                d.render(gpudev.config(w, h, 4096, seed=1012), d_truth)
        truth = d.pixels(d_truth, n)
        a, b = frames["a"], frames["b"]
        d.put(b, a)
        params = dict(ref.defaults(L), weight=spp)
        got = d.reproject(w, h, cam_b, cam_a, params=params)
        same_bytes(got, want(w, h, cam_b, b, cam_a, a, params=params), "cornell")                          # (a)
        hit = b["oid"] >= 0
        found = hit & (got[1] > spp)
        share = found.sum() / hit.sum()
        with_history = np.abs(got[0][found].astype(np.float64) - truth[found]).mean()
        without = np.abs(b["color"][found].astype(np.float64) - truth[found]).mean()
        print("share %.4f, error with history %.5f, without %.5f, over %d pixels" % (share, with_history, without, found.sum()))
        assert share >= 0.75, share                                                                       # (b)
        assert with_history < without, (with_history, without)                                            # (c)
