"""pt_ctx_reproject_var on the GPU against tests/reproject_var_ref.py, the restatement of the contract in include/ptrace.h in
numpy binary32.  Every comparison with the restatement is of bytes, for equality, and every output has guard floats behind it.
The frames are the smallest at which either kernel can go wrong: 1x1 and 7x5 (smaller than the window's halo), 257x3 (two
workgroups of kernel A with a one-lane tail, nine tiles of kernel B across with a one-pixel tail, the window leaving the frame
above and below everywhere) and 33x25 (two tiles across and four down, both with a one-pixel tail).  The cameras are
tests/test_gpu_reproject.py's four.  The history lengths are laid out by kernel B's tiles of 32 x 8 - some all long, some all
short, some mixed - so that a workgroup that returns early sits next to one that works."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_ref as dvr
import gpudev
import ptlib
import reproject_ref as ref
import reproject_var_ref as rv
import test_gpu_reproject as base
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtConfig, PtReprojectParams, PtReprojectVarParams
from reproject_ref import F32, I32

pytestmark = pytest.mark.gpu

GUARD = 64
FRAMES = base.FRAMES
CAMERAS = base.CAMERAS
CUR = base.CUR
MAXPIX = 96 * 64
PARAMS = dict(base.PARAMS, min_frames=4, radius=3)  # weight 4: a history of 16 samples is long
TILE = (32, 8)

NAMES = ("color", "depth", "oid", "normal", "hcolor", "hlen", "hmom", "hdepth", "hoid", "hnormal", "out", "len", "mom", "err",
         "albedo", "dn")
FLOATS = dict(color=3, depth=1, oid=1, normal=3, hcolor=3, hlen=1, hmom=2, hdepth=1, hoid=1, hnormal=3, out=3, len=1, mom=2, err=1,
              albedo=3, dn=3)
OUTS = (("out", 3), ("len", 1), ("mom", 2), ("err", 1))


class Dev(gpudev.Device):
    """one context and the planes of a call, the four outputs with guard floats behind whatever a call writes"""

    def __init__(self, L, max_pix=MAXPIX):
        super().__init__(L)
        for name in NAMES:
            self.alloc((max_pix * FLOATS[name] + GUARD) * 4, name)

    def put(self, cur, hist=None):
        for name, key in (("color", "color"), ("depth", "depth"), ("oid", "oid"), ("normal", "normal")):
            self.upload(name, cur[key])
        if hist is not None:
            for name, key in (("hcolor", "color"), ("hlen", "len"), ("hmom", "mom"), ("hdepth", "depth"), ("hoid", "oid"),
                              ("hnormal", "normal")):
                self.upload(name, hist[key])

    def _guards(self, n, in_place):
        for name, k in OUTS:  # (in place: the guard of the colour plane, behind the frame)
            self.fill_guarded("color" if name == "out" and in_place else name, n * k, GUARD, -3.0, tail_only=name == "out" and in_place)

    def _collect(self, n, in_place):
        got = [self.read_guarded("color" if name == "out" and in_place else name, n * k, GUARD, -3.0, name) for name, k in OUTS]
        return tuple(a.reshape(n, k) if k > 1 else a for a, (_, k) in zip(got, OUTS))

    def reproject_var(self, w, h, cam, hist_cam=None, normal=True, hist_normal=True, history=True, in_place=False, stream=None,
                      params=PARAMS, default_params=False, ctx=None):
        """the four outputs of one call: colour (n, 3), length (n,), moments (n, 2), error (n,)"""
        n = w * h
        self._guards(n, in_place)
        p = PtReprojectVarParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"],
                                 params["min_frames"], params["radius"], 0)
        a = ref.pt_camera(cam)
        b = ref.pt_camera(hist_cam) if hist_cam is not None else None
        P = self.p
        hist = [P["hcolor"], P["hlen"], P["hmom"], P["hdepth"], P["hoid"]] if history else [None] * 5
        rc = self.L.pt_ctx_reproject_var(ctx or self.ctx, w, h, None if default_params else C.byref(p), C.byref(a), P["color"],
                                         P["depth"], P["oid"], P["normal"] if normal else None, C.byref(b) if b is not None else None,
                                         *hist, P["hnormal"] if hist_normal else None, P["color" if in_place else "out"], P["len"],
                                         P["mom"], P["err"], stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        return self._collect(n, in_place)

    def reproject(self, w, h, cam, hist_cam, params=PARAMS):
        """pt_ctx_reproject on the planes as they are: (colour, length)"""
        n = w * h
        self.fill_guarded("out", n * 3, GUARD, -3.0)
        self.fill_guarded("len", n, GUARD, -3.0)
        p = PtReprojectParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"], 0)
        a, b = ref.pt_camera(cam), ref.pt_camera(hist_cam)
        P = self.p
        rc = self.L.pt_ctx_reproject(self.ctx, w, h, C.byref(p), C.byref(a), P["color"], P["depth"], P["oid"], P["normal"], C.byref(b),
                                     P["hcolor"], P["hlen"], P["hdepth"], P["hoid"], P["hnormal"], P["out"], P["len"], None)
        assert rc == 0, (rc, self.L.pt_last_error())
        return self.download("out", n * 3).reshape(n, 3), self.download("len", n)


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


# ------------------------------------------------------------------------------------------------------ the inputs
def tile_class(w, h):
    """per pixel: 0 mixed, 1 all long, 2 all short - by kernel B's tile, so that the three kinds are neighbours"""
    x, r = np.arange(w * h) % w, np.arange(w * h) // w
    return (x // TILE[0] + r // TILE[1]) % 3


_cache = {}


def synthetic(w, h):
    """tests/test_gpu_reproject.py's frames, with history moments, and laid out by tile: in a tile of class 1 the history is the
    frame's own surface (guides equal, ids >= 0, finite depths) with 16 samples, so under the identical camera every pixel of it
    ends long; in a tile of class 2 the history is empty, so every pixel ends short; the rest keeps the random lengths 0..16."""
    if (w, h) in _cache:
        return _cache[(w, h)]
    cur, hist = base.synthetic(w, h)
    rng = np.random.default_rng(w * 1000 + h)
    n = w * h
    cls = tile_class(w, h)
    lng = cls == 1
    cur["oid"][lng] = np.maximum(cur["oid"][lng], 0)
    cur["depth"][lng] = np.where(np.isfinite(cur["depth"][lng]), cur["depth"][lng], F32(9.0))
    cur["normal"][lng] = np.array([0.2, 0.3, 1.0], dtype=F32)
    for key in ("depth", "oid", "normal"):
        hist[key][lng] = cur[key][lng]
    hist["len"][lng] = 16.0
    hist["len"][cls == 2] = 0.0
    m1 = (rng.random(n) * 3).astype(F32)
    hist["mom"] = np.stack([m1, m1 * m1 + rng.random(n).astype(F32)], axis=1).astype(F32)
    _cache[(w, h)] = (cur, hist)
    return cur, hist


def want(w, h, cam, cur, hist_cam=None, hist=None, normal=True, hist_normal=True, params=PARAMS, parts=False):
    kw = {}
    if hist is not None:
        kw = dict(hist_cam=hist_cam, hist_color=hist["color"], hist_len=hist["len"], hist_moments=hist["mom"], hist_depth=hist["depth"],
                  hist_object_id=hist["oid"], hist_normal=hist["normal"] if hist_normal else None)
    return rv.reproject_var(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"] if normal else None, parts=parts, **kw,
                            **params)


def same_bytes(got, exp, what):
    for name, a, b in zip(("colour", "length", "moments", "error"), got, exp):
        gpudev.same_bytes(a, b, "%s %s" % (what, name))


# --------------------------------------------------------------------------------------------------- synthetic frames
@pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % s for s in FRAMES])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_is_the_restatement_and_the_old_kernel(dev, size, camera):
    w, h = size
    n = w * h
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    old = dev.reproject(w, h, cam, hist_cam)
    # the witness of the moments: the existing kernel fed (s, s*s, 0) as the colour and (m1, m2, 0) as the history colour
    s = rv.s_of(cur["color"])
    dev.upload("color", np.stack([s, s * s, np.zeros(n, F32)], axis=1).astype(F32))
    dev.upload("hcolor", np.concatenate([hist["mom"], np.zeros((n, 1), F32)], axis=1))
    witness = dev.reproject(w, h, cam, hist_cam)
    dev.put(cur, hist)
    for min_frames in (1, 4):
        for radius in (1, 2, 3):
            params = dict(PARAMS, min_frames=min_frames, radius=radius)
            got = dev.reproject_var(w, h, cam, hist_cam, params=params)
            exp = want(w, h, cam, cur, hist_cam, hist, params=params, parts=True)
            same_bytes(got, exp[:4], (camera, min_frames, radius))
            assert got[0].tobytes() == old[0].tobytes() and got[1].tobytes() == old[1].tobytes(), "pt_ctx_reproject's outputs"
            assert np.ascontiguousarray(got[2]).tobytes() == np.ascontiguousarray(witness[0][:, :2]).tobytes(), "the witness"
            assert witness[1].tobytes() == old[1].tobytes() and (witness[0][:, 2] == 0).all()
            long = exp[4]["long"]
            if min_frames == 1:
                assert long.all()  # kernel B returns everywhere
            elif camera == "identical" and w > TILE[0]:
                # the layout reaches what it is there for: tiles all long, all short and mixed, side by side
                cls = tile_class(w, h)
                assert long[cls == 1].all() and not long[cls == 2].any()
                assert 0 < long[cls == 0].mean() < 1
            if min_frames == 4 and n > 1:
                assert np.isfinite(got[3][~long]).any()


# ------------------------------------------------------------------------------------- thin, long and full-size frames
# tests/test_gpu_reproject.py's LARGE says what each shape crosses; kernel B's grid is one-dimensional, blockIdx.x % tiles_x and
# blockIdx.x / tiles_x, so tiles_x = 1 over 5000 tile rows (3 x 40 000), its transpose (65536 x 4: 2048 x 1) and one column of
# 32 768 tiles (1 x 262 144) are the shapes at which a wrong tiles_x shows.
LARGE = base.LARGE


@pytest.fixture(scope="module")
def bigdev(L):
    with Dev(L, base.MAXPIX_LARGE) as d:
        yield d


def no_fill_left(got):
    for a in got:
        assert not (a == -3.0).any()  # no output word still holds the fill pattern


@pytest.mark.parametrize("size", LARGE, ids=base.LARGE_IDS)
@pytest.mark.parametrize("camera", ["identical", "translated"])
def test_large_frames_are_the_restatement(bigdev, size, camera):
    w, h = size
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    bigdev.put(cur, hist)
    got = bigdev.reproject_var(w, h, cam, hist_cam)
    exp = want(w, h, cam, cur, hist_cam, hist, parts=True)
    same_bytes(got, exp[:4], (size, camera))
    no_fill_left(got)
    long = exp[4]["long"]
    print("%dx%d %s: %d of %d pixels short, tiles %s" % (w, h, camera, (~long).sum(), w * h, base.tiles_of(w, h)))
    assert 0 < long.mean() < 1 and np.isfinite(got[3][~long]).any()
    if camera == "identical" and w > TILE[0]:
        cls = tile_class(w, h)
        assert long[cls == 1].all() and not long[cls == 2].any() and 0 < long[cls == 0].mean() < 1


# Every pixel short: the first-frame form (each pixel ends with wt = 4 samples, below min_frames * wt = 16), so every workgroup of
# kernel B stages its tile and halo and every lane runs the window - which the mixed layouts above never ask of an interior tile.
# - 100 x 30: 4 x 4 tiles; tile (1, 1) has full neighbours on all four sides (W >= 65, H >= 17), the last column is 4 wide and the
#   last row 6 high;
# - 3 x 40 000: tiles_x = 1, 5000 tile rows, the window leaves the frame left and right of every pixel;
# - 1024 x 768: 32 x 96 full tiles, the 49-tap window over 786 432 pixels.
SHORT = ((100, 30), (3, 40000), (1024, 768))
_short = {}


def short_frame(w, h):
    """A frame for the window: the object ids and depths lie in blocks whose borders fall, in every tile of 32 x 8, on the tile's
    own border (x % 32 == 0, r % 8 == 0), inside it (x % 32 == 16) and three pixels before its far border (x % 32 == 29,
    r % 8 == 5) - the first column and row of the NEXT tile's halo, so a block's corner sits in a halo's corner.  A tenth of the
    pixels get a random id and plane, as in the other frames."""
    if (w, h) not in _short:
        cur, _ = base.synthetic(w, h)
        n = w * h
        rng = np.random.default_rng(w * 1000 + h + 7)
        x, r = np.arange(n) % w, np.arange(n) // w
        bx = (x // TILE[0]) * 3 + (x % TILE[0] >= 16) + (x % TILE[0] >= 29)
        by = (r // TILE[1]) * 2 + (r % TILE[1] >= 5)
        planes = np.array([2.0, 6.0, 6.25, 9.0, np.inf], dtype=F32)
        depth = np.where(rng.random(n) < 0.1, planes[rng.integers(0, 5, n)], planes[(bx + 2 * by) % 4]).astype(F32)
        oid = np.where(rng.random(n) < 0.1, rng.integers(-1, 3, n), (bx + by) % 3).astype(I32)
        _short[(w, h)] = dict(cur, depth=depth, oid=oid)
    return _short[(w, h)]


@pytest.mark.parametrize("size", SHORT, ids=["%dx%d" % s for s in SHORT])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_every_pixel_short(bigdev, size, radius):
    w, h = size
    tiles = base.tiles_of(w, h)
    assert tiles == {(100, 30): (4, 4), (3, 40000): (1, 5000), (1024, 768): (32, 96)}[size]
    if size == (100, 30):
        assert w >= 2 * TILE[0] + 1 and h >= 2 * TILE[1] + 1 and tiles[0] >= 3 and tiles[1] >= 3  # an interior tile exists
    cur = short_frame(w, h)
    bigdev.put(cur)
    params = dict(PARAMS, radius=radius)
    assert params["min_frames"] > 1
    got = bigdev.reproject_var(w, h, CUR, None, history=False, hist_normal=False, params=params)
    exp = want(w, h, CUR, cur, params=params, parts=True)
    assert not exp[4]["long"].any()  # the premise: every lane of every tile runs the window
    same_bytes(got, exp[:4], (size, radius))
    no_fill_left(got)
    cnt = exp[4]["cnt"]
    print("%dx%d radius %d: taps taken %d..%d, %d pixels without an estimate" % (w, h, radius, cnt.min(), cnt.max(), (cnt < 2).sum()))
    assert cnt.max() > cnt.min() and cnt.max() > 2 * radius + 1 and np.isfinite(got[3]).any()


@pytest.mark.parametrize("camera", ["identical", "translated"])
def test_optional_normals(dev, camera):
    w, h = 33, 25
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    both = dev.reproject_var(w, h, cam, hist_cam)
    results = []
    for normal, hist_normal in ((False, False), (False, True), (True, False)):
        got = dev.reproject_var(w, h, cam, hist_cam, normal=normal, hist_normal=hist_normal)
        same_bytes(got, want(w, h, cam, cur, hist_cam, hist, normal=normal, hist_normal=hist_normal), (camera, normal, hist_normal))
        results.append(got)
    assert all(all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(r, results[0]))
               for r in results)
    assert both[1].tobytes() != results[0][1].tobytes()


def test_first_frame_form(L, dev):
    for w, h in FRAMES:
        cur, hist = synthetic(w, h)
        dev.put(cur, hist)
        s = rv.s_of(cur["color"])
        for params in (PARAMS, dict(PARAMS, weight=0)):
            got = dev.reproject_var(w, h, CUR, None, history=False, hist_normal=False, params=params)
            same_bytes(got, want(w, h, CUR, cur, params=params), "first frame")
            assert got[0].tobytes() == cur["color"].tobytes() and (got[1] == (params["weight"] or 1)).all()
            assert got[2].tobytes() == np.stack([s, s * s], axis=1).tobytes()
        if w * h == 1:
            assert got[3][0] == np.inf  # a window of one pixel: no estimate
        else:
            assert np.isfinite(got[3]).any()
    # hist_cam and a lone history normal are not read
    w, h = FRAMES[-1]
    got = dev.reproject_var(w, h, CUR, None, history=False, hist_normal=True)
    same_bytes(got, want(w, h, CUR, cur), "lone normal")
    # a partial set - the moments missing - is refused on the device's side too
    a = ref.pt_camera(CUR)
    P = dev.p
    rc = L.pt_ctx_reproject_var(dev.ctx, w, h, None, C.byref(a), P["color"], P["depth"], P["oid"], None, C.byref(a), P["hcolor"], P["hlen"],
                                None, P["hdepth"], P["hoid"], None, P["out"], P["len"], P["mom"], P["err"], None)
    assert rc == -1 and "history" in L.pt_last_error().decode()


def test_defaults_stand_for_zero(L, dev):
    w, h = 33, 25
    cam, hist_cam = CAMERAS["translated"]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    d = rv.defaults(L)
    exp = want(w, h, cam, cur, hist_cam, hist, params=d)
    same_bytes(dev.reproject_var(w, h, cam, hist_cam, default_params=True), exp, "NULL params")
    zeros = dict(weight=0, max_history=0.0, depth_tol=0.0, normal_min=0.0, min_frames=0, radius=0)
    same_bytes(dev.reproject_var(w, h, cam, hist_cam, params=zeros), exp, "zeros")


@pytest.mark.parametrize("camera", ["identical", "translated"])
def test_in_place_and_on_a_stream(dev, camera):
    w, h = 33, 25
    cam, hist_cam = CAMERAS[camera]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    exp = want(w, h, cam, cur, hist_cam, hist)
    with dev.stream() as st:
        same_bytes(dev.reproject_var(w, h, cam, hist_cam, stream=st), exp, "stream")
        same_bytes(dev.reproject_var(w, h, cam, hist_cam), exp, "again")
        same_bytes(dev.reproject_var(w, h, cam, hist_cam, in_place=True, stream=st), exp, "in place")  # d_out_color == d_color


def test_scratch_grows_and_is_reused(L, dev):
    """one context called at 7x5, then 33x25 (the s plane grows), then 7x5 again (it is reused, larger than the frame): each call
    gives the bytes a fresh context gives"""
    cam, hist_cam = CAMERAS["translated"]
    with gpudev.Device(L) as one:
        for w, h in ((7, 5), (33, 25), (7, 5)):
            cur, hist = synthetic(w, h)
            dev.put(cur, hist)
            with gpudev.Device(L) as fresh:
                exp = dev.reproject_var(w, h, cam, hist_cam, ctx=fresh.ctx)
            same_bytes(dev.reproject_var(w, h, cam, hist_cam, ctx=one.ctx), exp, (w, h))
            same_bytes(exp, want(w, h, cam, cur, hist_cam, hist), (w, h))


def test_leaves_the_context_alone(L):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    w, h = 33, 25
    with Dev(L, w * h) as d:
        d.set_scene(sc)
        d.render(gpudev.config(w, h, 4, seed=3), d.p["dn"])
        rendered = d.download("dn", w * h * 3)
        cur, hist = synthetic(w, h)
        d.put(cur, hist)
        cam, hist_cam = CAMERAS["translated"]
        old = d.reproject(w, h, cam, hist_cam)
        same_bytes(d.reproject_var(w, h, cam, hist_cam), want(w, h, cam, cur, hist_cam, hist), "with a scene")
        for name, key in (("color", "color"), ("depth", "depth"), ("normal", "normal"), ("hcolor", "color"), ("hlen", "len"),
                          ("hmom", "mom")):
            src = cur if not name.startswith("h") else hist
            assert d.download(name, src[key].size).tobytes() == src[key].tobytes(), name  # the inputs are read only
        again = d.reproject(w, h, cam, hist_cam)
        assert again[0].tobytes() == old[0].tobytes() and again[1].tobytes() == old[1].tobytes()
        d.render(gpudev.config(w, h, 4, seed=3), d.p["dn"])
        assert d.download("dn", w * h * 3).tobytes() == rendered.tobytes()


# ------------------------------------------------------------------------------------------------------ the consumer
def denoise_var(L, d, w, h, color, sigma_var):
    """pt_ctx_denoise_var of the plane `color` with d_error as it stands, guided by albedo, normal and depth: (w*h, 3)"""
    levels, _, sigma_depth = dvr.defaults(L)
    p = ptlib.PtDenoiseVarParams(levels, sigma_var, sigma_depth, 0)
    P = d.p
    rc = L.pt_ctx_denoise_var(d.ctx, w, h, C.byref(p), P[color], P["err"], P["albedo"], P["normal"], P["depth"], P["dn"], None)
    assert rc == 0, (rc, L.pt_last_error())
    return d.download("dn", w * h * 3).reshape(w * h, 3), (levels, sigma_var, sigma_depth)


def test_error_map_feeds_denoise_var(L, dev):
    """d_error goes into pt_ctx_denoise_var as it is - finite estimates, zeros and +inf alike - and the result is the
    restatement's on the downloaded inputs"""
    w, h = 33, 25
    cam, hist_cam = CAMERAS["translated"]
    cur, hist = synthetic(w, h)
    dev.put(cur, hist)
    rng = np.random.default_rng(5)
    albedo = (rng.random((w * h, 3)) * 0.9 + 0.05).astype(F32)
    dev.upload("albedo", albedo)
    out, _, _, err = dev.reproject_var(w, h, cam, hist_cam)
    assert np.isfinite(err).any() and (err >= 0).all()
    got, (levels, sv, sd) = denoise_var(L, dev, w, h, "out", 2.0)
    exp = dvr.denoise_var(out, err, w, h, albedo, cur["normal"], cur["depth"], levels, sv, sd)
    assert got.tobytes() == exp.tobytes()
    assert got.tobytes() != out.tobytes()


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_cornell(L):
    """Frame A with the scene's camera, frame B one step of the study's orbit on (reproject_ref.ORBIT_DEGREES), each at the study's
    samples per pixel (reproject_ref.ORBIT_SPP) with its first-hit guides; A starts the history (the first-frame form, in place),
    B reprojects it; all at the defaults, weight = spp.  sigma_var is the study's.
    (a) the four outputs of both calls are the restatement's on the downloaded inputs, bit for bit;
    (b) on frame A every hit pixel has a finite e;
    (c) on frame A, pt_ctx_denoise_var fed with e has a lower mean absolute error over the hit pixels against A's truth (4096
        samples on the device) than the unfiltered frame;
    (d) on frame B its error is not above that of reprojection alone.
    The study (profiles/reproject_var_cpu_study.json, "chosen_result", 8 samples per frame) shows (c) and (d) on oracle inputs:
    frame 0: 0.0345 after pt_ctx_denoise_var against 0.1284 unfiltered; frame 1: 0.0412 against 0.0834 after reprojection alone."""
    import json
    import os
    w, h = ref.ORBIT_SIZE
    spp = ref.ORBIT_SPP
    n = w * h
    study = json.load(open(os.path.join(ptlib.ROOT, "profiles", "reproject_var_cpu_study.json")))
    sigma_var = study["chosen"]["sigma_var"]
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    cam_a = ref.cam_dict(sc.cam)
    cam_b = ref.orbit(cam_a, ref.ORBIT_DEGREES)
    params = dict(rv.defaults(L), weight=spp)
    with Dev(L, n) as d:
        d_truth = d.alloc(n * 12)
        hist = None
        for name, cam, hist_cam, seed in (("a", cam_a, None, 11), ("b", cam_b, cam_a, 12)):
            c = ref.pt_camera(cam)
            d.set_scene(sc, c)
            truth, _ = d.render(gpudev.config(w, h, 4096, seed=1000 + seed), d_truth)
            d.render(gpudev.config(w, h, spp, seed=seed), d.p["color"])
            cfg = PtConfig(w, h, spp, 0, seed, 0, 0, 0, 0)
            assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), d.p["albedo"], d.p["normal"], d.p["depth"], d.p["oid"], None) == 0, \
                L.pt_last_error()
            cur = dict(color=d.download("color", n * 3).reshape(n, 3), depth=d.download("depth", n), oid=d.download("oid", n, I32),
                       normal=d.download("normal", n * 3).reshape(n, 3), albedo=d.download("albedo", n * 3).reshape(n, 3))
            if hist is not None:
                d.put(cur, hist)
            got = d.reproject_var(w, h, cam, hist_cam, history=hist is not None, hist_normal=hist is not None, in_place=True,
                                  params=params)
            same_bytes(got, want(w, h, cam, cur, hist_cam, hist, params=params), name)                    # (a)
            hit = cur["oid"] >= 0
            dn, (levels, sv, sd) = denoise_var(L, d, w, h, "color", sigma_var)
            assert dn.tobytes() == dvr.denoise_var(got[0], got[3], w, h, cur["albedo"], cur["normal"], cur["depth"], levels, sv,
                                                   sd).tobytes()

            def mae(x):
                return np.abs(x[hit].astype(np.float64) - truth[hit]).mean()

            e_in, e_rep, e_dn = mae(cur["color"]), mae(got[0]), mae(dn)
            print("frame %s: unfiltered %.5f, reprojected %.5f, denoise_var %.5f, short %.4f" % (
                name, e_in, e_rep, e_dn, (got[1][hit] < params["min_frames"] * spp).mean()))
            if name == "a":
                assert np.isfinite(got[3][hit]).all()                                                     # (b)
                assert e_dn < e_in, (e_dn, e_in)                                                          # (c)
            else:
                assert (got[1][hit] > spp).mean() >= 0.75
                assert e_dn <= e_rep, (e_dn, e_rep)                                                       # (d)
            hist = dict(cur, color=got[0], len=got[1], mom=got[2])
