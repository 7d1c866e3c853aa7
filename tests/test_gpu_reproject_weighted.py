"""pt_ctx_reproject_var_weighted and pt_ctx_spp_plane on the GPU.  Every comparison is of bytes, for equality, and every output
has guard words behind it.
- A constant plane against pt_ctx_reproject_var_moved with that weight, and a NULL plane against the same call: the contract's
  consequence and its delegation.
- A mixed plane against tests/reproject_weighted_ref.py, the restatement of the contract in numpy binary32.
The frames: 1x1; 33x9, one past a tile of kernel B (32 x 8) both ways; 70x21, three tiles by three with tiles that have neighbours
on every side; 37x19, 703 pixels - not a multiple of the sixteen a lane of k_spp_plane takes.  The planes are
tests/test_gpu_reproject_moved.py's: history lengths laid out by kernel B's tiles (all long, all short, mixed), object ids 0..5
against a table of four records."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gpudev
import ptlib
import reproject_ref as ref
import reproject_var_ref as rv
import reproject_weighted_ref as wref
import test_gpu_reproject_moved as mbase
import test_gpu_reproject_var as vbase
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtAdaptiveParams, PtAdaptiveStats, PtConfig, PtReprojectVarParams, PtStats
from reproject_ref import F32, I32

pytestmark = pytest.mark.gpu

U32 = np.uint32
GUARD = vbase.GUARD
SIZES = ((1, 1), (33, 9), (70, 21), (37, 19))
IDS = ["%dx%d" % s for s in SIZES]
CUR = vbase.CUR
CAMERAS = {"identical": mbase.CAMERAS["identical"], "translated": mbase.CAMERAS["translated"]}
PARAMS = vbase.PARAMS   # weight 4, max_history 64, min_frames 4, radius 3
MOTION = mbase.MOTION
COUNTS = np.array([0, 1, 2, 4, 8, 16], dtype=U32)
SENTINEL = 0xDEADBEEF


class Dev(vbase.Dev):
    """tests/test_gpu_reproject_var.py's planes and guards, a plane of counts and a mask, and one method for the three calls"""

    def __init__(self, L, max_pix=vbase.MAXPIX):
        super().__init__(L, max_pix)
        self.alloc((max_pix + GUARD) * 4, "spp")
        self.alloc(max_pix + 64, "mask")

    def call(self, w, h, cam, hist_cam=None, spp=None, motion=None, normal=True, in_place=False, stream=None, params=PARAMS,
             weighted=True):
        """pt_ctx_reproject_var_weighted (spp: a host plane, uploaded; None: a NULL plane) or, weighted=False,
        pt_ctx_reproject_var_moved; hist_cam None: the first-frame form.  The four outputs, their guards checked."""
        n = w * h
        self._guards(n, in_place)
        p = PtReprojectVarParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"],
                                 params["min_frames"], params["radius"], 0)
        a = ref.pt_camera(cam)
        b = ref.pt_camera(hist_cam) if hist_cam is not None else None
        P = self.p
        hist = [P["hcolor"], P["hlen"], P["hmom"], P["hdepth"], P["hoid"]] if b is not None else [None] * 5
        t = mbase.mref.table(motion) if motion else None
        head = [self.ctx, w, h, C.byref(p), C.byref(a), P["color"], P["depth"], P["oid"], P["normal"] if normal else None]
        tail = [C.byref(b) if b is not None else None, *hist, P["hnormal"] if normal and b is not None else None,
                P["color" if in_place else "out"], P["len"], P["mom"], P["err"], t, len(motion) if motion else 0, stream]
        if weighted:
            if spp is not None:
                self.upload("spp", np.ascontiguousarray(spp, dtype=U32))
            rc = self.L.pt_ctx_reproject_var_weighted(*head, P["spp"] if spp is not None else None, *tail)
        else:
            rc = self.L.pt_ctx_reproject_var_moved(*head, *tail)
        assert rc == 0, (rc, self.L.pt_last_error())
        return self._collect(n, in_place)


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


def hist_kw(hist_cam, hist, normal=True):
    return dict(hist_cam=hist_cam, hist_color=hist["color"], hist_len=hist["len"], hist_moments=hist["mom"], hist_depth=hist["depth"],
                hist_object_id=hist["oid"], hist_normal=hist["normal"] if normal else None)


def want(w, h, cam, cur, spp, hist_cam=None, hist=None, motion=(), normal=True, params=PARAMS):
    kw = hist_kw(hist_cam, hist, normal) if hist is not None else {}
    return wref.reproject_var_weighted(w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"] if normal else None, spp=spp,
                                       motion=motion, **kw, **params)


# ---------------------------------------------------------------------------------- the consequence and the delegation
@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("weight", [1, 4])
def test_a_constant_plane_is_the_moved_call(dev, size, weight):
    """all four outputs, bit for bit: the first frame; across a camera move and under a still camera, with and without normals,
    with and without a non-IDENTITY table, out of place and in place.  The plane says `weight`; params.weight of the weighted
    call says something else, which no pixel with a count reads."""
    w, h = size
    cur, hist = mbase.synthetic(w, h)
    plane = np.full(w * h, weight, dtype=U32)
    uniform, other = dict(PARAMS, weight=weight), dict(PARAMS, weight=9)
    dev.put(cur, hist)
    vbase.same_bytes(dev.call(w, h, CUR, spp=plane, params=other), dev.call(w, h, CUR, params=uniform, weighted=False), "first frame")
    blended = 0
    for camera, (cam, hist_cam) in CAMERAS.items():
        for normal in (True, False):
            for motion in (None, MOTION):
                for in_place in (False, True):
                    dev.put(cur, hist)
                    exp = dev.call(w, h, cam, hist_cam, motion=motion, normal=normal, in_place=in_place, params=uniform, weighted=False)
                    dev.put(cur, hist)
                    got = dev.call(w, h, cam, hist_cam, spp=plane, motion=motion, normal=normal, in_place=in_place, params=other)
                    vbase.same_bytes(got, exp, (camera, normal, bool(motion), in_place))
                    blended += int((exp[1] > weight).sum())
    assert blended > 0


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_null_plane_is_the_moved_call(dev, size):
    w, h = size
    cur, hist = mbase.synthetic(w, h)
    for camera, (cam, hist_cam) in CAMERAS.items():
        for motion in (None, MOTION):
            dev.put(cur, hist)
            exp = dev.call(w, h, cam, hist_cam, motion=motion, weighted=False)
            vbase.same_bytes(dev.call(w, h, cam, hist_cam, spp=None, motion=motion), exp, (camera, bool(motion)))
            vbase.same_bytes(exp, mbase.want_var(w, h, camera, True, MOTION) if motion else
                             vbase.want(w, h, cam, cur, hist_cam, hist), "the moved call is its restatement")
    dev.put(cur, hist)
    vbase.same_bytes(dev.call(w, h, CUR, spp=None), dev.call(w, h, CUR, weighted=False), "first frame")


# ------------------------------------------------------------------------------------------------- the Python methods
def test_the_python_methods_are_the_direct_calls(dev):
    """The package's five Context.reproject* methods against the ctypes calls of these files, every output byte for byte: a 7x5
    frame with normals, a history seen from another camera, a table of two records of which one moves, and a plane that holds
    0, 2 and 8."""
    pkg = importlib.import_module("path-tracer-rust_amd")
    w, h = 7, 5
    n = w * h
    cur, hist = mbase.synthetic(w, h)
    cam, hist_cam = CAMERAS["translated"]
    motion = (MOTION[1], MOTION[0])  # object 0 translated, object 1 where it was
    plane = np.array([0, 2, 8], dtype=U32)[np.arange(n) % 3]
    P = {k: v.value for k, v in dev.p.items()}
    frame = (w, h, cam, P["color"], P["depth"], P["oid"])
    kw = dict(PARAMS, normal=P["normal"], history=dict(cam=hist_cam, color=P["hcolor"], len=P["hlen"], moments=P["hmom"],
                                                       depth=P["hdepth"], object_id=P["hoid"], normal=P["hnormal"]))
    plain_kw = {k: v for k, v in kw.items() if k not in ("min_frames", "radius")}

    def var_form(method, *more, **extra):
        dev.put(cur, hist)
        dev._guards(n, False)
        method(*frame, P["out"], P["len"], P["mom"], P["err"], *more, **extra, **kw)
        return dev._collect(n, False)

    def plain_form(method, *more):
        dev.put(cur, hist)
        dev.fill_guarded("out", n * 3, GUARD, -3.0)
        dev.fill_guarded("len", n, GUARD, -3.0)
        method(*frame, P["out"], P["len"], *more, **plain_kw)
        return dev.read_guarded("out", n * 3, GUARD, -3.0, "the colour output").reshape(n, 3), dev.read_guarded("len", n, GUARD, -3.0, "len")

    ctx = pkg.Context()
    try:
        dev.upload("spp", plane)
        got = var_form(ctx.reproject_var_weighted, spp=P["spp"], motion=motion)
        dev.put(cur, hist)
        exp = dev.call(w, h, cam, hist_cam, spp=plane, motion=motion)
        vbase.same_bytes(got, exp, "reproject_var_weighted")
        assert ((plane == 0) & (exp[1] > 0)).any() and (exp[1] > plane).any()  # history kept as it is, and history blended
        got = var_form(ctx.reproject_var_moved, motion)
        dev.put(cur, hist)
        moved = dev.call(w, h, cam, hist_cam, motion=motion, weighted=False)
        vbase.same_bytes(got, moved, "reproject_var_moved")
        got = var_form(ctx.reproject_var)
        dev.put(cur, hist)
        still = dev.reproject_var(w, h, cam, hist_cam)
        vbase.same_bytes(got, still, "reproject_var")
        assert moved[0].tobytes() != still[0].tobytes()  # the one record that moves was read
        got = plain_form(ctx.reproject_moved, motion)
        dev.put(cur, hist)
        mbase.same2(got, mbase.Dev.reproject_moved(dev, w, h, cam, hist_cam, motion), "reproject_moved")
        got = plain_form(ctx.reproject)
        dev.put(cur, hist)
        mbase.same2(got, dev.reproject(w, h, cam, hist_cam), "reproject")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------ a mixed plane
def mixed(w, h, layout):
    """(cur, hist, plane): the planes above and counts drawn from COUNTS per pixel or per 4x4 tile, with the cases the contract
    names put where the layout of the history reaches them (vbase.tile_class: 1 all long, 2 no history, 0 mixed)."""
    cur, hist = (dict((k, v.copy()) for k, v in f.items()) for f in mbase.synthetic(w, h))
    rng = np.random.default_rng(w * 7 + h + (layout == "tile"))
    n = w * h
    x, r = np.arange(n) % w, np.arange(n) // w
    if layout == "pixel":
        plane = COUNTS[rng.integers(0, len(COUNTS), n)]
    else:
        tiles = COUNTS[rng.integers(0, len(COUNTS), ((h + 3) // 4) * ((w + 3) // 4))]
        plane = tiles[(r // 4) * ((w + 3) // 4) + x // 4]
    plane = plane.astype(U32)
    if w > 32:
        # a short pixel in the last column of kernel B's first tile and its neighbour across the tile's edge: one surface, no
        # history (so both end short), counts 4 and 8
        for q, c in ((31, 4), (32, 8)):
            cur["oid"][q], cur["depth"][q], hist["len"][q], plane[q] = 2, F32(6.0), F32(0.0), c
    # a pixel without samples holds a NaN: its colour is not data
    bad = np.flatnonzero(plane == 0)
    cur["color"][bad, bad % 3] = np.nan
    return cur, hist, plane


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("layout", ["pixel", "tile"])
@pytest.mark.parametrize("radius", [1, 3])
def test_a_mixed_plane_is_the_restatement(dev, size, layout, radius):
    w, h = size
    n = w * h
    cur, hist, plane = mixed(w, h, layout)
    seen = dict(kept_long=0, kept_short=0, bare=0, over_cap=0)
    # (max_history 12: the counts 16 lie above the cap, and a pixel without samples is cut to it)
    for params in (dict(PARAMS, radius=radius), dict(PARAMS, radius=radius, max_history=12.0, min_frames=2)):
        for camera, (cam, hist_cam) in CAMERAS.items():
            for motion in ((), MOTION):
                dev.put(cur, hist)
                got = dev.call(w, h, cam, hist_cam, spp=plane, motion=motion, params=params)
                exp = want(w, h, cam, cur, plane, hist_cam, hist, motion=motion, params=params)
                vbase.same_bytes(got, exp, (camera, bool(motion), params["max_history"]))
                out, ln, mom, e = exp
                empty = plane == 0
                # a pixel without samples: the history's bits or, without one, the stored colour; never the NaN blended in
                kept = empty & (ln > 0)
                assert np.isfinite(out[kept]).all() and np.isfinite(mom[kept]).all()
                assert out[empty & ~kept].tobytes() == cur["color"][empty & ~kept].tobytes() and (e[empty & ~kept] == np.inf).all()
                seen["kept_long"] += int((kept & np.isfinite(e)).sum())
                seen["kept_short"] += int((kept & (e == np.inf)).sum())
                seen["bare"] += int((empty & ~kept).sum())
                seen["over_cap"] += int(((plane > params["max_history"]) & (ln == plane)).sum())
                if w > 32 and camera == "identical" and not motion:
                    # the staged halo of the counts: with the neighbour's count its own, pixel 31 would have taken it
                    s = rv.s_of(np.nan_to_num(cur["color"]))
                    _, with_counts = wref.spatial(w, h, s, cur["oid"], cur["depth"], plane, radius, params["depth_tol"])
                    _, without = rv.spatial(w, h, s, cur["oid"], cur["depth"], radius, params["depth_tol"])
                    assert ln[31] == 4 and ln[32] == 8 and with_counts[31] < without[31]
    print(size, layout, radius, seen)
    if n > 1:
        assert all(seen.values()), seen


@pytest.mark.parametrize("size", SIZES[1:], ids=IDS[1:])
def test_the_frame_after_a_pixel_without_samples_or_history(dev, size):
    """two frames under a still camera, the first frame's outputs the second's history: a pixel that had neither samples nor
    history carries len 0, and the tap that finds it is skipped (hist_len > 0 does not hold)"""
    w, h = size
    n = w * h
    cur, hist, plane = mixed(w, h, "pixel")
    cam = CUR
    dev.put(cur, hist)
    a = dev.call(w, h, cam, cam, spp=plane)
    ea = want(w, h, cam, cur, plane, cam, hist)
    vbase.same_bytes(a, ea, "frame 1")
    bare = (plane == 0) & (ea[1] == 0)
    assert bare.any()
    nxt = dict(cur, color=np.random.default_rng(3).random((n, 3)).astype(F32))
    plane2 = np.where(bare & (np.arange(n) % 2 == 0), U32(0), np.roll(plane, 1)).astype(U32)
    h2 = dict(color=a[0], len=a[1], mom=a[2], depth=cur["depth"], oid=cur["oid"], normal=cur["normal"])
    dev.put(nxt, h2)
    b = dev.call(w, h, cam, cam, spp=plane2)
    eb = want(w, h, cam, nxt, plane2, cam, h2)
    vbase.same_bytes(b, eb, "frame 2")
    again = bare & (plane2 == 0)
    assert again.any() and (eb[1][again] == 0).all() and eb[0][again].tobytes() == nxt["color"][again].tobytes()
    fresh = bare & (plane2 > 0) & (cur["oid"] >= 0)
    assert fresh.any() and (eb[1][fresh] == plane2[fresh]).all()  # step 1: the length is the pixel's own count


# ------------------------------------------------------------------------------------------- the adaptive plane, end to end
def test_the_adaptive_plane_end_to_end(L):
    """pt_ctx_render_adaptive on cornell at 64x48 with a cap of 64: its frame and its d_spp fed straight in, for two frames of
    the orbit, against the restatement on the downloaded buffers"""
    w, h, cap = 64, 48, 64
    n = w * h
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    cam0 = ref.cam_dict(sc.cam)
    params = dict(rv.defaults(L), weight=8)
    d = Dev(L, n)
    try:
        def frame(cam, seed):
            d.set_scene(sc, ref.pt_camera(cam))
            par, st, ast = PtAdaptiveParams(0.16, 4, 0), PtStats(), PtAdaptiveStats()
            cfg = gpudev.config(w, h, cap, backend=1, seed=seed)
            rc = L.pt_ctx_render_adaptive(d.ctx, C.byref(cfg), C.byref(par), d.p["color"], d.p["spp"], d.p["dn"], None, None, None, None,
                                          C.byref(st), C.byref(ast))
            assert rc == 0, L.pt_last_error()
            aov = PtConfig(w, h, 8, 0, seed, 0, 0, 0, 0)
            assert L.pt_ctx_render_aov(d.ctx, C.byref(aov), None, d.p["normal"], d.p["depth"], d.p["oid"], None) == 0, L.pt_last_error()
            return dict(color=d.download("color", n * 3).reshape(n, 3), depth=d.download("depth", n), oid=d.download("oid", n, I32),
                        normal=d.download("normal", n * 3).reshape(n, 3)), d.download("spp", n, U32)

        def run(cam, hist_cam):
            # (the plane is on the device already: pt_ctx_render_adaptive wrote it)
            d._guards(n, False)
            p = PtReprojectVarParams(params["weight"], params["max_history"], params["depth_tol"], params["normal_min"],
                                     params["min_frames"], params["radius"], 0)
            a, b = ref.pt_camera(cam), ref.pt_camera(hist_cam) if hist_cam else None
            P = d.p
            hist = [P["hcolor"], P["hlen"], P["hmom"], P["hdepth"], P["hoid"], P["hnormal"]] if b else [None] * 6
            rc = L.pt_ctx_reproject_var_weighted(d.ctx, w, h, C.byref(p), C.byref(a), P["color"], P["depth"], P["oid"], P["normal"],
                                                 P["spp"], C.byref(b) if b else None, *hist, P["out"], P["len"], P["mom"], P["err"],
                                                 None, 0, None)
            assert rc == 0, L.pt_last_error()
            return d._collect(n, False)

        fa, spp_a = frame(cam0, 21)
        counts = dict(zip(*[v.tolist() for v in np.unique(spp_a, return_counts=True)]))
        print("frame A, pixels by count:", counts)
        assert len(counts) >= 2 and spp_a.max() <= cap and spp_a.min() >= 1
        a = run(cam0, None)
        vbase.same_bytes(a, want(w, h, cam0, fa, spp_a, params=params), "frame A")
        assert a[1].tobytes() == spp_a.astype(F32).tobytes()
        cam1 = ref.orbit(cam0, ref.ORBIT_DEGREES)
        fb, spp_b = frame(cam1, 22)
        ha = dict(color=a[0], len=a[1], mom=a[2], depth=fa["depth"], oid=fa["oid"], normal=fa["normal"])
        for name, key in (("hcolor", "color"), ("hlen", "len"), ("hmom", "mom"), ("hdepth", "depth"), ("hoid", "oid"), ("hnormal", "normal")):
            d.upload(name, ha[key])
        b = run(cam1, cam0)
        vbase.same_bytes(b, want(w, h, cam1, fb, spp_b, cam0, ha, params=params), "frame B")
        # most pixels found their history (a pixel at the cap of 64 = max_history ends with 64 samples either way)
        low = spp_b < params["max_history"]
        assert low.any() and (b[1][low] > spp_b[low]).mean() > 0.5
    finally:
        d.close()


# --------------------------------------------------------------------------------------------------- pt_ctx_spp_plane
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_spp_plane_is_numpy(dev, size):
    w, h = size
    n = w * h
    mask = (np.random.default_rng(n).integers(0, 4, n) == 0).astype(np.uint8) * np.random.default_rng(n + 1).integers(1, 256, n).astype(np.uint8)

    def run(base, masked, m, offset=0, stream=None):
        dev.fill_guarded("spp", n, GUARD, SENTINEL, dtype=U32)
        if m is not None:
            dev.upload("mask", m, offset)
        rc = dev.L.pt_ctx_spp_plane(dev.ctx, w, h, base, dev._at("mask", offset) if m is not None else None, masked, dev.p["spp"], stream)
        assert rc == 0, (rc, dev.L.pt_last_error())
        got = dev.read_guarded("spp", n, GUARD, SENTINEL, "the plane", dtype=U32)
        gpudev.same_bytes(got, wref.spp_plane(n, base, m, masked), (base, masked, offset))
        return got

    assert (run(8, 32, None) == 8).all()
    got = run(8, 32, mask)
    assert n == 1 or (got == 32).any()
    run(8, 32, mask, offset=1)       # the mask pointer one byte into its allocation: the byte path
    run(2, 0, mask, offset=16)       # sixteen bytes in: the vector path again; a boost of 0 marks "not traced"
    assert (run(5, 5, mask) == 5).all()
    with dev.stream() as st:
        run(1, 0xFFFFFFFF, mask, stream=st)


# --------------------------------------------------------------------------------------------------------------- state
def test_leaves_the_held_frames_and_the_other_scratch_alone(L):
    """a held pt_ctx_accumulate frame, a held adaptive frame and pt_ctx_denoise_var's scratch in the context: what they give is
    the same before and after the two calls, the scene's tables hash as before, and the accumulate frame continued equals a
    fresh render"""
    w, h = 36, 12
    n = w * h
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    cur, hist, plane = mixed(w, h, "pixel")
    d, fresh = Dev(L, n), gpudev.Device(L, sc)
    try:
        d.set_scene(sc)
        d_out, d_spp, d_err = d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 4)
        st = PtStats()

        def held():
            lo, hi = C.c_uint32(), C.c_uint32()
            assert L.pt_ctx_accum_info(d.ctx, C.byref(gpudev.config(w, h, 1, seed=5)), C.byref(lo), C.byref(hi)) == 0, L.pt_last_error()
            assert L.pt_ctx_adaptive_resolve(d.ctx, C.byref(gpudev.config(w, h, 1, backend=1, seed=6)), d_out, d_spp, d_err, None) == 0
            hashes = (C.c_uint64 * 14)()
            assert L.pt_ctx_table_hashes(d.ctx, hashes) == 0
            return ((lo.value, hi.value), d.download(d_out, n * 3).tobytes(), d.download(d_spp, n, U32).tobytes(),
                    d.download(d_err, n).tobytes(), list(hashes))

        def filtered():
            p = ptlib.PtDenoiseVarParams(2, 2.0, 0.0, 1)
            assert L.pt_ctx_denoise_var(d.ctx, w, h, C.byref(p), d.p["hcolor"], d.p["hlen"], None, d.p["hnormal"], d.p["hdepth"],
                                        d.p["dn"], None) == 0, L.pt_last_error()
            return d.download("dn", n * 3).tobytes()

        assert L.pt_ctx_accumulate(d.ctx, C.byref(gpudev.config(w, h, 4, seed=5)), d_out, None, None, None, None, C.byref(st)) == 0
        par, ast = PtAdaptiveParams(0.16, 4, 0), PtAdaptiveStats()
        assert L.pt_ctx_accumulate_adaptive(d.ctx, C.byref(gpudev.config(w, h, 16, backend=1, seed=6)), C.byref(par), d_out, d_spp, d_err,
                                            None, None, None, None, C.byref(st), C.byref(ast)) == 0, L.pt_last_error()
        d.put(cur, hist)
        before = (held(), filtered())
        assert before[0][0] == (4, 4)
        got = d.call(w, h, CUR, CUR, spp=plane, motion=MOTION)
        vbase.same_bytes(got, want(w, h, CUR, cur, plane, CUR, hist, motion=MOTION), "with held frames")
        assert L.pt_ctx_spp_plane(d.ctx, w, h, 4, None, 16, d.p["spp"], None) == 0, L.pt_last_error()
        assert (held(), filtered()) == before
        assert L.pt_ctx_accumulate(d.ctx, C.byref(gpudev.config(w, h, 8, seed=5)), d_out, None, None, None, None, C.byref(st)) == 0
        assert st.samples == n * 4  # only the rest was traced
        assert d.download(d_out, n * 3).tobytes() == fresh.render(gpudev.config(w, h, 8, seed=5), fresh.alloc(n * 12))[0].tobytes()
    finally:
        d.close()
        fresh.close()
