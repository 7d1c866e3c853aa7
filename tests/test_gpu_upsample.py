"""pt_ctx_upsample on the GPU against tests/upsample_ref.py, the restatement of the contract in include/ptrace.h in numpy binary32.
Every comparison is of bytes, for equality, with guard floats behind both outputs.  The cases (upsample_ref.CASES, frame <- low
resolution) are the smallest that reach every path: one pixel, no integer ratio (7x5 <- 3x2), two workgroups with a one-lane tail
and taps off both row edges (257x3 <- 129x2), 33x25 <- 16x12, a low resolution LARGER than the frame (16x12 <- 33x25) and equal
sizes.  That their synthetic inputs reach every path is tests/test_upsample_abi.py's test_synthetic_inputs_reach_every_path."""
import ctypes as C

import numpy as np
import pytest

import ptlib
import upsample_ref as ref
from ptlib import PtConfig, PtStats, PtUpsampleParams
from upsample_ref import CASES, F32, I32, PARAMS

pytestmark = pytest.mark.gpu

GUARD = 64  # floats behind each output
MAXPIX = 48 * 32
NAMES = ("lcolor", "ldepth", "loid", "lnormal", "lalbedo", "depth", "oid", "normal", "albedo", "out", "weight")
FLOATS = dict(lcolor=3, ldepth=1, loid=1, lnormal=3, lalbedo=3, depth=1, oid=1, normal=3, albedo=3, out=3, weight=1)


def hip_runtime():
    """the HIP runtime the product is bound to: the copy already mapped into this process that is not torch's"""
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "/libamdhip64.so" in line}
    own = sorted(p for p in paths if "/torch/" not in p)
    assert own, "libptrace_hip.so has not mapped a HIP runtime: %r" % sorted(paths)
    hip = C.CDLL(own[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


class Dev:
    """one context and the eleven planes of a call, the two outputs with guard floats behind whatever a call writes"""

    def __init__(self, L, max_pix=MAXPIX):
        self.L = L
        self.ctx = C.c_void_p()
        assert L.pt_ctx_create(0, C.byref(self.ctx)) == 0, L.pt_last_error()
        self.hip = hip_runtime()
        self.p = {}
        for name in NAMES:
            self.p[name] = C.c_void_p()
            assert L.pt_device_malloc(0, (max_pix * FLOATS[name] + GUARD) * 4, C.byref(self.p[name])) == 0, L.pt_last_error()

    def upload(self, name, host):
        host = np.ascontiguousarray(host)
        assert self.hip.hipMemcpy(self.p[name], host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0  # host to device

    def download(self, name, count, dtype=F32):
        host = np.zeros(count, dtype=dtype)
        assert self.L.pt_device_download(0, host.ctypes.data_as(C.c_void_p), self.p[name], host.nbytes) == 0
        return host

    def put(self, hi, lo):
        for name, key in (("depth", "depth"), ("oid", "oid"), ("normal", "normal"), ("albedo", "albedo")):
            self.upload(name, hi[key])
        for name, key in (("lcolor", "color"), ("ldepth", "depth"), ("loid", "oid"), ("lnormal", "normal"), ("lalbedo", "albedo")):
            self.upload(name, lo[key])

    def upsample(self, W, H, w, h, normal=(True, True), albedo=(True, True), weight=True, stream=None, params=PARAMS,
                 null_params=False):
        """the two outputs of one call, (W*H, 3) and (W*H,) (None without d_out_weight); the guards behind them are checked on
        the way.  normal / albedo: (the frame's given, the low-resolution one given)."""
        n = W * H
        self.upload("out", np.full(n * 3 + GUARD, -3.0, dtype=F32))
        self.upload("weight", np.full(n + GUARD, -3.0, dtype=F32))
        p = PtUpsampleParams(params["depth_tol"], params["normal_min"], 0)
        P = self.p
        rc = self.L.pt_ctx_upsample(self.ctx, W, H, w, h, None if null_params else C.byref(p), P["lcolor"], P["ldepth"], P["loid"],
                                    P["lnormal"] if normal[1] else None, P["lalbedo"] if albedo[1] else None, P["depth"], P["oid"],
                                    P["normal"] if normal[0] else None, P["albedo"] if albedo[0] else None, P["out"],
                                    P["weight"] if weight else None, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.download("out", n * 3 + GUARD)
        wg = self.download("weight", n + GUARD)
        assert (got[n * 3:] == -3.0).all() and (wg[n:] == -3.0).all(), "floats behind an output were written"
        if not weight:
            assert (wg == -3.0).all(), "d_out_weight was NULL, yet the plane was written"
        return got[:n * 3].reshape(n, 3), (wg[:n] if weight else None)

    def close(self):
        for p in self.p.values():
            self.L.pt_device_free(0, p)
        self.L.pt_ctx_destroy(self.ctx)


@pytest.fixture(scope="module")
def L():
    L = ptlib.product()
    assert L.pt_device_count() >= 1
    return L


@pytest.fixture(scope="module")
def dev(L):
    d = Dev(L)
    yield d
    d.close()


@pytest.fixture(scope="module")
def inputs():
    """the synthetic planes of every case, made once and left unchanged"""
    return {c: ref.synthetic(*c) for c in CASES}


def same_bytes(got, exp, what):
    for name, a, b in (("colour", got[0], exp[0]), ("weight", got[1], exp[1])):
        if a is None:
            continue
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError("%s %s: %d of %d words differ, first at %s: %r vs %r" % (
                what, name, len(bad), a.size, bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


BIG = (33, 25, 16, 12)


# --------------------------------------------------------------------------------------------------- synthetic frames
@pytest.mark.parametrize("case", CASES, ids=["%dx%d<-%dx%d" % c for c in CASES])
def test_is_the_restatement(dev, inputs, case):
    hi, lo = inputs[case]
    dev.put(hi, lo)
    same_bytes(dev.upsample(*case), ref.want(*case, hi, lo), case)


@pytest.mark.parametrize("case", [BIG, (16, 12, 33, 25)], ids=["down", "up"])
def test_optional_normals(dev, inputs, case):
    hi, lo = inputs[case]
    dev.put(hi, lo)
    both = dev.upsample(*case)
    results = []
    for normal in ((False, False), (False, True), (True, False)):
        got = dev.upsample(*case, normal=normal)
        same_bytes(got, ref.want(*case, hi, lo, normal=normal), (case, normal))
        results.append(got)
    # the normal test runs only when both are given: the three forms agree, and differ from the call with both
    assert all(r[0].tobytes() == results[0][0].tobytes() and r[1].tobytes() == results[0][1].tobytes() for r in results)
    assert both[1].tobytes() != results[0][1].tobytes()


@pytest.mark.parametrize("case", [BIG, (16, 12, 33, 25)], ids=["down", "up"])
def test_optional_albedos(dev, inputs, case):
    hi, lo = inputs[case]
    dev.put(hi, lo)
    both = dev.upsample(*case)
    results = []
    for albedo in ((False, False), (False, True), (True, False)):
        for normal in ((True, True), (False, False)):
            got = dev.upsample(*case, albedo=albedo, normal=normal)
            same_bytes(got, ref.want(*case, hi, lo, albedo=albedo, normal=normal), (case, albedo, normal))
            if normal[0]:
                results.append(got)
    # demodulation runs only when both are given: the three forms agree; the taps do not depend on it, the colour does
    assert all(r[0].tobytes() == results[0][0].tobytes() for r in results)
    assert both[0].tobytes() != results[0][0].tobytes() and both[1].tobytes() == results[0][1].tobytes()
    same_bytes(dev.upsample(*case, normal=(False, False)), ref.want(*case, hi, lo, normal=(False, False)), "albedos alone")


def test_without_the_weight_plane(dev, inputs):
    hi, lo = inputs[BIG]
    dev.put(hi, lo)
    same_bytes(dev.upsample(*BIG, weight=False), ref.want(*BIG, hi, lo), "d_out_weight NULL")


def test_defaults_stand_for_zero(L, dev, inputs):
    hi, lo = inputs[BIG]
    dev.put(hi, lo)
    d = ref.defaults(L)
    exp = ref.want(*BIG, hi, lo, params=d)
    assert exp[1].tobytes() != ref.want(*BIG, hi, lo)[1].tobytes()  # the defaults are not the tests' parameters
    same_bytes(dev.upsample(*BIG, null_params=True), exp, "NULL params")
    same_bytes(dev.upsample(*BIG, params=dict(depth_tol=0.0, normal_min=0.0)), exp, "zeros")


def test_on_a_stream(dev, inputs):
    hi, lo = inputs[BIG]
    dev.put(hi, lo)
    exp = ref.want(*BIG, hi, lo)
    st = C.c_void_p()
    assert dev.hip.hipStreamCreate(C.byref(st)) == 0
    try:
        same_bytes(dev.upsample(*BIG, stream=st), exp, "stream")
        same_bytes(dev.upsample(*BIG), exp, "again")
    finally:
        assert dev.hip.hipStreamDestroy(st) == 0


# ---------------------------------------------------------------------------------------------------- no state touched
def render(L, ctx, d_out, w, h, spp, seed):
    cfg = PtConfig(w, h, spp, 0, seed, 0, 0, 0, 0)
    st = PtStats()
    assert L.pt_ctx_render(ctx, C.byref(cfg), d_out, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()


def test_leaves_the_context_alone(L, inputs):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    W, H, w, h = BIG
    d = Dev(L, W * H)
    d_frame = C.c_void_p()
    assert L.pt_device_malloc(0, W * H * 12, C.byref(d_frame)) == 0
    try:
        assert L.pt_ctx_set_scene(d.ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0, L.pt_last_error()
        render(L, d.ctx, d_frame, W, H, 4, 3)
        before = np.zeros(W * H * 3, dtype=F32)
        assert L.pt_device_download(0, before.ctypes.data_as(C.c_void_p), d_frame, before.nbytes) == 0
        hi, lo = inputs[BIG]
        d.put(hi, lo)
        same_bytes(d.upsample(*BIG), ref.want(*BIG, hi, lo), "with a scene")
        for name, src, key in (("depth", hi, "depth"), ("normal", hi, "normal"), ("albedo", hi, "albedo"), ("lcolor", lo, "color"),
                               ("ldepth", lo, "depth"), ("lnormal", lo, "normal"), ("lalbedo", lo, "albedo")):
            assert d.download(name, src[key].size).tobytes() == src[key].tobytes(), name  # the inputs are read only
        for name, src in (("oid", hi), ("loid", lo)):
            assert d.download(name, src["oid"].size, I32).tobytes() == src["oid"].tobytes(), name
        render(L, d.ctx, d_frame, W, H, 4, 3)
        after = np.zeros(W * H * 3, dtype=F32)
        assert L.pt_device_download(0, after.ctypes.data_as(C.c_void_p), d_frame, after.nbytes) == 0
        assert after.tobytes() == before.tobytes()
    finally:
        L.pt_device_free(0, d_frame)
        d.close()


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_cornell(L):
    """pt_ctx_render at 24x16 @ 4 spp, pt_ctx_render_aov at 24x16 and at 48x32, then pt_ctx_upsample with the defaults: the result
    is the restatement's on the downloaded planes, bit for bit.  The planes are a picture: most hit pixels find a tap."""
    (w, h), (W, H), spp = (24, 16), (48, 32), 4
    n, nl = W * H, w * h
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    d = Dev(L, n)
    try:
        assert L.pt_ctx_set_scene(d.ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0, L.pt_last_error()
        render(L, d.ctx, d.p["lcolor"], w, h, spp, 11)
        cfg = PtConfig(w, h, spp, 0, 11, 0, 0, 0, 0)
        assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), d.p["lalbedo"], d.p["lnormal"], d.p["ldepth"], d.p["loid"], None) == 0, \
            L.pt_last_error()
        cfg = PtConfig(W, H, spp, 0, 12, 0, 0, 0, 0)
        assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), d.p["albedo"], d.p["normal"], d.p["depth"], d.p["oid"], None) == 0, \
            L.pt_last_error()
        lo = dict(color=d.download("lcolor", nl * 3).reshape(nl, 3), depth=d.download("ldepth", nl), oid=d.download("loid", nl, I32),
                  normal=d.download("lnormal", nl * 3).reshape(nl, 3), albedo=d.download("lalbedo", nl * 3).reshape(nl, 3))
        hi = dict(depth=d.download("depth", n), oid=d.download("oid", n, I32), normal=d.download("normal", n * 3).reshape(n, 3),
                  albedo=d.download("albedo", n * 3).reshape(n, 3))
        params = ref.defaults(L)
        got = d.upsample(W, H, w, h, null_params=True)
        same_bytes(got, ref.want(W, H, w, h, hi, lo, params=params), "cornell")
        hit = hi["oid"] >= 0
        share = float((got[1][hit] > 0).mean())
        print("hit pixels %d of %d, with a tap %.4f, colour mean %.4f" % (hit.sum(), n, share, got[0].mean()))
        assert hit.sum() > n // 2 and share >= 0.75 and got[0].mean() > 0.01
    finally:
        d.close()
