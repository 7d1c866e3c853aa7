"""pt_ctx_upsample on the GPU against tests/upsample_ref.py, the restatement of the contract in include/ptrace.h in numpy binary32.
Every comparison is of bytes, for equality, with guard floats behind both outputs.  The cases (upsample_ref.CASES, frame <- low
resolution) are the smallest that reach every path: one pixel, no integer ratio (7x5 <- 3x2), two workgroups with a one-lane tail
and taps off both row edges (257x3 <- 129x2), 33x25 <- 16x12, a low resolution LARGER than the frame (16x12 <- 33x25) and equal
sizes.  upsample_ref.LARGE holds the shapes at the limits: axes of 2^14, the largest numerators of the three divisions, and the
documented 1024x768 <- 512x384 in the four template instances.  That the synthetic inputs of both tuples reach every path is
tests/test_upsample_abi.py's test_synthetic_inputs_reach_every_path."""
import ctypes as C

import pytest

import gpudev
import ptlib
import upsample_ref as ref
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtConfig, PtUpsampleParams
from upsample_ref import CASES, I32, PARAMS

pytestmark = pytest.mark.gpu

GUARD = 64  # floats behind each output
MAXPIX = 48 * 32
NAMES = ("lcolor", "ldepth", "loid", "lnormal", "lalbedo", "depth", "oid", "normal", "albedo", "out", "weight")
FLOATS = dict(lcolor=3, ldepth=1, loid=1, lnormal=3, lalbedo=3, depth=1, oid=1, normal=3, albedo=3, out=3, weight=1)


class Dev(gpudev.Device):
    """one context and the eleven planes of a call, the two outputs with guard floats behind whatever a call writes"""

    def __init__(self, L, max_pix=MAXPIX):
        super().__init__(L)
        for name in NAMES:
            self.alloc((max_pix * FLOATS[name] + GUARD) * 4, name)

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
        self.fill_guarded("out", n * 3, GUARD, -3.0)
        self.fill_guarded("weight", n, GUARD, -3.0)
        p = PtUpsampleParams(params["depth_tol"], params["normal_min"], 0)
        P = self.p
        rc = self.L.pt_ctx_upsample(self.ctx, W, H, w, h, None if null_params else C.byref(p), P["lcolor"], P["ldepth"], P["loid"],
                                    P["lnormal"] if normal[1] else None, P["lalbedo"] if albedo[1] else None, P["depth"], P["oid"],
                                    P["normal"] if normal[0] else None, P["albedo"] if albedo[0] else None, P["out"],
                                    P["weight"] if weight else None, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.read_guarded("out", n * 3, GUARD, -3.0, "the colour output").reshape(n, 3)
        if not weight:  # the whole plane is guard
            self.read_guarded("weight", 0, n + GUARD, -3.0, "the weight plane (d_out_weight was NULL)")
            return got, None
        return got, self.read_guarded("weight", n, GUARD, -3.0, "the weight output")


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


@pytest.fixture(scope="module")
def inputs():
    """the synthetic planes of every case, made once and left unchanged"""
    return {c: ref.synthetic(*c) for c in CASES}


def same_bytes(got, exp, what):
    for name, a, b in (("colour", got[0], exp[0]), ("weight", got[1], exp[1])):
        if a is not None:
            gpudev.same_bytes(a, b, "%s %s" % (what, name))


BIG = (33, 25, 16, 12)


# --------------------------------------------------------------------------------------------------- synthetic frames
@pytest.mark.parametrize("case", CASES, ids=["%dx%d<-%dx%d" % c for c in CASES])
def test_is_the_restatement(dev, inputs, case):
    hi, lo = inputs[case]
    dev.put(hi, lo)
    same_bytes(dev.upsample(*case), ref.want(*case, hi, lo), case)


# ------------------------------------------------------------------------------------- axis limits and full-size frames
# upsample_ref.LARGE says which constant each shape crosses.  The premises are asserted here from csrc/pt_upsample.h's numbers.
MAX_SIZE, DIV_BOUND = ref.MAX_SIZE, 1 << 30  # kUpsampleMaxSize; upsample_div is proved for numerators below 2^30
FRAME = (1024, 768, 512, 384)


@pytest.fixture(scope="module")
def bigdev(L):
    with Dev(L, max(max(c[0] * c[1], c[2] * c[3]) for c in ref.LARGE)) as d:
        yield d


_large = {}


def large_inputs(case):
    """the synthetic planes of a LARGE case, made once and left unchanged"""
    if case not in _large:
        _large[case] = ref.synthetic(*case)
    return _large[case]


def numerators(W, H, w, h):
    """the largest numerator each of the three divisions of a pixel sees: idx / W, ax / 2W, ar / 2H"""
    return W * H - 1, (2 * (W - 1) + 1) * w + W, (2 * (H - 1) + 1) * h + H


@pytest.mark.parametrize("case", ref.LARGE[:-1], ids=["%dx%d<-%dx%d" % c for c in ref.LARGE[:-1]])
def test_axis_limits_are_the_restatement(bigdev, case):
    W, H, w, h = case
    assert MAX_SIZE in case and max(case) <= MAX_SIZE
    assert max(numerators(*case)) > 1 << 10 and max(numerators(*case)) < DIV_BOUND  # above what the small cases reach, within the proof
    if case == (16384, 2, 16384, 3):
        assert numerators(*case)[1] == 1 << 29  # (2x + 1) * w + W at its bound exactly
    if case == (16384, 16, 16384, 16):
        assert numerators(*case)[0] == (1 << 18) - 1 and W == MAX_SIZE  # idx / W with W at the limit
    hi, lo = large_inputs(case)
    bigdev.put(hi, lo)
    same_bytes(bigdev.upsample(*case), ref.want(*case, hi, lo), case)


@pytest.mark.parametrize("normal", [True, False], ids=["normals", "no-normals"])
@pytest.mark.parametrize("albedo", [True, False], ids=["albedos", "no-albedos"])
def test_full_frame_in_every_instance(bigdev, normal, albedo):
    """1024x768 <- 512x384 (3072 workgroups of 256; numerators up to 786 431, 1 049 088 and 590 208) through each of k_upsample's
    four template instances, the whole frame against the restatement"""
    assert FRAME == ref.LARGE[-1] and -(-FRAME[0] * FRAME[1] // 256) == 3072
    assert numerators(*FRAME) == (786431, 1049088, 590208)
    hi, lo = large_inputs(FRAME)
    bigdev.put(hi, lo)
    kw = dict(normal=(normal, normal), albedo=(albedo, albedo))
    got = bigdev.upsample(*FRAME, **kw)
    same_bytes(got, ref.want(*FRAME, hi, lo, **kw), (FRAME, kw))
    assert not (got[0] == -3.0).any() and not (got[1] == -3.0).any()  # no pixel still holds the fill pattern


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
    with dev.stream() as st:
        same_bytes(dev.upsample(*BIG, stream=st), exp, "stream")
        same_bytes(dev.upsample(*BIG), exp, "again")


# ---------------------------------------------------------------------------------------------------- no state touched
def test_leaves_the_context_alone(L, inputs):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    W, H, w, h = BIG
    with Dev(L, W * H) as d:
        d_frame = d.alloc(W * H * 12)
        d.set_scene(sc)
        before, _ = d.render(gpudev.config(W, H, 4, seed=3), d_frame)
        hi, lo = inputs[BIG]
        d.put(hi, lo)
        same_bytes(d.upsample(*BIG), ref.want(*BIG, hi, lo), "with a scene")
        for name, src, key in (("depth", hi, "depth"), ("normal", hi, "normal"), ("albedo", hi, "albedo"), ("lcolor", lo, "color"),
                               ("ldepth", lo, "depth"), ("lnormal", lo, "normal"), ("lalbedo", lo, "albedo")):
            assert d.download(name, src[key].size).tobytes() == src[key].tobytes(), name  # the inputs are read only
        for name, src in (("oid", hi), ("loid", lo)):
            assert d.download(name, src["oid"].size, I32).tobytes() == src["oid"].tobytes(), name
        after, _ = d.render(gpudev.config(W, H, 4, seed=3), d_frame)
        assert after.tobytes() == before.tobytes()


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_cornell(L):
    """pt_ctx_render at 24x16 @ 4 spp, pt_ctx_render_aov at 24x16 and at 48x32, then pt_ctx_upsample with the defaults: the result
    is the restatement's on the downloaded planes, bit for bit.  The planes are a picture: most hit pixels find a tap."""
    (w, h), (W, H), spp = (24, 16), (48, 32), 4
    n, nl = W * H, w * h
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    with Dev(L, n) as d:
        d.set_scene(sc)
        d.render(gpudev.config(w, h, spp, seed=11), "lcolor")
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
