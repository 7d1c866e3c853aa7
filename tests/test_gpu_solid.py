"""pt_ctx_solid on the GPU against tests/solid_ref.py, the restatement of the contract in include/ptrace_solid.h in numpy
binary32.  Every comparison is of bits, for equality.

The kernel's units are four pixels per lane and 256 lanes per workgroup (1024 pixels), the grid is not capped, and a scalar form
takes the last npix % 4 pixels and every call with a plane that is not 16-byte aligned.  So the frames are 1x1, 3x1 (no whole
group), 5x1 (one group and a rest of one), 31x33 = 1023 (255 groups, a rest of three: two workgroups), 32x32 = 1024 (one
workgroup exactly, no rest), 41x25 = 1025 (256 groups and a rest of one in the second workgroup) and 67x33 = 2211.  Every size
runs with all planes aligned, with each plane in turn 4 and 12 bytes off, and with all of them 4 bytes off; out of place, in
place on the albedo and in place on the normals; with and without albedo; with each flag combination.  Every output carries a
guard before and behind it.

What the planes do NOT hold is a NaN or an infinity, and nothing in them makes one (depths are finite): which NaN an invalid
operation returns, and which of two NaN operands survives, IEEE 754 leaves to the implementation (x86's default NaN has the
sign bit set, the GPU's has not) - frames that make NaNs cannot be held to one restatement's bits on both.
tests/test_solid_abi.py puts them through pt_solid_pixel_host, where both sides run on one machine.  -0, denormals, zero normals and albedos above 1 are here.

The stream contract: tests/test_gpu_streams.py's trap (Case, Trap, expectation, verdict, by import) on a 67x33 frame, with the
looks table and without.  The looks table is HOST memory, read by the call itself before it returns: it has no decoy, only the
four planes have."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gpudev
import solid_ref as ref
from gpudev import L  # noqa: F401  (fixture)
from reproject_ref import cam_dict
from solid_ref import F32, HEADLIGHT, I32, REFLECT_SKY
from test_gpu_streams import D2D, FILL, Case, Trap, expectation, stop_on_a_hip_error, verdict

pytestmark = pytest.mark.gpu

GUARD = 64  # floats before and behind the output
SENTINEL = F32(-7.5)
SIZES = ((1, 1), (3, 1), (5, 1), (31, 33), (32, 32), (41, 25), (67, 33))
MAX_PIX = 67 * 33
CAM = dict(position=(0.5, 3.0, 4.0), direction=(-0.1, -0.6, -0.79), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
DIFFUSE, MIRROR, GLASS = ref.DIFFUSE, ref.SPECULAR, ref.REFRACT
# ids 0..5: plain, a mirror, a glass, a lamp, a glowing mirror, and the table's last record
LOOKS = [((0.0, 0.0, 0.0), DIFFUSE), ((0.0, 0.0, 0.0), MIRROR), ((0.0, 0.0, 0.0), GLASS), ((2.0, 1.5, 0.25), DIFFUSE),
         ((0.125, 0.0, 0.5), MIRROR), ((0.0, 0.25, 0.0), DIFFUSE)]
N_LOOKS = len(LOOKS)
PLANES = ("albedo", "normal", "depth", "oid", "out")
ALIGNED = dict.fromkeys(PLANES, 0)
OFFSETS = [ALIGNED] + [dict(ALIGNED, **{k: off}) for off in (4, 12) for k in PLANES] + [dict.fromkeys(PLANES, 4)]
SHININESS = {0: 0, HEADLIGHT: 10, REFLECT_SKY: 5, HEADLIGHT | REFLECT_SKY: 3}  # the exponent 1, 1024, 32, 8


def params_of(flags):
    return ref.params(flags=flags, light=(1.5, 4.0, 2.0), ambient=0.125, diffuse=0.75, specular=0.5, shininess_log2=SHININESS[flags],
                      background=(0.0, 0.25, 0.5), sky_top=(0.25, 0.5, 0.75), sky_bottom=(0.75, 0.75, 0.7))


class Dev(gpudev.Device):
    """one context and the planes of a call, each with room for an offset; the output with guards on both sides"""

    def __init__(self, L, max_pix=MAX_PIX):
        super().__init__(L)
        room = 16 + GUARD * 8
        self.d = {k: self.alloc(max_pix * (4 if k in ("depth", "oid") else 12) + room) for k in PLANES}

    def solid(self, w, h, p, cam, planes, looks=LOOKS, with_albedo=True, place="out", offsets=ALIGNED, stream=None):
        """the (w*h, 3) frame the call wrote, as uint32 bits.  place: "out", or the input plane the call runs in place on.
        Every plane starts GUARD floats + its offset into its allocation; the guards around the output are checked."""
        n = w * h
        base = GUARD * 4
        at = {k: base + offsets[k] for k in PLANES}
        at["out"] = at[place]
        for k in ("albedo", "normal", "depth", "oid"):
            self.upload(self.d[k], np.full(GUARD, SENTINEL, dtype=F32), offset=offsets[k])
            self.upload(self.d[k], planes[k], offset=at[k])
            self.upload(self.d[k], np.full(GUARD, SENTINEL, dtype=F32), offset=at[k] + planes[k].nbytes)
        if place == "out":
            self.upload(self.d["out"], np.full(n * 3 + 2 * GUARD, SENTINEL, dtype=F32), offset=offsets["out"])
        ptr = {k: C.c_void_p(self.d[place if k == "out" else k].value + at[k]) for k in PLANES}
        s = ref.struct(p) if p is not None else None
        c = ref.pt_camera(cam)
        arr = ref.looks_array(looks)
        rc = self.L.pt_ctx_solid(self.ctx, w, h, C.byref(s) if s is not None else None, C.byref(c), ptr["albedo"] if with_albedo else None,
                                 ptr["normal"], ptr["depth"], ptr["oid"], arr, len(looks) if looks is not None else 0, ptr["out"], stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.download(self.d[place], n * 3 + 2 * GUARD, offset=at["out"] - base)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n * 3:] == SENTINEL).all(), "d_out was written outside its %d floats" % (n * 3)
        for k in ("albedo", "normal", "depth", "oid"):  # the inputs are read only, but for the one the call runs in place on
            if k != place:
                assert self.download(self.d[k], planes[k].size, planes[k].dtype, offset=at[k]).tobytes() == planes[k].tobytes(), k
        return got[GUARD:GUARD + n * 3].reshape(n, 3).view(np.uint32)


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


def make_planes(w, h, seed):
    """random planes with what the kernel's paths need (lanes own pixels 4g .. 4g + 3)"""
    n = w * h
    rng = np.random.default_rng(seed)
    oid = rng.integers(0, N_LOOKS + 2, size=n).astype(I32)  # the table, n_looks and n_looks + 1
    oid[rng.random(n) < 0.1] = -1
    oid[rng.random(n) < 0.03] = 1 << 30  # far beyond
    oid[rng.random(n) < 0.02] = np.iinfo(I32).min
    if n >= 1023:
        oid[8:16] = -1                         # two lanes whose four pixels all miss
        oid[16:20] = (0, -1, 3, 1)             # a single miss among hits
        oid[20:24] = (N_LOOKS - 1, N_LOOKS, 1 << 30, 2)
        oid[256:512] = 4                       # a whole wave of one object: the uniform fetch of its record
        oid[512:768] = N_LOOKS + 5             # ... and of no record
        oid[n - 3:] = (1, -1, 3)[:3]           # the last pixels: the rest of the wide form where npix % 4 != 0
    depth = (0.5 + rng.random(n) * 12).astype(F32)
    depth[rng.random(n) < 0.02] = 0.0
    albedo = (rng.random((n, 3)) * 1.25).astype(F32)
    albedo[rng.random(n) < 0.1] *= F32(4.0)  # saturates the clamp
    normal = (rng.random((n, 3)) - 0.5).astype(F32)
    normal[rng.random(n) < 0.1] = 0.0
    for plane in (albedo, normal):  # -0 and denormals
        pick = rng.random((n, 3)) < 0.05
        plane.view(np.uint32)[pick] = rng.choice(np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32), size=int(pick.sum()))
    for a in (albedo, normal, depth):
        assert np.isfinite(a).all()
    return dict(albedo=albedo, normal=normal, depth=depth, oid=oid)


def assert_planes_reach_every_path(w, h, planes):
    """on the CPU, before any call: the planes hold what the kernel can go wrong on"""
    n = w * h
    oid, normal = planes["oid"], planes["normal"]
    groups = oid[:n - n % 4].reshape(-1, 4)
    assert ((groups < 0).all(axis=1)).any(), "a lane whose four pixels all miss"
    assert ((groups < 0).sum(axis=1) == 1).any(), "a lane with a single miss among hits"
    for k, what in ((1, "mirror"), (2, "glass"), (3, "emitter"), (N_LOOKS - 1, "n_looks - 1"), (N_LOOKS, "n_looks"), (1 << 30, "far beyond")):
        assert (oid == k).any(), what
    waves = oid[:n - n % 256].reshape(-1, 256)
    assert ((waves == waves[:, :1]).all(axis=1) & (waves[:, 0] >= 0) & (waves[:, 0] < N_LOOKS)).any(), "a wave of one object of the table"
    hit = oid >= 0
    assert (hit & (normal == 0).all(axis=1)).any(), "a zero normal"
    for flags in (0, HEADLIGHT):
        grey = ref.solid(w, h, dict(params_of(flags), ambient=0.0, specular=0.0, diffuse=1.0), CAM, oid, planes["depth"], normal)
        assert (hit & (grey[:, 0] == 0)).any() and (hit & (grey[:, 0] > 0)).any(), "pixels with ndl <= 0 and with ndl > 0"
        full = ref.solid(w, h, params_of(flags), CAM, oid, planes["depth"], normal, planes["albedo"], LOOKS)
        assert (hit[:, None] & (full == 1.0)).any() and (hit[:, None] & (full < 1.0) & (full > 0.0)).any(), "the clamp saturates somewhere"
    assert sorted(SHININESS.values())[0] == 0 and sorted(SHININESS.values())[-1] == 10


# ------------------------------------------------------------------------------------------------------ synthetic planes
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_every_form_at_every_size(dev, w, h):
    n = w * h
    seeds = (1,) if n >= 1023 else (1, 2, 3, 4)  # the tiny frames: several draws, so that hits, misses and both meet
    for seed in seeds:
        planes = make_planes(w, h, 1000 * n + seed)
        if n >= 1023:
            assert_planes_reach_every_path(w, h, planes)
        for flags in (0, HEADLIGHT, REFLECT_SKY, HEADLIGHT | REFLECT_SKY):
            p = params_of(flags)
            for with_albedo in (True, False):
                want = ref.solid(w, h, p, CAM, planes["oid"], planes["depth"], planes["normal"], planes["albedo"] if with_albedo else None,
                                 LOOKS).view(np.uint32)
                for offsets in OFFSETS:
                    for place in ("out", "albedo", "normal"):
                        if place == "albedo" and not with_albedo:
                            continue
                        got = dev.solid(w, h, p, CAM, planes, LOOKS, with_albedo, place, offsets)
                        gpudev.same_bytes(got, want, "%dx%d flags %d albedo %d %s %r" % (w, h, flags, with_albedo, place, offsets))
    if n < 1023:  # all four missed / none did, whatever the draws gave
        for oid in (np.full(n, -1, dtype=I32), np.full(n, 3, dtype=I32)):
            planes = dict(planes, oid=oid)
            p = params_of(HEADLIGHT | REFLECT_SKY)
            want = ref.solid(w, h, p, CAM, oid, planes["depth"], planes["normal"], planes["albedo"], LOOKS).view(np.uint32)
            for offsets in (OFFSETS[0], OFFSETS[-1]):
                gpudev.same_bytes(dev.solid(w, h, p, CAM, planes, offsets=offsets), want, "%dx%d one id %r" % (w, h, offsets))


def test_no_table_is_a_table_of_default_records(dev):
    w, h = 41, 25
    planes = make_planes(w, h, 77)
    none = [((0.0, 0.0, 0.0), DIFFUSE)] * N_LOOKS
    for flags in (HEADLIGHT, HEADLIGHT | REFLECT_SKY):
        p = params_of(flags)
        want = ref.solid(w, h, p, CAM, planes["oid"], planes["depth"], planes["normal"], planes["albedo"], None).view(np.uint32)
        for offsets in (OFFSETS[0], OFFSETS[-1]):
            a = dev.solid(w, h, p, CAM, planes, None, offsets=offsets)
            b = dev.solid(w, h, p, CAM, planes, none, offsets=offsets)
            gpudev.same_bytes(a, want, "looks NULL")
            gpudev.same_bytes(b, a, "an all-default table")
    with_table = dev.solid(w, h, params_of(HEADLIGHT | REFLECT_SKY), CAM, planes, LOOKS)
    assert with_table.tobytes() != a.tobytes()  # ... and the table matters


def test_null_params_are_the_defaults(dev):
    w, h = 41, 25
    planes = make_planes(w, h, 78)
    want = ref.solid(w, h, ref.params(), CAM, planes["oid"], planes["depth"], planes["normal"], planes["albedo"], LOOKS).view(np.uint32)
    gpudev.same_bytes(dev.solid(w, h, None, CAM, planes, LOOKS), want, "params NULL")
    gpudev.same_bytes(dev.solid(w, h, ref.from_struct(ref.struct(ref.params())), CAM, planes, LOOKS), want, "the defaults written out")


# ------------------------------------------------------------------------------------------------------- a rendered frame
def scene_looks(sc):
    return [(tuple(sc.objs[i].emission), int(sc.objs[i].reflect_type)) for i in range(sc.n_objs)]


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("sid", ["cornell", "three-spheres"])
def test_a_frame_of_render_aov(L, sid, spp):
    """the guides of pt_ctx_render_aov, the looks of the scene (pt_solid_look_of): device == restatement on the downloaded guides"""
    pkg = importlib.import_module("path-tracer-rust_amd")
    sc = gpudev.scene(sid)
    w, h = 48, 32
    n = w * h
    looks = scene_looks(sc)
    arr = pkg.solid_looks([sc.objs[i] for i in range(sc.n_objs)])
    assert [(tuple(r.emission), r.reflect_type) for r in arr] == looks
    p = ref.params(flags=HEADLIGHT | REFLECT_SKY, ambient=0.1, diffuse=0.5, specular=0.25)  # at most 0.85 without emission
    with gpudev.Device(L, sc) as d:
        d_alb, d_n, d_z, d_id, d_out = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 4), d.alloc(n * 12)
        cfg = gpudev.config(w, h, spp, seed=7)
        assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), d_alb, d_n, d_z, d_id, None) == 0, L.pt_last_error()
        alb, nrm, z, oid = d.pixels(d_alb, n), d.pixels(d_n, n), d.download(d_z, n), d.download(d_id, n, I32)
        s, c = ref.struct(p), sc.cam
        assert L.pt_ctx_solid(d.ctx, w, h, C.byref(s), C.byref(c), d_alb, d_n, d_z, d_id, arr, len(arr), d_out, None) == 0, L.pt_last_error()
        got = d.pixels(d_out, n)
        assert L.pt_ctx_solid(d.ctx, w, h, C.byref(s), C.byref(c), None, d_n, d_z, d_id, arr, len(arr), d_n, None) == 0, L.pt_last_error()
        clay = d.pixels(d_n, n)
    hit = oid >= 0
    assert np.isfinite(alb[hit]).all() and np.isfinite(nrm[hit]).all() and np.isfinite(z[hit]).all()
    z = np.where(hit, z, F32(1.0))  # a miss's depth is +inf and is not read: keep the restatement's discarded lanes free of NaNs
    cam = cam_dict(sc.cam)
    want = ref.solid(w, h, p, cam, oid, z, nrm, alb, looks)
    gpudev.same_bytes(got.view(np.uint32), want.view(np.uint32), "%s at %d spp" % (sid, spp))
    gpudev.same_bytes(clay.view(np.uint32), ref.solid(w, h, p, cam, oid, z, nrm, None, looks).view(np.uint32), "clay, in place on the normals")
    if sid == "cornell":
        kinds = {k: [i for i, (e, t) in enumerate(looks) if t == k and max(e) == 0] for k in (MIRROR, GLASS)}
        lamps = [i for i, (e, _) in enumerate(looks) if max(e) > 0]
        assert kinds[MIRROR] and kinds[GLASS] and lamps
        for ids, what in ((kinds[MIRROR], "mirror"), (kinds[GLASS], "glass"), (lamps, "lamp")):
            assert np.isin(oid, ids).any(), "no pixel of the %s" % what
        lamp = np.isin(oid, lamps)
        ceiling = F32(0.999) * (F32(p["specular"]) + F32(p["ambient"]) + F32(p["diffuse"]))  # a 0.999 sphere fully lit, no emission
        assert ceiling < 1 and (got[lamp] > ceiling).all()
        unlit = ref.solid(w, h, p, cam, oid, z, nrm, alb, None)
        assert (unlit[lamp] < 1.0).all()  # ... which the guides alone do not give
    else:
        assert (~hit).any() and hit.any()
        assert (got[~hit] == np.array(p["background"], dtype=F32)).all()


# ------------------------------------------------------------------------------------------------------------ the stream
PW, PH = 67, 33


@pytest.fixture(scope="module")
def streams():
    """two non-blocking streams created one after the other, and a blocking one"""
    with gpudev.stream(nonblocking=True) as a, gpudev.stream(nonblocking=True) as b, gpudev.stream() as c:
        yield {"nonblocking-1": a, "nonblocking-2": b, "blocking": c}


def solid_case(dev, with_looks):
    """the four planes behind the gate (decoys: the same planes, every pixel moved), the looks table in host memory.  A light at
    a fixed position: under a headlight ld is -d whatever the depth, and the depth plane's decoy would change nothing."""
    n = PW * PH
    planes = make_planes(PW, PH, 6733)
    p = ref.struct(params_of(REFLECT_SKY))
    cam = ref.pt_camera(CAM)
    arr = ref.looks_array(LOOKS) if with_looks else None

    def call(P, st):
        return dev.L.pt_ctx_solid(dev.ctx, PW, PH, C.byref(p), C.byref(cam), P["albedo"], P["normal"], P["depth"], P["oid"], arr,
                                  N_LOOKS if with_looks else 0, P["out"], st), {}
    inputs = {k: (planes[k], np.roll(planes[k], 101 + 7 * i, axis=0)) for i, k in enumerate(("albedo", "normal", "depth", "oid"))}
    return Case(dev, call, inputs=inputs, outputs={"out": (n * 3, F32)})


@pytest.mark.parametrize("stream", ["nonblocking-1", "nonblocking-2", "blocking"])
@pytest.mark.parametrize("with_looks", [True, False], ids=["looks", "no-looks"])
def test_the_call_is_ordered_on_the_callers_stream(dev, streams, with_looks, stream):
    A = streams[stream]
    trap = Trap(solid_case(dev, with_looks))
    try:
        what = "pt_ctx_solid (%s) on a %s stream" % ("looks" if with_looks else "no looks", stream)
        want, decoyed, T = expectation(trap, what)
        gate = trap.arm(A)
        try:
            gate.open_after(T)
            rc, host = trap.case.call(trap.P, A)
            finished, timed_out = gate.finished, gate.timed_out
        finally:
            trap.disarm(gate, A)
        stop_on_a_hip_error(dev.L, rc)
        assert rc == 0, (what, rc, dev.L.pt_last_error())
        assert finished, "%s: the call returned while the gate still held the caller's stream" % what
        assert not timed_out, "%s: the gate ran into its timeout" % what
        verdict(trap, trap.read(host), want, decoyed, what)
    finally:
        trap.close()


def test_the_trap_catches_a_call_on_another_stream(dev, streams):
    """The control, as tests/test_gpu_streams.py makes its own: the trap set up on A and pt_ctx_solid called on a second
    non-blocking stream B.  It returns while A is still gated, and once A has run the output is the decoys' result or the caller's
    0xA5, never the expected bytes.  A B whose call only returns when the gate times out shares a hardware queue with A: the next
    stream is tried, four at the most."""
    A = streams["nonblocking-1"]
    trap = Trap(solid_case(dev, True))
    others = []
    try:
        want, decoyed, _T = expectation(trap, "control")
        for attempt in range(1, 5):
            cm = gpudev.stream(nonblocking=True)
            B = cm.__enter__()
            others.append(cm)
            trap.fill(True)
            gate = gpudev.Gate(A, timeout=0.5)
            try:
                for name in trap.case.inputs:
                    assert trap.hip.hipMemcpyAsync(trap.P[name], trap.staged[name], trap.size[name], D2D, A) == 0
                for name in trap.case.outputs:
                    assert trap.hip.hipMemsetAsync(trap.P[name], FILL, trap.size[name], A) == 0
                rc, _host = trap.case.call(trap.P, B)
                held = not gate.finished
            finally:
                trap.disarm(gate, A)
            stop_on_a_hip_error(dev.L, rc)
            assert rc == 0, (rc, dev.L.pt_last_error())
            if not held:
                continue  # B waited for A's gate: the two share a hardware queue
            out = trap.read({})["out"]
            assert out.tobytes() != want["out"].tobytes(), "a call on another stream gave the expected bytes: the trap has no power"
            assert out.tobytes() == decoyed["out"].tobytes() or (out.view(np.uint8) == FILL).all(), "neither the decoys' result nor 0xA5"
            return
        raise AssertionError("no stream out of four is independent of the gated one: the trap has no power on this machine")
    finally:
        for cm in others:
            cm.__exit__(None, None, None)
        trap.close()
