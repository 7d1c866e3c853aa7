"""Every entry point of include/ptrace.h that takes a caller's `hip_stream`, held to the contract of pt_ctx_render's paragraph:
what the call reads from and writes to caller memory is ordered on that stream, behind whatever the caller queued there before
the call, and has completed when the call returns.

THE TRAP.  The caller's stream A is held by a gate (gpudev.Gate: a host function that waits to be opened, two seconds at the
most).  Behind the gate, on A, wait the copies that bring the REAL inputs into the input buffers - until then they hold a DECOY,
another valid input - and a memset of every output buffer to 0xA5.  Then the call is made with hip_stream = A while a timer opens
the gate.  A library that orders its work on A reads the real inputs and writes over the 0xA5; one that works on another stream
reads the decoy (its output is the decoy's result), or writes before the memset (the output ends as 0xA5), or returns while the
gate still holds A.  The expected bytes are the same call's with a NULL stream and the real inputs in place: the other GPU
modules hold those to their restatements.  Before the trap every input is shown to matter (its decoy alone changes some output)
and the expected outputs are shown not to be the fill.

Every case runs on two non-blocking streams created one after the other (with few hardware queues one of them may share a queue
with the context's own stream and pass by accident) and the first case of a family on a blocking stream (hipStreamCreate) too.
test_the_trap_catches_a_call_on_another_stream is the control: the same trap with the call made on a second stream B has to end
in the decoy's result or in 0xA5.

What the trap cannot see: ordering against a stream that shares a hardware queue with the gated one.

Frames are 32 x 24 on cornell at 2 to 4 samples per pixel - 8 and 16 where a noise estimate needs both half buffers (a frame of
4 samples has an empty half B) - and the image passes run at 67 x 33, odd in both axes and more than one workgroup.  The two
denoisers choose the LDS or the global form of a level by its step (1, 2, 4: LDS; from 8 on: global), not by the size of the
frame: five levels run both forms in one call.

tests/test_streams_abi.py compares CASES with the header, so that an entry point with a `hip_stream` cannot go without a case."""
import ctypes as C
import time

import numpy as np
import pytest

import gpudev
import masked_ref
import ptlib
import reproject_ref
import test_gpu_reproject_moved as mbase
import test_gpu_reproject_var as vbase
import upsample_ref
from gpudev import L  # noqa: F401  (fixture)
from ptlib import (PtAdaptiveParams, PtAdaptiveStats, PtAovParams, PtDenoiseParams, PtDenoiseVarParams, PtNoiseStats, PtNoiseTarget,
                   PtPresentParams, PtReprojectParams, PtReprojectVarParams, PtSelectParams, PtStats, PtUpsampleParams)

pytestmark = pytest.mark.gpu

F32, I32, U32, U8 = np.float32, np.int32, np.uint32, np.uint8
abi = ptlib.abi
GUARD = 64                 # bytes behind every buffer
SENTINEL, FILL = 0x5A, 0xA5  # the guards and what an output holds before the trap; what the caller's memset leaves
D2D = 3                    # hipMemcpyDeviceToDevice
W, H, SEED = 32, 24, 5     # the frames of the render family
PW, PH = 67, 33            # the image passes
T_MIN = 0.020


class Case:
    """One call.  inputs: {name: (real, decoy)} - device buffers the call reads; outputs: {name: (elements, dtype)} - device
    buffers it writes; inout: the inputs it also writes.  call(P, stream) -> (rc, {name: host result}) with P the device
    pointers by name; prepare(): what has to be in the context before every call, made with a NULL stream."""

    def __init__(self, dev, call, inputs=None, outputs=None, inout=(), prepare=None):
        self.dev, self.call, self.inputs, self.outputs = dev, call, inputs or {}, outputs or {}
        self.inout, self.prepare = tuple(inout), prepare


class Env:
    """the module's contexts and inputs: a plain context and a noise-tracking one on cornell, the planes of two rendered frames"""

    def __init__(self, L):
        self.L = L
        self.sc = gpudev.scene("cornell")
        self.d = gpudev.Device(L, self.sc)
        self.nd = gpudev.Device(L, self.sc)
        assert L.pt_ctx_accum_track_noise(self.nd.ctx, 1) == 0, L.pt_last_error()
        self.comm = None
        self._frames = None

    def close(self):
        if self.comm is not None:
            self.L.pt_comm_destroy(self.comm)
        self.d.close()
        self.nd.close()

    def frames(self):
        """two cornell frames of PW x PH at 8 samples, from two cameras and two seeds: colour, the noise estimate, the guides"""
        if self._frames is None:
            d, L, n = self.nd, self.L, PW * PH
            bufs = {k: d.alloc(n * 4 * f) for k, f in (("color", 3), ("error", 1), ("albedo", 3), ("normal", 3), ("depth", 1), ("oid", 1))}
            out = []
            for k in (0, 1):
                cam = ptlib.make_camera([self.sc.cam.position[0] + 0.4 * k, self.sc.cam.position[1], self.sc.cam.position[2]],
                                        list(self.sc.cam.direction), self.sc.cam.focal_length, self.sc.cam.sensor_width,
                                        self.sc.cam.aspect_ratio)
                d.set_scene(self.sc, cam)
                cfg = gpudev.config(PW, PH, 8, seed=11 + k)
                d.render(cfg, bufs["color"], accumulate=True)
                ns = PtNoiseStats()
                assert L.pt_ctx_accum_noise(d.ctx, C.byref(cfg), bufs["error"], C.byref(ns), None) == 0, L.pt_last_error()
                assert L.pt_ctx_render_aov(d.ctx, C.byref(gpudev.config(PW, PH, 2, seed=11 + k)), bufs["albedo"], bufs["normal"],
                                           bufs["depth"], bufs["oid"], None) == 0, L.pt_last_error()
                f = {name: d.download(p, n * (3 if name in ("color", "albedo", "normal") else 1), I32 if name == "oid" else F32)
                     for name, p in bufs.items()}
                assert np.isfinite(f["error"]).all()
                out.append(f)
            d.set_scene(self.sc)
            assert L.pt_ctx_accum_reset(d.ctx) == 0
            for p in bufs.values():
                d.free(p)
            self._frames = out
        return self._frames


@pytest.fixture(scope="module")
def env(L):
    e = Env(L)
    yield e
    e.close()


@pytest.fixture(scope="module")
def streams():
    """two non-blocking streams created one after the other, and a blocking one"""
    with gpudev.stream(nonblocking=True) as a, gpudev.stream(nonblocking=True) as b, gpudev.stream() as c:
        yield {"nonblocking-1": a, "nonblocking-2": b, "blocking": c}


# ------------------------------------------------------------------------------------------------------------ the cases
def cfg_of(spp, backend=0, flags=0, w=W, h=H, seed=SEED, **kw):
    return gpudev.config(w, h, spp, backend=backend, seed=seed, flags=flags, **kw)


def stats_of(st):
    return (st.ray_bounces, st.samples)


def fields_of(s):
    """a result struct as a tuple of its fields' values (not its bytes: the padding is nobody's)"""
    return tuple(tuple(v) if isinstance(v, C.Array) else v for v in (getattr(s, name) for name, _ in s._fields_))


def ok(L, rc):
    assert rc == 0, (rc, L.pt_last_error())


def render_case(env, spp=3, **kw):
    cfg = cfg_of(spp, **kw)
    n = env.L.pt_config_pixels(C.byref(cfg))

    def call(P, st):
        s = PtStats()
        rc = env.L.pt_ctx_render(env.d.ctx, C.byref(cfg), P["rgb"], st, None, None, None, C.byref(s))
        return rc, {"stats": stats_of(s)}
    return Case(env.d, call, outputs={"rgb": (n * 3, F32)})


def accumulate_case(env, refine):
    L, d = env.L, env.d

    def prepare():
        ok(L, L.pt_ctx_accum_reset(d.ctx))
        if refine:  # the held frame at 2 samples: the call adds the other two (and clears nothing)
            scratch = d.alloc(W * H * 12)
            d.render(cfg_of(2), scratch, accumulate=True)
            d.free(scratch)

    def call(P, st):
        s = PtStats()
        rc = L.pt_ctx_accumulate(d.ctx, C.byref(cfg_of(4)), P["rgb"], st, None, None, None, C.byref(s))
        return rc, {"stats": stats_of(s)}
    return Case(d, call, outputs={"rgb": (W * H * 3, F32)}, prepare=prepare)


def until_case(env):
    L, d = env.L, env.nd

    def call(P, st):
        s, ns, tgt = PtStats(), PtNoiseStats(), PtNoiseTarget(1e-6, 0.0, 0.0, 8)  # never met: 8 samples, then the cap of 16
        rc = L.pt_ctx_accumulate_until(d.ctx, C.byref(cfg_of(16)), C.byref(tgt), P["rgb"], st, None, None, None, C.byref(s), C.byref(ns))
        return rc, {"stats": stats_of(s), "noise": fields_of(ns)}
    return Case(d, call, outputs={"rgb": (W * H * 3, F32)}, prepare=lambda: ok(L, L.pt_ctx_accum_reset(d.ctx)))


def noise_case(env):
    L, d = env.L, env.nd

    def prepare():
        ok(L, L.pt_ctx_accum_reset(d.ctx))
        scratch = d.alloc(W * H * 12)
        d.render(cfg_of(8), scratch, accumulate=True)  # 4 samples in each half
        d.free(scratch)

    def call(P, st):
        ns = PtNoiseStats()
        rc = L.pt_ctx_accum_noise(d.ctx, C.byref(cfg_of(8)), P["error"], C.byref(ns), st)
        return rc, {"noise": fields_of(ns)}
    return Case(d, call, outputs={"error": (W * H, F32)}, prepare=prepare)


ADAPTIVE = (0.02, 8, 8)  # tile_error, tile, min_spp: levels at 8 and at the cap of 16
ADAPTIVE_OUT = {"rgb": (W * H * 3, F32), "spp": (W * H, U32), "error": (W * H, F32)}


def adaptive_case(env, held):
    L, d = env.L, env.d
    fn = L.pt_ctx_accumulate_adaptive if held else L.pt_ctx_render_adaptive

    def call(P, st):
        par, s, a = PtAdaptiveParams(*ADAPTIVE), PtStats(), PtAdaptiveStats()
        rc = fn(d.ctx, C.byref(cfg_of(16)), C.byref(par), P["rgb"], P["spp"], P["error"], st, None, None, None, C.byref(s), C.byref(a))
        return rc, {"stats": stats_of(s), "astats": fields_of(a)}
    return Case(d, call, outputs=ADAPTIVE_OUT, prepare=lambda: ok(L, L.pt_ctx_adaptive_reset(d.ctx)))


def resolve_case(env):
    L, d = env.L, env.d

    def prepare():
        par, a = PtAdaptiveParams(*ADAPTIVE), PtAdaptiveStats()
        scratch = d.alloc(W * H * 12)
        ok(L, L.pt_ctx_render_adaptive(d.ctx, C.byref(cfg_of(16)), C.byref(par), scratch, None, None, None, None, None, None, None,
                                       C.byref(a)))
        d.free(scratch)

    def call(P, st):
        return L.pt_ctx_adaptive_resolve(d.ctx, C.byref(cfg_of(16)), P["rgb"], P["spp"], P["error"], st), {}
    return Case(d, call, outputs=ADAPTIVE_OUT, prepare=prepare)


AOV_OUT = {"albedo": (W * H * 3, F32), "normal": (W * H * 3, F32), "depth": (W * H, F32), "oid": (W * H, I32)}


def aov_case(env, ex):
    L, d = env.L, env.d

    def call(P, st):
        if not ex:
            return L.pt_ctx_render_aov(d.ctx, C.byref(cfg_of(2)), P["albedo"], P["normal"], P["depth"], P["oid"], st), {}
        par = PtAovParams(abi.PT_AOV_THROUGH_DELTA, 4)
        return L.pt_ctx_render_aov_ex(d.ctx, C.byref(cfg_of(2)), C.byref(par), P["albedo"], P["normal"], P["depth"], P["oid"],
                                      P["chain"], st), {}
    return Case(d, call, outputs=dict(AOV_OUT, chain=(W * H, U32)) if ex else AOV_OUT)


def mask_of(n, w):
    """a mask with every kind of neighbourhood: a checkerboard in the upper half, single pixels below, bytes other than 1"""
    i = np.arange(n)
    m = np.where(i < n // 2, ((i % w) + (i // w)) % 2, i % 7 == 0).astype(U8)
    m[m != 0] = np.where(i[m != 0] % 3 == 0, 0x80, 1)
    return m


def masked_case(env):
    L, d = env.L, env.d
    n = W * H
    rng = np.random.default_rng(9)
    kept = rng.random((n, 3)).astype(F32)  # what the frame holds where the mask is 0: the call leaves it

    def call(P, st):
        s, count = PtStats(), C.c_uint32(12345)
        rc = L.pt_ctx_render_masked(d.ctx, C.byref(cfg_of(4)), P["mask"], P["rgb"], st, None, C.byref(s), C.byref(count))
        return rc, {"stats": stats_of(s), "n_pixels": count.value}
    return Case(d, call, inputs={"mask": (mask_of(n, W), np.zeros(n, dtype=U8)), "rgb": (kept, np.zeros((n, 3), dtype=F32))},
                inout=("rgb",))


def select_case(env):
    L, d = env.L, env.d
    n, par = PW * PH, masked_ref.PARAMS
    planes = {"weight": (masked_ref.plane(n, par["weight_max"], 1), masked_ref.plane(n, par["weight_max"], 3)),
              "len": (masked_ref.plane(n, par["len_max"], 2), masked_ref.plane(n, par["len_max"], 4))}

    def call(P, st):
        p, count = PtSelectParams(par["weight_max"], par["len_max"], 0), C.c_uint32(12345)
        rc = L.pt_ctx_select_pixels(d.ctx, PW, PH, C.byref(p), P["weight"], P["len"], P["mask"], C.byref(count), st)
        return rc, {"n_selected": count.value}
    return Case(d, call, inputs=planes, outputs={"mask": (n, U8)})


def spp_plane_case(env):
    L, d = env.L, env.d
    n = PW * PH

    def call(P, st):
        return L.pt_ctx_spp_plane(d.ctx, PW, PH, 2, P["mask"], 8, P["spp"], st), {}
    return Case(d, call, inputs={"mask": (mask_of(n, PW), np.zeros(n, dtype=U8))}, outputs={"spp": (n, U32)})


def denoise_case(env, var, in_place):
    L, d = env.L, env.d
    real, decoy = env.frames()
    names = ("color", "error", "albedo", "normal", "depth") if var else ("color", "albedo", "normal", "depth")
    levels = 5  # steps 1, 2, 4 in the LDS form, 8 and 16 in the global one

    def call(P, st):
        out = P["color" if in_place else "out"]
        if var:
            p = PtDenoiseVarParams(levels, 0.0, 0.0, 0)
            return L.pt_ctx_denoise_var(d.ctx, PW, PH, C.byref(p), P["color"], P["error"], P["albedo"], P["normal"], P["depth"], out, st), {}
        p = PtDenoiseParams(levels, 0.0, 0.0, 0.0, 0)
        return L.pt_ctx_denoise(d.ctx, PW, PH, C.byref(p), P["color"], P["albedo"], P["normal"], P["depth"], out, st), {}
    return Case(d, call, inputs={k: (real[k], decoy[k]) for k in names}, outputs={} if in_place else {"out": (PW * PH * 3, F32)},
                inout=("color",) if in_place else ())


def present_case(env, ow=0, oh=0):
    L, d = env.L, env.d
    real, decoy = env.frames()

    def call(P, st):
        p = PtPresentParams(ow, oh, 0.0, abi.PT_PRESENT_RGBA8, 0)
        return L.pt_ctx_present(d.ctx, PW, PH, C.byref(p), P["rgb"], P["out"], st), {}
    return Case(d, call, inputs={"rgb": (real["color"], decoy["color"])}, outputs={"out": ((ow or PW) * (oh or PH) * 4, U8)})


def rolled(a, k):
    """the same plane, every pixel moved k places: as valid as the plane itself (the ids index the same table)"""
    return np.roll(a, k, axis=0)


REPROJECT = ("reproject", "reproject_var", "reproject_moved", "reproject_var_moved", "reproject_var_weighted")


def reproject_case(env, kind):
    L, d = env.L, env.d
    var, moved, weighted = "var" in kind, "moved" in kind or "weighted" in kind, "weighted" in kind
    n = PW * PH
    cur, hist = mbase.synthetic(PW, PH)
    cam, hist_cam = (reproject_ref.pt_camera(c) for c in mbase.CAMERAS["translated"])
    table = mbase.mref.table(mbase.MOTION)
    planes = [("color", cur["color"]), ("depth", cur["depth"]), ("oid", cur["oid"]), ("normal", cur["normal"]),
              ("hcolor", hist["color"]), ("hlen", hist["len"]), ("hdepth", hist["depth"]), ("hoid", hist["oid"]), ("hnormal", hist["normal"])]
    if var:
        planes.append(("hmom", hist["mom"]))
    inputs = {name: (a, rolled(a, 101 + 7 * i)) for i, (name, a) in enumerate(planes)}
    if weighted:  # counts 0 .. 16 against a plane of ones
        inputs["spp"] = (np.array([0, 1, 2, 4, 8, 16], dtype=U32)[(np.arange(n) // 5) % 6], np.ones(n, dtype=U32))
    outputs = {"out": (n * 3, F32), "len": (n, F32)}
    if var:
        outputs.update(mom=(n * 2, F32), err=(n, F32))
    V = vbase.PARAMS

    def call(P, st):
        head = [d.ctx, PW, PH]
        if var:
            p = PtReprojectVarParams(V["weight"], V["max_history"], V["depth_tol"], V["normal_min"], V["min_frames"], V["radius"], 0)
        else:
            p = PtReprojectParams(V["weight"], V["max_history"], V["depth_tol"], V["normal_min"], 0)
        args = head + [C.byref(p), C.byref(cam), P["color"], P["depth"], P["oid"], P["normal"]] + ([P["spp"]] if weighted else [])
        args += [C.byref(hist_cam), P["hcolor"], P["hlen"]] + ([P["hmom"]] if var else []) + [P["hdepth"], P["hoid"], P["hnormal"]]
        args += [P["out"], P["len"]] + ([P["mom"], P["err"]] if var else []) + ([table, len(mbase.MOTION)] if moved else []) + [st]
        return getattr(L, "pt_ctx_" + kind)(*args), {}
    return Case(d, call, inputs=inputs, outputs=outputs)


def upsample_case(env):
    L, d = env.L, env.d
    lw, lh = PW // 2, PH // 2
    hi, lo = upsample_ref.synthetic(PW, PH, lw, lh)
    planes = [("l" + k, lo[k]) for k in ("color", "depth", "oid", "normal", "albedo")] + [(k, hi[k]) for k in ("depth", "oid", "normal", "albedo")]
    par = upsample_ref.PARAMS

    def call(P, st):
        p = PtUpsampleParams(par["depth_tol"], par["normal_min"], 0)
        return L.pt_ctx_upsample(d.ctx, PW, PH, lw, lh, C.byref(p), P["lcolor"], P["ldepth"], P["loid"], P["lnormal"], P["lalbedo"],
                                 P["depth"], P["oid"], P["normal"], P["albedo"], P["out"], P["weight"], st), {}
    return Case(d, call, inputs={name: (a, rolled(a, 53 + 11 * i)) for i, (name, a) in enumerate(planes)},
                outputs={"out": (PW * PH * 3, F32), "weight": (PW * PH, F32)})


def gather_case(env):
    """tests/test_gpu_parity.py's world of one rank: the rank's own frame comes back, here with d_local_rgb behind the gate"""
    L, d = env.L, env.d
    if env.comm is None:
        ident, comm = C.create_string_buffer(128), C.c_void_p()
        ok(L, L.pt_comm_unique_id(ident))
        ok(L, L.pt_comm_create(0, 0, 1, ident, C.byref(comm)))
        env.comm = comm
    n = W * H
    scratch = d.alloc(n * 12)
    frame, _ = d.render(cfg_of(3), scratch)
    d.free(scratch)
    cfg = cfg_of(3)
    cfg.chunk_pixels = W

    def call(P, st):
        return L.pt_comm_gather_frame(env.comm, C.byref(cfg), P["local"], P["frame"], st), {}
    return Case(d, call, inputs={"local": (frame, np.zeros((n, 3), dtype=F32))}, outputs={"frame": (n * 3, F32)})


MEGA, SEPARATE, NO_BVH = abi.PT_BACKEND_MEGAKERNEL, abi.PT_FLAG_SEPARATE_KERNELS, abi.PT_FLAG_NO_BVH
PIPES2 = abi.PT_FLAG_PIPELINES(2)
# (case id, the header's entry point, family, how the case is made)
CASES = [
    ("render-wavefront", "pt_ctx_render", "render", lambda e: render_case(e)),
    ("render-megakernel", "pt_ctx_render", "render", lambda e: render_case(e, backend=MEGA)),
    ("render-separate-kernels", "pt_ctx_render", "render", lambda e: render_case(e, flags=SEPARATE)),
    ("render-no-bvh", "pt_ctx_render", "render", lambda e: render_case(e, flags=NO_BVH)),
    ("render-chunks", "pt_ctx_render", "render", lambda e: render_case(e, chunks=(W, 1, 2))),
    ("render-pipelines", "pt_ctx_render", "pipelines", lambda e: render_case(e, flags=PIPES2)),
    ("render-pipelines-chunks", "pt_ctx_render", "pipelines", lambda e: render_case(e, flags=PIPES2, chunks=(W, 1, 2))),
    ("accumulate-fresh", "pt_ctx_accumulate", "accumulate", lambda e: accumulate_case(e, False)),
    ("accumulate-refine", "pt_ctx_accumulate", "accumulate", lambda e: accumulate_case(e, True)),
    ("accumulate-until", "pt_ctx_accumulate_until", "noise", until_case),
    ("accum-noise", "pt_ctx_accum_noise", "noise", noise_case),
    ("render-adaptive", "pt_ctx_render_adaptive", "adaptive", lambda e: adaptive_case(e, False)),
    ("accumulate-adaptive", "pt_ctx_accumulate_adaptive", "adaptive", lambda e: adaptive_case(e, True)),
    ("adaptive-resolve", "pt_ctx_adaptive_resolve", "adaptive", resolve_case),
    ("render-aov", "pt_ctx_render_aov", "aov", lambda e: aov_case(e, False)),
    ("render-aov-ex", "pt_ctx_render_aov_ex", "aov", lambda e: aov_case(e, True)),
    ("render-masked", "pt_ctx_render_masked", "masked", masked_case),
    ("select-pixels", "pt_ctx_select_pixels", "masked", select_case),
    ("spp-plane", "pt_ctx_spp_plane", "masked", spp_plane_case),
    ("denoise", "pt_ctx_denoise", "denoise", lambda e: denoise_case(e, False, False)),
    ("denoise-in-place", "pt_ctx_denoise", "denoise", lambda e: denoise_case(e, False, True)),
    ("denoise-var", "pt_ctx_denoise_var", "denoise", lambda e: denoise_case(e, True, False)),
    ("denoise-var-in-place", "pt_ctx_denoise_var", "denoise", lambda e: denoise_case(e, True, True)),
    ("present-same-size", "pt_ctx_present", "present", lambda e: present_case(e)),
    ("present-resized", "pt_ctx_present", "present", lambda e: present_case(e, 40, 21)),
] + [(k.replace("_", "-"), "pt_ctx_" + k, "reproject", lambda e, k=k: reproject_case(e, k)) for k in REPROJECT] + [
    ("upsample", "pt_ctx_upsample", "upsample", upsample_case),
    ("gather-frame-world-1", "pt_comm_gather_frame", "gather", gather_case),
]
_first = {}
for _id, _entry, _family, _make in CASES:
    _first.setdefault(_family, _id)
RUNS = [(c, s) for c in CASES for s in ("nonblocking-1", "nonblocking-2")] + [(c, "blocking") for c in CASES if _first[c[2]] == c[0]]


# ------------------------------------------------------------------------------------------------------------- the driver
class Trap:
    """the buffers of one case on its device, and the steps of the driver"""

    def __init__(self, case):
        self.case, self.d, self.hip = case, case.dev, gpudev.hip_runtime()
        self.size, self.dtype, self.P, self.staged = {}, {}, {}, {}
        for name, (real, decoy) in case.inputs.items():
            real, decoy = np.ascontiguousarray(real), np.ascontiguousarray(decoy)
            assert real.dtype == decoy.dtype and real.shape == decoy.shape, name
            self.size[name], self.dtype[name] = real.nbytes, real.dtype
            self.staged[name] = self.d.alloc(real.nbytes)  # the real input on the device, for the copy behind the gate
            self.d.upload(self.staged[name], real)
        for name, (count, dtype) in case.outputs.items():
            self.size[name], self.dtype[name] = count * np.dtype(dtype).itemsize, np.dtype(dtype)
        for name, nbytes in self.size.items():
            self.P[name] = self.d.alloc(nbytes + GUARD)
        self.read_back = tuple(case.outputs) + case.inout

    def close(self):
        for p in list(self.P.values()) + list(self.staged.values()):
            self.d.free(p)

    def fill(self, decoys=()):
        """synchronously: the real inputs but for `decoys` (True: all of them), sentinels in the outputs and in every guard"""
        for name, (real, decoy) in self.case.inputs.items():
            self.d.upload(self.P[name], decoy if decoys is True or name in decoys else real)
            self.d.upload(self.P[name], np.full(GUARD, SENTINEL, dtype=U8), self.size[name])
        for name in self.case.outputs:
            self.d.upload(self.P[name], np.full(self.size[name] + GUARD, SENTINEL, dtype=U8))

    def run(self, stream=None):
        """prepare, call: (rc, what the call wrote - device buffers by name and host results - and the seconds it took)"""
        if self.case.prepare:
            self.case.prepare()
        t0 = time.perf_counter()
        rc, host = self.case.call(self.P, stream)
        seconds = time.perf_counter() - t0
        stop_on_a_hip_error(self.d.L, rc)
        return rc, host, seconds

    def read(self, host):
        got = dict(host)
        for name in self.read_back:
            raw = self.d.download(self.P[name], self.size[name] + GUARD, U8)
            assert (raw[self.size[name]:] == SENTINEL).all(), "%s was written past its %d bytes" % (name, self.size[name])
            got[name] = raw[:self.size[name]].view(self.dtype[name])
        return got

    def null_stream(self, decoys=()):
        self.fill(decoys)
        rc, host, seconds = self.run()
        assert rc == 0, (rc, self.d.L.pt_last_error())
        return self.read(host), seconds

    def arm(self, A):
        """decoys and sentinels in place, the gate on A, and behind it the real inputs and the memsets"""
        self.fill(True)
        if self.case.prepare:
            self.case.prepare()
        gate = gpudev.Gate(A)
        try:
            for name in self.case.inputs:
                assert self.hip.hipMemcpyAsync(self.P[name], self.staged[name], self.size[name], D2D, A) == 0
            for name in self.case.outputs:
                assert self.hip.hipMemsetAsync(self.P[name], FILL, self.size[name], A) == 0
        except BaseException:
            self.disarm(gate, A)
            raise
        return gate

    def disarm(self, gate, A):
        gate.close()
        assert self.hip.hipStreamSynchronize(A) == 0


def stop_on_a_hip_error(L, rc):
    """a HIP runtime error is no finding of this module and leaves the device in no state to go on with: the session ends"""
    if rc == abi.PT_ERR_HIP:
        pytest.exit("a call failed in the HIP runtime: %s" % L.pt_last_error(), returncode=3)


def differs(a, b):
    return any(np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() if isinstance(a[k], np.ndarray) else a[k] != b[k] for k in a)


def verdict(trap, got, want, decoyed, what):
    """the outputs are the expected bytes - or which mistake they show"""
    for name in want:
        if isinstance(want[name], np.ndarray):
            if got[name].tobytes() == want[name].tobytes():
                continue
            if decoyed is not None and got[name].tobytes() == decoyed[name].tobytes():
                raise AssertionError("%s: %s is the decoy's result: the inputs were read before the caller's copies on the stream" % (what, name))
            if name in trap.case.outputs and (got[name].view(U8) == FILL).all():
                raise AssertionError("%s: %s holds the caller's 0xA5: it was written before the memset queued on the stream" % (what, name))
            gpudev.same_bytes(got[name], want[name], "%s: %s" % (what, name))
        else:
            assert got[name] == want[name], "%s: %s is %r, not %r" % (what, name, got[name], want[name])


def expectation(trap, what):
    """steps 1 and 2: the expected outputs, the decoys' outputs (None without inputs) and T"""
    want, seconds = trap.null_stream()
    again, seconds = trap.null_stream()  # (the first call of a kind also sizes the context's scratch: time the second)
    assert not differs(want, again), "%s: two NULL-stream calls differ" % what
    for name in trap.case.outputs:
        filled = want[name].view(U8)
        assert not (filled == FILL).all() and not (filled == SENTINEL).all(), "%s: %s is not written, or is the fill" % (what, name)
    decoyed = None
    if trap.case.inputs:
        for name in trap.case.inputs:  # every input matters on its own
            alone, _ = trap.null_stream((name,))
            assert differs(alone, want), "%s: the decoy of %s changes no output: the case cannot see it" % (what, name)
        decoyed, _ = trap.null_stream(True)
        assert differs(decoyed, want), "%s: the decoys change no output" % what
    return want, decoyed, max(T_MIN, 4 * seconds)


@pytest.mark.parametrize("case,stream", RUNS, ids=["%s-%s" % (c[0], s) for c, s in RUNS])
def test_the_call_is_ordered_on_the_callers_stream(env, streams, case, stream):
    cid, entry, _family, make = case
    A = streams[stream]
    trap = Trap(make(env))
    try:
        want, decoyed, T = expectation(trap, cid)
        what = "%s (%s) on a %s stream, gate opened after T = %.1f ms" % (cid, entry, stream, T * 1e3)
        print("T %s %s %.1f ms" % (cid, stream, T * 1e3))
        gate = trap.arm(A)
        try:
            gate.open_after(T)
            rc, host = trap.case.call(trap.P, A)
            finished, timed_out = gate.finished, gate.timed_out
        finally:
            trap.disarm(gate, A)
        stop_on_a_hip_error(env.L, rc)
        assert rc == 0, (what, rc, env.L.pt_last_error())
        assert finished, "%s: the call returned while the gate still held the caller's stream" % what
        assert not timed_out, "%s: the gate ran into its timeout" % what
        verdict(trap, trap.read(host), want, decoyed, what)
    finally:
        trap.close()


def test_the_trap_catches_a_call_on_another_stream(env, streams):
    """The control.  pt_ctx_present with the trap set up on A and the call made on a second non-blocking stream B: it returns
    while A is still gated, and once A has run the output is the decoy's result or the caller's 0xA5, never the expected bytes.
    A B whose call only returns when the gate times out (0.5 s here) shares a hardware queue with A: the next stream is tried,
    four at the most, and with none independent the control fails - the module would prove nothing on such a machine."""
    A = streams["nonblocking-1"]
    trap = Trap(present_case(env))
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
            stop_on_a_hip_error(env.L, rc)
            assert rc == 0, (rc, env.L.pt_last_error())
            if not held:
                continue  # B waited for A's gate: the two share a hardware queue
            print("control: independent B found at attempt %d" % attempt)
            got = trap.read({})
            out = got["out"]
            assert out.tobytes() != want["out"].tobytes(), "a call on another stream gave the expected bytes: the trap has no power"
            assert out.tobytes() == decoyed["out"].tobytes() or (out == FILL).all(), "neither the decoy's result nor 0xA5"
            return
        raise AssertionError("no stream out of four is independent of the gated one: the trap has no power on this machine")
    finally:
        for cm in others:
            cm.__exit__(None, None, None)
        trap.close()
