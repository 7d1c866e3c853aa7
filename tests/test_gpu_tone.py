"""The tone stage on the GPU - pt_ctx_tonemap, pt_ctx_meter, pt_ctx_accum_hdr - against tests/tone_ref.py, the restatement of
include/ptrace_tone.h in numpy.  Every comparison is of bits or of integer counts, for equality.

The kernels' units are four pixels per lane and 256 lanes per workgroup, and a lane-per-pixel form takes the last npix % 4
pixels and every call with a plane that is not 16-byte aligned.  So the frames are 1x1 (no whole group), 7x3 = 21 (five groups and
a rest of one) and 67x33 = 2211 (552 groups, a rest of three, three workgroups).  The frames hold the edge table of tone_ref.py -
every bin edge, its predecessor, NaN, +-0, +-inf, denormals, 2^32 and beyond - tiled: no output of the stage is a NaN, so the
bits are the same on every machine.

The meter's frames: the same sizes, a 256x64 frame of one colour (every lane of every wave at one bin: the wave-wide combine), a
frame with every edge once, rectangles (one pixel; touching the last row and column; a left edge that is no multiple of 4), a
checkerboard of ids, two calls in a row, and the maximum with NaN and +inf in the frame.

pt_ctx_accum_hdr: cornell at 32x24 from a camera that looks up at the lamp, against the resolve of the raw sums
pt_ctx_accum_save writes; a band with chunks (an odd number of pixels: the lane-per-pixel form); a second accumulate; a frame of
1600x1024 in parts of 2^20 pixels with different counts.

The stream contract: the trap of tests/test_gpu_streams.py rebuilt on gpudev.Gate - the caller's stream is held by a gate, behind
it wait the copy of the real input over a decoy and a memset of the output; a call that is ordered on the stream reads the real
input and writes over the memset, and has not returned while the gate holds."""
import ctypes as C
import struct

import numpy as np
import pytest

import gpudev
import noise_ref
import ptlib
import tone_ref as ref
from gpudev import L  # noqa: F401  (fixture)
from tone_ref import ACES, CLAMP, F32, LUMA, REINHARD, U32

pytestmark = pytest.mark.gpu

ta = ref.tone_abi
I32 = np.int32
GUARD = 64  # floats before and behind the output
SENTINEL = F32(-7.5)
SIZES = ((1, 1), (7, 3), (67, 33))
MAX_PIX = 256 * 64


def table_frame(w, h, seed=0):
    """(w*h, 3): the edge table tiled over the frame, each value beside two others of the table; small frames get a random cut"""
    t = ref.edge_table()
    n = w * h
    rng = np.random.default_rng(seed + n)
    flat = np.resize(np.stack([t, np.roll(t, 7), np.roll(t, 101)], axis=1).reshape(-1), n * 3) if n * 3 >= t.size else rng.choice(t, size=n * 3)
    return np.ascontiguousarray(flat, dtype=F32).reshape(n, 3)


class Dev(gpudev.Device):
    def __init__(self, L, scene=None, cam=None):
        super().__init__(L, scene, cam)
        room = (MAX_PIX * 3 + 2 * GUARD + 8) * 4
        self.rgb, self.out, self.ids = self.alloc(room), self.alloc(room), self.alloc(MAX_PIX * 4 + 64)

    def tonemap(self, w, h, rgb, params, in_place=False, off_in=0, off_out=0, stream=None):
        """the (w*h, 3) frame the call wrote, as bits; the guards around the output are checked, and the input where it is not the output"""
        n3 = w * h * 3
        src = np.concatenate([np.full(GUARD, SENTINEL, dtype=F32), rgb.reshape(-1), np.full(GUARD, SENTINEL, dtype=F32)])
        self.upload(self.rgb, src, offset=off_in)
        if not in_place:
            self.upload(self.out, np.full(n3 + 2 * GUARD, SENTINEL, dtype=F32), offset=off_out)
        d_in = C.c_void_p(self.rgb.value + off_in + GUARD * 4)
        d_out = d_in if in_place else C.c_void_p(self.out.value + off_out + GUARD * 4)
        rc = self.L.pt_ctx_tonemap(self.ctx, w, h, C.byref(params) if params is not None else None, d_in, d_out, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.download(self.rgb if in_place else self.out, n3 + 2 * GUARD, offset=off_in if in_place else off_out)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n3:] == SENTINEL).all(), "d_out was written outside its %d floats" % n3
        if not in_place:
            assert self.download(self.rgb, src.size, offset=off_in).tobytes() == src.tobytes(), "d_rgb was written"
        return got[GUARD:GUARD + n3].reshape(-1, 3).view(U32)

    def meter(self, w, h, rgb, rect=None, ids=None, flags=None, off=0, stream=None):
        self.upload(self.rgb, rgb, offset=off)
        if ids is not None:
            self.upload(self.ids, np.ascontiguousarray(ids, dtype=I32), offset=off)
        p = ta.pt_meter_params(ta.PT_METER_SKIP_MISSES if ids is not None else 0, *(rect or (0, 0, 0, 0)))
        if flags is not None:
            p.flags = flags
        out = ta.pt_meter_stats()
        rc = self.L.pt_ctx_meter(self.ctx, w, h, C.byref(p) if (rect or ids is not None or flags is not None) else None,
                                 C.c_void_p(self.rgb.value + off), C.c_void_p(self.ids.value + off) if ids is not None else None,
                                 C.byref(out), stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        return out


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


def same_stats(got, want, what):
    pixels, dark, hist, mx = want
    assert got.pixels == pixels and got.dark == dark, (what, got.pixels, pixels, got.dark, dark)
    assert list(got.histogram) == hist.tolist(), what
    assert ref.bits(F32(got.max_luminance)).tolist() == ref.bits(F32(mx)).tolist(), (what, got.max_luminance, mx)
    assert got.pixels == got.dark + sum(got.histogram)


# ------------------------------------------------------------------------------------------------------------ tonemap
@pytest.mark.parametrize("flags", [0, LUMA])
@pytest.mark.parametrize("curve", [CLAMP, REINHARD, ACES])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_tonemap_is_the_restatement(dev, size, curve, flags):
    w, h = size
    rgb = table_frame(w, h)
    if w * h >= 2211:
        assert np.isin(ref.edge_table().view(U32), rgb.view(U32)).all()  # the whole table is in the frame
    for exposure, white in ((1.0, 4.0), (0.37, 1.5)):
        p = ta.pt_tonemap_params(curve, flags, exposure, white)
        want = ref.tonemap(rgb, curve, flags, exposure, white).view(U32)
        got = dev.tonemap(w, h, rgb, p)
        gpudev.same_bytes(got, want, "tonemap %dx%d curve %d flags %d exposure %g" % (w, h, curve, flags, exposure))
        gpudev.same_bytes(dev.tonemap(w, h, rgb, p, in_place=True), want, "in place")
        # a plane 4 bytes off takes the lane-per-pixel form: the same bytes
        gpudev.same_bytes(dev.tonemap(w, h, rgb, p, off_in=4), want, "d_rgb 4 bytes off")
        gpudev.same_bytes(dev.tonemap(w, h, rgb, p, off_out=4), want, "d_out 4 bytes off")
        gpudev.same_bytes(dev.tonemap(w, h, rgb, p, in_place=True, off_in=12), want, "in place, 12 bytes off")


def test_tonemap_defaults_and_the_clamp_identity(dev, L):
    w, h = 67, 33
    rgb = table_frame(w, h, seed=3)
    gpudev.same_bytes(dev.tonemap(w, h, rgb, None), ref.tonemap(rgb, ACES, 0, 1.0, 4.0).view(U32), "NULL params")
    # PT_TONE_CLAMP at exposure e, presented at exposure 1 == the source presented at exposure e
    e = 0.3
    mapped = dev.tonemap(w, h, rgb, ta.pt_tonemap_params(CLAMP, 0, e, 4.0)).view(F32).reshape(-1)
    a, b = np.zeros(mapped.size, dtype=np.uint8), np.zeros(mapped.size, dtype=np.uint8)
    flat = np.ascontiguousarray(rgb.reshape(-1))
    assert L.pt_present_quantize_host(mapped.ctypes.data_as(C.c_void_p), mapped.size, 1.0, a.ctypes.data_as(C.c_void_p)) == 0
    assert L.pt_present_quantize_host(flat.ctypes.data_as(C.c_void_p), flat.size, e, b.ctypes.data_as(C.c_void_p)) == 0
    assert a.tolist() == b.tolist() and len(set(a.tolist())) > 50  # (the frame spreads over the bytes)


# -------------------------------------------------------------------------------------------------------------- meter
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_meter_is_the_restatement(dev, size):
    w, h = size
    rgb = table_frame(w, h, seed=1)
    same_stats(dev.meter(w, h, rgb), ref.meter(rgb, w, h), "aligned")
    same_stats(dev.meter(w, h, rgb, off=4), ref.meter(rgb, w, h), "4 bytes off")  # pixel by pixel


def test_meter_one_colour(dev):
    """256 x 64 pixels of one colour: every lane of every wave at one bin, which takes all 16 384"""
    w, h = 256, 64
    for colour, dark in (((0.5, 0.25, 2.0), False), ((0.0, 0.0, 0.0), True)):
        rgb = np.tile(np.array(colour, dtype=F32), (w * h, 1))
        got = dev.meter(w, h, rgb)
        same_stats(got, ref.meter(rgb, w, h), colour)
        assert got.dark == (w * h if dark else 0) and max(got.histogram) == (0 if dark else w * h)
    # one pixel of another bin in the middle of a wave: the wave falls back to the per-lane adds
    rgb = np.tile(np.array((0.5, 0.25, 2.0), dtype=F32), (w * h, 1))
    rgb[777] = (40.0, 40.0, 40.0)
    got = dev.meter(w, h, rgb)
    same_stats(got, ref.meter(rgb, w, h), "one odd pixel")
    assert sorted(got.histogram)[-2:] == [1, w * h - 1]


def test_meter_every_edge_once(dev):
    """a grey frame holding every bin edge, every predecessor and every special once: Y = ((0.2126 v + 0.7152 v) + 0.0722 v)"""
    t = ref.edge_table()
    pad = (-len(t)) % 10
    v = np.concatenate([t, np.zeros(pad, dtype=F32)])
    rgb = np.zeros((len(v), 3), dtype=F32)
    with np.errstate(all="ignore"):
        rgb[:, 1] = v / F32(0.7152)  # the luminance is about v; exactly which bin is the restatement's business
    w, h = 10, len(v) // 10
    want = ref.meter(rgb, w, h)
    assert (want[2] > 0).sum() > 200 and want[1] > 5  # (the inputs reach most bins and the dark count)
    same_stats(dev.meter(w, h, rgb), want, "edges")


def test_meter_rectangles_and_ids(dev):
    w, h = 67, 33
    rgb = table_frame(w, h, seed=2)
    for rect in ((5, 7, 6, 8),            # one pixel
                 (60, 30, 67, 33),        # touching the last row and column
                 (66, 32, 67, 33),        # the last pixel
                 (3, 0, 31, 33),          # a left edge that is no multiple of 4, all rows
                 (1, 1, 2, 32), (0, 4, 67, 9), (0, 0, 67, 33), (0, 0, 66, 33), (0, 0, 1, 1)):
        same_stats(dev.meter(w, h, rgb, rect=rect), ref.meter(rgb, w, h, rect=rect), rect)
        same_stats(dev.meter(w, h, rgb, rect=rect, off=8), ref.meter(rgb, w, h, rect=rect), (rect, "8 bytes off"))
    i = np.arange(w * h)
    board = np.where(((i % w) + (i // w)) % 2 == 0, 3, -1).astype(I32)
    got = dev.meter(w, h, rgb, ids=board)
    same_stats(got, ref.meter(rgb, w, h, ids=board), "checkerboard")
    assert got.pixels == int((board >= 0).sum())
    same_stats(dev.meter(w, h, rgb, ids=board, rect=(3, 2, 40, 31)), ref.meter(rgb, w, h, rect=(3, 2, 40, 31), ids=board), "board in a rectangle")
    same_stats(dev.meter(w, h, rgb, ids=board, off=4), ref.meter(rgb, w, h, ids=board), "board, 4 bytes off")
    none = np.full(w * h, -1, dtype=I32)
    got = dev.meter(w, h, rgb, ids=none)
    assert got.pixels == 0 and got.dark == 0 and sum(got.histogram) == 0 and got.max_luminance == 0.0
    # the ids without the flag are not read
    same_stats(dev.meter(w, h, rgb, ids=none, flags=0), ref.meter(rgb, w, h), "no flag")


def test_meter_twice_and_the_maximum(dev):
    w, h = 67, 33
    rng = np.random.default_rng(4)
    rgb = (rng.random((w * h, 3)) * 3).astype(F32)
    want = ref.meter(rgb, w, h)
    same_stats(dev.meter(w, h, rgb), want, "first")
    same_stats(dev.meter(w, h, rgb), want, "second: not the sum of both")
    assert 0 < want[3] < 3.1
    rgb[100] = np.nan
    rgb[200, 2] = np.nan
    same_stats(dev.meter(w, h, rgb), ref.meter(rgb, w, h), "NaN is dark and no maximum")
    rgb[300, 0] = np.inf
    got = dev.meter(w, h, rgb)
    same_stats(got, ref.meter(rgb, w, h), "+inf")
    assert got.max_luminance == np.inf and got.histogram[255] >= 1
    tiny = np.zeros((w * h, 3), dtype=F32)
    tiny[5, 1] = 1e-30  # dark, yet the largest Y > 0
    tiny[6, 0] = -4.0
    got = dev.meter(w, h, tiny)
    same_stats(got, ref.meter(tiny, w, h), "tiny")
    assert got.dark == w * h and 0 < got.max_luminance < 1e-30


# ---------------------------------------------------------------------------------------------------- pt_ctx_accum_hdr
UP = (0.0, 0.35, -0.93)  # cornell's camera turned up at the lamp (chosen with the CPU oracle: 508 of 768 pixels saturate)
W, H, SEED = 32, 24, 5


def lamp_scene():
    sc = gpudev.scene("cornell")
    d = np.array(UP) / np.linalg.norm(UP)
    cam = ptlib.make_camera(list(sc.cam.position), [float(v) for v in d], sc.cam.focal_length, sc.cam.sensor_width, sc.cam.aspect_ratio)
    return sc, cam


def checkpoint(L, d, tmp_path, name):
    path = tmp_path / name
    assert L.pt_ctx_accum_save(d.ctx, str(path).encode()) == 0, L.pt_last_error()
    return noise_ref.parse_checkpoint(path.read_bytes())


def hdr_reference(ck):
    """(total, 3) float32 from the checkpoint's raw sums, each pixel over its part's count"""
    counts = np.repeat(ck["counts"], ck["part_px"])[:ck["total"]]
    return ref.hdr_resolve(ck["sums"].T, counts[:, None])


def hdr_call(L, d, cfg, out, n, stream=None):
    d.upload(out, np.full(n * 3 + GUARD, SENTINEL, dtype=F32))
    rc = L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), out, stream)
    assert rc == 0, (rc, L.pt_last_error())
    got = d.download(out, n * 3 + GUARD)
    assert (got[n * 3:] == SENTINEL).all(), "d_out_rgb was written past its %d floats" % (n * 3)
    return got[:n * 3].reshape(n, 3)


@pytest.mark.parametrize("layout", ["whole", "band+chunks"])
def test_accum_hdr_is_the_held_sums_without_the_clamp(L, tmp_path, layout):
    sc, cam = lamp_scene()
    kw = {} if layout == "whole" else dict(band=(37, 700), chunks=(13, 1, 2))
    with gpudev.Device(L, sc, cam) as d:
        out = d.alloc((W * H * 3 + GUARD) * 4)
        held = None
        for spp in (16, 32):  # the second call accumulates on
            cfg = gpudev.config(W, H, spp, seed=SEED, **kw)
            n = L.pt_config_pixels(C.byref(cfg))
            assert (n % 2 == 1) == (layout != "whole")  # the band's frame takes the lane-per-pixel form
            clamped, _ = d.render(cfg, out, accumulate=True)
            before = checkpoint(L, d, tmp_path, "before")
            want = hdr_reference(before)
            assert (want > 1).sum() > 20 and want.max() > 1.5, "the lamp is not in view: nothing exceeds 1"
            lo, hi = C.c_uint32(), C.c_uint32()
            probe = gpudev.config(W, H, 1, seed=SEED, backend=1, **kw)  # only the key matters: another spp and backend
            got = hdr_call(L, d, probe, out, n)
            gpudev.same_bytes(got, want, "%s at %d spp" % (layout, spp))
            gpudev.same_bytes(np.clip(got, F32(0), F32(1)), clamped, "its clamp is pt_ctx_accumulate's frame")
            assert held is None or not np.array_equal(held, got)
            held = got
            # the call changed nothing that is held
            assert L.pt_ctx_accum_info(d.ctx, C.byref(cfg), C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (spp, spp)
            after = checkpoint(L, d, tmp_path, "after")
            assert (tmp_path / "before").read_bytes() == (tmp_path / "after").read_bytes()
            assert after["counts"].tolist() == [spp]
        # another frame than the held one, and none at all
        for other in (gpudev.config(W, H + 1, 16, seed=SEED), gpudev.config(W, H, 16, seed=SEED + 1)):
            assert L.pt_ctx_accum_hdr(d.ctx, C.byref(other), out, None) == ptlib.abi.PT_ERR_INVALID
            assert "held" in L.pt_last_error().decode() or "holds" in L.pt_last_error().decode()
        assert L.pt_ctx_accum_reset(d.ctx) == 0
        assert L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), out, None) == ptlib.abi.PT_ERR_INVALID


def test_accum_hdr_tracked_frame_leaves_half_a(L, tmp_path):
    sc, cam = lamp_scene()
    with gpudev.Device(L, sc, cam) as d:
        assert L.pt_ctx_accum_track_noise(d.ctx, 1) == 0
        out = d.alloc((W * H * 3 + GUARD) * 4)
        cfg = gpudev.config(W, H, 8, seed=SEED)
        d.render(cfg, out, accumulate=True)
        before = checkpoint(L, d, tmp_path, "before")
        assert before["a"] is not None
        gpudev.same_bytes(hdr_call(L, d, cfg, out, W * H), hdr_reference(before), "tracked")
        checkpoint(L, d, tmp_path, "after")
        assert (tmp_path / "before").read_bytes() == (tmp_path / "after").read_bytes()


def test_accum_hdr_many_parts(L, tmp_path):
    """1600 x 1024 = 1 638 400 pixels in two parts of 2^20 and 589 824 pixels, at 1 sample.  Then the parts get DIFFERENT counts,
    as a cancelled call leaves them: the checkpoint's counts are edited to 3 and 2, the file sealed again and loaded, and every
    pixel has to be divided by its own part's count"""
    sc, cam = lamp_scene()
    w, h = 1600, 1024
    with gpudev.Device(L, sc, cam) as d:
        n = w * h
        out = d.alloc((n * 3 + GUARD) * 4)
        cfg = gpudev.config(w, h, 1, seed=SEED)
        clamped, _ = d.render(cfg, out, accumulate=True)
        ck = checkpoint(L, d, tmp_path, "ck")
        assert ck["part_px"] == 1 << 20 and ck["counts"].tolist() == [1, 1]
        want = hdr_reference(ck)
        assert (want > 1).sum() > 1000
        got = hdr_call(L, d, cfg, out, n)
        gpudev.same_bytes(got, want, "two parts")
        gpudev.same_bytes(np.clip(got, F32(0), F32(1)), clamped, "its clamp")
        raw = bytearray((tmp_path / "ck").read_bytes()[:-8])
        assert struct.unpack_from("<2I", raw, 68) == (1, 1)
        struct.pack_into("<2I", raw, 68, 3, 2)
        raw = bytes(raw)
        (tmp_path / "edited").write_bytes(raw + struct.pack("<Q", L.pt_siphash(1, 3, 0, 0, raw, len(raw))))
        assert L.pt_ctx_accum_load(d.ctx, str(tmp_path / "edited").encode()) == 0, L.pt_last_error()
        edited = noise_ref.parse_checkpoint((tmp_path / "edited").read_bytes())
        assert edited["counts"].tolist() == [3, 2]
        want2 = hdr_reference(edited)
        edge = 1 << 20
        assert want2[edge - 1].tolist() == ref.hdr_resolve(ck["sums"].T[edge - 1], 3).tolist()
        assert want2[edge].tolist() == ref.hdr_resolve(ck["sums"].T[edge], 2).tolist()
        gpudev.same_bytes(hdr_call(L, d, cfg, out, n), want2, "two parts with counts 3 and 2")


# ------------------------------------------------------------------------------------------------------------ streams
FILL = 0xA5
D2D = 3


def trapped(dev, A, call, inp, real, decoy, outp, out_bytes, T=0.05):
    """the call made on the gated stream A: behind the gate wait the copy of `real` over the decoy in `inp` and a memset of `outp`
    to 0xA5.  Returns what call(A) returned, once the gate has been seen finished at the call's return."""
    hip = gpudev.hip_runtime()
    staged = None
    if inp is not None:
        staged = dev.alloc(real.nbytes)
        dev.upload(staged, real)
        dev.upload(inp, decoy)
    gate = gpudev.Gate(A)
    try:
        if inp is not None:
            assert hip.hipMemcpyAsync(inp, staged, real.nbytes, D2D, A) == 0
        if outp is not None:
            assert hip.hipMemsetAsync(outp, FILL, out_bytes, A) == 0
        gate.open_after(T)
        res = call(A)
        finished, timed_out = gate.finished, gate.timed_out
    finally:
        gate.close()
        assert hip.hipStreamSynchronize(A) == 0
        if staged is not None:
            dev.free(staged)
    assert finished, "the call returned while the gate still held the caller's stream"
    assert not timed_out, "the gate ran into its timeout"
    return res


@pytest.fixture(scope="module")
def streams():
    with gpudev.stream(nonblocking=True) as a, gpudev.stream(nonblocking=True) as b, gpudev.stream() as c:
        yield {"nonblocking-1": a, "nonblocking-2": b, "blocking": c}


STREAMS = ("nonblocking-1", "nonblocking-2", "blocking")


@pytest.mark.parametrize("stream", STREAMS)
def test_tonemap_is_ordered_on_the_callers_stream(dev, streams, stream):
    w, h = 67, 33
    n3 = w * h * 3
    real, decoy = table_frame(w, h, seed=5), (np.random.default_rng(6).random((w * h, 3)) * 4).astype(F32)
    p = ta.pt_tonemap_params(ACES, LUMA, 0.5, 4.0)
    want, wrong = ref.tonemap(real, ACES, LUMA, 0.5, 4.0), ref.tonemap(decoy, ACES, LUMA, 0.5, 4.0)
    assert want.tobytes() != wrong.tobytes()

    def call(A):
        rc = dev.L.pt_ctx_tonemap(dev.ctx, w, h, C.byref(p), dev.rgb, dev.out, A)
        assert rc == 0, (rc, dev.L.pt_last_error())
        return dev.download(dev.out, n3).reshape(-1, 3)

    dev.upload(dev.rgb, real)
    gpudev.same_bytes(call(None), want, "NULL stream")
    got = trapped(dev, streams[stream], call, dev.rgb, real, decoy, dev.out, n3 * 4)
    assert got.tobytes() != wrong.tobytes(), "the decoy's result: d_rgb was read before the caller's copy on the stream"
    assert not (got.view(np.uint8) == FILL).all(), "the caller's 0xA5: d_out was written before the memset queued on the stream"
    gpudev.same_bytes(got, want, "tonemap on a %s stream" % stream)


@pytest.mark.parametrize("stream", STREAMS)
def test_meter_is_ordered_on_the_callers_stream(dev, streams, stream):
    w, h = 67, 33
    real, decoy = table_frame(w, h, seed=7), (np.random.default_rng(8).random((w * h, 3)) * 4).astype(F32)
    want = ref.meter(real, w, h)
    assert want[2].tolist() != ref.meter(decoy, w, h)[2].tolist()

    def call(A):
        out = ta.pt_meter_stats()
        rc = dev.L.pt_ctx_meter(dev.ctx, w, h, None, dev.rgb, None, C.byref(out), A)
        assert rc == 0, (rc, dev.L.pt_last_error())
        return out

    got = trapped(dev, streams[stream], call, dev.rgb, real, decoy, None, 0)
    same_stats(got, want, "meter on a %s stream" % stream)


@pytest.mark.parametrize("stream", STREAMS)
def test_accum_hdr_is_ordered_on_the_callers_stream(L, streams, stream):
    sc, cam = lamp_scene()
    with gpudev.Device(L, sc, cam) as d:
        n3 = W * H * 3
        out = d.alloc(n3 * 4)
        cfg = gpudev.config(W, H, 4, seed=SEED)
        d.render(cfg, out, accumulate=True)

        def call(A):
            rc = L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), out, A)
            assert rc == 0, (rc, L.pt_last_error())
            return d.download(out, n3)

        want = call(None)
        assert want.max() > 1
        got = trapped(d, streams[stream], call, None, None, None, out, n3 * 4)
        assert not (got.view(np.uint8) == FILL).all(), "the caller's 0xA5: d_out_rgb was written before the memset queued on the stream"
        gpudev.same_bytes(got, want, "accum_hdr on a %s stream" % stream)
