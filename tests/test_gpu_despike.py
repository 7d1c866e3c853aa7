"""pt_ctx_despike on the GPU against tests/despike_ref.py, the restatement of include/ptrace_despike.h in numpy.  Every
comparison is of bits or of integer counts, for equality.

The kernel's unit is a workgroup per tile of 32 x 8 pixels with a halo of `radius` in LDS, so the frames (despike_frames.py) are
1x1, 1x7 and 7x1 (no neighbour, one axis), 31x7 (less than a tile), 32x8 (one), 33x9 (one pixel and one row more: four tiles),
64x16, 67x19 and 96x64 (seams on every side, a tail), each at both radii, ranks 1..4, with and without the flag (ids: a random
three-colour Voronoi map with misses), with and without d_mask and `out`, and with the planes 4 bytes off.  One frame of
1024x768 with a thousand plants catches grid arithmetic.  On a background in [0.5, 1] and threshold 2 the clipped set is the
planted set where the header says so.

The stream contract: the trap of tests/test_gpu_streams.py rebuilt on gpudev.Gate - the caller's stream is held by a gate, behind
it wait the copy of the real input over a decoy and a memset of the output; a call that is ordered on the stream reads the real
input and writes over the memset, and has not returned while the gate holds.

End to end: cornell at 96x64 and 16 samples through pt_ctx_accumulate -> pt_ctx_accum_hdr -> pt_ctx_despike."""
import ctypes as C

import numpy as np
import pytest

import despike_frames as frames
import despike_ref as ref
import gpudev
import ptlib
from despike_ref import F32, I32, U32
from gpudev import L  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

da = ref.despike_abi
GUARD = 64  # floats (bytes of the mask) before and behind an output
SENTINEL, MASK_SENTINEL = F32(-7.5), 0xEE
MAX_PIX = 96 * 64
T, FLOOR = 2.0, 0.25  # the tests' threshold and floor: the background cannot spike at a threshold >= 2


class Dev(gpudev.Device):
    def __init__(self, L, max_pix=MAX_PIX):
        super().__init__(L)
        room = (max_pix * 3 + 2 * GUARD + 8) * 4
        self.rgb, self.out = self.alloc(room), self.alloc(room)
        self.ids, self.mask = self.alloc(max_pix * 4 + 64), self.alloc(max_pix + 2 * GUARD + 8)

    def despike(self, w, h, rgb, params, ids=None, mask=True, stats=True, off_in=0, off_out=0, off_mask=0, stream=None):
        """(out (w*h, 3) float32, mask or None, (pixels, spikes, nonfinite) or None); the guards around both outputs are checked,
        and the input"""
        n = w * h
        src = np.concatenate([np.full(GUARD, SENTINEL, dtype=F32), rgb.reshape(-1), np.full(GUARD, SENTINEL, dtype=F32)])
        self.upload(self.rgb, src, offset=off_in)
        self.upload(self.out, np.full(n * 3 + 2 * GUARD, SENTINEL, dtype=F32), offset=off_out)
        self.upload(self.mask, np.full(n + 2 * GUARD, MASK_SENTINEL, dtype=np.uint8), offset=off_mask)
        if ids is not None:
            self.upload(self.ids, np.ascontiguousarray(ids, dtype=I32), offset=off_in)
        st = da.pt_despike_stats(99, 99, 99)
        rc = self.L.pt_ctx_despike(self.ctx, w, h, C.byref(params) if params is not None else None,
                                   C.c_void_p(self.rgb.value + off_in + GUARD * 4),
                                   C.c_void_p(self.ids.value + off_in) if ids is not None else None,
                                   C.c_void_p(self.out.value + off_out + GUARD * 4),
                                   C.c_void_p(self.mask.value + off_mask + GUARD) if mask else None,
                                   C.byref(st) if stats else None, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.download(self.out, n * 3 + 2 * GUARD, offset=off_out)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n * 3:] == SENTINEL).all(), "d_out was written outside its %d floats" % (n * 3)
        m = self.download(self.mask, n + 2 * GUARD, dtype=np.uint8, offset=off_mask)
        assert (m[:GUARD] == MASK_SENTINEL).all() and (m[GUARD + n:] == MASK_SENTINEL).all(), "d_mask was written outside its %d bytes" % n
        if not mask:
            assert (m == MASK_SENTINEL).all(), "a mask was written without d_mask"
        assert self.download(self.rgb, src.size, offset=off_in).tobytes() == src.tobytes(), "d_rgb was written"
        return (got[GUARD:GUARD + n * 3].reshape(-1, 3), m[GUARD:GUARD + n] if mask else None,
                (st.pixels, st.spikes, st.nonfinite) if stats else None)


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


def same(got, want, what):
    out, mask, st = got
    wout, wmask, wst = want
    gpudev.same_bytes(out.view(U32), wout.view(U32), what + ": d_out")
    if mask is not None:
        gpudev.same_bytes(mask, wmask, what + ": d_mask")
    if st is not None:
        assert st == wst, (what, st, wst)


# -------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("size", frames.SIZES, ids=["%dx%d" % s for s in frames.SIZES])
def test_despike_is_the_restatement(dev, size):
    w, h = size
    rgb, ids, plan = frames.planted(w, h)
    if w * h >= 96 * 64:
        assert all(len(v) for v in plan.values())  # everything is planted in the largest frame
    for radius, rank, flag in frames.COMBOS:
        p = da.pt_despike_params(radius, rank, flag, T, FLOOR)
        i = ids if flag else None
        want = ref.despike(rgb, w, h, radius, rank, flag, T, FLOOR, ids)
        what = "%dx%d radius %d rank %d flag %d" % (w, h, radius, rank, flag)
        same(dev.despike(w, h, rgb, p, i), want, what)
        same(dev.despike(w, h, rgb, p, i), want, what + ", again: the counters were cleared")
        # without the mask, without the stats, without both: the frame's bytes are the same
        same(dev.despike(w, h, rgb, p, i, mask=False), want, what + ", no mask")
        same(dev.despike(w, h, rgb, p, i, stats=False), want, what + ", no stats")
        same(dev.despike(w, h, rgb, p, i, mask=False, stats=False), want, what + ", neither")
        # planes that are only 4-byte aligned (the mask: 1-byte): the same bytes
        same(dev.despike(w, h, rgb, p, i, off_in=4), want, what + ", d_rgb and ids 4 bytes off")
        same(dev.despike(w, h, rgb, p, i, off_out=4, off_mask=1), want, what + ", d_out 4 bytes off, d_mask 1")
        same(dev.despike(w, h, rgb, p, i, off_in=8, off_out=12, off_mask=3), want, what + ", 8 and 12 bytes off")


def test_the_clipped_set_is_the_planted_set(dev):
    w, h = 96, 64
    rgb, ids, plan = frames.planted(w, h)
    for rank in (1, 2):
        out, mask, st = dev.despike(w, h, rgb, da.pt_despike_params(1, rank, 0, T, FLOOR))
        clipped = set(np.flatnonzero(mask == 1).tolist())
        want = set(plan["isolated"]) | (set(plan["pairs"]) | set(plan["line_ends"]) if rank == 2 else set())
        assert clipped == want, (rank, sorted(clipped ^ want))
        assert set(np.flatnonzero(mask == 2).tolist()) == set(plan["nonfinite"])
        assert st == (w * h, len(want), len(plan["nonfinite"]))
        inner = sorted(set(plan["line"]) - set(plan["line_ends"]))
        gpudev.same_bytes(out[inner], rgb[inner], "the line's inner pixels survive")
        assert (out[plan["nonfinite"]].view(U32) == 0).all()  # +0 in every channel
        untouched = np.setdiff1d(np.arange(w * h), sorted(want | set(plan["nonfinite"])))
        gpudev.same_bytes(out[untouched].view(U32), rgb[untouched].view(U32), "every other pixel keeps its bits, a -0 among them")
        # a clipped pixel lands on its limit: far below the spike, at or above the floor
        y = ref.luma(out[sorted(want)])
        assert (y >= FLOOR).all() and (y <= T * 1.0 + FLOOR + 1e-4).all()


def test_defaults_one_colour_and_the_early_out(dev):
    w, h = 67, 19
    rgb, ids, _ = frames.planted(w, h)
    same(dev.despike(w, h, rgb, None), ref.despike(rgb, w, h), "NULL params")
    d = da.pt_despike_params()
    assert dev.L.pt_despike_defaults(C.byref(d)) == 0 and (d.radius, d.rank, d.flags, d.threshold, d.floor) == (1, 3, 0, 2.0, 0.25)
    one = np.tile(np.array((0.3, 7.0, 2.0), dtype=F32), (w * h, 1))
    out, mask, st = dev.despike(w, h, one, da.pt_despike_params(2, 3, 0, 1.0, 0.0))
    assert out.tobytes() == one.tobytes() and not mask.any() and st == (w * h, 0, 0)
    # a floor above every pixel but the non-finite ones: every wave takes the early-out, and the bytes are the window's
    dim = np.where(np.isfinite(rgb), np.minimum(rgb, F32(1)), rgb).astype(F32)
    for radius, rank in ((1, 1), (2, 4)):
        want = ref.despike(dim, w, h, radius, rank, 0, T, 8.0)
        assert want[2][1] == 0 and want[2][2] > 0
        same(dev.despike(w, h, dim, da.pt_despike_params(radius, rank, 0, T, 8.0)), want, "floor 8, radius %d" % radius)
    # one pixel above the floor in an otherwise dim frame: its wave alone runs the window
    dim[5 * w + 40] = 600.0
    want = ref.despike(dim, w, h, 1, 1, 0, T, 8.0)
    assert want[2][1] == 1
    same(dev.despike(w, h, dim, da.pt_despike_params(1, 1, 0, T, 8.0)), want, "one candidate")


def test_a_large_frame(L):
    """1024 x 768: 3072 tiles, a thousand plants"""
    w, h = 1024, 768
    rgb, ids, at = frames.scattered(w, h, 1000, seed=3)
    with Dev(L, w * h) as d:
        for radius, rank, flag in ((1, 2, 0), (2, 4, 1)):
            want = ref.despike(rgb, w, h, radius, rank, flag, T, FLOOR, ids)
            assert want[2][1] > 300 and want[2][2] > 100
            if not flag:
                assert set(np.flatnonzero(want[1]).tolist()) <= set(at.tolist())
            same(d.despike(w, h, rgb, da.pt_despike_params(radius, rank, flag, T, FLOOR), ids if flag else None), want,
                 "1024x768 radius %d rank %d flag %d" % (radius, rank, flag))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_outputs(dev):
    w, h = 33, 9
    n = w * h
    rgb, ids, _ = frames.planted(w, h)
    dev.upload(dev.rgb, rgb)
    dev.upload(dev.ids, ids)
    dev.upload(dev.out, np.full(n * 3, SENTINEL, dtype=F32))
    dev.upload(dev.mask, np.full(n, MASK_SENTINEL, dtype=np.uint8))
    st = da.pt_despike_stats(77, 77, 77)
    P = da.pt_despike_params
    nan, inf = float("nan"), float("inf")
    ok = P(1, 2, 0, T, FLOOR)
    cases = [(P(0, 2, 0, T, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "radius"), (P(3, 2, 0, T, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "radius"),
             (P(1, 0, 0, T, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "rank"), (P(2, 5, 0, T, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "rank"),
             (P(1, 2, 2, T, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "flags"), (P(1, 2, 0, 0.5, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "threshold"),
             (P(1, 2, 0, nan, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "threshold"), (P(1, 2, 0, inf, FLOOR), w, h, dev.rgb, dev.ids, dev.out, "threshold"),
             (P(1, 2, 0, T, -1.0), w, h, dev.rgb, dev.ids, dev.out, "floor"), (P(1, 2, 0, T, nan), w, h, dev.rgb, dev.ids, dev.out, "floor"),
             (ok, 0, h, dev.rgb, dev.ids, dev.out, "width and height"), (ok, w, 0, dev.rgb, dev.ids, dev.out, "width and height"),
             (ok, 1 << 15, 1 << 15, dev.rgb, dev.ids, dev.out, "2^28"), (ok, w, h, None, dev.ids, dev.out, "d_rgb"),
             (ok, w, h, dev.rgb, dev.ids, None, "d_out is NULL"), (ok, w, h, dev.out, dev.ids, dev.out, "d_out is d_rgb"),
             (P(1, 2, 1, T, FLOOR), w, h, dev.rgb, None, dev.out, "d_object_id")]
    for i, (p, cw, ch, src, idp, dst, word) in enumerate(cases):
        rc = dev.L.pt_ctx_despike(dev.ctx, cw, ch, C.byref(p), src, idp, dst, dev.mask, C.byref(st), None)
        assert rc == ptlib.abi.PT_ERR_INVALID and word in dev.L.pt_last_error().decode(), (i, rc, dev.L.pt_last_error())
    assert dev.L.pt_ctx_despike(None, w, h, C.byref(ok), dev.rgb, dev.ids, dev.out, dev.mask, C.byref(st), None) == ptlib.abi.PT_ERR_INVALID
    assert (dev.download(dev.out, n * 3) == SENTINEL).all() and (dev.download(dev.mask, n, dtype=np.uint8) == MASK_SENTINEL).all()
    assert (st.pixels, st.spikes, st.nonfinite) == (77, 77, 77)
    gpudev.same_bytes(dev.download(dev.rgb, n * 3).reshape(-1, 3), rgb, "d_rgb")


# ------------------------------------------------------------------------------------------------------------ streams
FILL = 0xA5
D2D = 3


def trapped(dev, A, call, inp, real, decoy, outp, out_bytes, T=0.05):
    """the call made on the gated stream A: behind the gate wait the copy of `real` over the decoy in `inp` and a memset of `outp`
    to 0xA5.  Returns what call(A) returned, once the gate has been seen finished at the call's return."""
    hip = gpudev.hip_runtime()
    staged = dev.alloc(real.nbytes)
    dev.upload(staged, real)
    dev.upload(inp, decoy)
    gate = gpudev.Gate(A)
    try:
        assert hip.hipMemcpyAsync(inp, staged, real.nbytes, D2D, A) == 0
        assert hip.hipMemsetAsync(outp, FILL, out_bytes, A) == 0
        gate.open_after(T)
        res = call(A)
        finished, timed_out = gate.finished, gate.timed_out
    finally:
        gate.close()
        assert hip.hipStreamSynchronize(A) == 0
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
def test_despike_is_ordered_on_the_callers_stream(dev, streams, stream):
    w, h = 67, 19
    n = w * h
    real, _, _ = frames.planted(w, h)
    decoy, _, _ = frames.planted(w, h, seed=5)
    decoy[::7] = 300.0
    p = da.pt_despike_params(2, 2, 0, T, FLOOR)
    want, wrong = ref.despike(real, w, h, 2, 2, 0, T, FLOOR), ref.despike(decoy, w, h, 2, 2, 0, T, FLOOR)
    assert want[0].tobytes() != wrong[0].tobytes() and want[2] != wrong[2]

    def call(A):
        st = da.pt_despike_stats()
        rc = dev.L.pt_ctx_despike(dev.ctx, w, h, C.byref(p), dev.rgb, None, dev.out, dev.mask, C.byref(st), A)
        assert rc == 0, (rc, dev.L.pt_last_error())
        return dev.download(dev.out, n * 3).reshape(-1, 3), dev.download(dev.mask, n, dtype=np.uint8), (st.pixels, st.spikes, st.nonfinite)

    dev.upload(dev.rgb, real)
    same(call(None), want, "NULL stream")
    got = trapped(dev, streams[stream], call, dev.rgb, real, decoy, dev.out, n * 12)
    assert got[0].tobytes() != wrong[0].tobytes(), "the decoy's result: d_rgb was read before the caller's copy on the stream"
    assert not (got[0].view(np.uint8) == FILL).all(), "the caller's 0xA5: d_out was written before the memset queued on the stream"
    same(got, want, "despike on a %s stream" % stream)


# --------------------------------------------------------------------------------------------------------- end to end
def test_cornell_through_accumulate_hdr_despike(L):
    w, h, spp = 96, 64, 16
    n = w * h
    sc = gpudev.scene("cornell")
    with gpudev.Device(L, sc) as d:
        frame, hdr, out, mask = d.alloc(n * 12), d.alloc(n * 12), d.alloc(n * 12), d.alloc(n)
        cfg = gpudev.config(w, h, spp, seed=9)
        clamped, _ = d.render(cfg, frame, accumulate=True)
        assert L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), hdr, None) == 0, L.pt_last_error()
        src = d.pixels(hdr, n)
        gpudev.same_bytes(np.clip(src, F32(0), F32(1)), clamped, "the HDR frame's clamp is pt_ctx_accumulate's frame")
        for p in (None, da.pt_despike_params(2, 2, 0, 2.0, 0.25)):
            st = da.pt_despike_stats()
            assert L.pt_ctx_despike(d.ctx, w, h, C.byref(p) if p is not None else None, hdr, None, out, mask, C.byref(st), None) == 0, L.pt_last_error()
            want = ref.despike(src, w, h) if p is None else ref.despike(src, w, h, 2, 2, 0, 2.0, 0.25)
            same((d.pixels(out, n), d.download(mask, n, dtype=np.uint8), (st.pixels, st.spikes, st.nonfinite)), want, "cornell")
        # the call read the frame and changed nothing that is held or was handed out
        gpudev.same_bytes(d.pixels(frame, n), clamped, "pt_ctx_accumulate's output")
        gpudev.same_bytes(d.pixels(hdr, n), src, "the HDR frame")
        assert L.pt_ctx_accum_hdr(d.ctx, C.byref(cfg), out, None) == 0
        gpudev.same_bytes(d.pixels(out, n), src, "the held frame, resolved again")
