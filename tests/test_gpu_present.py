"""pt_ctx_present on the GPU against tests/present_ref.py, the restatement of the contract in include/ptrace.h with Python
integers and numpy binary32 / binary64.  Every comparison is of bytes, for equality.  The frames are the smallest that reach every
path: the same-size stream (33 x 25: two workgroups would need 257 pixels - 825 gives four, with a tail), the two resampling
passes on shrinking, enlarging, an axis that keeps its size, one output pixel, several lanes per output pixel (130 -> 64 does not
group, 67 -> 1 does: 67 >= 8), and 257 x 129 -> 100 x 50, which spans several workgroups and a wave's tail."""
import ctypes as C
import os

import numpy as np
import pytest

import gpudev
import present_ref as ref
import ptlib
from present_ref import F32, FRAMEBUFFER_ORDER, ONE_BITS, RGB8, RGBA8
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtPresentParams

pytestmark = pytest.mark.gpu

PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
GUARD = 64
RESAMPLE = (((7, 5), (3, 2)), ((8, 8), (4, 4)), ((7, 5), (7, 2)), ((5, 3), (11, 7)), ((67, 33), (1, 1)), ((130, 3), (64, 1)),
            ((257, 129), (100, 50)))


class Dev(gpudev.Device):
    """one context, a frame buffer and an output buffer with guard bytes behind whatever a call writes"""

    def __init__(self, L, max_pix=257 * 129, max_out=257 * 129):
        super().__init__(L)
        self.d_rgb, self.d_out = self.alloc(max_pix * 12), self.alloc(max_out * 4 + GUARD)

    def put(self, frame):
        self.upload(self.d_rgb, np.ascontiguousarray(frame, dtype=F32))

    def present(self, w, h, ow=0, oh=0, exposure=0.0, fmt=RGBA8, flags=0, stream=None, d_rgb=None, params=True):
        """the bytes the call wrote, (oh, ow, bpp); the guard behind them is checked on the way"""
        bpp = 4 if fmt == RGBA8 else 3
        n = (ow or w) * (oh or h) * bpp
        self.fill_guarded(self.d_out, n, GUARD, 0xA5, np.uint8)
        p = PtPresentParams(ow, oh, exposure, fmt, flags)
        rc = self.L.pt_ctx_present(self.ctx, w, h, C.byref(p) if params else None, d_rgb or self.d_rgb, self.d_out, stream)
        assert rc == 0, (rc, self.L.pt_last_error())
        return self.read_guarded(self.d_out, n, GUARD, 0xA5, "d_out", np.uint8).reshape(oh or h, ow or w, bpp)


@pytest.fixture(scope="module")
def table(L):
    return ref.thresholds(L)


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


def to_int(L, values):
    f = L.pt_to_int_with_gamma_correction
    v = np.asarray(values, dtype=F32)
    return np.array([f(float(x)) for x in v.ravel()], dtype=np.uint8).reshape(v.shape)


def threshold_frame(table, rng, npix):
    """npix x 3 values on both sides of the thresholds: a threshold's bit pattern moved by -2..2 ulps, and a tenth anywhere"""
    k = rng.integers(1, 256, size=npix * 3)
    bits = table[k].astype(np.int64) + rng.integers(-2, 3, size=npix * 3)
    v = ref.bits_to_f32(bits.astype(np.uint32)).copy()
    anywhere = rng.random(npix * 3) < 0.1
    v[anywhere] = (rng.random(int(anywhere.sum())) * 1.25 - 0.125).astype(F32)
    return v.reshape(npix, 3)


# -------------------------------------------------------------------------------------------------------- same size
def test_same_size_is_the_host_function_at_every_threshold(L, dev, table):
    w, h = 33, 25
    one = F32(1.0)
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 2.0 ** -33, 1.0, np.nextafter(one, F32(2)), 2.0, -1.0, np.inf, -np.inf,
                         np.nan, 3e38], dtype=F32)
    t = table[1:].astype(np.int64)
    bits = np.concatenate([t - 1, t, np.minimum(t + 1, 0x7F800000)]).astype(np.uint32)
    v = np.concatenate([ref.bits_to_f32(bits), specials])
    assert v.size <= w * h * 3
    frame = np.resize(v, w * h * 3).reshape(w * h, 3)
    dev.put(frame)
    want = to_int(L, frame)[::-1].reshape(h, w, 3)  # display order
    for fmt in (RGBA8, RGB8):
        got = dev.present(w, h, fmt=fmt)
        assert np.array_equal(got[:, :, :3], want), fmt
        assert np.array_equal(got, ref.present(table, frame, w, h, fmt=fmt)), fmt
        if fmt == RGBA8:
            assert (got[:, :, 3] == 255).all()
    # NULL params = all zero; out_width, out_height = the frame's own size is the same path
    assert np.array_equal(dev.present(w, h, params=False)[:, :, :3], want)
    assert np.array_equal(dev.present(w, h, w, h, fmt=RGB8), want)


def test_order(L, dev, table, tmp_path):
    w, h = 5, 3
    frame = ((np.arange(w * h * 3, dtype=F32) + F32(0.5)) / F32(w * h * 3)).reshape(w * h, 3)
    dev.put(frame)
    got = dev.present(w, h, fmt=RGB8)
    host = to_int(L, frame)
    assert len({tuple(px) for px in host.tolist()}) == w * h  # distinct pixels: a wrong order cannot hide
    for y in range(h):
        for x in range(w):
            assert np.array_equal(got[y, x], host[w * h - 1 - (y * w + x)]), (x, y)
    path = tmp_path / "f.ppm"
    assert L.pt_write_ppm(os.fsencode(str(path)), frame.ctypes.data_as(C.POINTER(C.c_float)), w, h, 1, b"order", 0) == 0
    assert np.array_equal(got, ref.read_p3(str(path)))
    got = dev.present(w, h, fmt=RGB8, flags=FRAMEBUFFER_ORDER)
    assert np.array_equal(got, host.reshape(h, w, 3))
    # ... and the same two orders through the resampling form
    for flags in (0, FRAMEBUFFER_ORDER):
        assert np.array_equal(dev.present(w, h, 3, 2, fmt=RGB8, flags=flags), ref.present(table, frame, w, h, 3, 2, fmt=RGB8, flags=flags))


# ------------------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("src,dst", RESAMPLE)
def test_resampling_is_the_restatement(dev, table, src, dst):
    (w, h), (ow, oh) = src, dst
    frame = threshold_frame(table, np.random.default_rng(w * 1000 + ow), w * h)
    dev.put(frame)
    want = ref.present(table, frame, w, h, ow, oh)
    got = dev.present(w, h, ow, oh)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(dev.present(w, h, ow, oh, fmt=RGB8), want[:, :, :3])


def test_resampling_a_constant_frame_lands_on_the_thresholds(dev, table):
    """T[k] in every pixel averages to T[k] exactly (its 24 bits survive the 32.32 fixed point for k >= 2^-8's); the float below
    it to the byte below"""
    w, h, ow, oh = 7, 5, 3, 2
    for k in (40, 128, 255):
        for d, want in ((0, k), (-1, k - 1)):
            c = ref.bits_to_f32([int(table[k]) + d])[0]
            assert c >= 2.0 ** -8
            dev.put(np.full((w * h, 3), c, dtype=F32))
            assert (dev.present(w, h, ow, oh, fmt=RGB8) == want).all(), (k, d)


# --------------------------------------------------------------------------------------------------------- exposure
def test_exposure(L, dev, table):
    w, h = 9, 7
    rng = np.random.default_rng(5)
    frame = threshold_frame(table, rng, w * h)
    frame[:4] = [[1e-8, -1e-8, 0.0], [3e38, -3e38, 1.0], [np.inf, -np.inf, np.nan], [0.5, 0.25, 2.0]]
    dev.put(frame)
    same = dev.present(w, h, exposure=0.0)
    assert np.array_equal(same, dev.present(w, h, exposure=1.0))
    for e in (2.0, 0.5, 1e30):
        assert np.array_equal(dev.present(w, h, exposure=e), ref.present(table, frame, w, h, exposure=e)), e
        assert np.array_equal(dev.present(w, h, 4, 3, exposure=e), ref.present(table, frame, w, h, 4, 3, exposure=e)), e
    big = dev.present(w, h, exposure=1e30, fmt=RGB8, flags=FRAMEBUFFER_ORDER).reshape(w * h, 3)
    assert big[0].tolist() == [255, 0, 0] and big[1].tolist() == [255, 0, 255] and big[2].tolist() == [255, 0, 0]
    for bad in (-1.0, float("inf"), float("nan")):
        p = PtPresentParams(0, 0, bad, 0, 0)
        assert L.pt_ctx_present(dev.ctx, w, h, C.byref(p), dev.d_rgb, dev.d_out, None) == PT_ERR_INVALID


# ---------------------------------------------------------------------------------------------- boundaries, streams
def test_streams_and_repeats(dev, table):
    w, h = 67, 33
    frame = threshold_frame(table, np.random.default_rng(11), w * h)
    dev.put(frame)
    with dev.stream() as st:
        for ow, oh, fmt in ((0, 0, RGBA8), (0, 0, RGB8), (31, 9, RGBA8), (31, 9, RGB8), (1, 1, RGB8)):
            a = dev.present(w, h, ow, oh, fmt=fmt)  # (the guard bytes behind d_out are checked by every call)
            assert np.array_equal(a, dev.present(w, h, ow, oh, fmt=fmt, stream=st)), (ow, oh, fmt)
            assert np.array_equal(a, dev.present(w, h, ow, oh, fmt=fmt)), (ow, oh, fmt)


# ---------------------------------------------------------------------------------------------------- no state touched
def test_leaves_the_context_alone(L, table):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    w, h = 32, 24
    with Dev(L, w * h, w * h) as d:
        d.set_scene(sc)
        cfg = gpudev.config(w, h, 4, seed=3)
        d.render(cfg, d.d_rgb, accumulate=True)
        d_dn = d.alloc(w * h * 12)

        def info():
            lo, hi = C.c_uint32(), C.c_uint32()
            assert L.pt_ctx_accum_info(d.ctx, C.byref(cfg), C.byref(lo), C.byref(hi)) == 0
            return lo.value, hi.value

        def denoise():
            assert L.pt_ctx_denoise(d.ctx, w, h, None, d.d_rgb, None, None, None, d_dn, None) == 0, L.pt_last_error()
            return d.download(d_dn, w * h * 12, np.uint8)

        before, dn_before = info(), denoise()
        assert before == (4, 4)
        frame = d.pixels(d.d_rgb, w * h)
        assert np.array_equal(d.present(w, h, 13, 5), ref.present(table, frame, w, h, 13, 5))
        assert np.array_equal(d.present(w, h), ref.present(table, frame, w, h))
        assert info() == before
        assert np.array_equal(denoise(), dn_before)
        assert np.array_equal(d.pixels(d.d_rgb, w * h), frame)  # the frame itself is read only


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_render_present_and_callback(L, table, tmp_path):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    w, h, spp = 64, 48, 8
    with Dev(L, w * h, w * h) as d:
        d_snap = d.alloc(w * h * 12)
        d.set_scene(sc)
        seen = []

        def on_progress(user, frac):
            n = C.c_uint32()
            if seen or L.pt_ctx_snapshot(d.ctx, d_snap, C.byref(n)) != 0:
                return
            p = PtPresentParams(32, 24, 0.0, RGB8, 0)
            rc = L.pt_ctx_present(d.ctx, w, h, C.byref(p), d_snap, d.d_out, None)
            seen.append((rc, n.value, d.pixels(d_snap, w * h), d.download(d.d_out, 32 * 24 * 3, np.uint8)))

        cb = ptlib.PROGRESS_FN(on_progress)
        cfg = gpudev.config(w, h, spp, seed=8, rays_per_pass=1)  # passes of one sample: the callback fires between them
        cfg.progress_ms = ptlib.PROGRESS_EVERY_PASS
        frame, _ = d.render(cfg, d.d_rgb, cb=cb)
        assert len(seen) == 1
        rc, n, snap, got = seen[0]
        assert rc == 0 and 1 <= n <= spp
        assert np.array_equal(got.reshape(24, 32, 3), ref.present(table, snap.reshape(w * h, 3), w, h, 32, 24, fmt=RGB8))
        # the finished frame
        path = tmp_path / "f.ppm"
        assert L.pt_write_ppm(os.fsencode(str(path)), frame.ctypes.data_as(C.POINTER(C.c_float)), w, h, spp, b"cornell", 0) == 0
        assert np.array_equal(d.present(w, h, fmt=RGB8), ref.read_p3(str(path)))
        assert np.array_equal(d.present(w, h, 32, 24), ref.present(table, frame, w, h, 32, 24))
