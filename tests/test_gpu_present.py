"""pt_ctx_present on the GPU against tests/present_ref.py, the restatement of the contract in include/ptrace.h with Python
integers and numpy binary32 / binary64.  Every comparison is of bytes, for equality.  The frames are the smallest that reach every
path: the same-size stream (33 x 25: two workgroups would need 257 pixels - 825 gives four, with a tail), the two resampling
passes on shrinking, enlarging, an axis that keeps its size, one output pixel, several lanes per output pixel (130 -> 64 does not
group, 67 -> 1 does: 67 >= 8), and 257 x 129 -> 100 x 50, which spans several workgroups and a wave's tail.  The full-size cases
behind them cross what the small ones cannot: every `group` of the column pass, every grid-stride loop's second turn, gridDim.y's
cap, and sums of 2^53 and more; each asserts, from the launcher's rule restated here, that it takes the path it is there for."""
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


# ------------------------------------------------------------------------- full-size frames: every group, every grid wrap
# The launch rules of csrc/pt_present.hip, restated, so that each case below can assert that it reaches the path it is there for:
# a retune of the launcher then fails the premise instead of silently losing the coverage.
BLOCK, MAX_GRID, MAX_GRID_Y = 256, 2048, 32768  # kPresentBlock, kPresentMaxGrid, kPresentMaxGridY


def grid_for(n, per_block, cap=MAX_GRID):
    blocks = -(-n // per_block)
    if blocks <= 1:
        return 1
    turns = -(-blocks // cap)
    return -(-blocks // turns)


def turns_of(n, per_block):
    """how often the grid-stride loop over n items runs in the busiest workgroup"""
    return -(-n // (grid_for(n, per_block) * per_block))


def group_of(w, ow):
    """launch_present's lanes per output pixel: doubles while group * 8 * OW <= W, at most 64"""
    g = 1
    while g < 64 and g * 8 * ow <= w:
        g *= 2
    return g


@pytest.fixture(scope="module")
def bigdev(L):
    # the largest source is 4096 x 1024 (test_sums_beyond_2_53), the largest output 2100 x 1000 (test_same_size_grid_turns)
    with Dev(L, 4096 * 1024, 2100 * 1000) as d:
        yield d


# (W, H, OW, OH, group).  OW = 1: the widths 8..15, 16..31, ..., >= 256 give group 2, 4, ..., 64 in turn (g * 8 <= W); none is a
# multiple of its group, so the lanes of a group hold spans of different lengths and the last ones may hold nothing.  OW = 3:
# g * 24 <= W, 500 stops at 32 and 800 at 64.  Heights 1 to 3.
GROUPS = ((5, 1, 1, 1, 1), (13, 2, 1, 1, 2), (21, 3, 1, 2, 4), (45, 1, 1, 1, 8), (100, 2, 1, 1, 16), (200, 3, 1, 2, 32),
          (300, 1, 1, 1, 64), (500, 2, 3, 1, 32), (800, 3, 3, 2, 64))


@pytest.mark.parametrize("w,h,ow,oh,group", GROUPS, ids=["%dx%d->%dx%d:g%d" % c for c in GROUPS])
def test_every_group_of_the_column_pass(dev, table, w, h, ow, oh, group):
    assert group_of(w, ow) == group and (group == 1 or w % group != 0)
    frame = threshold_frame(table, np.random.default_rng(w * 1000 + ow), w * h)
    dev.put(frame)
    for flags in (0, FRAMEBUFFER_ORDER):
        want = ref.present(table, frame, w, h, ow, oh, flags=flags)  # the slow, independent form
        assert np.array_equal(want, ref.present(table, frame, w, h, ow, oh, flags=flags, separable=True))
        got = dev.present(w, h, ow, oh, flags=flags)
        assert np.array_equal(got, want), (flags, got.tolist(), want.tolist())
        assert np.array_equal(dev.present(w, h, ow, oh, fmt=RGB8, flags=flags), want[:, :, :3]), flags


def test_groups_cover_every_power_of_two():
    assert sorted({c[4] for c in GROUPS}) == [1, 2, 4, 8, 16, 32, 64]


# k_present_same's grid-stride loop takes a second turn above kPresentMaxGrid * kPresentBlock = 524 288 pixels:
# 1056 x 520 = 549 120 > 524 288 (two turns), 2100 x 1000 = 2 100 000 > 4 * 524 288 (five).  With `flip` the source index is
# npix - 1 - o, so both orders run.
@pytest.mark.parametrize("w,h,turns", [(1056, 520, 2), (2100, 1000, 5)], ids=["1056x520", "2100x1000"])
def test_same_size_grid_turns(L, bigdev, table, w, h, turns):
    npix = w * h
    assert npix > (turns - 1) * MAX_GRID * BLOCK and turns_of(npix, BLOCK) == turns
    frame = threshold_frame(table, np.random.default_rng(w), npix)
    bigdev.put(frame)
    host = ref.quantize_host(L, frame)  # the host instantiation of the kernel's per-value steps, in framebuffer order
    for flags in (0, FRAMEBUFFER_ORDER):
        want = ref.present(table, frame, w, h, flags=flags, separable=True)
        assert np.array_equal(want[:, :, :3].reshape(npix, 3), host if flags else host[::-1])
        for fmt in (RGBA8, RGB8):
            got = bigdev.present(w, h, fmt=fmt, flags=flags)
            exp = want if fmt == RGBA8 else want[:, :, :3]
            assert np.array_equal(got, exp), (flags, fmt, np.argwhere(got != exp)[:5])


# The two resampling kernels' loops wrapping, each case named by the constant it crosses:
# - "rows-y": OH = 40 000 > kPresentMaxGridY = 32 768, so gridDim.y is capped and both kernels' Y loops take a second turn;
# - "rows-x": W = 600 000 > kPresentMaxGrid * kPresentBlock = 524 288, k_present_rows' x loop takes a second turn; the column pass
#   runs at group 64 over spans of 600 columns;
# - "cols-x": OW = 600 000 > kPresentMaxGrid * (kPresentBlock / group) = 524 288 at group 1, k_present_cols' X loop takes a second
#   turn.
WRAPS = {"rows-y": ((3, 50000), (2, 40000)), "rows-x": ((600000, 2), (1000, 1)), "cols-x": ((4, 2), (600000, 1))}


@pytest.mark.parametrize("case", list(WRAPS))
def test_resampling_grid_wraps(bigdev, table, case):
    (w, h), (ow, oh) = WRAPS[case]
    group = group_of(w, ow)
    if case == "rows-y":
        assert oh > MAX_GRID_Y
    elif case == "rows-x":
        assert w > MAX_GRID * BLOCK and turns_of(w, BLOCK) == 2 and group == 64
    else:
        assert group == 1 and ow > MAX_GRID * BLOCK and turns_of(ow, BLOCK // group) == 2
    frame = threshold_frame(table, np.random.default_rng(w * 1000 + ow), w * h)
    bigdev.put(frame)
    for flags in (0, FRAMEBUFFER_ORDER):
        want = ref.present(table, frame, w, h, ow, oh, flags=flags, separable=True)
        got = bigdev.present(w, h, ow, oh, flags=flags)
        assert np.array_equal(got, want), (flags, np.argwhere(got != want)[:5])
        assert np.array_equal(bigdev.present(w, h, ow, oh, fmt=RGB8, flags=flags), want[:, :, :3]), flags


def test_sums_beyond_2_53(bigdev, table):
    """S >= 2^53, where present_mean's u64 -> binary64 conversion first rounds: it needs W*H*c > 2^21, here 4096 x 1024 = 2^22
    pixels of channels in [0.5, 1).  The premise is asserted on the restatement's integers: every output channel has S >= 2^53.
    These S are multiples of 2^8 - a value of [0.5, 1) has 24 bits, so its q = c * 2^32 ends in eight zeros - and binary64 holds
    each exactly: that the conversion really ROUNDS is test_conversion_of_sums_rounds_to_nearest_even's premise, on a frame built
    for it.  The same frame at constant 1.0 has S = W*H*2^32 exactly and the byte must be 255."""
    w, h = 4096, 1024
    npix = w * h
    rng = np.random.default_rng(53)
    frame = ref.bits_to_f32((0x3F000000 + rng.integers(0, 1 << 23, size=npix * 3)).astype(np.uint32)).reshape(npix, 3)
    assert frame.min() >= 0.5 and frame.max() < 1.0
    bigdev.put(frame)
    div = np.float64(npix) * np.float64(4294967296.0)
    for ow, oh in ((1, 1), (3, 2)):
        S = ref.sums_separable(frame, w, h, ow, oh)
        ints = [int(v) for v in S.ravel()]
        assert min(ints) >= 1 << 53 and max(ints) < 1 << 60
        want = ref.byte_sorted(table, (S.astype(np.float64) / div).astype(F32))
        for fmt in (RGBA8, RGB8):
            got = bigdev.present(w, h, ow, oh, fmt=fmt)
            assert np.array_equal(got[:, :, :3], want), (ow, oh, fmt, got.tolist(), want.tolist(), ints)
    bigdev.put(np.ones((npix, 3), dtype=F32))
    for ow, oh in ((1, 1), (3, 2)):
        assert (ref.sums_separable(np.ones((npix, 3), dtype=F32), w, h, ow, oh) == np.uint64(npix << 32)).all()
        assert (bigdev.present(w, h, ow, oh) == 255).all(), (ow, oh)


def frame_for_sums(targets, npix):
    """A frame of npix pixels whose channel c sums to targets[c] exactly in step 4's fixed point (one output pixel, every weight
    1): pixel 0 holds the target's low eight bits (j * 2^-32, j < 256), the others one of two neighbouring multiples of 2^-24."""
    out = np.zeros((npix, 3), dtype=F32)
    for c, target in enumerate(targets):
        j = target % 256
        rest = target - j
        qb = rest // (npix - 1) // 256 * 256
        more, left = divmod(rest - qb * (npix - 1), 256)
        assert left == 0 and 0 <= more <= npix - 1 and qb + 256 <= 1 << 32
        q = np.full(npix, qb, dtype=np.int64)
        q[1:1 + more] += 256
        q[0] = j
        assert int(q.sum()) == target
        out[:, c] = (q.astype(np.float64) / 4294967296.0).astype(F32)
        assert ((out[:, c].astype(np.float64) * 4294967296.0).astype(np.int64) == q).all()  # each value is held exactly
    return out


def test_conversion_of_sums_rounds_to_nearest_even(bigdev, table):
    """The contract's mean is (float)((double)S / divisor): S is rounded to binary64 FIRST, to nearest even, then divided, then
    rounded to binary32 - two roundings, on purpose.  At S >= 2^53 the first one is real, and this frame makes it decide a byte.
    4096 x 1024 -> 1 x 1, so the divisor is 2^54 and the division exact.  T[k] = M * 2^-24 is a threshold in [0.5, 1) with M
    even; tie = (M - 1/2) * 2^30 is the S halfway between T[k] and the float below it.
    - S = tie - 1 is odd, halfway between the binary64 values tie - 2 and tie: nearest even is tie, which then ties to T[k]:
      byte k.  A conversion that truncates gives tie - 2, and the exact quotient (one rounding) lies below the tie: both k - 1.
    - S = tie - 3 goes to tie - 4: byte k - 1.  A conversion that rounds halves up gives tie - 2, the same byte; one that rounds
      everything up gives tie - 2 as well.
    - S = tie + 1 goes to tie (nearest even, down): byte k.
    All of it is asserted on the restatement's integers before the device is asked."""
    w, h = 4096, 1024
    npix = w * h
    k = next(k for k in range(1, 256) if 0x3F000000 <= table[k] < ONE_BITS and table[k] % 2 == 0)
    M = (int(table[k]) & 0x7FFFFF) | 0x800000
    tie = (2 * M - 1) << 29
    targets = (tie - 1, tie - 3, tie + 1)
    frame = frame_for_sums(targets, npix)
    S = ref.sums_separable(frame, w, h, 1, 1)
    assert [int(v) for v in S.ravel()] == list(targets)
    assert all(1 << 53 <= v < 1 << 54 and int(float(v)) != v for v in targets)  # binary64 holds none of them: the conversion rounds
    assert [int(float(v)) for v in targets] == [tie, tie - 4, tie]
    want = ref.byte_sorted(table, (S.astype(np.float64) / (np.float64(npix) * np.float64(4294967296.0))).astype(F32))
    assert want.ravel().tolist() == [k, k - 1, k]
    once = ref.byte_sorted(table, np.array([float(np.float32(v / 2.0 ** 54)) for v in (tie - 2,)], dtype=F32))  # what truncating gives
    assert once.tolist() == [k - 1]
    bigdev.put(frame)
    for fmt in (RGBA8, RGB8):
        for flags in (0, FRAMEBUFFER_ORDER):
            got = bigdev.present(w, h, 1, 1, fmt=fmt, flags=flags)
            assert got[0, 0, :3].tolist() == [k, k - 1, k], (fmt, flags, got.tolist(), k)


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
