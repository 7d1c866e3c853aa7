"""pt_ctx_overlay on the GPU against tests/overlay_ref.py, the restatement of the contract in
include/ptrace_overlay.h in numpy binary32.
Every comparison is of bits, for equality.  The frames are the smallest that reach every path of the kernel's 32 x 8 tiles:
1 x 1, 31 x 7 (inside one tile), 33 x 9 (one past a tile on both axes: four workgroups, three of them slivers) and 64 x 16 (2 x 2
whole tiles); the sky and the grid run at 48 x 32.  Out of place the output carries a guard behind it, in place the frame does."""
import ctypes as C

import numpy as np
import pytest

import gpudev
import overlay_ref as ref
import present_ref
import ptlib
from gpudev import L  # noqa: F401  (fixture)
from overlay_ref import F32, GRID, I32, SKY
from ptlib import PtPresentParams
from reproject_ref import cam_dict

pytestmark = pytest.mark.gpu

GUARD = 96
SENTINEL = F32(-7.5)
SIZES = ((1, 1), (31, 7), (33, 9), (64, 16))
TILE_W, TILE_H = 32, 8  # kOverlayTileW, kOverlayTileH
ABOVE = dict(position=(0.5, 3.0, 4.0), direction=(-0.1, -0.6, -0.79), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
BELOW = dict(position=(0.5, -3.0, 4.0), direction=(0.0, -0.6, -0.8), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
TILTED = dict(position=(1.0, 0.25, 6.0), direction=(-0.15, 0.0, -0.98), focal_length=0.035, sensor_width=0.036, aspect_ratio=1.5)
OUTLINE = dict(outline_color=(0.0, 1.0, 0.0), fill_color=(1.0, 0.5, 0.0))
SPECIAL_BITS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000], dtype=np.uint32)


class Dev(gpudev.Device):
    """one context and the planes of a call: the frame and the output with guard floats behind what a call may write"""

    def __init__(self, L, max_pix=64 * 48):
        super().__init__(L)
        self.d_rgb, self.d_out = self.alloc((max_pix * 3 + GUARD) * 4), self.alloc((max_pix * 3 + GUARD) * 4)
        self.d_id, self.d_z = self.alloc(max_pix * 4), self.alloc(max_pix * 4)

    def overlay(self, w, h, p, cam, rgb, oid=None, z=None, in_place=False, pass_planes=True):
        """the (w*h, 3) frame the call wrote, as uint32 bits; the guard behind it is checked on the way.  p None: params NULL."""
        n = w * h * 3
        self.upload(self.d_rgb, np.ascontiguousarray(rgb, dtype=F32))
        self.fill_guarded(self.d_rgb, n, GUARD, SENTINEL, tail_only=True)
        if oid is not None:
            self.upload(self.d_id, np.ascontiguousarray(oid, dtype=I32))
        if z is not None:
            self.upload(self.d_z, np.ascontiguousarray(z, dtype=F32))
        d_out = self.d_rgb if in_place else self.d_out
        if not in_place:
            self.fill_guarded(self.d_out, n, GUARD, SENTINEL)
        s = ref.struct(p) if p is not None else None
        c = ref.pt_camera(cam) if cam is not None else None
        rc = self.L.pt_ctx_overlay(self.ctx, w, h, C.byref(s) if s is not None else None, C.byref(c) if c is not None else None, self.d_rgb,
                                   self.d_id if oid is not None and pass_planes else None, self.d_z if z is not None and pass_planes else None,
                                   d_out)
        assert rc == 0, (rc, self.L.pt_last_error())
        got = self.read_guarded(d_out, n, GUARD, SENTINEL, "d_out").reshape(w * h, 3)
        if not in_place:  # the input is read only
            assert self.download(self.d_rgb, n).tobytes() == np.ascontiguousarray(rgb, dtype=F32).tobytes()
        return got.view(np.uint32)

    def both(self, w, h, p, cam, rgb, oid=None, z=None):
        """out of place, then in place: the same bits"""
        a = self.overlay(w, h, p, cam, rgb, oid, z)
        b = self.overlay(w, h, p, cam, rgb, oid, z, in_place=True)
        gpudev.same_bytes(b, a, "in place vs out of place")
        return a


@pytest.fixture(scope="module")
def dev(L):
    with Dev(L) as d:
        yield d


def frame(rng, n, specials=True):
    rgb = rng.random((n, 3)).astype(F32)
    if specials:  # NaN payloads, -0, a denormal, infinities
        pick = rng.random((n, 3)) < 0.1
        rgb.view(np.uint32)[pick] = rng.choice(SPECIAL_BITS, size=int(pick.sum()))
    return rgb


def check(dev, w, h, p, cam, rgb, oid=None, z=None):
    """device == restatement, bit for bit, both ways of running it; untouched pixels keep their input's bits.  -> touched"""
    want, touched = ref.overlay(w, h, p, cam, rgb, oid, z)
    got = dev.both(w, h, p, cam, rgb, oid, z)
    gpudev.same_bytes(got, want.view(np.uint32), "%dx%d" % (w, h))
    assert (got[~touched] == np.ascontiguousarray(rgb, dtype=F32).view(np.uint32)[~touched]).all()
    return touched


def single(w, h, x, r, obj=1):
    oid = np.zeros((h, w), dtype=I32)
    oid[r, x] = obj
    return oid.reshape(w * h)


# ------------------------------------------------------------------------------------------------------- selections
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_random_selection_at_every_size(dev, w, h):
    rng = np.random.default_rng(w * 100 + h)
    oid = rng.integers(-1, 5, size=w * h).astype(I32)
    oid[rng.random(w * h) < 0.92] = 0  # most pixels belong to an object that is not selected
    rgb = frame(rng, w * h)
    for fill in (0.0, 0.25):
        for radius in (0, 3):
            p = ref.params(selected=(1, 3), radius=radius, outline_alpha=0.75, fill_alpha=fill, **OUTLINE)
            touched = check(dev, w, h, p, None, rgb, oid)
            if w * h > 1:
                assert touched.any() and not touched.all()
    # the one pixel of the 1 x 1 frame, selected: no outline anywhere, the fill alone
    if (w, h) == (1, 1):
        p = ref.params(selected=(2,), fill_alpha=1.0, **OUTLINE)
        got = dev.both(1, 1, p, None, rgb, np.array([2], dtype=I32))
        assert got.view(F32).tolist() == [[1.0, 0.5, 0.0]]


@pytest.mark.parametrize("w,h", SIZES[1:], ids=["%dx%d" % s for s in SIZES[1:]])
def test_a_selected_pixel_in_each_corner_at_the_largest_radius(dev, w, h):
    """the halo of 8 lies outside the frame on two sides of every corner"""
    rgb = frame(np.random.default_rng(w), w * h)
    p = ref.params(selected=(1,), radius=8, **OUTLINE)
    for x, r in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        touched = check(dev, w, h, p, None, rgb, single(w, h, x, r)).reshape(h, w)
        box = np.zeros((h, w), dtype=bool)
        box[max(r - 8, 0):r + 9, max(x - 8, 0):x + 9] = True
        box[r, x] = False  # the object's own pixel keeps its colour
        assert np.array_equal(touched, box), (x, r)


@pytest.mark.parametrize("radius", [1, 2, 3, 8])
def test_neighbours_in_the_next_tile_at_distance_r_and_r_plus_1(dev, radius):
    """64 x 16 is 2 x 2 tiles.  A selected pixel R short of the tile's edge: the first column, row and corner pixel of the next tiles
    are at distance exactly R and outlined, the ones behind them at R + 1 and not.  And the mirror image from the last tile."""
    w, h, R = 64, 16, radius
    rgb = frame(np.random.default_rng(R), w * h, specials=False)
    p = ref.params(selected=(1,), radius=R, **OUTLINE)
    for (x, r), (ex, er), (fx, fr) in (((TILE_W - R, TILE_H - R), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1)),
                                       ((TILE_W - 1 + R, TILE_H - 1 + R), (TILE_W - 1, TILE_H - 1), (TILE_W - 2, TILE_H - 2))):
        touched = check(dev, w, h, p, None, rgb, single(w, h, x, r)).reshape(h, w)
        got = dev.overlay(w, h, p, None, rgb, single(w, h, x, r)).view(F32).reshape(h, w, 3)
        for qx, qr in ((ex, r), (x, er), (ex, er)):  # on the row's axis, on the column's, on the diagonal: distance R
            assert touched[qr, qx] and got[qr, qx].tolist() == [0.0, 1.0, 0.0], (qx, qr)
        for qx, qr in ((fx, r), (x, fr), (fx, fr), (fx, er), (ex, fr)):  # R + 1
            assert not touched[qr, qx] and np.array_equal(got[qr, qx], rgb.reshape(h, w, 3)[qr, qx]), (qx, qr)


def test_a_tile_without_a_selected_pixel_whose_halo_holds_one(dev):
    """the early-out's trap: the vote has to ask the halo too"""
    w, h = 64, 16
    rgb = frame(np.random.default_rng(3), w * h)
    p = ref.params(selected=(1,), radius=2, **OUTLINE)
    for x, r, tile in ((TILE_W, 0, (0, 0)), (TILE_W - 1, TILE_H, (0, 0)), (TILE_W, TILE_H, (0, 0)), (TILE_W - 1, TILE_H - 1, (1, 1)),
                       (TILE_W - 1, TILE_H, (1, 0))):
        oid = single(w, h, x, r)
        tx, ty = tile
        inside = np.zeros((h, w), dtype=bool)
        inside[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W] = True
        assert not (ref.mask(oid, (1,)).reshape(h, w) & inside).any()  # the tile holds no selected pixel ...
        touched = check(dev, w, h, p, None, rgb, oid).reshape(h, w)
        assert (touched & inside).any(), (x, r, tile)  # ... and some of its pixels are outlined


def test_sixteen_ids_and_a_plane_of_misses(dev):
    w, h = 33, 9
    rng = np.random.default_rng(16)
    rgb = frame(rng, w * h)
    listed = tuple(range(3, 18)) + (70000,)  # one far above any id of the plane
    assert len(listed) == ref.MAX_SELECTED
    p = ref.params(selected=listed, radius=2, fill_alpha=0.5, **OUTLINE)
    oid = rng.integers(-1, 20, size=w * h).astype(I32)
    touched = check(dev, w, h, p, None, rgb, oid)
    assert touched.any()
    oid[5] = 70000
    check(dev, w, h, p, None, rgb, oid)
    # a plane full of -1: nothing is selected, whatever is listed - the output is the input
    got = dev.both(w, h, p, None, rgb, np.full(w * h, -1, dtype=I32))
    gpudev.same_bytes(got, rgb.view(np.uint32), "a plane of misses")
    # the last listed id alone decides
    p = ref.params(selected=(70000,) * 15 + (2,), radius=1, **OUTLINE)
    assert check(dev, w, h, p, None, rgb, rng.integers(0, 4, size=w * h).astype(I32)).any()


@pytest.mark.parametrize("radius", range(1, 9))
def test_every_radius_on_one_mask(dev, radius):
    w, h = 64, 16
    rng = np.random.default_rng(64)
    oid = np.zeros(w * h, dtype=I32)
    oid[rng.choice(w * h, size=6, replace=False)] = 4
    oid.reshape(h, w)[6:10, 30:35] = 4  # a block across the four tiles' corner
    rgb = frame(rng, w * h)
    p = ref.params(selected=(4,), radius=radius, outline_alpha=0.5, **OUTLINE)
    touched = check(dev, w, h, p, None, rgb, oid)
    M = ref.mask(oid, (4,))
    assert np.array_equal(touched, ref.window(M, w, h, radius) & ~M)


# -------------------------------------------------------------------------------------------------- bit preservation
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_null_params_copy_the_bits(dev, w, h):
    rgb = frame(np.random.default_rng(h), w * h)
    rgb.view(np.uint32)[0, :] = (0x7FC12345, 0x80000000, 0xFFC00001)  # a NaN's payload, -0, a negative NaN
    assert (rgb.view(np.uint32) == 0x7FC12345).any() and (rgb.view(np.uint32) == 0x80000000).any()
    for oid in (None, np.ones(w * h, dtype=I32)):
        got = dev.both(w, h, None, None, rgb, oid)
        gpudev.same_bytes(got, rgb.view(np.uint32), "params NULL")
    # a listed object that is nowhere in the frame, and planes that are passed though nothing reads them
    got = dev.both(w, h, ref.params(selected=(9,), fill_alpha=1.0), ABOVE, rgb, np.ones(w * h, dtype=I32), np.ones(w * h, dtype=F32))
    gpudev.same_bytes(got, rgb.view(np.uint32), "nothing selected in the frame")


# ---------------------------------------------------------------------------------------------------- sky and grid
@pytest.fixture(scope="module")
def planes():
    """synthetic id and depth planes at 48 x 32, shared: misses in blocks, objects at depths either side of the ground"""
    w, h = 48, 32
    rng = np.random.default_rng(4832)
    oid = rng.integers(0, 3, size=(h, w)).astype(I32)
    oid[:10, :] = -1
    oid[20:26, 5:30] = -1
    oid[rng.random((h, w)) < 0.1] = -1
    oid = oid.reshape(w * h)
    z = np.where(oid < 0, F32(np.inf), (0.5 + 14.0 * rng.random(w * h)).astype(F32)).astype(F32)
    return w, h, oid, z, frame(rng, w * h)


@pytest.mark.parametrize("flags", [SKY, GRID, SKY | GRID])
@pytest.mark.parametrize("cam_name", ["above", "below", "tilted"])
def test_sky_and_grid(dev, planes, cam_name, flags):
    w, h, oid, z, rgb = planes
    cam = dict(above=ABOVE, below=BELOW, tilted=TILTED)[cam_name]
    d, Lc = ref.ray(cam, w, h, np.arange(w * h))
    if cam_name == "above":
        assert (d[:, 1] < 0).all() and Lc[1] > 0
    elif cam_name == "below":
        assert (d[:, 1] < 0).all() and Lc[1] < 0  # t < 0 everywhere
    else:
        assert (d[:, 1] < 0).any() and (d[:, 1] > 0).any() and Lc[1] > 0  # d.y changes sign within the frame
    p = ref.params(flags=flags, selected=(1,), radius=2, fill_alpha=0.25, sky_top=(0.25, 0.5, 0.75), sky_bottom=(0.75, 0.75, 0.7),
                   grid_color=(0.5, 0.5, 0.5), grid_alpha=0.6, grid_y=0.0, grid_spacing=0.5, grid_half_width=0.04, grid_extent=6.0, **OUTLINE)
    check(dev, w, h, p, cam, rgb, oid, z)
    # the flags alone: what they touch is the sky's pixels and the grid's
    alone = dict(p, selected=(), fill_alpha=0.0)
    touched = check(dev, w, h, alone, cam, rgb, oid if flags & SKY else None, z if flags & GRID else None)
    sky = (oid < 0) if flags & SKY else np.zeros(w * h, dtype=bool)
    assert (touched & sky).sum() == sky.sum()
    lines = touched & ~sky
    if flags & GRID:
        assert lines.any() if cam_name != "below" else not lines.any()
        if cam_name == "above" and not flags & SKY:
            with np.errstate(all="ignore"):
                t = (F32(0.0) - Lc[1]) / d[:, 1]
            assert (lines & (oid < 0)).any() and not (lines & (z <= t)).any()  # seen through a miss, hidden by what is nearer
    else:
        assert not lines.any()
    # the default alphas and a plane the call may leave out
    if flags == GRID:
        got = dev.overlay(w, h, dict(alone, grid_alpha=0.0), cam, rgb, oid, z, pass_planes=True)
        want, _ = ref.overlay(w, h, dict(alone, grid_alpha=1.0), cam, rgb, None, z)
        gpudev.same_bytes(got, want.view(np.uint32), "grid_alpha 0 = 1")


# ------------------------------------------------------------------------------------------------------ the whole loop
def test_render_aov_overlay_present_on_cornell(L):
    sc = gpudev.scene("cornell")
    w, h = 64, 48
    n = w * h
    table = present_ref.thresholds(L)
    with Dev(L) as d:
        d.set_scene(sc)
        cfg = gpudev.config(w, h, 1, seed=7)
        rgb, _ = d.render(cfg, d.d_rgb)
        assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), None, None, d.d_z, d.d_id, None) == 0, L.pt_last_error()
        oid, z = d.download(d.d_id, n, I32), d.download(d.d_z, n)
        centre = int(oid[(h // 2) * w + w // 2])
        assert centre >= 0
        cam = cam_dict(sc.cam)
        p = dict(ref.defaults(L, cam), flags=SKY | GRID, selected=(centre,), fill_alpha=0.25, fill_color=(1.0, 0.5, 0.0))
        want, touched = ref.overlay(w, h, p, cam, rgb, oid, z)
        M = ref.mask(oid, (centre,))
        assert M.any() and (touched & M).sum() == M.sum()                   # some fill pixel ...
        assert (ref.window(M, w, h, 2) & ~M).any()                          # ... and some outline pixel
        s, c = ref.struct(p), ref.pt_camera(cam)
        assert L.pt_ctx_overlay(d.ctx, w, h, C.byref(s), C.byref(c), d.d_rgb, d.d_id, d.d_z, d.d_out) == 0, L.pt_last_error()
        gpudev.same_bytes(d.download(d.d_out, n * 3).view(np.uint32), want.view(np.uint32).ravel(), "overlay on cornell")
        d_px = d.alloc(32 * 24 * 4)
        pp = PtPresentParams(32, 24, 0.0, present_ref.RGBA8, 0)
        assert L.pt_ctx_present(d.ctx, w, h, C.byref(pp), d.d_out, d_px, None) == 0, L.pt_last_error()
        got = d.download(d_px, 32 * 24 * 4, np.uint8).reshape(24, 32, 4)
        assert np.array_equal(got, present_ref.present(table, want, w, h, 32, 24))
        # in place, as the loop runs it, and the frame's planes are read only
        assert L.pt_ctx_overlay(d.ctx, w, h, C.byref(s), C.byref(c), d.d_rgb, d.d_id, d.d_z, d.d_rgb) == 0, L.pt_last_error()
        gpudev.same_bytes(d.download(d.d_rgb, n * 3).view(np.uint32), want.view(np.uint32).ravel(), "in place")
        assert np.array_equal(d.download(d.d_id, n, I32), oid) and d.download(d.d_z, n).tobytes() == z.tobytes()
