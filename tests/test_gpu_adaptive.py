"""pt_ctx_render_adaptive on the GPU.  Everything is exact: a pixel that ends with n samples is pt_ctx_render's pixel at spp = n,
and the closing decisions, the error map and the statistics are those tests/adaptive_ref.py replays from the error maps of
UNIFORM frames (a tracked context: pt_ctx_accumulate at n_0, n_1, ... and pt_ctx_accum_noise after each)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import gpudev
import noise_ref
import ptlib
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtAdaptiveParams, PtAdaptiveStats, PtStats
from test_gpu_accumulate import MEGA, NO_BVH
from test_gpu_noise import NDev

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_CANCELLED = ptlib.abi.PT_ERR_INVALID, ptlib.abi.PT_CANCELLED
W, H, TILE, TILE_ERROR, CAP, SEED = 96, 64, 8, 0.08, 256, 8
f32 = np.float32


def cfg_of(spp, backend=MEGA, seed=SEED, w=W, h=H, **kw):
    return gpudev.config(w, h, spp, backend=backend, seed=seed, **kw)


@pytest.fixture(scope="module")
def scenes():
    return {sid: ptlib.load_scene_py(ptlib.scene_path(sid)) for sid in ("cornell", "mesh")}


class ADev(NDev):
    """NDev with a count map and the adaptive call"""

    def __init__(self, L, sc, npix_max, tracked=False):
        super().__init__(L, sc, npix_max, tracked=tracked)
        self.d_spp = self.alloc(npix_max * 4)

    def adaptive(self, cfg, tile_error, tile=TILE, min_spp=0, want=0, cancel=None, cb=None, maps=True):
        par, st, ast = PtAdaptiveParams(tile_error, tile, min_spp), PtStats(), PtAdaptiveStats()
        rc = self.L.pt_ctx_render_adaptive(self.ctx, C.byref(cfg), C.byref(par), self.d_out, self.d_spp if maps else None,
                                           self.d_err if maps else None, None, C.cast(cancel, C.c_void_p) if cancel else None,
                                           C.cast(cb, C.c_void_p) if cb else None, None, C.byref(st), C.byref(ast))
        assert rc == want, (rc, self.L.pt_last_error())
        if rc not in (0, PT_CANCELLED):
            return None
        n = self.L.pt_config_pixels(C.byref(cfg))
        spp, err = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=f32)
        if maps:
            spp, err = self.download(self.d_spp, n, np.uint32), self.download(self.d_err, n)
        return dict(img=self.pixels(self.d_out, n), spp=spp, err=err, st=st, ast=ast)


_uniform = {}


def uniform(L, scenes, sid, flags, w=W, h=H, band=None, min_spp=0, cap=CAP):
    """Computed once per frame and shared: the levels, per level the error map of the uniform tracked frame and
    pt_ctx_render's image and bounces at that count."""
    key = (sid, flags, w, h, band, min_spp, cap)
    if key in _uniform:
        return _uniform[key]
    lv = adaptive_ref.levels(min_spp, cap)
    tracked, plain = NDev(L, scenes[sid], w * h, tracked=True), NDev(L, scenes[sid], w * h, tracked=False)
    maps, images, bounces = [], {}, {}
    try:
        for (n_a, n_b), t in zip(adaptive_ref.halves(lv), lv):
            cfg = cfg_of(t, w=w, h=h, flags=flags, band=band)
            tracked.accumulate(cfg)
            if n_a and n_b:
                ns, e = tracked.noise(cfg)
                assert (ns.spp_a_min, ns.spp_b_min) == (n_a, n_b)  # the halves the header promises for these calls
                maps.append(e)
            else:
                maps.append(None)
            images[t], st = plain.render(cfg)
            bounces[t] = st.ray_bounces
    finally:
        tracked.close()
        plain.close()
    _uniform[key] = dict(levels=lv, maps=maps, images=images, bounces=bounces)
    return _uniform[key]


def check_pixels(r, u):
    """test 1: every pixel is pt_ctx_render's at its own count; the sample totals agree"""
    for c in np.unique(r["spp"]):
        sel = r["spp"] == c
        want = u["images"][int(c)][sel] if c else np.zeros((int(sel.sum()), 3), dtype=f32)
        assert np.array_equal(r["img"][sel].view(np.uint32), want.view(np.uint32)), int(c)
    assert r["st"].samples == int(r["spp"].sum(dtype=np.uint64)) == r["ast"].samples


def check_replay(r, u, w, rows, tile, tile_error, stop_after=None):
    """test 2: the decisions, the error map and the statistics are the replay's"""
    want = adaptive_ref.replay(u["maps"], w, rows, tile, tile_error, u["levels"], stop_after=stop_after)
    ast = r["ast"]
    print("levels %s closed %s open %d of %d, mean error %.6g, samples %d" % (
        want["level_spp"], want["tiles_closed"], want["tiles_open"], want["tiles"], want["mean_error"], want["samples"]))
    assert np.array_equal(r["spp"], want["spp"])
    assert np.array_equal(r["err"].view(np.uint32), want["error"].view(np.uint32))
    assert (ast.tiles, ast.tiles_open, ast.levels) == (want["tiles"], want["tiles_open"], len(want["level_spp"]))
    assert list(ast.level_spp[:ast.levels]) == want["level_spp"] and list(ast.tiles_closed[:ast.levels]) == want["tiles_closed"]
    assert ast.samples == want["samples"] and ast.mean_error == want["mean_error"]
    return want


CASES = [("cornell", 0), ("mesh", 0), ("mesh", NO_BVH)]


@pytest.mark.parametrize("sid,flags", CASES)
def test_pixels_decisions_and_a_really_adaptive_frame(L, scenes, sid, flags):
    u = uniform(L, scenes, sid, flags)
    with ADev(L, scenes[sid], W * H) as d:
        r = d.adaptive(cfg_of(CAP, flags=flags), TILE_ERROR)
    check_pixels(r, u)
    want = check_replay(r, u, W, H, TILE, TILE_ERROR)
    # test 3, on the replay built from the uniform frames (not on the code under test): the frame is really adaptive
    # (the share counts the tiles that closed at some level, the cap's own included, against those the cap left open: the
    # CPU study's 76 of 96 on cornell is 7 + 3 + 2 + 7 + 57)
    closed = want["closed_at"]
    finished = want["tiles"] - want["tiles_open"]
    share = finished / want["tiles"]
    print("%s: closing levels %s, %d of %d tiles closed, the others open at the cap (%.3f)" % (
        sid, np.unique(closed[closed >= 0]).tolist(), finished, want["tiles"], share))
    assert len(np.unique(closed[closed >= 0])) >= 3
    assert 0.4 <= share <= 0.95


@pytest.mark.parametrize("sid,flags", CASES)
def test_ends_of_the_range(L, scenes, sid, flags):
    u = uniform(L, scenes, sid, flags)
    with ADev(L, scenes[sid], W * H) as d:
        r0 = d.adaptive(cfg_of(CAP, flags=flags), 0.0)
        r12 = d.adaptive(cfg_of(CAP, flags=flags), 12.0)
    # tile_error 0: nothing closes unless E is 0; every pixel of a tile still open is pt_ctx_render's at the cap
    check_pixels(r0, u)
    check_replay(r0, u, W, H, TILE, 0.0)
    tid, _ = adaptive_ref.tile_ids(W, H, TILE)
    open_px = r0["spp"] == CAP
    assert np.array_equal(r0["img"][open_px].view(np.uint32), u["images"][CAP][open_px].view(np.uint32))
    if sum(r0["ast"].tiles_closed[:r0["ast"].levels]) == 0:
        assert open_px.all() and r0["st"].ray_bounces == u["bounces"][CAP]
    # tile_error 12, the estimate's upper bound: every tile closes at n_0
    check_pixels(r12, u)
    assert (r12["spp"] == 16).all() and r12["ast"].levels == 1 and r12["ast"].tiles_closed[0] == r12["ast"].tiles == 96
    assert r12["ast"].tiles_open == 0 and np.array_equal(r12["err"].view(np.uint32), u["maps"][0].view(np.uint32))
    assert r12["st"].ray_bounces == u["bounces"][16]


def test_partial_tiles_on_both_edges(L, scenes):
    w, h, tile, cap, te = 100, 70, 16, 64, 0.12  # 7 x 5 tiles, the right column 4 wide, the bottom row 6 high
    u = uniform(L, scenes, "cornell", 0, w=w, h=h, cap=cap)
    with ADev(L, scenes["cornell"], w * h) as d:
        r = d.adaptive(cfg_of(cap, w=w, h=h), te, tile=tile)
        r4 = d.adaptive(cfg_of(cap, w=w, h=h), te, tile=4)
        r32 = d.adaptive(cfg_of(cap, w=w, h=h), te, tile=32)
    assert r["ast"].tiles == 35
    for res, t in ((r, tile), (r4, 4), (r32, 32)):
        check_pixels(res, u)
        check_replay(res, u, w, h, t, te)


def test_full_size_frame_takes_the_resolve_loop_round_twice(L, scenes):
    """1056 x 520 in tiles of 4 at a cap of 32: 549 120 pixels > 2048 * 256 = 524 288 (stride_grid's cap times kTileBlock), so
    k_tile_resolve's grid-stride loop takes a second turn and k_tile_select's runs over 34 320 tiles (135 workgroups);
    k_tile_level takes 34 320 open tiles, 16 to a workgroup.  The levels are 16 and 32.  The same frame in tiles of 32 (33 x 17 of
    them, the bottom row 8 high) is k_tile_level's four-trip form: 1024 pixels a tile, 256 a trip.  Everything is exact,
    as on the small frames: check_pixels and check_replay through uniform().  The maps are optional: without them the image and the
    statistics are the same.  Then the held form of the same frame, and pt_ctx_adaptive_resolve - the resolve kernel launched on
    its own - gives the three outputs again."""
    w, h, tile, cap, te = 1056, 520, 4, 32, 0.12
    npix = w * h
    assert npix == 549120 and npix > 2048 * 256 and -(-npix // 256) > 2048  # the resolve loop's second turn
    tid, n_tiles = adaptive_ref.tile_ids(w, h, tile)
    assert n_tiles == 34320 and n_tiles > 10000 and (1 << (2 * 5)) // 256 == 4  # tens of thousands of tiles; four trips at edge 32
    u = uniform(L, scenes, "cornell", 0, w=w, h=h, cap=cap)
    assert u["levels"] == [16, 32]
    with ADev(L, scenes["cornell"], npix) as d:
        cfg = cfg_of(cap, w=w, h=h)
        r = d.adaptive(cfg, te, tile=tile)
        bare = d.adaptive(cfg, te, tile=tile, maps=False)
        r32 = d.adaptive(cfg, te, tile=32)
        # the held form, and the resolve of what it holds into the same three buffers
        par, st, ast = PtAdaptiveParams(te, tile, 0), PtStats(), PtAdaptiveStats()
        rc = L.pt_ctx_accumulate_adaptive(d.ctx, C.byref(cfg), C.byref(par), d.d_out, d.d_spp, d.d_err, None, None, None, None,
                                          C.byref(st), C.byref(ast))
        assert rc == 0, (rc, L.pt_last_error())
        held = dict(img=d.pixels(d.d_out, npix), spp=d.download(d.d_spp, npix, np.uint32), err=d.download(d.d_err, npix))
        d.upload(d.d_out, np.full(npix * 3, -3.0, dtype=f32))
        d.upload(d.d_spp, np.full(npix, 0xA5A5A5A5, dtype=np.uint32))
        d.upload(d.d_err, np.full(npix, -3.0, dtype=f32))
        assert L.pt_ctx_adaptive_resolve(d.ctx, C.byref(cfg), d.d_out, d.d_spp, d.d_err, None) == 0, L.pt_last_error()
        resolved = dict(img=d.pixels(d.d_out, npix), spp=d.download(d.d_spp, npix, np.uint32), err=d.download(d.d_err, npix))
    check_pixels(r, u)
    want = check_replay(r, u, w, h, tile, te)
    # on the replay built from the uniform frames: both levels run, some tiles close at the first and some go on
    assert want["tiles"] == n_tiles and want["level_spp"] == [16, 32] and 0 < want["tiles_closed"][0] < n_tiles
    assert np.array_equal(bare["img"].view(np.uint32), r["img"].view(np.uint32))
    assert (bare["st"].samples, bare["st"].ray_bounces) == (r["st"].samples, r["st"].ray_bounces)
    for name in ("samples", "mean_error", "tiles_open"):
        assert getattr(bare["ast"], name) == getattr(r["ast"], name), name
    check_pixels(r32, u)
    check_replay(r32, u, w, h, 32, te)
    assert r32["ast"].tiles == 33 * 17
    for k in ("img", "spp", "err"):
        assert np.array_equal(held[k].view(np.uint32), r[k].view(np.uint32)), ("held", k)
        assert np.array_equal(resolved[k].view(np.uint32), r[k].view(np.uint32)), ("resolved", k)
    assert (ast.samples, ast.mean_error, ast.tiles, ast.tiles_open) == (r["ast"].samples, r["ast"].mean_error, n_tiles, r["ast"].tiles_open)


def test_a_band_of_whole_rows_and_the_band_refusals(L, scenes):
    band = (20 * W, 46 * W)  # 26 rows from row 20: tiles are counted from the band's first row (3 full tile rows and 2 rows)
    u = uniform(L, scenes, "mesh", 0, band=band, cap=64)
    with ADev(L, scenes["mesh"], W * H) as d:
        r = d.adaptive(cfg_of(64, band=band), 0.12)
        assert r["ast"].tiles == 12 * 4 and len(r["spp"]) == 26 * W
        check_pixels(r, u)
        check_replay(r, u, W, 26, TILE, 0.12)
        for cfg, text in ((cfg_of(64, band=(10, 900)), "whole image rows"), (cfg_of(64, band=(0, 10 * W + 1)), "whole image rows"),
                          (cfg_of(64, chunks=(W, 0, 2)), "chunk_step"), (cfg_of(64, flags=2 << 8), "PIPELINES"),
                          (cfg_of(0), "")):
            assert d.adaptive(cfg, 0.1, want=PT_ERR_INVALID) is None
            assert text in L.pt_last_error().decode(), (text, L.pt_last_error())


def test_cancel_between_levels(L, scenes):
    u = uniform(L, scenes, "cornell", 0)
    d = ADev(L, scenes["cornell"], W * H)
    flag = (C.c_uint8 * 1)(0)
    calls = []

    def on_progress(user, frac):
        calls.append(frac)
        if len(calls) == 2:  # the callbacks come between levels: the second one after the second level
            flag[0] = 1

    cb = ptlib.PROGRESS_FN(on_progress)
    cfg = cfg_of(CAP)
    cfg.progress_ms = ptlib.PROGRESS_EVERY_PASS
    try:
        r = d.adaptive(cfg, TILE_ERROR, want=PT_CANCELLED, cancel=flag, cb=cb)
        assert r["ast"].levels == 2 and list(r["ast"].level_spp[:2]) == [16, 32]
        assert set(np.unique(r["spp"]).tolist()) <= {16, 32}
        assert 0.0 < calls[0] < calls[1] < 1.0
        check_pixels(r, u)
        check_replay(r, u, W, H, TILE, TILE_ERROR, stop_after=2)
        flag[0] = 0
        full = d.adaptive(cfg_of(CAP), TILE_ERROR)  # the same context, afterwards: the whole frame
        check_pixels(full, u)
        check_replay(full, u, W, H, TILE, TILE_ERROR)
    finally:
        d.close()


def test_isolation_from_the_held_frame_and_between_calls(L, scenes):
    u = uniform(L, scenes, "cornell", 0)
    with ADev(L, scenes["cornell"], W * H) as d:
        d.accumulate(cfg_of(8, w=W, h=H))
        assert d.info(cfg_of(8, w=W, h=H)) == (8, 8)
        a = d.adaptive(cfg_of(CAP), TILE_ERROR)
        assert d.info(cfg_of(8, w=W, h=H)) == (8, 8)  # the held frame is as it was
        img16, st = d.accumulate(cfg_of(16, w=W, h=H))
        assert st.samples == W * H * 8  # only the samples it did not hold
        assert np.array_equal(img16.view(np.uint32), u["images"][16].view(np.uint32))
        b = d.adaptive(cfg_of(CAP), TILE_ERROR, maps=False)  # the scratch is reused: nothing of the first call is left in it
        c = d.adaptive(cfg_of(CAP), TILE_ERROR)
        for k in ("img", "spp", "err"):
            assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), k
        assert np.array_equal(a["img"].view(np.uint32), b["img"].view(np.uint32))
        for x in (b, c):
            assert (x["st"].samples, x["st"].ray_bounces, x["ast"].mean_error) == (a["st"].samples, a["st"].ray_bounces, a["ast"].mean_error)


def test_the_tile_pass_rounds_are_counted(L, scenes):
    """Rounds only batch the samples, so no image shows how many there were: pt_stats.passes does.  32 x 32 in tiles of 8, one
    level of 16 samples (min_spp = cap = 16; tile_error 0 leaves every tile open), rays_per_pass = 4096: the level's runs are [0, 8)
    and [8, 16), each over 16 tiles x 64 = 1024 entries in rounds of 4096 / 1024 = 4 samples - two launches per run, four in all."""
    w = h = 32
    with ADev(L, scenes["cornell"], w * h) as d:
        r = d.adaptive(cfg_of(16, w=w, h=h, rays_per_pass=4096), 0.0, min_spp=16)
        whole = d.adaptive(cfg_of(16, w=w, h=h), 0.0, min_spp=16)
    assert r["ast"].levels == 1 and r["ast"].level_spp[0] == 16
    assert r["st"].passes == 4 and whole["st"].passes == 2
    assert r["st"].samples == r["ast"].samples == w * h * 16 and (r["spp"] == 16).all()
    assert r["st"].ray_bounces == whole["st"].ray_bounces
    assert np.array_equal(r["img"].view(np.uint32), whole["img"].view(np.uint32))
