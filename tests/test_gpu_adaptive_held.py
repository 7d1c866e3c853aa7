"""pt_ctx_accumulate_adaptive on the GPU: the adaptive frame held across calls.  Everything is exact.  The reference is never the
new call: it is pt_ctx_render_adaptive from scratch, pt_ctx_render at a pixel's own count, or tests/adaptive_ref.py's replay
over the error maps of a tracked pt_ctx_accumulate frame."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref
import gpudev
import ptlib
from ptlib import PtAdaptiveInfo, PtAdaptiveParams, PtAdaptiveStats, PtStats
from test_adaptive_held_abi import NONE, adaptive_checkpoint, parse_adaptive_checkpoint
from test_gpu_accumulate import NO_BVH
from gpudev import L  # noqa: F401  (fixture)
from test_gpu_adaptive import CAP, H, SEED, TILE, TILE_ERROR, W, ADev
from test_gpu_noise import NDev

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_CANCELLED, PT_ERR_PARSE = ptlib.abi.PT_ERR_INVALID, ptlib.abi.PT_CANCELLED, ptlib.abi.PT_ERR_PARSE
f32 = np.float32
CASES = [("cornell", 0), ("mesh", 0), ("mesh", NO_BVH)]


def cfg_of(spp, backend=ptlib.BACKEND_MEGAKERNEL, seed=SEED, w=W, h=H, **kw):
    return gpudev.config(w, h, spp, backend=backend, seed=seed, **kw)


@pytest.fixture(scope="module")
def scenes():
    return {sid: ptlib.load_scene_py(ptlib.scene_path(sid)) for sid in ("cornell", "mesh")}


class HDev(ADev):
    """ADev with the held adaptive frame's calls and a second set of output buffers (for pt_ctx_adaptive_resolve)"""

    def __init__(self, L, sc, npix_max):
        super().__init__(L, sc, npix_max)
        self.extra = [self.alloc(npix_max * size) for size in (12, 4, 4)]

    def _maps(self, n, d_out, d_spp, d_err):
        return dict(img=self.pixels(d_out, n), spp=self.download(d_spp, n, np.uint32), err=self.download(d_err, n))

    def held(self, cfg, tile_error, tile=TILE, min_spp=0, want=0, cancel=None, cb=None):
        par, st, ast = PtAdaptiveParams(tile_error, tile, min_spp), PtStats(), PtAdaptiveStats()
        rc = self.L.pt_ctx_accumulate_adaptive(self.ctx, C.byref(cfg), C.byref(par), self.d_out, self.d_spp, self.d_err, None,
                                               C.cast(cancel, C.c_void_p) if cancel else None,
                                               C.cast(cb, C.c_void_p) if cb else None, None, C.byref(st), C.byref(ast))
        assert rc == want, (rc, self.L.pt_last_error())
        if rc not in (0, PT_CANCELLED):
            return None
        r = self._maps(self.L.pt_config_pixels(C.byref(cfg)), self.d_out, self.d_spp, self.d_err)
        r.update(st=st, ast=ast)
        return r

    def ainfo(self, cfg, tile_error, tile=TILE, min_spp=0):
        par, out = PtAdaptiveParams(tile_error, tile, min_spp), PtAdaptiveInfo()
        assert self.L.pt_ctx_adaptive_info(self.ctx, C.byref(cfg), C.byref(par), C.byref(out)) == 0, self.L.pt_last_error()
        return out

    def resolve(self, cfg, want=0):
        rc = self.L.pt_ctx_adaptive_resolve(self.ctx, C.byref(cfg), self.extra[0], self.extra[1], self.extra[2], None)
        assert rc == want, (rc, self.L.pt_last_error())
        return self._maps(self.L.pt_config_pixels(C.byref(cfg)), *self.extra) if rc == 0 else None


_scratch = {}


def scratch(L, scenes, sid, flags, tile_error, cap=CAP, tile=TILE, w=W, h=H, min_spp=0, seed=SEED):
    """the reference, computed once and shared: pt_ctx_render_adaptive from zero on a context of its own"""
    key = (sid, flags, tile_error, cap, tile, w, h, min_spp, seed)
    if key not in _scratch:
        with ADev(L, scenes[sid], w * h) as d:
            _scratch[key] = d.adaptive(cfg_of(cap, w=w, h=h, flags=flags, seed=seed), tile_error, tile=tile, min_spp=min_spp)
    return _scratch[key]


def same_frame(r, ref):
    """img / spp / err bits, samples and mean_error of the held frame against a from-scratch render"""
    for k in ("img", "spp", "err"):
        assert np.array_equal(r[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert r["ast"].samples == ref["ast"].samples and r["ast"].mean_error == ref["ast"].mean_error
    assert (r["ast"].tiles, r["ast"].tiles_open) == (ref["ast"].tiles, ref["ast"].tiles_open)


def cancel_after(n):
    """(flag, callback, calls): the callback raises the flag at its n-th call - the callbacks come between steps"""
    flag, calls = (C.c_uint8 * 1)(0), []

    def on_progress(user, frac):
        calls.append(frac)
        if len(calls) == n:
            flag[0] = 1

    return flag, ptlib.PROGRESS_FN(on_progress), calls


def every_pass(cfg):
    cfg.progress_ms = ptlib.PROGRESS_EVERY_PASS
    return cfg


@pytest.mark.parametrize("sid,flags", CASES)
def test_cleaner(L, scenes, sid, flags):
    """0.16, then 0.08, at a cap of 256: the frame is pt_ctx_render_adaptive(256, 0.08) from scratch, and the second call traced
    only the difference.  The condition below is checked on the two from-scratch references: tiles that closed under 0.16 at two
    or more distinct counts take more samples under 0.08 - otherwise a broken reopen would not show.  It holds for 0.16: of the
    tiles that closed at 16 / 32 / 64 / 128 under it, cornell takes 4 / 14 / 45 / 24 further under 0.08, mesh 2 / 8 / 46 / 33."""
    x1, x2 = 0.16, 0.08
    r1, r2 = scratch(L, scenes, sid, flags, x1), scratch(L, scenes, sid, flags, x2)
    tid, n_tiles = adaptive_ref.tile_ids(W, H, TILE)
    first = np.array([np.nonzero(tid == t)[0][0] for t in range(n_tiles)])
    c1, c2 = r1["spp"][first], r2["spp"][first]
    reopened = sorted(set(c1[c2 > c1].tolist()))
    print("%s: tiles closed under %g that go on under %g, by the count they closed at: %s" % (
        sid, x1, x2, {c: int(((c1 == c) & (c2 > c1)).sum()) for c in reopened}))
    assert len(reopened) >= 2 and (c2 >= c1).all()
    with HDev(L, scenes[sid], W * H) as d:
        a = d.held(cfg_of(CAP, flags=flags), x1)
        same_frame(a, r1)
        assert (a["st"].samples, a["st"].ray_bounces) == (r1["st"].samples, r1["st"].ray_bounces)
        b = d.held(cfg_of(CAP, flags=flags), x2)
    same_frame(b, r2)
    assert b["st"].samples == r2["st"].samples - r1["st"].samples
    assert b["st"].ray_bounces == r2["st"].ray_bounces - r1["st"].ray_bounces
    assert b["st"].samples > 0 and b["ast"].levels >= 2


@pytest.mark.parametrize("sid,flags", CASES)
def test_higher_cap(L, scenes, sid, flags):
    ref64, ref = scratch(L, scenes, sid, flags, TILE_ERROR, cap=64), scratch(L, scenes, sid, flags, TILE_ERROR)
    with HDev(L, scenes[sid], W * H) as d:
        a = d.held(cfg_of(64, flags=flags), TILE_ERROR)
        same_frame(a, ref64)
        b = d.held(cfg_of(CAP, flags=flags), TILE_ERROR)
    same_frame(b, ref)
    assert list(b["ast"].level_spp[:b["ast"].levels]) == [128, 256]
    assert b["st"].samples == ref["st"].samples - ref64["st"].samples
    assert b["st"].ray_bounces == ref["st"].ray_bounces - ref64["st"].ray_bounces


def test_stop_and_continue(L, scenes):
    ref = scratch(L, scenes, "cornell", 0, TILE_ERROR)
    d = HDev(L, scenes["cornell"], W * H)
    flag, calls, seen = (C.c_uint8 * 1)(0), [], []

    def on_progress(user, frac):
        calls.append(frac)
        if len(calls) == 2:  # after the second step: the preview of what a cancel here returns, then the cancel
            seen.append(d.resolve(cfg_of(CAP)))
            flag[0] = 1

    cb = ptlib.PROGRESS_FN(on_progress)
    try:
        r = d.held(every_pass(cfg_of(CAP)), TILE_ERROR, want=PT_CANCELLED, cancel=flag, cb=cb)
        assert r["ast"].levels == 2 and list(r["ast"].level_spp[:2]) == [16, 32] and 0.0 < calls[0] < calls[1] < 1.0
        assert set(np.unique(r["spp"]).tolist()) <= {16, 32}
        for k in ("img", "spp", "err"):
            assert np.array_equal(seen[0][k].view(np.uint32), r[k].view(np.uint32)), k
        info = d.ainfo(cfg_of(CAP), TILE_ERROR)
        assert {info.spp_min, info.spp_max} <= {16, 32} and info.samples == r["ast"].samples == int(r["spp"].sum(dtype=np.uint64))
        assert (info.tiles, info.tiles_open, info.tiles_at_cap) == (r["ast"].tiles, r["ast"].tiles_open, 0)
        assert info.mean_error == r["ast"].mean_error
        flag[0] = 0
        full = d.held(cfg_of(CAP), TILE_ERROR)
        same_frame(full, ref)
        assert full["st"].samples == ref["st"].samples - r["ast"].samples
        assert list(full["ast"].level_spp[:full["ast"].levels]) == [64, 128, 256]
        assert d.resolve(cfg_of(CAP, seed=SEED + 1), want=PT_ERR_INVALID) is None  # another frame than the held one
    finally:
        d.close()


def test_off_ladder_cap(L, scenes):
    """A cap of 100, then 256: the tiles open at 100 go to 128 - 16 samples to half B, which holds fewer, then 12 to A - and on.
    Every pixel is pt_ctx_render's at its own count, and decisions, counts and the error map are the replay's over the level
    list [16, 32, 64, 100, 128, 256], from a tracked frame accumulated at exactly those counts (at 128 it holds 64 + 64)."""
    lv = [16, 32, 64, 100, 128, 256]
    tracked, plain = NDev(L, scenes["cornell"], W * H, tracked=True), NDev(L, scenes["cornell"], W * H, tracked=False)
    maps, images = [], {}
    try:
        for t in lv:
            tracked.accumulate(cfg_of(t))
            ns, e = tracked.noise(cfg_of(t))
            if t == 100:
                assert (ns.spp_a_min, ns.spp_b_min) == (52, 48)
            if t == 128:
                assert (ns.spp_a_min, ns.spp_b_min) == (64, 64)  # the half with fewer samples first
            maps.append(e)
            images[t], _ = plain.render(cfg_of(t))
    finally:
        tracked.close()
        plain.close()
    with HDev(L, scenes["cornell"], W * H) as d:
        a = d.held(cfg_of(100), TILE_ERROR)
        b = d.held(cfg_of(CAP), TILE_ERROR)
    want100 = adaptive_ref.replay(maps, W, H, TILE, TILE_ERROR, lv, stop_after=4)
    want = adaptive_ref.replay(maps, W, H, TILE, TILE_ERROR, lv)
    print("closed per level %s, open at the cap %d" % (want["tiles_closed"], want["tiles_open"]))
    assert want["tiles_closed"][4] + want["tiles_closed"][5] + want["tiles_open"] > 0  # some tiles do go past 100
    for r, w_ in ((a, want100), (b, want)):
        for c in np.unique(r["spp"]):  # every pixel is pt_ctx_render's at its own count
            sel = r["spp"] == c
            assert np.array_equal(r["img"][sel].view(np.uint32), images[int(c)][sel].view(np.uint32)), int(c)
        assert np.array_equal(r["spp"], w_["spp"]) and np.array_equal(r["err"].view(np.uint32), w_["error"].view(np.uint32))
        assert (r["ast"].tiles_open, r["ast"].samples, r["ast"].mean_error) == (w_["tiles_open"], w_["samples"], w_["mean_error"])
    assert set(np.unique(b["spp"]).tolist()) <= set(lv)
    assert list(a["ast"].level_spp[:a["ast"].levels]) == lv[:4] and list(a["ast"].tiles_closed[:4]) == want["tiles_closed"][:4]
    assert list(b["ast"].level_spp[:b["ast"].levels]) == lv[4:] and list(b["ast"].tiles_closed[:2]) == want["tiles_closed"][4:]


def test_looser_target_traces_nothing(L, scenes):
    ref = scratch(L, scenes, "cornell", 0, TILE_ERROR)
    with HDev(L, scenes["cornell"], W * H) as d:
        a = d.held(cfg_of(CAP), TILE_ERROR)
        assert a["ast"].tiles_open > 0  # (the reference frame leaves tiles open at the cap)
        b = d.held(cfg_of(CAP), 0.32)
        assert (b["st"].samples, b["st"].ray_bounces, b["st"].passes, b["ast"].levels) == (0, 0, 0, 0)
        for k in ("img", "spp", "err"):
            assert np.array_equal(b[k].view(np.uint32), ref[k].view(np.uint32)), k
        assert b["ast"].tiles_open < a["ast"].tiles_open and b["ast"].samples == ref["ast"].samples
        assert b["ast"].mean_error == ref["ast"].mean_error
        i8, i32, lo = d.ainfo(cfg_of(CAP), TILE_ERROR), d.ainfo(cfg_of(CAP), 0.32), d.ainfo(cfg_of(64), TILE_ERROR)
        assert (i8.tiles_open, i8.tiles_at_cap) == (a["ast"].tiles_open, a["ast"].tiles_open)  # open at the cap, all of them
        assert i32.tiles_open == b["ast"].tiles_open and i32.samples == i8.samples == ref["ast"].samples
        assert (i8.spp_min, i8.spp_max) == (int(ref["spp"].min()), int(ref["spp"].max()))
        assert lo.tiles_at_cap == lo.tiles_open == i8.tiles_open  # a cap below what is held: no error, nothing to take
        c = d.held(cfg_of(64), TILE_ERROR)  # ... and such a call removes nothing
        assert c["st"].samples == 0 and np.array_equal(c["spp"], ref["spp"])
        e = d.held(cfg_of(CAP), TILE_ERROR)  # back to the tighter target: the tiles reopen, at the cap - nothing to trace either
        assert e["st"].samples == 0 and e["ast"].tiles_open == a["ast"].tiles_open


def test_isolation_and_the_key(L, scenes):
    ref = scratch(L, scenes, "cornell", 0, TILE_ERROR)
    with HDev(L, scenes["cornell"], W * H) as d:
        img8, _ = d.accumulate(cfg_of(8))
        a = d.held(cfg_of(64), TILE_ERROR)
        assert d.info(cfg_of(8)) == (8, 8)  # pt_ctx_accumulate's held frame is as it was ...
        img16, st = d.accumulate(cfg_of(16))
        assert st.samples == W * H * 8
        assert d.ainfo(cfg_of(64), TILE_ERROR).samples == a["ast"].samples  # ... and so is the adaptive one after that call
        plain, _ = d.render(cfg_of(16))
        assert np.array_equal(plain.view(np.uint32), img16.view(np.uint32))
        # pt_ctx_render_adaptive after a held frame: its from-zero result, and its frame is the held one afterwards
        full = d.adaptive(cfg_of(CAP), TILE_ERROR)
        same_frame(full, ref)
        assert (full["st"].samples, full["st"].ray_bounces) == (ref["st"].samples, ref["st"].ray_bounces)
        assert d.ainfo(cfg_of(CAP), TILE_ERROR).samples == ref["ast"].samples
        assert d.held(cfg_of(CAP), TILE_ERROR)["st"].samples == 0
        # another key drops the frame: the call starts from zero, and the old key names nothing any more
        for kw, cfg in ((dict(tile=16), cfg_of(64)), (dict(), cfg_of(64, seed=SEED + 1)), (dict(min_spp=24), cfg_of(64))):
            want = scratch(L, scenes, "cornell", 0, TILE_ERROR, cap=64, tile=kw.get("tile", TILE), min_spp=kw.get("min_spp", 0),
                           seed=cfg.seed)
            r = d.held(cfg, TILE_ERROR, **kw)
            same_frame(r, want)
            assert r["st"].samples == want["st"].samples
            assert d.ainfo(cfg_of(CAP), TILE_ERROR).tiles == 0 and d.ainfo(cfg, TILE_ERROR, **kw).tiles == want["ast"].tiles
            assert d.held(cfg_of(CAP), TILE_ERROR)["st"].samples == ref["st"].samples  # (back to the first key: from zero again)
        d.set_scene(scenes["cornell"])  # pt_ctx_set_scene drops it too
        assert d.ainfo(cfg_of(CAP), TILE_ERROR).tiles == 0
        assert d.resolve(cfg_of(CAP), want=PT_ERR_INVALID) is None
        assert L.pt_ctx_adaptive_save(d.ctx, b"/nonexistent/x") == PT_ERR_INVALID
        assert L.pt_ctx_adaptive_reset(d.ctx) == 0


def test_checkpoint(L, scenes, tmp_path):
    ref = scratch(L, scenes, "mesh", 0, TILE_ERROR)
    path = str(tmp_path / "frame.ptad").encode()
    d, e = HDev(L, scenes["mesh"], W * H), HDev(L, scenes["cornell"], W * H)
    flag, cb, _ = cancel_after(2)
    try:
        r = d.held(every_pass(cfg_of(CAP)), TILE_ERROR, want=PT_CANCELLED, cancel=flag, cb=cb)
        assert L.pt_ctx_adaptive_save(d.ctx, path) == 0, L.pt_last_error()
        ck = parse_adaptive_checkpoint(open(path, "rb").read())
        assert (ck["tile"], ck["n0"], ck["total"], len(ck["table"])) == (TILE, 16, W * H, 96)
        assert sum(64 * t[0] for t in ck["table"]) == r["ast"].samples and {t[0] for t in ck["table"]} <= {16, 32}
        # another scene; a damaged file: refused, and what the context holds stays
        before = e.held(cfg_of(16), TILE_ERROR)
        assert L.pt_ctx_adaptive_load(e.ctx, path) == PT_ERR_INVALID and "another scene" in L.pt_last_error().decode()
        bad = bytearray(open(path, "rb").read())
        bad[100] ^= 1
        (tmp_path / "bad.ptad").write_bytes(bytes(bad))
        assert L.pt_ctx_adaptive_load(e.ctx, str(tmp_path / "bad.ptad").encode()) == PT_ERR_PARSE
        assert L.pt_ctx_adaptive_load(e.ctx, str(tmp_path / "none.ptad").encode()) == -6
        assert e.ainfo(cfg_of(16), TILE_ERROR).samples == before["ast"].samples
        e.set_scene(scenes["mesh"])  # a fresh frame state under the checkpoint's scene
        assert L.pt_ctx_adaptive_load(e.ctx, path) == 0, L.pt_last_error()
        assert e.ainfo(cfg_of(CAP), TILE_ERROR).samples == r["ast"].samples
        got = e.resolve(cfg_of(CAP))
        for k in ("img", "spp", "err"):
            assert np.array_equal(got[k].view(np.uint32), r[k].view(np.uint32)), k
        full = e.held(cfg_of(CAP), TILE_ERROR)
        same_frame(full, ref)
        assert full["st"].samples == ref["st"].samples - r["ast"].samples
    finally:
        d.close()
        e.close()


def test_saved_files_are_the_documented_layout(L, scenes, tmp_path):
    """What pt_ctx_adaptive_save writes is the layout include/ptrace.h documents, byte for byte: the file's parsed fields and its
    own planes, put together again by the builder of the codec test, are the file; its counts are what pt_ctx_adaptive_info
    reports; and a fresh context that loads it saves the same bytes.  16 x 8 in tiles of 4 at the smallest min_spp (1: n_0 = 8;
    0 stands for 16) and the smallest cap (1 sample, below n_0: no tile has an E), and at a cap of n_0, where every tile has one."""
    w, h, tile, min_spp = 16, 8, 4, 1
    for cap in (1, 8):
        first, second = tmp_path / ("first%d.ptad" % cap), tmp_path / ("second%d.ptad" % cap)
        with HDev(L, scenes["cornell"], w * h) as d:
            d.held(cfg_of(cap, w=w, h=h), TILE_ERROR, tile=tile, min_spp=min_spp)
            info = d.ainfo(cfg_of(cap, w=w, h=h), TILE_ERROR, tile=tile, min_spp=min_spp)
            assert L.pt_ctx_adaptive_save(d.ctx, str(first).encode()) == 0, L.pt_last_error()
        data = first.read_bytes()
        f = parse_adaptive_checkpoint(data)
        assert (f["version"], f["key"], f["tile"], f["n0"], f["total"]) == (1, (w, h, 0, w * h, 0, 0, 0, SEED), tile, 8, w * h)
        assert adaptive_checkpoint(L, f["key"], f["tile"], f["n0"], f["fp"], f["total"], f["table"], f["sums"], f["a"]) == data
        counts = [t[0] for t in f["table"]]
        assert (len(counts), min(counts), max(counts)) == (info.tiles, info.spp_min, info.spp_max) == (8, cap, cap)
        assert sum(tile * tile * c for c in counts) == info.samples
        assert all((t[2] == NONE) == (cap == 1) for t in f["table"])
        with HDev(L, scenes["cornell"], w * h) as d:
            assert L.pt_ctx_adaptive_load(d.ctx, str(first).encode()) == 0, L.pt_last_error()
            assert L.pt_ctx_adaptive_save(d.ctx, str(second).encode()) == 0, L.pt_last_error()
        assert second.read_bytes() == data


def test_cli_adaptive_checkpoint(tmp_path):
    cli = os.path.join(ptlib.PKG, "ptrace")
    assert os.path.exists(cli), "the CLI is built with the library"

    def run(out, *args):
        r = subprocess.run([cli, "64", "32", "cornell", "--root", ptlib.ROOT, "--out", str(tmp_path / out), *args], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        files = [f for f in os.listdir(tmp_path / out) if f.endswith(".ppm")]
        assert len(files) == 1
        return r.stdout, open(tmp_path / out / files[0]).read().split("255\n", 1)[1]

    ck = str(tmp_path / "cli.ptad")
    out1, first = run("a", "--adaptive", "0.2", "--adaptive-checkpoint", ck)
    assert os.path.exists(ck) and "Resuming" not in out1
    out2, second = run("b", "--adaptive", "0.05", "--adaptive-checkpoint", ck)
    assert "Resuming from" in out2
    _, one_shot = run("c", "--adaptive", "0.05", "--seed", "0")  # (the checkpoint runs default to seed 0)
    assert second == one_shot and first != second
    r = subprocess.run([cli, "64", "32", "cornell", "--root", ptlib.ROOT, "--adaptive-checkpoint", ck], capture_output=True, text=True)
    assert r.returncode == 1 and "--adaptive-checkpoint needs --adaptive" in r.stderr


def test_partial_tiles(L, scenes):
    w, h, tile, te = 100, 70, 16, 0.12  # 7 x 5 tiles, the right column 4 wide, the bottom row 6 high
    ref = scratch(L, scenes, "cornell", 0, te, cap=64, tile=tile, w=w, h=h)
    ref32 = scratch(L, scenes, "cornell", 0, te, cap=32, tile=tile, w=w, h=h)
    with HDev(L, scenes["cornell"], w * h) as d:
        a = d.held(cfg_of(32, w=w, h=h), te, tile=tile)
        same_frame(a, ref32)
        b = d.held(cfg_of(64, w=w, h=h), te, tile=tile)
    same_frame(b, ref)
    assert b["ast"].tiles == 35 and b["st"].samples == ref["st"].samples - ref32["st"].samples
