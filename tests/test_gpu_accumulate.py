"""Progressive accumulation on the GPU (pt_ctx_accumulate, pt_ctx_accum_*): a frame rendered to T samples per pixel over
several calls - refined, cancelled and resumed, across backends and scan forms, through a checkpoint file - is pt_ctx_render's
frame at T, bit for bit ("direct" below: pt_ctx_render with the same config at the total spp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpudev
import ptlib
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtStats

pytestmark = pytest.mark.gpu

WAVE, MEGA = ptlib.BACKEND_WAVEFRONT, ptlib.BACKEND_MEGAKERNEL
NO_BVH, SEPARATE = ptlib.abi.PT_FLAG_NO_BVH, ptlib.abi.PT_FLAG_SEPARATE_KERNELS
PT_ERR_INVALID, PT_CANCELLED, PT_ERR_IO, PT_ERR_PARSE = ptlib.abi.PT_ERR_INVALID, ptlib.abi.PT_CANCELLED, ptlib.abi.PT_ERR_IO, ptlib.abi.PT_ERR_PARSE
W, H, SEED = 64, 40, 8
TOL = 1e-4


class Dev(gpudev.Device):
    """One context, one scene, one device output buffer large enough for the call."""

    def __init__(self, L, sc, npix_max):
        super().__init__(L, sc)
        self.d_out, self.d_snap = self.alloc(npix_max * 12), self.alloc(npix_max * 12)

    def render(self, cfg, ptr=None, **kw):
        """direct: pt_ctx_render, (image, stats)"""
        return super().render(cfg, ptr or self.d_out, **kw)

    def accumulate(self, cfg, **kw):
        return self.render(cfg, accumulate=True, **kw)

    def info(self, cfg):
        lo, hi = C.c_uint32(), C.c_uint32()
        assert self.L.pt_ctx_accum_info(self.ctx, C.byref(cfg), C.byref(lo), C.byref(hi)) == 0, self.L.pt_last_error()
        return lo.value, hi.value


def cfg_of(spp, backend=WAVE, seed=SEED, w=W, h=H, **kw):
    return gpudev.config(w, h, spp, backend=backend, seed=seed, **kw)


@pytest.fixture(scope="module")
def cornell():
    return ptlib.load_scene_py(ptlib.scene_path("cornell"))


@pytest.fixture(scope="module")
def mesh():
    return ptlib.load_scene_py(ptlib.scene_path("mesh"))


@pytest.fixture
def dev(L, cornell):
    d = Dev(L, cornell, 2 * W * H)  # (room for the larger frames of the key-change test)
    yield d
    d.close()


def test_refinement_equals_one_call(dev):
    npix = W * H
    prev = 0
    for t in (3, 8, 20):
        img, st = dev.accumulate(cfg_of(t))
        assert st.samples == npix * (t - prev), (t, st.samples)
        assert st.ray_bounces > 0
        assert dev.info(cfg_of(t)) == (t, t)
        prev = t
    direct, _ = dev.render(cfg_of(20))
    assert np.array_equal(img, direct)
    # nothing left to trace: only the resolve, zero rays
    again, st = dev.accumulate(cfg_of(20))
    assert np.array_equal(again, direct) and st.samples == 0 and st.ray_bounces == 0 and st.passes == 0


@pytest.mark.parametrize("scene", ["cornell", "mesh"])
def test_switching_backend_and_scan_between_calls(L, request, scene):
    sc = request.getfixturevalue(scene)
    with Dev(L, sc, W * H) as d:
        npix = W * H
        steps = [(2, WAVE, 0, 0), (5, MEGA, 0, npix), (9, WAVE, SEPARATE, 2 * npix), (12, WAVE, 0, npix),
                 (16, MEGA, 0, 0)]
        if scene == "mesh":
            steps += [(18, WAVE, NO_BVH, npix), (21, MEGA, NO_BVH, 0), (23, WAVE, NO_BVH | SEPARATE, 0)]
        prev = 0
        for t, backend, flags, rpp in steps:
            img, st = d.accumulate(cfg_of(t, backend, flags=flags, rays_per_pass=rpp))
            assert st.samples == npix * (t - prev), (t, backend, flags)
            prev = t
        direct, _ = d.render(cfg_of(prev))
        assert np.array_equal(img, direct)
        direct_mega, _ = d.render(cfg_of(prev, MEGA))
        assert np.array_equal(img, direct_mega)


@pytest.mark.parametrize("backend", [WAVE, MEGA])
def test_cancel_and_resume(dev, backend):
    L, npix, T = dev.L, W * H, 16
    flag = (C.c_uint8 * 1)(0)
    snaps = []

    def on_progress(user, frac):
        if frac >= 0.4 and not flag[0]:
            n = C.c_uint32()
            assert L.pt_ctx_snapshot(dev.ctx, dev.d_snap, C.byref(n)) == 0, L.pt_last_error()
            snaps.append((n.value, dev.pixels(dev.d_snap, npix)))
            flag[0] = 1

    cb = ptlib.PROGRESS_FN(on_progress)
    cfg = cfg_of(T, backend, rays_per_pass=2 * npix)  # eight passes / rounds of two samples
    cfg.progress_ms = ptlib.PROGRESS_EVERY_PASS
    img, st = dev.accumulate(cfg, cancel=flag, cb=cb, want=PT_CANCELLED)
    k, k2 = dev.info(cfg)
    assert k == k2 and 0 < k < T, (k, k2)
    assert st.samples == npix * k
    direct_k, _ = dev.render(cfg_of(k))
    assert np.array_equal(img, direct_k)
    assert len(snaps) == 1
    n_snap, snap = snaps[0]
    assert 0 < n_snap <= k
    direct_n, _ = dev.render(cfg_of(n_snap))
    assert np.array_equal(snap, direct_n)
    # resume: the rest of the samples, then the frame at T
    img2, st2 = dev.accumulate(cfg_of(T, backend))
    assert st2.samples == npix * (T - k)
    direct_t, _ = dev.render(cfg_of(T))
    assert np.array_equal(img2, direct_t)


def test_calls_in_parts(L, cornell, tmp_path):
    """A call of more than 1.5 Mi pixels keeps a count per part of 2^20 pixels: a cancel in the second part leaves part one
    at T, part two at its own count and part three at the samples of the call before (not black); resuming - wavefront, or
    the megakernel on the uneven counts - gives the direct frame."""
    w, h = 2048, 1040  # 2 129 920 pixels: parts of 1 048 576 + 1 048 576 + 32 768
    npix, part = w * h, 1 << 20
    with Dev(L, cornell, npix) as d:
        _, st = d.accumulate(cfg_of(2, w=w, h=h))
        assert st.samples == 2 * npix and d.info(cfg_of(2, w=w, h=h)) == (2, 2)
        flag = (C.c_uint8 * 1)(0)
        snaps = []

        def on_progress(user, frac):
            if frac > 0.5 and not flag[0]:  # (part one ends at 0.49 of the call)
                n = C.c_uint32()
                assert L.pt_ctx_snapshot(d.ctx, d.d_snap, C.byref(n)) == 0, L.pt_last_error()
                snaps.append((n.value, d.pixels(d.d_snap, npix)))
                flag[0] = 1

        cb = ptlib.PROGRESS_FN(on_progress)
        T = 5
        cfg = cfg_of(T, w=w, h=h, rays_per_pass=part)  # one sample per pass
        cfg.progress_ms = ptlib.PROGRESS_EVERY_PASS
        got, st = d.accumulate(cfg, cancel=flag, cb=cb, want=PT_CANCELLED)
        lo, hi = d.info(cfg)
        assert hi == T and 2 <= lo < T
        k = (st.samples - part * (T - 2)) // part + 2  # part two's count
        assert st.samples == part * (T - 2) + part * (k - 2) and 2 < k < T and lo == 2
        band = lambda b, e, s: d.render(cfg_of(s, w=w, h=h, band=(b, e)))[0]
        assert np.array_equal(got[:part], band(0, part, T))
        assert np.array_equal(got[part:2 * part], band(part, 2 * part, k))
        assert np.array_equal(got[2 * part:], band(2 * part, npix, 2))  # earlier samples, not black
        assert got[2 * part:].any()
        n_snap, snap = snaps[0]
        assert n_snap == k and np.array_equal(snap, got)
        ckpt = str(tmp_path / "parts.ptacc")
        assert L.pt_ctx_accum_save(d.ctx, ckpt.encode()) == 0, L.pt_last_error()
        direct, _ = d.render(cfg_of(T, w=w, h=h))
        img, st = d.accumulate(cfg_of(T, w=w, h=h))
        assert st.samples == part * (T - k) + (npix - 2 * part) * (T - 2)
        assert np.array_equal(img, direct)
        # the megakernel on the uneven counts (part by part)
        assert L.pt_ctx_accum_load(d.ctx, ckpt.encode()) == 0, L.pt_last_error()
        assert d.info(cfg) == (2, T)
        img, st = d.accumulate(cfg_of(T, MEGA, w=w, h=h))
        assert st.samples == part * (T - k) + (npix - 2 * part) * (T - 2)
        assert np.array_equal(img, direct)


@pytest.mark.parametrize("kind", ["band", "chunks"])
def test_band_and_chunked_frames(dev, kind):
    extra = {"band": dict(band=(500, 1900)), "chunks": dict(chunks=(64, 1, 3))}[kind]
    n = dev.L.pt_config_pixels(C.byref(cfg_of(1, **extra)))
    _, st = dev.accumulate(cfg_of(4, **extra))
    assert st.samples == 4 * n
    img, st = dev.accumulate(cfg_of(11, MEGA, **extra))
    assert st.samples == 7 * n
    direct, _ = dev.render(cfg_of(11, **extra))
    assert np.array_equal(img, direct)
    # the whole frame is another frame
    assert dev.info(cfg_of(11)) == (0, 0) and dev.info(cfg_of(11, **extra)) == (11, 11)


def test_key_changes_start_from_zero(dev, cornell):
    L = dev.L

    def fresh(cfg, t):
        n = L.pt_config_pixels(C.byref(cfg))
        img, st = dev.accumulate(cfg)
        assert st.samples == n * t
        direct, _ = dev.render(cfg)
        assert np.array_equal(img, direct)

    dev.accumulate(cfg_of(4))
    fresh(cfg_of(6, seed=SEED + 1), 6)
    assert dev.info(cfg_of(6)) == (0, 0) and dev.info(cfg_of(6, seed=SEED + 1)) == (6, 6)
    fresh(cfg_of(6, w=W + 2), 6)
    fresh(cfg_of(6, w=W + 2, band=(10, 900)), 6)
    dev.set_scene(cornell)  # the same scene again: what the kernels read was uploaded anew
    assert dev.info(cfg_of(6, w=W + 2, band=(10, 900))) == (0, 0)
    fresh(cfg_of(6, w=W + 2, band=(10, 900)), 6)
    # samples cannot be removed; pipelines are refused; neither disturbs what is held
    st = PtStats()
    for bad in (cfg_of(5, w=W + 2, band=(10, 900)), cfg_of(8, w=W + 2, band=(10, 900), flags=2 << 8)):
        assert L.pt_ctx_accumulate(dev.ctx, C.byref(bad), dev.d_out, None, None, None, None, C.byref(st)) == PT_ERR_INVALID
    big = cfg_of(1)
    big.spp = (1 << 24) + 1
    assert L.pt_ctx_accumulate(dev.ctx, C.byref(big), dev.d_out, None, None, None, None, C.byref(st)) == PT_ERR_INVALID
    assert dev.info(cfg_of(6, w=W + 2, band=(10, 900))) == (6, 6)
    # a pt_ctx_render of another frame between two accumulate calls does not disturb the held sums
    dev.accumulate(cfg_of(4))
    dev.render(cfg_of(7, seed=99, w=W - 4, backend=MEGA))
    dev.render(cfg_of(3, seed=99))
    img, st = dev.accumulate(cfg_of(10))
    assert st.samples == W * H * 6
    assert np.array_equal(img, dev.render(cfg_of(10))[0])
    assert L.pt_ctx_accum_reset(dev.ctx) == 0 and dev.info(cfg_of(10)) == (0, 0)
    assert L.pt_ctx_accum_save(dev.ctx, b"/nonexistent-dir/x.ptacc") == PT_ERR_INVALID  # nothing held


def test_checkpoint_round_trip_and_damaged_files(L, cornell, mesh, tmp_path):
    path = tmp_path / "c.ptacc"
    d = Dev(L, cornell, W * H)
    d.accumulate(cfg_of(5))
    assert L.pt_ctx_accum_save(d.ctx, str(path).encode()) == 0, L.pt_last_error()
    d.close()
    data = path.read_bytes()
    assert data[:8] == b"PTACCUM1" and len(data) == 68 + 4 + 24 * W * H + 8
    with Dev(L, cornell, W * H) as d:
        assert d.info(cfg_of(12)) == (0, 0)
        assert L.pt_ctx_accum_load(d.ctx, str(path).encode()) == 0, L.pt_last_error()
        assert d.info(cfg_of(12)) == (5, 5)
        img, st = d.accumulate(cfg_of(12))
        assert st.samples == W * H * 7
        assert np.array_equal(img, d.render(cfg_of(12))[0])
        # damaged files, each with its code; the held sums stay as they were
        damaged = {
            "truncated": (data[:-100], PT_ERR_PARSE),
            "flipped": (data[:1000] + bytes([data[1000] ^ 0x10]) + data[1001:], PT_ERR_PARSE),
            "magic": (b"PTACCUM2" + data[8:], PT_ERR_PARSE),
            "header_only": (data[:40], PT_ERR_PARSE),
            "empty": (b"", PT_ERR_PARSE),
        }
        for name, (blob, want) in damaged.items():
            p = tmp_path / (name + ".ptacc")
            p.write_bytes(blob)
            assert L.pt_ctx_accum_load(d.ctx, str(p).encode()) == want, name
        assert L.pt_ctx_accum_load(d.ctx, str(tmp_path / "missing.ptacc").encode()) == PT_ERR_IO
        assert d.info(cfg_of(12)) == (12, 12)
        # another scene
        d.set_scene(mesh)
        assert L.pt_ctx_accum_load(d.ctx, str(path).encode()) == PT_ERR_INVALID
        assert d.info(cfg_of(12)) == (0, 0)


def test_saved_files_are_the_documented_layout(L, cornell, tmp_path):
    """What pt_ctx_accum_save writes is the layout include/ptrace.h documents, byte for byte: the file's parsed fields and its own
    planes, put together again by the builder of the codec test, are the file; its counts are what pt_ctx_accum_info reports; and
    a fresh context that loads it saves the same bytes.  A plain frame at 3 samples, a noise-tracked one at 8."""
    from noise_ref import parse_checkpoint
    from test_host_logic import _checkpoint
    w, h = 16, 8
    for spp, track in ((3, False), (8, True)):
        first, second = tmp_path / ("first%d.ptacc" % spp), tmp_path / ("second%d.ptacc" % spp)
        with Dev(L, cornell, w * h) as d:
            assert L.pt_ctx_accum_track_noise(d.ctx, int(track)) == 0
            d.accumulate(cfg_of(spp, w=w, h=h))
            held = d.info(cfg_of(spp, w=w, h=h))
            assert L.pt_ctx_accum_save(d.ctx, str(first).encode()) == 0, L.pt_last_error()
        data = first.read_bytes()
        f = parse_checkpoint(data)
        key = tuple(f[k] for k in ("width", "height", "idx_begin", "idx_end", "chunk_pixels", "chunk_first", "chunk_step", "seed"))
        assert f["version"] == (2 if track else 1) and key == (w, h, 0, w * h, 0, 0, 0, SEED) and f["total"] == w * h
        rebuilt = _checkpoint(L, key, f["fingerprint"], f["total"], f["part_px"], f["counts"].tolist(),
                              f["n_a"].tolist() if track else None, f["sums"].tobytes(), f["a"].tobytes() if track else None)
        assert rebuilt == data
        assert (int(f["counts"].min()), int(f["counts"].max())) == held == (spp, spp)
        assert not track or f["n_a"].tolist() == [4]  # samples [0, 4) of a tracked frame's first call go to half A
        with Dev(L, cornell, w * h) as d:
            assert L.pt_ctx_accum_load(d.ctx, str(first).encode()) == 0, L.pt_last_error()
            assert L.pt_ctx_accum_save(d.ctx, str(second).encode()) == 0, L.pt_last_error()
        assert second.read_bytes() == data


def test_three_calls_against_the_oracle(dev, cornell):
    for t in (2, 5, 9):
        img, _ = dev.accumulate(cfg_of(t, MEGA if t == 5 else WAVE))
    want, _, _ = ptlib.oracle_render(cornell, W, H, 9, SEED)
    assert np.abs(img - want).max() <= TOL


def test_cli_checkpoint(tmp_path):
    cli = os.path.join(ptlib.PKG, "ptrace")
    ckpt = str(tmp_path / "f.ptacc")

    def run(*args):
        return subprocess.run([cli, *args, "--root", ptlib.ROOT, "--seed", "3"], cwd=str(tmp_path), capture_output=True,
                              text=True, timeout=300)

    def ppm(out):
        files = [f for f in os.listdir(out) if f.endswith(".ppm")]
        assert len(files) == 1
        body = open(os.path.join(out, files[0])).read().split("255\n", 1)[1]
        return np.array(body.split(), dtype=np.int64)

    r = run("4", "24", "cornell", "--checkpoint", ckpt, "--out", str(tmp_path / "a"))
    assert r.returncode == 0 and "Resuming" not in r.stdout, r.stdout + r.stderr
    assert os.path.exists(ckpt)
    r = run("8", "24", "cornell", "--checkpoint", ckpt, "--out", str(tmp_path / "b"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Resuming from 4 samples per pixel" in r.stdout
    r2 = run("8", "24", "cornell", "--out", str(tmp_path / "c"))
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert np.array_equal(ppm(tmp_path / "b"), ppm(tmp_path / "c"))
    # a checkpoint of another scene
    r = run("8", "24", "three-spheres", "--checkpoint", ckpt, "--out", str(tmp_path / "d"))
    assert r.returncode == 1 and "another scene" in r.stderr, r.stdout + r.stderr
    # ... and of another frame of this scene (another size)
    r = run("8", "30", "cornell", "--checkpoint", ckpt, "--out", str(tmp_path / "e"))
    assert r.returncode == 1 and "another frame" in r.stderr, r.stdout + r.stderr
