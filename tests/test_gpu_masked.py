"""pt_ctx_select_pixels and pt_ctx_render_masked on the GPU.  Every comparison is of bytes, for equality, with guard bytes or
floats behind each output.  The select pass is held to tests/masked_ref.py, the restatement of the predicate in numpy binary32;
a retraced pixel is held to pt_ctx_render with the same cfg - never to the call under test.  The frames are 67x41 (no multiple of
64 in either direction, 2747 pixels: one workgroup of the compaction and a three-byte tail behind its last whole 16-byte group)
and one of 1025x1024 with two selected pixels (65 workgroups, an odd width)."""
import ctypes as C

import numpy as np
import pytest

import gpudev
import masked_ref as ref
import ptlib
from masked_ref import F32, U8
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtAdaptiveParams, PtAdaptiveStats, PtConfig, PtSelectParams, PtStats

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_CANCELLED = ptlib.abi.PT_ERR_INVALID, ptlib.abi.PT_CANCELLED
NO_BVH = ptlib.abi.PT_FLAG_NO_BVH
GUARD = 64          # floats or bytes behind each output
SENTINEL = F32(-3)  # no resolved colour: they are clamped to [0, 1]
W, H, SEED = 67, 41, 7
N = W * H
MASKS = ("empty", "first", "last", "63", "64", "65", "row", "checker", "ones", "random")


class Dev(gpudev.Device):
    """a context (with a scene, if one is given) and device buffers that go with it"""

    def __init__(self, L, sid=None):
        super().__init__(L, ptlib.load_scene_py(ptlib.scene_path(sid)) if sid else None)

    def render(self, cfg, d_out=None):
        """pt_ctx_render: (the frame as (pixels, 3), its stats)"""
        return super().render(cfg, d_out or self.alloc(self.L.pt_config_pixels(C.byref(cfg)) * 12))

    def masked(self, cfg, mask, want=0, cancel=None, mask_offset=0, d_mask=None, d_rgb=None, fill=True):
        """pt_ctx_render_masked into a frame of sentinels: (the frame as (pixels, 3), *n_pixels, the stats); the floats behind
        the frame are checked on the way"""
        n = self.L.pt_config_pixels(C.byref(cfg))
        d_mask = d_mask or self.alloc(n + 16)
        d_rgb = d_rgb or self.alloc((n * 3 + GUARD) * 4)
        self.upload(d_mask, np.asarray(mask, dtype=U8), mask_offset)
        if fill:
            self.fill_guarded(d_rgb, n * 3, GUARD, SENTINEL)
        st, count = PtStats(), C.c_uint32(12345)
        rc = self.L.pt_ctx_render_masked(self.ctx, C.byref(cfg), C.c_void_p(d_mask.value + mask_offset), d_rgb, None,
                                         C.cast(cancel, C.c_void_p) if cancel else None, C.byref(st), C.byref(count))
        assert rc == want, (rc, self.L.pt_last_error())
        return self.read_guarded(d_rgb, n * 3, GUARD, SENTINEL, "the frame").reshape(n, 3), count.value, st


def cfg_of(spp, w=W, h=H, backend=0, seed=SEED, **kw):
    return gpudev.config(w, h, spp, backend=backend, seed=seed, **kw)


@pytest.fixture(scope="module")
def devs(L):
    d = {sid: Dev(L, sid) for sid in ("cornell", "mesh")}
    yield d
    for v in d.values():
        v.close()


_frames = {}


def reference(devs, sid, spp):
    """pt_ctx_render's frame and stats, made once per (scene, spp) and left unchanged"""
    if (sid, spp) not in _frames:
        _frames[(sid, spp)] = devs[sid].render(cfg_of(spp))
    return _frames[(sid, spp)]


def make_mask(name, n=N, w=W):
    rng = np.random.default_rng(2026)
    m = np.zeros(n, dtype=U8)
    if name == "first":
        m[0] = 1
    elif name == "last":
        m[n - 1] = 1
    elif name in ("63", "64", "65"):
        m[rng.permutation(n)[:int(name)]] = 1
    elif name == "row":
        m[17 * w:18 * w] = 1
    elif name == "checker":
        m[((np.arange(n) % w) + (np.arange(n) // w)) % 2 == 0] = 1
    elif name == "ones":
        m[:] = 1
    elif name == "random":
        m[rng.random(n) < 0.03] = 1
    return m


def check_frame(got, count, mask, R, what):
    sel = np.asarray(mask) != 0
    assert count == int(sel.sum()), (what, count, int(sel.sum()))
    a, b = got[sel].view(np.uint32), R[sel].view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d of %d words of the selected pixels differ from pt_ctx_render's, first at %s: %r vs %r" % (
            what, len(bad), a.size, bad[0], got[sel][tuple(bad[0])], R[sel][tuple(bad[0])]))
    assert (got[~sel] == SENTINEL).all(), "%s: %d floats outside the mask were written" % (what, int((got[~sel] != SENTINEL).sum()))


# ------------------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("shift", (0, 1), ids=["aligned", "unaligned"])
@pytest.mark.parametrize("size", ref.SIZES, ids=["%dx%d" % s for s in ref.SIZES])
def test_select_is_the_restatement(L, devs, size, shift):
    """each plane alone and both together; `shift` moves the planes by one float and the mask by one byte, off the alignment the
    wide loads and stores need"""
    d = devs["cornell"]
    w, h = size
    n = w * h
    weight, length = ref.plane(n, ref.PARAMS["weight_max"], 1 + n), ref.plane(n, ref.PARAMS["len_max"], 2 + n)
    d_w, d_l, d_m = d.alloc(n * 4 + 16), d.alloc(n * 4 + 16), d.alloc(n + GUARD + 16)
    d.upload(d_w, weight, 4 * shift)
    d.upload(d_l, length, 4 * shift)
    p = PtSelectParams(ref.PARAMS["weight_max"], ref.PARAMS["len_max"], 0)
    for form in (1, 2, 3):
        d.upload(d_m, np.full(n + GUARD + 1, 0xAB, dtype=U8))
        exp, ones = ref.select(weight if form & 1 else None, length if form & 2 else None, **ref.PARAMS)
        count = C.c_uint32(12345)
        rc = L.pt_ctx_select_pixels(d.ctx, w, h, C.byref(p), C.c_void_p(d_w.value + 4 * shift) if form & 1 else None,
                                    C.c_void_p(d_l.value + 4 * shift) if form & 2 else None, C.c_void_p(d_m.value + shift),
                                    C.byref(count) if form != 2 else None, None)
        assert rc == 0, L.pt_last_error()
        got = d.download(d_m, n + GUARD + 1, U8)
        assert (got[:shift] == 0xAB).all() and (got[shift + n:] == 0xAB).all(), "bytes around the mask were written"
        assert got[shift:shift + n].tobytes() == exp.tobytes(), (size, form, np.flatnonzero(got[shift:shift + n] != exp)[:8])
        assert count.value == (ones if form != 2 else 12345)  # a NULL n_selected is accepted
    # the planes are read only
    assert d.download(d_w, n, offset=4 * shift).tobytes() == weight.tobytes()
    assert d.download(d_l, n, offset=4 * shift).tobytes() == length.tobytes()


def test_select_counts_over_many_workgroups(L, devs):
    """1025x1024: the strided grid's lanes make more than one trip; the count is the restatement's"""
    d = devs["cornell"]
    w, h = 1025, 1024
    n = w * h
    weight = ref.plane(n, 0.0, 3)
    d_w, d_m = d.alloc(n * 4), d.alloc(n + GUARD)
    d.upload(d_w, weight)
    d.fill_guarded(d_m, n, GUARD, 0xAB, U8)
    p, count = PtSelectParams(0.0, 0.0, 0), C.c_uint32(0)
    assert L.pt_ctx_select_pixels(d.ctx, w, h, C.byref(p), d_w, None, d_m, C.byref(count), None) == 0, L.pt_last_error()
    exp, ones = ref.select(weight=weight, weight_max=0.0)
    got = d.read_guarded(d_m, n, GUARD, 0xAB, "the mask", U8)
    assert got.tobytes() == exp.tobytes() and count.value == ones


# ----------------------------------------------------------------------------------------------------- render masked
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("sid", ("cornell", "mesh"))
def test_masked_pixels_are_pt_ctx_renders(devs, sid, name):
    R, rst = reference(devs, sid, 8)
    mask = make_mask(name)
    got, count, st = devs[sid].masked(cfg_of(8), mask)
    check_frame(got, count, mask, R, (sid, name))
    assert st.samples == count * 8
    if name == "empty":
        assert (st.ray_bounces, st.passes, st.samples) == (0, 0, 0)
    else:
        assert st.passes >= 1 and st.ray_bounces >= st.samples
    if name == "ones":  # every pixel: the counters are the frame call's
        assert (st.ray_bounces, st.samples) == (rst.ray_bounces, rst.samples)


def test_a_sample_count_that_is_not_whole_groups(devs):
    R, _ = reference(devs, "cornell", 5)
    mask = make_mask("random")
    got, count, st = devs["cornell"].masked(cfg_of(5), mask)
    check_frame(got, count, mask, R, "spp 5")
    assert st.samples == count * 5


def test_any_nonzero_byte_selects_and_the_mask_may_be_unaligned(devs):
    R, _ = reference(devs, "mesh", 8)
    mask = make_mask("random")
    idx = np.flatnonzero(mask)
    mask[idx[::2]] = 2
    mask[idx[1::3]] = 255
    for offset in (0, 1):
        got, count, _ = devs["mesh"].masked(cfg_of(8), mask, mask_offset=offset)
        check_frame(got, count, mask, R, ("byte values", offset))


def test_a_list_that_has_to_grow(L):
    """a fresh context's first call selects every pixel: the list starts short, is grown to the length and the pass runs again"""
    with Dev(L, "cornell") as d:
        cfg = cfg_of(8)
        R, _ = d.render(cfg)
        mask = make_mask("ones")
        got, count, _ = d.masked(cfg, mask)
        check_frame(got, count, mask, R, "grown")


def test_no_bvh_gives_the_same_bytes(devs):
    R, _ = reference(devs, "mesh", 8)
    mask = make_mask("checker")
    got, count, _ = devs["mesh"].masked(cfg_of(8, flags=NO_BVH), mask)
    check_frame(got, count, mask, R, "NO_BVH")


def test_a_band_of_whole_rows(L, devs):
    R, _ = reference(devs, "cornell", 8)
    d = devs["cornell"]
    b, e = 2 * W, 7 * W
    mask = make_mask("checker", n=e - b)
    got, count, _ = d.masked(cfg_of(8, band=(b, e)), mask)
    check_frame(got, count, mask, R[b:e], "band")
    d.masked(cfg_of(8, band=(b + 1, e)), mask[1:], want=PT_ERR_INVALID)
    assert "whole image rows" in L.pt_last_error().decode()


def test_two_pixels_of_a_large_frame(devs):
    """the first and the last pixel of 1025x1024 at 4 samples: 65 workgroups of the compaction, all but two of them empty, and
    wide mask loads at an odd width.  pt_ctx_render's pixels come from the frame's first and last row (the RNG is keyed on the
    frame's pixel index: a band's pixels are the frame's)."""
    d = devs["cornell"]
    w, h, spp = 1025, 1024, 4
    n = w * h
    first, _ = d.render(cfg_of(spp, w, h, band=(0, w)))
    last, _ = d.render(cfg_of(spp, w, h, band=(n - w, n)))
    mask = np.zeros(n, dtype=U8)
    mask[0] = mask[n - 1] = 1
    got, count, st = d.masked(cfg_of(spp, w, h), mask)
    assert count == 2 and st.samples == 2 * spp
    assert got[0].tobytes() == first[0].tobytes() and got[n - 1].tobytes() == last[w - 1].tobytes()
    assert (got[1:n - 1] == SENTINEL).all()


def test_a_raised_cancel_byte_leaves_the_frame_alone(L, devs):
    flag = (C.c_uint8 * 1)(1)
    mask = make_mask("checker")
    got, count, st = devs["cornell"].masked(cfg_of(8), mask, want=PT_CANCELLED, cancel=flag)
    assert (got == SENTINEL).all() and st.samples == 0
    assert "cancelled" in L.pt_last_error().decode()
    # the context goes on as before
    R, _ = reference(devs, "cornell", 8)
    got, count, _ = devs["cornell"].masked(cfg_of(8), mask)
    check_frame(got, count, mask, R, "after a cancelled call")


def test_refusals_that_need_a_context(L, devs):
    """each call breaks one rule and every rule checked after it"""
    with Dev(L) as bare:
        p = bare.alloc(64)
        n = C.c_uint32(77)

        def call(d, cfg):
            rc = L.pt_ctx_render_masked(d.ctx, C.byref(cfg), p, p, None, None, None, C.byref(n))
            return rc, L.pt_last_error().decode()

        bad = PtConfig(W, H, 0, 0, 1, 2 * W + 1, 7 * W, 0, 0x200, 0, 0, 2)
        rc, msg = call(bare, bad)
        assert rc == PT_ERR_INVALID and "no scene" in msg
        d = devs["cornell"]
        rc, msg = call(d, bad)
        assert rc == PT_ERR_INVALID and "whole image rows" in msg
        bad.idx_begin = 2 * W
        rc, msg = call(d, bad)
        assert rc == PT_ERR_INVALID and "chunk_step" in msg
        bad.chunk_step = 0
        rc, msg = call(d, bad)
        assert rc == PT_ERR_INVALID and "PT_FLAG_PIPELINES" in msg
        bad.flags = 0
        rc, msg = call(d, bad)
        assert rc == PT_ERR_INVALID and "positive" in msg  # pt_ctx_render's own: spp 0
        bad.spp, bad.backend = 1, 7
        rc, msg = call(d, bad)
        assert rc == PT_ERR_INVALID and "backend" in msg
        assert n.value == 77


# ------------------------------------------------------------------------------------------------------------- state
def test_leaves_the_held_frames_alone(L):
    """a held pt_ctx_accumulate frame and a held adaptive frame (32x24, tiles of 4) in the context: pt_ctx_accum_info and
    pt_ctx_adaptive_resolve give the same before and after a masked call; the accumulate frame continued equals pt_ctx_render;
    the adaptive frame continued to a higher cap equals pt_ctx_render_adaptive from scratch"""
    w, h, tile, tile_error = 32, 24, 4, 0.16
    n = w * h
    d, fresh = Dev(L, "cornell"), Dev(L, "cornell")
    try:
        d_out, d_spp, d_err = d.alloc(n * 12), d.alloc(n * 4), d.alloc(n * 4)

        def info():
            lo, hi = C.c_uint32(), C.c_uint32()
            assert L.pt_ctx_accum_info(d.ctx, C.byref(cfg_of(1, w, h, seed=5)), C.byref(lo), C.byref(hi)) == 0, L.pt_last_error()
            return lo.value, hi.value

        def resolved():
            assert L.pt_ctx_adaptive_resolve(d.ctx, C.byref(cfg_of(1, w, h, 1, seed=6)), d_out, d_spp, d_err, None) == 0, L.pt_last_error()
            return d.download(d_out, n * 3).tobytes(), d.download(d_spp, n, np.uint32).tobytes(), d.download(d_err, n).tobytes()

        def adaptive(dev, call, cap, outs):
            par, st, ast = PtAdaptiveParams(tile_error, tile, 0), PtStats(), PtAdaptiveStats()
            rc = call(dev.ctx, C.byref(cfg_of(cap, w, h, 1, seed=6)), C.byref(par), outs[0], outs[1], outs[2], None, None, None, None,
                      C.byref(st), C.byref(ast))
            assert rc == 0, L.pt_last_error()
            return (dev.download(outs[0], n * 3).tobytes(), dev.download(outs[1], n, np.uint32).tobytes(),
                    dev.download(outs[2], n).tobytes(), ast.samples)

        st = PtStats()
        assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg_of(4, w, h, seed=5)), d_out, None, None, None, None, C.byref(st)) == 0
        adaptive(d, L.pt_ctx_accumulate_adaptive, 16, (d_out, d_spp, d_err))
        before = (info(), resolved())
        assert before[0] == (4, 4)
        # the masked call: another seed and count, enough pixels for the scratch the adaptive calls share with it
        mcfg = cfg_of(8, w, h, seed=9)
        R, _ = fresh.render(mcfg)
        mask = make_mask("checker", n=n, w=w)
        got, count, _ = d.masked(mcfg, mask)
        check_frame(got, count, mask, R, "with held frames")
        assert (info(), resolved()) == before
        assert L.pt_ctx_accumulate(d.ctx, C.byref(cfg_of(8, w, h, seed=5)), d_out, None, None, None, None, C.byref(st)) == 0
        assert st.samples == n * 4  # only the rest was traced
        assert d.download(d_out, n * 3).tobytes() == fresh.render(cfg_of(8, w, h, seed=5))[0].tobytes()
        cont = adaptive(d, L.pt_ctx_accumulate_adaptive, 64, (d_out, d_spp, d_err))
        f_outs = (fresh.alloc(n * 12), fresh.alloc(n * 4), fresh.alloc(n * 4))
        scratch = adaptive(fresh, L.pt_ctx_render_adaptive, 64, f_outs)
        assert cont == scratch
        spp = np.frombuffer(cont[1], dtype=np.uint32)
        print("pixels by the count their tile ended with:", dict(zip(*[a.tolist() for a in np.unique(spp, return_counts=True)])))
    finally:
        d.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------------- composition
def test_upsample_select_retrace(L):
    """pt_ctx_upsample 33x25 <- 16x12 on cornell with a weight plane, pt_ctx_select_pixels(weight_max 0), pt_ctx_render_masked:
    the frame is the upsampled one with exactly the weight-0 pixels replaced by pt_ctx_render's"""
    (w, h), (Wf, Hf), spp = (16, 12), (33, 25), 4
    n, nl = Wf * Hf, w * h
    with Dev(L, "cornell") as d:
        lo = dict(color=d.alloc(nl * 12), albedo=d.alloc(nl * 12), normal=d.alloc(nl * 12), depth=d.alloc(nl * 4), oid=d.alloc(nl * 4))
        hi = dict(albedo=d.alloc(n * 12), normal=d.alloc(n * 12), depth=d.alloc(n * 4), oid=d.alloc(n * 4))
        d_up, d_weight, d_mask = d.alloc((n * 3 + GUARD) * 4), d.alloc(n * 4), d.alloc(n)
        lcfg, cfg = cfg_of(spp, w, h), cfg_of(spp, Wf, Hf)
        d.render(lcfg, lo["color"])
        assert L.pt_ctx_render_aov(d.ctx, C.byref(lcfg), lo["albedo"], lo["normal"], lo["depth"], lo["oid"], None) == 0, L.pt_last_error()
        assert L.pt_ctx_render_aov(d.ctx, C.byref(cfg), hi["albedo"], hi["normal"], hi["depth"], hi["oid"], None) == 0, L.pt_last_error()
        d.fill_guarded(d_up, n * 3, GUARD, SENTINEL)
        assert L.pt_ctx_upsample(d.ctx, Wf, Hf, w, h, None, lo["color"], lo["depth"], lo["oid"], lo["normal"], lo["albedo"], hi["depth"],
                                 hi["oid"], hi["normal"], hi["albedo"], d_up, d_weight, None) == 0, L.pt_last_error()
        up = d.download(d_up, n * 3).reshape(n, 3)
        weight = d.download(d_weight, n)
        p, ones = PtSelectParams(0.0, 0.0, 0), C.c_uint32(0)
        assert L.pt_ctx_select_pixels(d.ctx, Wf, Hf, C.byref(p), d_weight, None, d_mask, C.byref(ones), None) == 0, L.pt_last_error()
        fallback = weight == 0
        assert d.download(d_mask, n, U8).tobytes() == fallback.astype(U8).tobytes() and ones.value == int(fallback.sum())
        print("fallback pixels: %d of %d" % (ones.value, n))
        assert 0 < ones.value < n
        count = C.c_uint32(0)
        assert L.pt_ctx_render_masked(d.ctx, C.byref(cfg), d_mask, d_up, None, None, None, C.byref(count)) == 0, L.pt_last_error()
        got = d.read_guarded(d_up, n * 3, GUARD, SENTINEL, "the upsampled frame").reshape(n, 3)
        assert count.value == ones.value
        R, _ = d.render(cfg)
        assert got[fallback].tobytes() == R[fallback].tobytes() and got[~fallback].tobytes() == up[~fallback].tobytes()
