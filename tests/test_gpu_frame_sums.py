"""The pixel accumulator on the GPU against tests/frame_sums.py, with == on integers.  -m gpu.

1. Frames: the raw 32.32 sums pt_ctx_accum_save writes - every pixel, every channel - are the integers the restatement chains
   down the oracle's paths, for every pass-kernel form; the float frames pt_ctx_accumulate and pt_ctx_render give are those sums
   through the restated k_resolve, bit for bit, pixels above 1 and black pixels among them.  Then cornell on the default form
   across passes, on a band, and in the two halves of a tracked frame.
2. to_fixed and k_resolve at their edges, through pt_ctx_radiance: at depth 11 the first hit has new_depth = 12 = MAX_DEPTH, so
   radiance() returns the surface's emission whatever the draws are (mod.rs:677-683); n samples give exactly n * to_fixed(e),
   resolved over n and not clamped.  tests/test_frame_sums.py proves on the CPU that these cases tell a divide in double, a
   multiply by the reciprocal and a rounded low word from the real arithmetic.
3. The door: a colour or emission the sums are not defined for is refused and the context's scene is left as it was."""
import ctypes as C
import time

import numpy as np
import pytest

import boundary_rays as br
import frame_sums as fs
import gpudev
import noise_ref
import ptlib
from ptlib import PtConfig, PtObject, PtStats, _np_f
from gpudev import L, same_bytes  # noqa: F401  (L: fixture)
from test_gpu_boundary_rays import PASS_FORMS
from test_gpu_noise import deal

pytestmark = pytest.mark.gpu

PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
# test_gpu_boundary_rays' forms and the megakernel that scans every triangle (k_mega)
FORMS = PASS_FORMS + [("mega_no_bvh", {}, ptlib.BACKEND_MEGAKERNEL, ptlib.FLAG_NO_BVH, (None, None))]
FORM_IDS = [f[0] for f in FORMS]
FULL_TABLE_FORMS = ("pass_cand", "mega")
BVH_MIN_TRIS = 16  # csrc/pt_device.h kBvhMinTris: a mesh of that many triangles gets a BVH


def _has_bvh(sc):
    return any(sc.objs[i].kind == ptlib.PT_MESH and sc.objs[i].tri_count >= BVH_MIN_TRIS for i in range(sc.n_objs))


def _set_scene(L, ctx, sc, form):
    """the scene set, and the context's kernel for the form's flags the one the form is named for"""
    name, _, _, flags, kernels = form
    gpudev.set_scene(L, ctx, sc)
    want = kernels[0] if _has_bvh(sc) else kernels[1]
    if want is not None:
        assert L.pt_ctx_pass_kernel(ctx, flags).decode() == want, (name, sc.id)


def _saved(L, ctx, path):
    assert L.pt_ctx_accum_save(ctx, str(path).encode()) == 0, L.pt_last_error()
    return noise_ref.parse_checkpoint(open(path, "rb").read())


def assert_planes(got, want, what):
    """(3, n) uint64 planes equal, or the first differing (pixel, channel) with both values"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).T)  # (pixel, channel), pixel-major
    if len(bad):
        p, c = (int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d sums differ, first at pixel %d channel %d: device %d (0x%x), restated %d (0x%x)" % (
            what, len(bad), got.size, p, c, int(got[c, p]), int(got[c, p]), int(want[c, p]), int(want[c, p])))


# ---- 1. frames, raw sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_pixel_sum_is_the_restated_integer(L, form, tmp_path):
    """Each walked frame accumulated to its sample count on this form: the checkpoint's three planes are the restated integers,
    every pixel and every channel; the frame the call returned and pt_ctx_render's are those sums resolved and clamped, bit for
    bit (pixels that are exactly 1.0 and exactly 0.0 among them); the bounce counts are the walk's ray count."""
    name, env, backend, flags, _ = form
    dev = gpudev.Device(L, env=env)
    ctx, out = dev.ctx, dev.alloc(16 * 12 * 12)
    compared = 0
    try:
        for frame in fs.WALKS:
            sid, w, h, spp, seed = frame
            W, sums = fs.frame(*frame)
            total = fs.total_over(sums, range(spp))
            what = "%s %s seed %x" % (name, sid, seed)
            _set_scene(L, ctx, W.scene, form)
            cfg = PtConfig(w, h, spp, backend, seed, 0, 0, 0, flags)
            img, st = dev.render(cfg, out, accumulate=True)
            f = _saved(L, ctx, tmp_path / "frame.ptacc")
            assert f["version"] == 1 and f["counts"].tolist() == [spp] and f["total"] == w * h, what
            assert_planes(f["sums"], fs.planes(total), what)
            compared += f["sums"].size
            want = fs.resolved(total, spp, clamp=True)
            assert (want == 1.0).any() and (want == 0.0).any()
            same_bytes(img, want, what + " pt_ctx_accumulate's frame")
            assert st.ray_bounces == W.n, (what, st.ray_bounces, W.n)
            img, st = dev.render(cfg, out)
            same_bytes(img, want, what + " pt_ctx_render's frame")
            assert st.ray_bounces == W.n, (what, st.ray_bounces, W.n)
    finally:
        dev.close()
    print("%s: %d pixel sums compared, all equal" % (name, compared))


@pytest.fixture(scope="module")
def cornell():
    frame = fs.WALKS[0]
    assert frame[0] == "cornell"
    W, sums = fs.frame(*frame)
    return frame, W, sums


def test_sums_cross_launches(L, cornell, tmp_path):
    """rays_per_pass = the frame's pixels: one sample per pass, every pixel's sum is added to by 8 launches"""
    (sid, w, h, spp, seed), W, sums = cornell
    form = FORMS[0]
    dev = gpudev.Device(L)
    ctx, out = dev.ctx, dev.alloc(w * h * 12)
    try:
        _set_scene(L, ctx, W.scene, form)
        img, st = dev.render(PtConfig(w, h, spp, 0, seed, 0, 0, w * h, 0), out, accumulate=True)
        assert st.passes == spp and st.ray_bounces == W.n, st.passes
        total = fs.total_over(sums, range(spp))
        assert_planes(_saved(L, ctx, tmp_path / "passes.ptacc")["sums"], fs.planes(total), "8 passes")
        same_bytes(img, fs.resolved(total, spp, clamp=True), "8 passes")
    finally:
        dev.close()


def test_a_band_holds_its_pixels_sums(L, cornell, tmp_path):
    """the band [37, 151) of cornell - neither end on a row or a wave boundary - holds restated[37:151]"""
    (sid, w, h, spp, seed), W, sums = cornell
    b, e = 37, 151
    dev = gpudev.Device(L)
    ctx, out = dev.ctx, dev.alloc(w * h * 12)
    try:
        _set_scene(L, ctx, W.scene, FORMS[0])
        img, st = dev.render(PtConfig(w, h, spp, 0, seed, b, e, 0, 0), out, accumulate=True)
        f = _saved(L, ctx, tmp_path / "band.ptacc")
        assert (f["idx_begin"], f["idx_end"], f["total"]) == (b, e, e - b)
        total = fs.total_over(sums, range(spp))
        assert_planes(f["sums"], fs.planes(total, b, e), "band")
        same_bytes(img, fs.resolved(total[b:e], spp, clamp=True), "band")
        assert st.ray_bounces == sum(1 for k in W.keys if b <= k[0] < e)
    finally:
        dev.close()


def test_half_a_holds_the_samples_the_schedule_deals_it(L, cornell, tmp_path):
    """A tracked frame brought to 2 samples, then to 8.  include/ptrace.h (pt_ctx_accum_track_noise): a call from c to T traces
    [c, m) then [m, T), m = min(T, c + 4 * ceil((T - c) / 8)), each run to the half that holds fewer samples, a tie to A -
    test_gpu_noise.deal states that rule: [0, 2) -> A, [2, 6) -> B, [6, 8) -> A.  The held planes are the whole frame's, and
    half A's (k_accum_scatter_half) the restated sums of exactly samples {0, 1, 6, 7}."""
    (sid, w, h, spp, seed), W, sums = cornell
    runs, n_a = [], 0
    for c, t in ((0, 2), (2, spp)):
        r, n_a = deal(c, n_a, t)
        runs += r
    assert runs == [(0, 2, True), (2, 6, False), (6, 8, True)] and n_a == 4
    in_a = [s for s0, s1, to_a in runs if to_a for s in range(s0, s1)]
    dev = gpudev.Device(L)
    ctx, out = dev.ctx, dev.alloc(w * h * 12)
    try:
        _set_scene(L, ctx, W.scene, FORMS[0])
        assert L.pt_ctx_accum_track_noise(ctx, 1) == 0, L.pt_last_error()
        dev.render(PtConfig(w, h, 2, 0, seed, 0, 0, 0, 0), out, accumulate=True)
        f = _saved(L, ctx, tmp_path / "half2.ptacc")
        assert f["version"] == 2 and f["counts"].tolist() == [2] and f["n_a"].tolist() == [2]
        assert_planes(f["sums"], fs.planes(fs.total_over(sums, range(2))), "held at 2")
        assert_planes(f["a"], fs.planes(fs.total_over(sums, range(2))), "half A at 2")
        img, _ = dev.render(PtConfig(w, h, spp, 0, seed, 0, 0, 0, 0), out, accumulate=True)
        f = _saved(L, ctx, tmp_path / "half8.ptacc")
        assert f["version"] == 2 and f["counts"].tolist() == [spp] and f["n_a"].tolist() == [len(in_a)]
        total = fs.total_over(sums, range(spp))
        assert_planes(f["sums"], fs.planes(total), "held at 8")
        assert_planes(f["a"], fs.planes(fs.total_over(sums, in_a)), "half A at 8")
        same_bytes(img, fs.resolved(total, spp, clamp=True), "tracked frame")
    finally:
        dev.close()


# ---- 2. to_fixed and k_resolve at their edges ---------------------------------------------------------------------------------
PROBE_O, PROBE_D, PROBE_DEPTH = (0.0, 0.0, -5.0), (0.0, 0.0, -1.0), 11
SPHERE = dict(position=(0.0, 0.0, -10.0), radius=1.0, color=(0.5, 0.5, 0.5), emission=(1.0, 2.0, 3.0), reflect="Diffuse")


@pytest.fixture(scope="module")
def probe_scenes():
    """[(scene, index of the emitting sphere)]: the sphere alone, and beside the smallest BVH mesh boundary_rays builds (16
    triangles around (-1.2, 0, 0)), which the ray - from z = -5 down the z axis to the sphere at z = -10 - leaves behind"""
    cam = ptlib.make_camera((0.0, 0.0, 3.0), (0.0, 0.0, -1.0))
    alone = ptlib.Scene("probe_sphere", cam, [ptlib.make_sphere(**SPHERE)], [])
    small = next(sc for fam, sc in br.build_scenes(20261016) if sc.id == "bvh_small")
    mesh = small.objs[0]
    assert mesh.kind == ptlib.PT_MESH and mesh.tri_offset == 0 and mesh.tri_count == BVH_MIN_TRIS
    assert mesh.tri_count == min(small.objs[i].tri_count for i in range(small.n_objs))
    m = PtObject.from_buffer_copy(mesh)
    beside = ptlib.Scene("probe_sphere_bvh", cam, [m, ptlib.make_sphere(**SPHERE)], [small.tris[k] for k in range(mesh.tri_count)])
    out = [(alone, 0), (beside, 1)]
    for sc, index in out:
        t, oid, _, _, _ = ptlib.oracle_intersect(sc, [PROBE_O], [PROBE_D])
        assert int(oid[0]) == index and float(t[0]) == 4.0, (sc.id, oid, t)
    assert not _has_bvh(alone) and _has_bvh(beside)
    return out


def _radiance(L, ctx, n, backend, flags):
    out, st = np.zeros(3, np.float32), PtStats()
    rc = L.pt_ctx_radiance(ctx, _np_f(np.array(PROBE_O, np.float32)), _np_f(np.array(PROBE_D, np.float32)), PROBE_DEPTH, n, 7, 3,
                           backend, flags, _np_f(out), C.byref(st))
    assert rc == 0, L.pt_last_error()
    return out, st.ray_bounces


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_to_fixed_and_resolve_at_their_edges(L, form, probe_scenes):
    """frame_sums.table_cases through pt_ctx_radiance on the sphere alone and beside a BVH mesh, the emission changed by a
    material edit (pt_ctx_set_object) between cases: each channel's 32 bits are resolve(n * to_fixed(e), n), one bounce per
    sample.  The full table on the default wavefront form and the megakernel, n in {1, 3, 65, 1000} on the others."""
    name, env, backend, flags, _ = form
    cases = fs.table_cases(fs.SAMPLE_COUNTS if name in FULL_TABLE_FORMS else fs.SUBSET_COUNTS)
    dev = gpudev.Device(L, env=env)
    ctx = dev.ctx
    n_calls, secs = 0, 0.0
    try:
        for sc, index in probe_scenes:
            _set_scene(L, ctx, sc, form)
            obj = PtObject.from_buffer_copy(sc.objs[index])
            for n, triple in cases:
                obj.emission = ptlib.f3(*[float(e) for e in triple])
                assert L.pt_ctx_set_object(ctx, index, C.byref(obj), None) == 0, L.pt_last_error()  # a material edit
                t0 = time.perf_counter()
                got, bounces = _radiance(L, ctx, n, backend, flags)
                secs += time.perf_counter() - t0
                n_calls += 1
                want = np.array([fs.resolve(n * fs.to_fixed(e), n, clamp=False) for e in triple], np.float32)
                assert bounces == n, (name, sc.id, n, bounces)
                assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (
                    name, sc.id, n, [float(e) for e in triple], got.tolist(), want.tolist())
    finally:
        dev.close()
    print("%s: %d pt_ctx_radiance calls, %.3f ms per call" % (name, n_calls, 1e3 * secs / max(n_calls, 1)))


# ---- 3. the door --------------------------------------------------------------------------------------------------------------
def test_the_door_leaves_the_scene_untouched(L, probe_scenes):
    """pt_ctx_set_object, pt_ctx_set_scene and pt_render refuse an emission or colour component that is infinite, NaN or negative
    with PT_ERR_INVALID and a message naming the field; the context keeps the scene it had: the same tables, the same radiance"""
    sc, index = probe_scenes[1]
    dev = gpudev.Device(L)
    ctx = dev.ctx
    try:
        _set_scene(L, ctx, sc, FORMS[0])
        before = (C.c_uint64 * 14)()
        assert L.pt_ctx_table_hashes(ctx, before) == 0
        want, _ = _radiance(L, ctx, 3, 0, 0)
        assert want.tolist() == [1.0, 2.0, 3.0]
        for field, k, v in (("emission", 0, float("inf")), ("emission", 2, float("nan")), ("emission", 1, -1.0),
                            ("color", 1, -0.5), ("color", 2, float("inf"))):
            bad = PtObject.from_buffer_copy(sc.objs[index])
            getattr(bad, field)[k] = v
            assert L.pt_ctx_set_object(ctx, index, C.byref(bad), None) == PT_ERR_INVALID
            assert field.encode() in L.pt_last_error() and b"negative or not finite" in L.pt_last_error()
            objs = (PtObject * sc.n_objs)(*[sc.objs[i] for i in range(sc.n_objs)])
            objs[index] = bad
            assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), objs, sc.n_objs, sc.tris, sc.n_tris) == PT_ERR_INVALID
            assert ("object %d" % index).encode() in L.pt_last_error() and field.encode() in L.pt_last_error()
            frame = np.full((4 * 4, 3), 7.0, np.float32)
            cfg = PtConfig(4, 4, 1, 0, 1, 0, 0, 0, 0)
            assert L.pt_render(C.byref(cfg), C.byref(sc.cam), objs, sc.n_objs, sc.tris, sc.n_tris, _np_f(frame), None, None, None,
                               None) == PT_ERR_INVALID
            assert (frame == 7.0).all()
        after = (C.c_uint64 * 14)()
        assert L.pt_ctx_table_hashes(ctx, after) == 0 and list(after) == list(before)
        got, _ = _radiance(L, ctx, 3, 0, 0)
        assert got.tolist() == want.tolist()
    finally:
        dev.close()
