"""The hot-path intersect kernels on boundary rays and generated geometry (tests/boundary_rays.py), against the oracle.  -m gpu.

Ray by ray and bit for bit against pto_intersect_batch: the single-ray query (k_query), the wavefront's intersect step
(k_intersect_cand, or k_intersect<true> for BVH scenes) with and without PT_FLAG_NO_BVH, intersect_bounds and
orbit_point.  Through pt_ctx_radiance, which starts a real pass from a given ray, the pass kernels that shade inline:
k_pass_cand (flat and BVH forms: candidate filters, bvh_wants, the walk queue), the same under PT_WALK_QUEUE_CAP=128,
k_pass_bvh, k_pass, the separate kernels and k_mega_cand.  A pt_ctx_radiance call is one ray - one active lane - so its
walk queue never holds more than a few entries and the depth-first second walk of a small queue does not run there; the
frames of every generated scene through every device path (full waves) are where that form is compared."""
import ctypes as C
import time

import numpy as np
import pytest

import boundary_rays as br
import gpudev
import ptlib
from gpudev import L, new_ctx, set_scene  # noqa: F401  (L: fixture)
from ptlib import PtStats, _np_f

pytestmark = pytest.mark.gpu

SEED = 20261016
TOL = 1e-4
COUNTS = (1, 63, 64, 65, 4095, 4097)  # partial waves and partial streams; then the full set
FLAG_SEPARATE_KERNELS = ptlib.abi.PT_FLAG_SEPARATE_KERNELS
# pt_ctx_radiance probes (test_pass_kernels_first_hit): every target of these ray families with all its variants ...
PROBE_ALL_KINDS = ("tie", "box", "tiny_dir", "sphere")
# ... and of every other family this many targets, those whose oracle verdict flips across their variants first
PROBE_OTHER_TARGETS = 20


@pytest.fixture(scope="module")
def sets():
    return br.build(SEED)


@pytest.fixture(scope="module")
def gpu(L):
    ctx = new_ctx(L)
    yield L, ctx
    L.pt_ctx_destroy(ctx)


def _has_bvh(rs):
    return len(rs.tables["bvh_meshes"]) > 0


def _stream_ids(sc, oid, tid):
    """(object, triangle-in-object) of the oracle -> the hit id of pt_ctx_intersect_streams."""
    off = np.array([sc.objs[i].tri_offset for i in range(sc.n_objs)], np.int64)
    return np.where(oid < 0, -1, np.where(tid < 0, oid, sc.n_objs + off[np.maximum(oid, 0)] + tid)).astype(np.int32)


def _slices(n):
    return [c for c in COUNTS if c < n] + [n]


def test_tables_match_the_contexts_kernels(gpu, sets):
    """The dumped tables describe the scene pt_ctx_set_scene made: a scene has BVH walks in its pass kernel exactly when the
    dump holds BVH meshes, and the candidate scan exactly when the dump says the records fit."""
    L, ctx = gpu
    for rs in sets:
        set_scene(L, ctx, rs.scene)
        name = L.pt_ctx_pass_kernel(ctx, 0).decode()
        assert name == ("k_pass_cand_bvh" if _has_bvh(rs) else "k_pass_cand"), (rs.scene.id, name)
        assert L.pt_ctx_pass_kernel(ctx, ptlib.FLAG_NO_BVH).decode() == "k_pass"


def test_query_kernel_ray_by_ray(gpu, sets):
    """pt_ctx_intersect (k_query): t, object, triangle, point and normal of every boundary ray equal the oracle's, bit for
    bit, for 1, 63, 64, 65, 4 095, 4 097 rays and the whole set of every scene."""
    L, ctx = gpu
    for rs in sets:
        sc = rs.scene
        set_scene(L, ctx, sc)
        want = ptlib.oracle_intersect(sc, rs.o, rs.d)
        for m in _slices(rs.n):
            o, d = np.ascontiguousarray(rs.o[:m]), np.ascontiguousarray(rs.d[:m])
            t, oid, tid = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32)
            x, nr = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
            rc = L.pt_ctx_intersect(ctx, _np_f(o), _np_f(d), m, _np_f(t), oid.ctypes.data_as(ptlib.i32p),
                                    tid.ctypes.data_as(ptlib.i32p), _np_f(x), _np_f(nr))
            assert rc == 0, L.pt_last_error()
            bad = (oid != want[1][:m]) | (tid != want[2][:m]) | (t.view(np.uint32) != want[0][:m].view(np.uint32))
            assert not bad.any(), (sc.id, m, int(bad.sum()), [br.RAY_KINDS[k] for k in np.unique(rs.kind[:m][bad])])
            assert np.array_equal(x.view(np.uint32), want[3][:m].view(np.uint32)), (sc.id, m, "x")
            assert np.array_equal(nr.view(np.uint32), want[4][:m].view(np.uint32)), (sc.id, m, "normal")


@pytest.mark.parametrize("flags", [0, ptlib.FLAG_NO_BVH], ids=["scan", "no_bvh"])
def test_stream_intersect_kernels_on_boundary_rays(gpu, sets, flags):
    """pt_ctx_intersect_streams - the wavefront's own intersect step (candidate filters, ring, dense batches; parked walks
    for BVH scenes; with PT_FLAG_NO_BVH every triangle) - on every boundary ray: the same primitive and the same distance
    bits as the oracle, +inf on a miss, for the same ray counts."""
    L, ctx = gpu
    for rs in sets:
        sc = rs.scene
        set_scene(L, ctx, sc)
        t0, oid0, tid0, _, _ = ptlib.oracle_intersect(sc, rs.o, rs.d)
        want = _stream_ids(sc, oid0, tid0)
        for m in _slices(rs.n):
            o, d = np.ascontiguousarray(rs.o[:m]), np.ascontiguousarray(rs.d[:m])
            t, ids = np.zeros(m, np.float32), np.zeros(m, np.int32)
            rc = L.pt_ctx_intersect_streams(ctx, _np_f(o), _np_f(d), m, flags, _np_f(t), ids.ctypes.data_as(ptlib.i32p))
            assert rc == 0, L.pt_last_error()
            hit = want[:m] >= 0
            bad = (ids != want[:m]) | (hit & (t.view(np.uint32) != t0[:m].view(np.uint32))) | (~hit & (t != np.inf))
            assert not bad.any(), (sc.id, flags, m, int(bad.sum()), [br.RAY_KINDS[k] for k in np.unique(rs.kind[:m][bad])])


def test_bounds_and_orbit_point_on_boundary_rays(gpu, sets):
    """pt_ctx_intersect_bounds of every object and pt_ctx_orbit_point against the oracle's counterparts, bit for bit, for the
    same ray counts (the whole set: at most 20 000 rays of it)."""
    L, ctx = gpu
    O = ptlib.oracle()
    for rs in sets:
        sc = rs.scene
        set_scene(L, ctx, sc)
        boxes = ptlib.oracle_boxes(sc)
        ps = sc.pto()
        for m in _slices(min(rs.n, 20000)):
            o, d = np.ascontiguousarray(rs.o[:m]), np.ascontiguousarray(rs.d[:m])
            for k in range(sc.n_objs):
                res = []
                for fn, first in ((O.pto_intersect_bounds_batch, None), (L.pt_ctx_intersect_bounds, ctx)):
                    hit, t = np.zeros(m, np.int32), np.zeros(m, np.float32)
                    x, nr = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
                    if first is None:
                        fn(C.byref(ps), boxes, k, _np_f(o), _np_f(d), m, hit.ctypes.data_as(ptlib.i32p), _np_f(t), _np_f(x),
                           _np_f(nr))
                    else:
                        assert fn(first, k, _np_f(o), _np_f(d), m, hit.ctypes.data_as(ptlib.i32p), _np_f(t), _np_f(x),
                                  _np_f(nr)) == 0, L.pt_last_error()
                    res.append((hit, t.view(np.uint32), x.view(np.uint32), nr.view(np.uint32)))
                for a, b, what in zip(res[0], res[1], ("hit", "t", "x", "n")):
                    assert np.array_equal(a, b), (sc.id, m, k, what, int((a != b).sum()))
            res = []
            for fn, first in ((O.pto_orbit_point_batch, None), (L.pt_ctx_orbit_point, ctx)):
                f, oid = np.zeros(m, np.int32), np.zeros(m, np.int32)
                p, t = np.zeros((m, 3), np.float32), np.zeros(m, np.float32)
                if first is None:
                    fn(C.byref(ps), boxes, _np_f(o), _np_f(d), m, f.ctypes.data_as(ptlib.i32p), _np_f(p),
                       oid.ctypes.data_as(ptlib.i32p), _np_f(t))
                else:
                    assert fn(first, _np_f(o), _np_f(d), m, f.ctypes.data_as(ptlib.i32p), _np_f(p), oid.ctypes.data_as(ptlib.i32p),
                              _np_f(t)) == 0, L.pt_last_error()
                res.append((f, oid, p.view(np.uint32), t.view(np.uint32)))
            for a, b, what in zip(res[0], res[1], ("found", "object", "point", "t")):
                assert np.array_equal(a, b), (sc.id, m, what, int((a != b).sum()))


# the pass-kernel forms pt_ctx_radiance reaches: (name, tuning variables of the context, backend, flags, kernel the context
# must report for a scene with BVH meshes / without)
PASS_FORMS = [
    ("pass_cand", {}, 0, 0, ("k_pass_cand_bvh", "k_pass_cand")),
    ("pass_cand_small_queue", {"PT_WALK_QUEUE_CAP": "128"}, 0, 0, ("k_pass_cand_bvh", "k_pass_cand")),
    ("pass_bvh", {"PT_CAND_BVH": "0"}, 0, 0, ("k_pass_bvh", "k_pass_cand")),
    ("pass_no_bvh", {}, 0, ptlib.FLAG_NO_BVH, ("k_pass", "k_pass")),
    ("separate", {}, 0, FLAG_SEPARATE_KERNELS, ("k_intersect", "k_intersect_cand")),
    ("mega", {}, 1, 0, (None, None)),
]


def _probe_rays(rs):
    """The rays probed through pt_ctx_radiance, stratified by ray family: every target of PROBE_ALL_KINDS, and of each other
    family PROBE_OTHER_TARGETS targets (those whose oracle verdict flips across their variants first, then at random);
    each target with all its variants."""
    t, oid, tid, _, _ = ptlib.oracle_intersect(rs.scene, rs.o, rs.d)
    flips = br.verdict_flips(np.where(oid < 0, -1, oid.astype(np.int64) * (1 << 20) + np.maximum(tid, 0)))
    kinds = rs.kind[::br.VARIANTS]
    rng = np.random.default_rng(7)
    targets = []
    for k, name in enumerate(br.RAY_KINDS):
        mine = np.flatnonzero(kinds == k)
        if name not in PROBE_ALL_KINDS:
            mine = np.concatenate([rng.permutation(mine[flips[mine]]), rng.permutation(mine[~flips[mine]])])[:PROBE_OTHER_TARGETS]
        targets.append(np.sort(mine))
    targets = np.concatenate(targets)
    return (targets[:, None] * br.VARIANTS + np.arange(br.VARIANTS)[None, :]).reshape(-1)


def _radiance(L, ctx, o, d, depth, n, seed, pixel, backend, flags):
    out = np.zeros(3, np.float32)
    st = PtStats()
    rc = L.pt_ctx_radiance(ctx, _np_f(np.ascontiguousarray(o, np.float32)), _np_f(np.ascontiguousarray(d, np.float32)),
                           depth, n, seed, pixel, backend, flags, _np_f(out), C.byref(st))
    assert rc == 0, L.pt_last_error()
    return out, st.ray_bounces


def test_pass_kernels_first_hit(gpu, sets):
    """Every pass-kernel form through pt_ctx_radiance on boundary rays: every tie, box, tiny-component and sphere target and
    a share of every other ray family, with all their ulp variants.  (a) The scene made black with a distinct emission per
    object: at depth 5 roulette always stops at the first hit (max_reflection = 0, pt_oracle.c), so the radiance is exactly
    the emission of the object the kernel's intersection found, or zero on a miss - bit for bit the oracle's, with one
    intersect_scene evaluation.  (b) The same rays at depth 0 with the scene's colours kept: a different triangle or t
    changes the rest of the path (same bounce count, radiance as the shading known-answer tests compare it)."""
    L, _ = gpu
    ctxs = [(name, new_ctx(L, env), backend, flags, kernels) for name, env, backend, flags, kernels in PASS_FORMS]
    n_calls, secs, per_kind = 0, 0.0, np.zeros(len(br.RAY_KINDS), np.int64)
    try:
        for rs in sets:
            first = br.first_hit_variant(rs.scene)
            shaded = br.first_hit_variant(rs.scene, keep_color=True)
            pick = _probe_rays(rs)
            per_kind += np.bincount(rs.kind[pick], minlength=len(br.RAY_KINDS))
            want = {}
            for tag, sc, depth, seed in (("first", first, 5, 3), ("shaded", shaded, 0, 5)):
                rgb, bounces = np.zeros((len(pick), 3), np.float32), np.zeros(len(pick), np.int64)
                for j, i in enumerate(pick):
                    ref, cnt = ptlib.oracle_radiance(sc, rs.o[i], rs.d[i], depth, 1, seed, int(i))
                    rgb[j], bounces[j] = ref, cnt.ray_bounces
                want[tag] = (sc, depth, seed, rgb, bounces)
            assert np.all(want["first"][4] == 1)
            for name, ctx, backend, flags, kernels in ctxs:
                for tag in ("first", "shaded"):
                    sc, depth, seed, ref, ref_b = want[tag]
                    set_scene(L, ctx, sc)
                    want_kernel = kernels[0] if _has_bvh(rs) else kernels[1]
                    if want_kernel is not None:
                        assert L.pt_ctx_pass_kernel(ctx, flags).decode() == want_kernel, (name, rs.scene.id)
                    got, got_b = np.zeros((len(pick), 3), np.float32), np.zeros(len(pick), np.int64)
                    t0 = time.perf_counter()
                    for j, i in enumerate(pick):
                        got[j], got_b[j] = _radiance(L, ctx, rs.o[i], rs.d[i], depth, 1, seed, int(i), backend, flags)
                    secs += time.perf_counter() - t0
                    n_calls += len(pick)
                    where = lambda bad: [(int(pick[j]), br.RAY_KINDS[rs.kind[pick[j]]]) for j in np.flatnonzero(bad)[:5]]
                    bad = got_b != ref_b
                    assert not bad.any(), (name, tag, rs.scene.id, int(bad.sum()), where(bad))
                    if tag == "first":
                        bad = np.any(got.view(np.uint32) != ref.view(np.uint32), axis=1)
                    else:
                        bad = ~np.all(np.isclose(got, ref, rtol=2e-6, atol=0), axis=1)
                    assert not bad.any(), (name, tag, rs.scene.id, int(bad.sum()), where(bad))
    finally:
        for c in ctxs:
            L.pt_ctx_destroy(c[1])
    print("pt_ctx_radiance: %d calls, %.3f ms per call; rays per family %s" %
          (n_calls, 1e3 * secs / max(n_calls, 1), dict(zip(br.RAY_KINDS, per_kind.tolist()))))


def test_frames_of_the_generated_scenes(gpu, sets):
    """A frame of every generated scene through every device path: bounce count equal to the oracle's, image within TOL of
    the oracle's, and all device paths the same image bit for bit."""
    L, _ = gpu
    w, h, spp = 40, 28, 4
    paths = [(name, env, backend, flags) for name, env, backend, flags, _ in PASS_FORMS]
    devs = {name: gpudev.Device(L, env=env) for name, env, _, _ in paths}
    outs = {name: dev.alloc(w * h * 12) for name, dev in devs.items()}
    try:
        for k, rs in enumerate(sets):
            sc = br.first_hit_variant(rs.scene, keep_color=True)
            want, cnt, _ = ptlib.oracle_render(sc, w, h, spp, 40 + k)
            ref = None
            for name, env, backend, flags in paths:
                dev = devs[name]
                set_scene(L, dev.ctx, sc)
                img, st = dev.render(gpudev.config(w, h, spp, backend=backend, seed=40 + k, flags=flags), outs[name])
                assert st.ray_bounces == cnt.ray_bounces, (rs.scene.id, name, st.ray_bounces, cnt.ray_bounces)
                assert float(np.abs(img - want).max()) <= TOL, (rs.scene.id, name)
                if ref is None:
                    ref = img
                else:
                    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (rs.scene.id, name)
    finally:
        for dev in devs.values():
            dev.close()
