"""shade_surface at the edges of what its square roots now assume.  The diffuse basis, the diffuse direction, sqrt(1 - r2) and the
glass body's tdir take f_sqrt's fast path WITHOUT the range test (csrc/pt_math.h: f_sqrt_ranged, normalize_ranged; the bound
stands at each call site of csrc/pt_device.h), sincos_f32 is the fused form, and cand_spheres accepts on the far root alone.
Here the device (pt_ctx_scatter) meets tests/kats_scatter.py's restatement, bit for bit, on items chosen where those
preconditions are tightest:

- given surfaces, one launch: normals along each axis and its negation; |w.x| on both sides of 0.1f (the basis switches its helper
  axis there: the squared length of the cross product is smallest, 0.01, just above it) with the rest of the normal in y, in z and
  in both; unit normals as a normalisation leaves them (|n|^2 = 1 +- a few ulp); glass entered and left at normal incidence and on
  both sides of total internal reflection (cos2t -> 0); draws whose 24-bit r2 is 0, 1 and 2^24 - 1 (1 - r2 = 1, 1 - 2^-24, 2^-24)
  and whose r1 index is 0, 2^24 - 1 and m 2^21 +- 1 for m = 1..7: every quarter turn the reduction switches at (n = 0..4) and
  every axis a quadrant starts on.
- cornell by rank, one launch: each of its four spheres (mirror, glass, emitter, matte) hit at the pole and at grazing incidence
  (0.1 % of the radius inside the silhouette), the glass sphere also from inside: at the centre (normal incidence) and on chords
  on both sides of total internal reflection.  The hit and its normal are the oracle's intersect_scene; the step is the restatement's.

Every item is compared: directions and weights of every child, depth, branch, n_rays, the hit point.  Nothing is skipped.
The draws cannot be injected: (pixel, sample) of r1_last and r2_one below were found like kats_scatter.DRAWS, by the sweep of
tools/find_scatter_draws.py (its philox7 over samples 0 .. 2^24 - 1 of pixel 0, tag (1 << 8) | 1) for word 1 >> 8 = 2^24 - 1 and
word 2 >> 8 = 1; test_draws_are_the_extremes re-checks all of them on the CPU."""
import numpy as np
import pytest

import gpudev
import kats_scatter as ks
import ptlib
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtScatterOut
import scatter_walk as sw
from scatter_walk import bits

f32 = np.float32
EXTRA_DRAWS = {"r1_last": (0, 5916095), "r2_one": (0, 7511904)}  # name -> (pixel, sample); depth 0, branch 1
DRAW_WORDS = dict([(n, (w, k)) for n, w, k, _, _ in ks.DRAW_TARGETS if n.startswith("r")] +
                  [("r1_last", (1, (1 << 24) - 1)), ("r2_one", (2, 1))])
GREY, BLACK = ks.v3(0.75, 0.5, 0.25), ks.v3(0, 0, 0)


def _unit(v):
    """v normalised in binary32 as the reference normalises: unit to within rounding, not exactly"""
    return ks.normalize(ks.v3(*v))


def _case(name, d, n, reflect, depth=0, branch=1, pixel=7, sample=3, x=(0.5, -0.25, 2.0)):
    return dict(name=name, d=ks.v3(*d), n=ks.v3(*n), reflect=reflect, depth=depth, branch=branch, pixel=pixel, sample=sample,
                color=GREY, emission=BLACK, x=ks.v3(*x), o=ks.v3(*x) - ks.v3(*d))


def _given_cases():
    out = []
    # ---- the basis: axes, and |w.x| around 0.1f with the remainder of the unit normal in y, in z, in both
    for i, axis in enumerate("xyz"):
        for s in (1.0, -1.0):
            n = [0.0, 0.0, 0.0]
            n[i] = s
            out.append(_case("axis_%s%s" % ("+" if s > 0 else "-", axis), [-v for v in n], n, ks.DIFFUSE))
    for sign in (1.0, -1.0):
        for k in (-1, 0, 1):
            wx = f32(sign) * ks.ulps(0.1, k)
            rest = np.sqrt(ks.ONE - wx * wx)
            h = f32(np.sqrt(0.5)) * rest
            for tag, n in (("y", (wx, rest, 0)), ("z", (wx, 0, rest)), ("yz", (wx, h, -h))):
                out.append(_case("wx_%s0.1f%+dulp_%s" % ("+" if sign > 0 else "-", k, tag), [-v for v in n], n, ks.DIFFUSE,
                                 pixel=20 + k, sample=5))
    rng = np.random.default_rng(20261019)
    for j in range(12):  # normals as a normalisation leaves them, with draws of their own; some seen from behind (flipped)
        n = _unit(rng.standard_normal(3))
        d = _unit(rng.standard_normal(3))
        out.append(_case("unit_normal_%d" % j, d, n, ks.DIFFUSE if j % 3 else ks.REFRACT, depth=j % 4, pixel=100 + j, sample=j))
    # ---- the draws: r2 = 0, 2^-24, 1 - 2^-24; r1 index 0, 2^24 - 1 and around every eighth of a turn
    draws = dict(ks.DRAWS)
    draws.update(EXTRA_DRAWS)
    for name in sorted(DRAW_WORDS):
        pixel, sample = draws[name]
        for j, n in enumerate(((0, 0, 1), _unit((0.1, 0.7, -0.7)))):
            out.append(_case("draw_%s_n%d" % (name, j), _unit((0.28, -0.96, -0.5)), n, ks.DIFFUSE, 0, 1, pixel, sample))
    # ---- glass: entering and leaving at normal incidence, entering at grazing incidence, leaving around cos2t = 0
    for depth in (0, 2):  # new_depth 1: both subtrees; 3: one of them
        out.append(_case("glass_in_normal_d%d" % depth, (0, 0, -1), (0, 0, 1), ks.REFRACT, depth))
        out.append(_case("glass_out_normal_d%d" % depth, (0, 0, 1), (0, 0, 1), ks.REFRACT, depth))
        out.append(_case("glass_in_grazing_d%d" % depth, _unit((1, 0, -(2.0 ** -10))), (0, 0, 1), ks.REFRACT, depth))
        for k in (-2, -1, 0, 1, 2):
            z = ks.ulps(ks.GLASS_INSIDE_Z, k)
            out.append(_case("glass_out_tir%+dulp_d%d" % (k, depth), (np.sqrt(ks.ONE - z * z), 0, z), (0, 0, 1), ks.REFRACT, depth))
            n = _unit((0.3, -0.2, 0.9))  # the same incidence on a tilted surface: d = sin t + cos n, t a unit tangent
            t = _unit(ks.cross(n, ks.v3(0, 1, 0)))
            out.append(_case("glass_out_tilted_tir%+dulp_d%d" % (k, depth), t * np.sqrt(ks.ONE - z * z) + n * z, n, ks.REFRACT, depth))
    return out


GIVEN_CASES = _given_cases()


def _sphere_rays(sc):
    """(name, origin, direction, depth, sphere) on cornell's four spheres"""
    rays = []
    for i in range(4):
        o = sc.objs[i]
        assert o.kind == ptlib.PT_SPHERE
        c, r = ks.v3(*o.position), f32(o.radius)
        up = c + ks.v3(0, r + f32(0.25), 0)
        for depth in (0, 3):
            rays.append(("sphere%d_pole_d%d" % (i, depth), up, ks.v3(0, -1, 0), depth, i))
            rays.append(("sphere%d_grazing_d%d" % (i, depth), up + ks.v3(r * f32(0.999), 0, 0), ks.v3(0, -1, 0), depth, i))
            rays.append(("sphere%d_oblique_d%d" % (i, depth), c + _unit((0.3, 0.8, 0.52)) * (r + f32(0.25)), -_unit((0.3, 0.8, 0.52)), depth, i))
    glass = [i for i in range(4) if sc.objs[i].reflect_type == ks.REFRACT]
    assert len(glass) == 1
    c, r = ks.v3(*sc.objs[glass[0]].position), f32(sc.objs[glass[0]].radius)
    for depth in (0, 2):
        rays.append(("glass_centre_d%d" % depth, c, _unit((0.48, 0.6, 0.64)), depth, glass[0]))
        for frac in (0.5, 0.66, 0.6666, 0.6667, 0.67, 0.9):  # sin(incidence) = frac: total internal reflection above 2/3
            rays.append(("glass_chord_%g_d%d" % (frac, depth), c + ks.v3(r * f32(frac), 0, 0), ks.v3(0, 1, 0), depth, glass[0]))
    return rays


def _scatter(L, ctx, form, items, surfs, seed):
    out = (PtScatterOut * len(items))()
    for o in out:
        o.hit = 12345
    assert L.pt_ctx_scatter(ctx, seed, form, items, surfs, len(items), out) == 0, L.pt_last_error().decode()
    return out


def _compare(name, o, want, depth):
    """one device result against kats_scatter.scatter's: every child, bit for bit"""
    assert o.deferred == 0, name
    assert o.n_rays == len(want["children"]), (name, o.n_rays, want["kind"])
    got = ((o.d0, o.thr0, o.depth0, o.branch0), (o.d1, o.thr1, o.depth1, o.branch1))
    for (d, w, cdepth, cbranch), (gd, gw, gdepth, gbranch) in zip(want["children"], got):
        assert bits(gd) == d.tobytes(), (name, want["kind"], list(gd), d)
        assert bits(gw) == w.tobytes(), (name, want["kind"], list(gw), w)
        assert (gdepth, gbranch) == (cdepth, cbranch) and cdepth == depth + 1, name
    return want["kind"]


@pytest.mark.gpu
def test_given_surfaces_at_the_edges(L):
    assert 64 <= len(GIVEN_CASES) <= 256
    with gpudev.Device(L) as dev:
        items, surfs = sw.case_arrays(GIVEN_CASES)
        got = _scatter(L, dev.ctx, sw.GIVEN, items, surfs, ks.SEED)
    kinds = {}
    for c, o in zip(GIVEN_CASES, got):
        assert o.hit == 0 and bits(o.x) == c["x"].tobytes(), c["name"]
        kind = _compare(c["name"], o, ks.expected(c, thr=(1, 1, 1)), c["depth"])
        kinds[kind] = kinds.get(kind, 0) + 1
    assert sum(kinds.values()) == len(GIVEN_CASES)
    assert set(kinds) >= {"diffuse", "split", "tir", "choice_trans"}, kinds


@pytest.mark.gpu
def test_cornell_spheres_at_pole_and_grazing(L):
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    rays = _sphere_rays(sc)
    o = np.array([r[1] for r in rays], dtype=f32)
    d = np.array([r[2] for r in rays], dtype=f32)
    t, oid, _, x, nrm = ptlib.oracle_intersect(sc, o, d)
    for r, hit in zip(rays, oid):
        assert hit == r[4], (r[0], hit)  # the ray reaches the sphere it was aimed at
    items = (ptlib.PtScatterItem * len(rays))(*[sw.item(o[i], d[i], (1, 1, 1), 40 + i, 2 * i + 1, rays[i][3], 1) for i in range(len(rays))])
    with gpudev.Device(L, sc) as dev:
        ctx = dev.ctx
        got = _scatter(L, ctx, sw.BY_RANK, items, None, ks.SEED)
    kinds = set()
    for i, (r, g) in enumerate(zip(rays, got)):
        obj = sc.objs[r[4]]
        assert g.hit == r[4] and bits(g.x) == x[i].tobytes(), (r[0], g.hit)
        u = ks.draws(ks.SEED, 40 + i, 2 * i + 1, r[3], 1)
        want = ks.scatter(d[i], nrm[i], obj.color, obj.emission, obj.reflect_type, r[3], 1, u, thr=(1, 1, 1))
        kinds.add(_compare(r[0], g, want, r[3]))
        assert bits(g.contrib) == want["contrib"].tobytes() and bool(g.emits) == any(v != 0 for v in obj.emission), r[0]
    assert kinds >= {"diffuse", "mirror", "split", "tir"}, kinds


def test_draws_are_the_extremes():
    """CPU: the committed counters give the 24-bit values their names promise (kats_scatter's Philox, depth 0, branch 1)"""
    draws = dict(ks.DRAWS)
    draws.update(EXTRA_DRAWS)
    for name, (word, k) in DRAW_WORDS.items():
        pixel, sample = draws[name]
        u = ks.draws(ks.SEED, pixel, sample, 0, 1)
        assert u[word] == f32(k) * f32(2.0 ** -24), (name, u)
    assert {k for _, k in DRAW_WORDS.values()} >= {0, 1, (1 << 24) - 1} | {m << 21 for m in range(1, 8)}
    # the r1 indices sit in every quarter turn the reduction can name
    assert {ks.quadrant(k) for w, k in DRAW_WORDS.values() if w == 1} == {0, 1, 2, 3, 4}
