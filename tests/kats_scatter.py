"""ONE radiance() invocation after `intersect_scene` returned Some (src/render/mod.rs:665-789), restated INDEPENDENTLY in numpy
binary32 from the Rust text:

    let mut color = object.material.color;  let max_reflection = color.x.max(color.y.max(color.z));            // :667-668
    let normal_towards_ray = if hit.normal.dot(ray.direction) < 0.0 { hit.normal } else { hit.normal * -1.0 };  // :669-673
    let new_depth = depth + 1;                                                                                  // :676
    if new_depth > 5 { if rand01() < max_reflection && new_depth < MAX_DEPTH { color = color * (1.0 / max_reflection) }
                       else { return emmission } }                                                               // :677-683
    Diffuse:  r1 = 2.0 * PI * rand01(); r2 = rand01(); r2s = r2.sqrt(); w = normal_towards_ray;                 // :691-694
              u = (if w.x.abs() > 0.1 { (0,1,0) } else { (1,0,0) }).cross(w).normalize(); v = w.cross(u);       // :695-702
              d = (u * r1.cos() * r2s + v * r1.sin() * r2s + w * (1.0 - r2).sqrt()).normalize()                 // :703-704
    Specular: direction - normal * 2.0 * normal.dot(direction)                                                  // :722-723
    Refract:  into = normal.dot(normal_towards_ray) > 0.0; nnt = if into { 1.0 / 1.5 } else { 1.5 / 1.0 };       // :736-739
              ddn = direction.dot(normal_towards_ray); cos2t = 1.0 - nnt.powi(2) * (1.0 - ddn.powi(2));         // :740-741
              cos2t < 0.0: the reflected ray alone                                                              // :743-744
              tdir = (direction * nnt - normal * (if into { 1.0 } else { -1.0 } * (ddn * nnt + cos2t.sqrt()))).normalize()
              r0 = a * a / (b * b) (a = 0.5, b = 2.5); c = 1.0 - (if into { -ddn } else { tdir.dot(normal) });  // :750-753
              re = r0 + (1.0 - r0) * c.powi(5); tr = 1.0 - re; p = 0.25 + 0.5 * re; rp = re / p; tp = tr / (1.0 - p)
              new_depth > 2: rand01() < p ? reflected * rp : transmitted * tp;  else both, * re and * tr        // :760-786

with glam 0.30.8's scalar Vec3 (dot = (xx' + yy') + zz'; cross = (yz' - y'z, zx' - z'x, xy' - x'y); normalize = v * (1 /
length); + and * by component), powi(2) = x * x, powi(5) = c * ((c * c) * (c * c)), f32::sin / f32::cos = the platform libm's
sinf / cosf (through ctypes; numpy's float32 sin is another routine) and every intermediate a np.float32.  Nothing is imported
from the oracle or the product.  The draws are the parity contract's: words 0 (roulette), 1 (r1 / the
choice) and 2 (r2) of Philox4x32-7 with counter (pixel, sample, (branch << 8) | new_depth, 0), key = seed - kats_camera's
Philox, which Random123's vectors pin - mapped to [0, 1) as rand 0.8.5 does.

scatter() returns the emission, the alive flag and the children: direction, weight w with
    radiance = emission + sum over children of w (*) radiance(child),
child depth and branch.  w is colour' (diffuse, mirror, total internal reflection), fl(colour' * Re), fl(colour' * Tr) (split),
fl(colour' * RP), fl(colour' * TP) (choice), colour' being the colour after the roulette's rescale.

THE ONE THING HERE THAT IS NOT THE RUST TEXT: with an incoming throughput `thr` the device carries weights DOWN the path, so the
contract for its thr0 / thr1 is fl(fl(thr * colour') * factor) per channel (factor: none, Re, Tr, RP or TP) and contrib = fl(thr *
emission).  With thr = (1, 1, 1) both are the table above bit for bit, 1 * x being x.

CASES are the edge cases (module end): every input a binary32 value, every boundary with its 1 and 2 ulp neighbours on both
sides, each with the outcome the restatement must report for it (tests/test_scatter_abi.py asserts those on the CPU,
tests/test_gpu_scatter.py runs them on the device).  Draws cannot be injected: the (pixel, sample) pairs of DRAWS were found by
tools/find_scatter_draws.py, a search over this module's Philox, and are re-checked by the tests.
"""
import ctypes
import ctypes.util

import numpy as np

from kats_camera import philox4x32, unit

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.argtypes = _libm.cosf.argtypes = [ctypes.c_float]
_libm.sinf.restype = _libm.cosf.restype = ctypes.c_float

DIFFUSE, SPECULAR, REFRACT = 0, 1, 2
MAX_DEPTH = 12
ONE, TWO, ZERO = f32(1.0), f32(2.0), f32(0.0)
PI = f32(3.141592653589793)  # std::f32::consts::PI
ONES = np.ones(3, dtype=f32)


def sinf(x):
    return f32(_libm.sinf(float(x)))


def cosf(x):
    return f32(_libm.cosf(float(x)))


def v3(*a):
    return np.array(a, dtype=f32)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], dtype=f32)


def normalize(v):
    return v * (ONE / np.sqrt(dot(v, v)))


def draws(seed, pixel, sample, depth, branch):
    """the three rand01() a radiance(ray, depth) call of branch `branch` may take: roulette, r1 / choice, r2"""
    w = philox4x32([pixel, sample, (branch << 8) | (depth + 1), 0], [seed & 0xFFFFFFFF, seed >> 32])
    return unit(w[0]), unit(w[1]), unit(w[2])


def scatter(d, n, color, emission, reflect, depth, branch, u, thr=None):
    """d: ray.direction, n: hit.normal, u: draws().  Returns a dict: emission, alive, kind ('dead', 'diffuse', 'mirror', 'tir',
    'split', 'choice_refl', 'choice_trans'), children [(direction, weight, depth, branch)], contrib (thr given), and what the
    step decided on the way (flipped, axis, cos2t, re, tr, p), for the boundary assertions."""
    with np.errstate(all="ignore"):
        d, n, color, emission = v3(*d), v3(*n), v3(*color), v3(*emission)
        out = dict(emission=emission, alive=True, kind="dead", children=[])
        if thr is not None:
            thr = v3(*thr)
            out["contrib"] = thr * emission
        max_reflection = max(color[0], max(color[1], color[2]))
        flipped = not (dot(n, d) < ZERO)
        nl = n * f32(-1.0) if flipped else n
        out["flipped"] = flipped
        new_depth = depth + 1
        if new_depth > 5:
            if u[0] < max_reflection and new_depth < MAX_DEPTH:
                color = color * (ONE / max_reflection)
            else:
                out["alive"] = False
                return out
        carried = color if thr is None else thr * color

        def child(direction, factor=None, b=branch):
            out["children"].append((direction, carried if factor is None else carried * factor, new_depth, b))

        if reflect == DIFFUSE:
            r1 = TWO * PI * u[1]
            r2 = u[2]
            r2s = np.sqrt(r2)
            w = nl
            out["axis"] = "Y" if abs(w[0]) > f32(0.1) else "X"
            uu = normalize(cross(v3(0, 1, 0) if out["axis"] == "Y" else v3(1, 0, 0), w))
            vv = cross(w, uu)
            out["kind"] = "diffuse"
            child(normalize(uu * cosf(r1) * r2s + vv * sinf(r1) * r2s + w * np.sqrt(ONE - r2)))
            return out
        refl = d - n * TWO * dot(n, d)
        if reflect == SPECULAR:
            out["kind"] = "mirror"
            child(refl)
            return out
        into = bool(dot(n, nl) > ZERO)
        nc, nt = ONE, f32(1.5)
        nnt = nc / nt if into else nt / nc
        ddn = dot(d, nl)
        cos2t = ONE - (nnt * nnt) * (ONE - ddn * ddn)
        out.update(into=into, cos2t=cos2t)
        if cos2t < ZERO:
            out["kind"] = "tir"
            child(refl)
            return out
        tdir = normalize(d * nnt - n * ((ONE if into else f32(-1.0)) * (ddn * nnt + np.sqrt(cos2t))))
        a, b = nt - nc, nt + nc
        r0 = a * a / (b * b)
        c = ONE - (-ddn if into else dot(tdir, n))
        re = r0 + (ONE - r0) * (c * ((c * c) * (c * c)))
        tr = ONE - re
        p = f32(0.25) + f32(0.5) * re
        rp = re / p
        tp = tr / (ONE - p)
        out.update(re=re, tr=tr, p=p)
        if new_depth > 2:
            if u[1] < p:
                out["kind"] = "choice_refl"
                child(refl, rp)
            else:
                out["kind"] = "choice_trans"
                child(tdir, tp)
        else:
            out["kind"] = "split"
            child(refl, re, 2 * branch)
            child(tdir, tr, 2 * branch + 1)
        return out


def quadrant(k):
    """which quarter turn sinf / cosf reduce r1 = 2 pi k 2^-24 to: rint(r1 * 2 / pi), in binary64 (a diagnostic for the cases'
    own assertions, not part of the restatement)"""
    r1 = TWO * PI * (f32(k) * f32(2.0 ** -24))
    return int(np.rint(np.float64(r1) * 2.0 / np.pi))


# ------------------------------------------------------------------------------------------------------------- the cases
SEED = 0x5CA77E12D1FF05E

# (pixel, sample) whose draw of the block (SEED; pixel, sample, tag) has the wanted 24 bits, found by tools/find_scatter_draws.py:
# name -> (word, k = word >> 8, depth, branch, pixel, sample)
R1_TURNS = [m << 21 for m in range(1, 8)]  # r1 = m pi / 4: sinf / cosf change quadrant at the odd m, an axis is crossed at the even
DRAW_TARGETS = ([("r1_k0", 1, 0, 0, 1)] + [("r1_k%d%+d" % (k, e), 1, k + e, 0, 1) for k in R1_TURNS for e in (-1, 0, 1)]
                + [("r2_zero", 2, 0, 0, 1), ("r2_last", 2, (1 << 24) - 1, 0, 1)])
DRAWS = {
    "r1_k0": (1, 9575405),
    "r1_k2097152-1": (2, 9966653),
    "r1_k2097152+0": (1, 7312627),
    "r1_k2097152+1": (0, 11853238),
    "r1_k4194304-1": (1, 5561070),
    "r1_k4194304+0": (0, 805765),
    "r1_k4194304+1": (1, 14748480),
    "r1_k6291456-1": (0, 7974264),
    "r1_k6291456+0": (2, 10504471),
    "r1_k6291456+1": (2, 2686151),
    "r1_k8388608-1": (1, 326397),
    "r1_k8388608+0": (1, 10641136),
    "r1_k8388608+1": (0, 1514646),
    "r1_k10485760-1": (0, 1842403),
    "r1_k10485760+0": (0, 15442670),
    "r1_k10485760+1": (0, 3653314),
    "r1_k12582912-1": (1, 13512451),
    "r1_k12582912+0": (0, 1924807),
    "r1_k12582912+1": (0, 3305016),
    "r1_k14680064-1": (0, 1663536),
    "r1_k14680064+0": (0, 4859122),
    "r1_k14680064+1": (1, 265878),
    "r2_zero": (0, 9582848),
    "r2_last": (0, 238371),
    "choice_eq_p": (2, 11111963),
    "choice_eq_p_next": (1, 10055898),
    "choice_eq_p_prev": (1, 3857063),
    "choice_eq_p_next2": (0, 212071),
    "choice_eq_p_prev2": (0, 6343906),
}


def ulps(x, k):
    """x moved by k units in the last place (k < 0: towards -inf)"""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


def _unit_xy(wx):
    """a normal (wx, fl(sqrt(1 - wx^2)), 0): unit to rounding, its x exactly wx"""
    wx = f32(wx)
    return v3(wx, np.sqrt(ONE - wx * wx), 0)


GLASS_INSIDE_Z = None  # set below: the smallest d.z from inside for which cos2t is not negative


def _walk_to_tir_edge():
    """from inside (n = +z, d.z > 0) ddn = -d.z exactly and cos2t = 1 - 2.25 (1 - ddn^2) changes sign at ddn^2 = 5/9: walk the
    ulps of d.z from fl(sqrt(5/9)) until the restated cos2t flips"""
    def cos2t(z):
        return scatter(v3(np.sqrt(ONE - z * z), 0, z), v3(0, 0, 1), ONES, ONES * 0, REFRACT, 0, 1, (ZERO, ZERO, ZERO))["cos2t"]

    z = f32(np.sqrt(5.0 / 9.0))
    step = -1 if not cos2t(z) < ZERO else 1
    for _ in range(64):
        z2 = ulps(z, step)
        if (cos2t(z) < ZERO) != (cos2t(z2) < ZERO):
            return max(z, z2)
        z = z2
    raise AssertionError("no sign change of cos2t within 64 ulps of sqrt(5/9)")


def _cases():
    out = []
    grey, black = v3(0.75, 0.5, 0.25), v3(0, 0, 0)

    def add(name, d, n, reflect, depth=0, branch=1, pixel=7, sample=3, color=grey, emission=black, x=(0.5, -0.25, 2.0), **expect):
        out.append(dict(name=name, d=v3(*d), n=v3(*n), reflect=reflect, depth=depth, branch=branch, pixel=pixel, sample=sample,
                        color=v3(*color), emission=v3(*emission), x=v3(*x), o=v3(*x) - v3(*d), expect=expect))

    # ---- diffuse: the basis
    for i, axis in enumerate("xyz"):
        for s in (1.0, -1.0):
            n = [0.0, 0.0, 0.0]
            n[i] = s
            add("diffuse_w_%s%s" % ("+" if s > 0 else "-", axis), [-v for v in n], n, DIFFUSE, kind="diffuse", flipped=False,
                axis="Y" if i == 0 else "X")
    for sign in (1.0, -1.0):
        for k in (-2, -1, 0, 1, 2):  # |w.x| = 0.1f is NOT greater: the X axis
            wx = f32(sign) * ulps(0.1, k)
            add("diffuse_wx_%s0.1f%+dulp" % ("+" if sign > 0 else "-", k), (0, -1, 0), _unit_xy(wx), DIFFUSE, kind="diffuse",
                axis="Y" if k > 0 else "X")
        add("diffuse_wx_%szero" % ("+" if sign > 0 else "-"), (0, -1, 0), (sign * 0.0, 1, 0), DIFFUSE, kind="diffuse", axis="X")
        # ... and reached through the flipped normal: w.x = -n.x
        add("diffuse_flipped_wx_%s0.1f" % ("+" if sign > 0 else "-"), (0, 1, 0), _unit_xy(-sign * f32(0.1)), DIFFUSE, kind="diffuse",
            flipped=True, axis="X")
    # ---- diffuse: the draws
    for name, word, k, depth, branch in DRAW_TARGETS:
        if name.startswith("r") and name in DRAWS:
            pixel, sample = DRAWS[name]
            for n in ((0, 0, 1), _unit_xy(0.6)):
                add("diffuse_%s_n%d" % (name, 0 if n[0] == 0 else 1), (0.28, -0.96, -0.5), n, DIFFUSE, depth, branch, pixel, sample,
                    kind="diffuse", draw=(word, k))
    # ---- facing
    tiny = np.nextafter(ZERO, ONE)
    for k in (-2, -1, 0, 1, 2):  # dot(n, d) = k denormal ulps: < 0 only below zero
        for reflect in (DIFFUSE, REFRACT):
            add("facing_dot_%+dulp_%d" % (k, reflect), (1, 0, f32(k) * tiny), (0, 0, 1), reflect, flipped=k >= 0)
    add("facing_d_is_minus_n", (-0.6, 0, -0.8), (0.6, 0, 0.8), DIFFUSE, flipped=False)
    add("facing_d_is_n", (0.6, 0, 0.8), (0.6, 0, 0.8), SPECULAR, flipped=True)
    # ---- roulette
    for depth in (4, 5, 10, 11):  # new_depth 5 (no roulette), 6, 11, 12 (MAX_DEPTH: dies whatever the draw)
        for reflect in (DIFFUSE, SPECULAR, REFRACT):
            add("roulette_depth%d_%d" % (depth, reflect), (0.6, 0, -0.8), (0, 0, 1), reflect, depth, color=(2, 1, 0.5),
                alive=depth < 11, emission=(3, 0, 0))
    for depth, pixel, sample in ((5, 11, 5), (10, 12, 6)):
        u0 = draws(SEED, pixel, sample, depth, 1)[0]
        for ch in range(3):  # the maximum in each channel; a draw EQUAL to it is not below it
            for k in (-2, -1, 0, 1, 2):
                color = [f32(0.0625)] * 3
                color[ch] = ulps(u0, k)
                add("roulette_draw_eq_max%+dulp_ch%d_depth%d" % (k, ch, depth), (0, 0, -1), (0, 0, 1), SPECULAR, depth, 1, pixel, sample,
                    color=color, emission=(0, 1, 0), alive=k > 0)
    for mx, alive in ((0.0, False), (1.0, True), (2.0, True)):
        for reflect in (DIFFUSE, SPECULAR, REFRACT):
            add("roulette_max%g_%d" % (mx, reflect), (0, 0.6, -0.8), (0, 0, 1), reflect, 7, color=(mx, mx * 0.5, 0), alive=alive)
    # ---- mirror
    add("mirror_normal", (0, 0, -1), (0, 0, 1), SPECULAR, kind="mirror")
    add("mirror_grazing", (1, 0, -(2.0 ** -12)), (0, 0, 1), SPECULAR, kind="mirror")
    add("mirror_oblique", (0.6, 0.0, -0.8), _unit_xy(0.28), SPECULAR, kind="mirror")
    # ---- glass
    for depth, kind in ((0, "split"), (1, "split"), (2, None), (6, None)):  # new_depth 2 | 3: both subtrees, then one
        add("glass_into_depth%d" % depth, (0.6, 0, -0.8), (0, 0, 1), REFRACT, depth, into=True, **(dict(kind=kind) if kind else {}))
        add("glass_out_depth%d" % depth, (0.6, 0, 0.8), (0, 0, 1), REFRACT, depth, into=False, **(dict(kind=kind) if kind else {}))
        add("glass_normal_depth%d" % depth, (0, 0, -1), (0, 0, 1), REFRACT, depth, into=True)
        add("glass_grazing_depth%d" % depth, (1, 0, -(2.0 ** -12)), (0, 0, 1), REFRACT, depth, into=True)
        add("glass_grazing_out_depth%d" % depth, (1, 0, 2.0 ** -12), (0, 0, 1), REFRACT, depth, into=False, kind="tir")
    z0 = GLASS_INSIDE_Z
    for k in (-2, -1, 0, 1, 2):  # from inside, ddn on both sides of cos2t = 0
        z = ulps(z0, k)
        for depth in (0, 2):
            add("glass_tir_edge%+dulp_depth%d" % (k, depth), (np.sqrt(ONE - z * z), 0, z), (0, 0, 1), REFRACT, depth, into=False,
                tir=k < 0)
    for b in (1, 2, 3):  # 1 -> 2, 3; 2 -> 4, 5; 3 -> 6, 7
        add("glass_branch%d" % b, (0.6, 0, -0.8), (0, 0, 1), REFRACT, 0 if b == 1 else 1, b, kind="split", branches=(2 * b, 2 * b + 1))
    for name in ("choice_eq_p", "choice_eq_p_next", "choice_eq_p_prev", "choice_eq_p_next2", "choice_eq_p_prev2"):
        if name in DRAWS:
            pixel, sample = DRAWS[name]
            add("glass_" + name, CHOICE_D, (0, 0, 1), REFRACT, 2, 1, pixel, sample,
                kind="choice_refl" if "prev" in name else "choice_trans")
    return out


GLASS_INSIDE_Z = _walk_to_tir_edge()
# The choice: a draw EQUAL to p is not below it (the transmitted ray).  A draw is a multiple of 2^-24, which p = 0.25 + 0.5 re is
# for every p >= 0.5 and for half the values below; 0.27f at normal incidence is not, so the first of these incidences whose p is.
def _choice_incidence():
    for d in ((0.6, 0, -0.8), (0.8, 0, -0.6), (0.96, 0, -0.28), (0.28, 0, -0.96), (1, 0, -0.125), (1, 0, -(2.0 ** -12))):
        p = scatter(d, (0, 0, 1), ONES, ONES * 0, REFRACT, 2, 1, (ZERO, ZERO, ZERO))["p"]
        k = int(np.float64(p) * 2.0 ** 24)
        if f32(k) * f32(2.0 ** -24) == p:
            return d, k
    raise AssertionError("no incidence with p a multiple of 2^-24")


CHOICE_D, CHOICE_K = _choice_incidence()
DRAW_TARGETS += [("choice_eq_p", 1, CHOICE_K, 2, 1), ("choice_eq_p_next", 1, CHOICE_K + 1, 2, 1),
                 ("choice_eq_p_prev", 1, CHOICE_K - 1, 2, 1), ("choice_eq_p_next2", 1, CHOICE_K + 2, 2, 1),
                 ("choice_eq_p_prev2", 1, CHOICE_K - 2, 2, 1)]
CASES = _cases()


def expected(case, thr=None):
    u = draws(SEED, case["pixel"], case["sample"], case["depth"], case["branch"])
    return scatter(case["d"], case["n"], case["color"], case["emission"], case["reflect"], case["depth"], case["branch"], u, thr)
