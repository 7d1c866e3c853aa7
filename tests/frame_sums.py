"""What a frame's accumulator must hold, to the bit, restated on the CPU from the oracle's paths: the raw 32.32 sum of every
(sample, pixel, channel) of a scatter_walk walk, and the frame they resolve to.  No product call is made here.

- to_fixed restates csrc/pt_device.h's to_fixed in binary32 (the one copy in the tests; tests/test_gpu_aov.py's vectorised form
  is held to it);
- walk_sums carries the throughput down every path of a walk with tests/kats_scatter.py (thr0 / thr1 = fl(fl(thr * colour') *
  factor), contrib = fl(thr * emission)) and adds to_fixed(contrib) into the ray's (sample, pixel);
- resolve restates k_resolve (csrc/pt_kernels.hip): (float)((double)sum * 2^-32) / (float)count, clamped if asked;
- EMISSIONS x SAMPLE_COUNTS is the table tests/test_gpu_frame_sums.py probes through pt_ctx_radiance, and resolve_* / to_fixed_*
  the wrong variants tests/test_frame_sums.py proves that table tells from the real arithmetic."""
import functools

import numpy as np

import kats_scatter
import scatter_walk

f32 = np.float32
SATURATED = f32(4294967040.0)  # 2^32 - 256, the largest binary32 below 2^32
TWO32 = f32(4294967296.0)
WRAP = 1 << 64

# the whole-frame walks: scatter_walk.FRAMES at its seed, and three-spheres at a seed above 2^32 (a non-zero high key word)
BIG_SEED = kats_scatter.SEED
WALKS = [f + (scatter_walk.SEED,) for f in scatter_walk.FRAMES] + [("three-spheres", 16, 12, 8, BIG_SEED)]
WALK_IDS = ["%s-seed%x" % (f[0], f[4]) for f in WALKS]


def to_fixed(v, round_lo=False):
    """pt_device.h's to_fixed for a finite v >= 0 (or +inf), binary32 throughout, as a Python int.  round_lo: the WRONG variant
    that rounds the low word to nearest instead of truncating it."""
    v = f32(v)
    assert not v < 0 and v == v, v
    c = v if v < SATURATED else SATURATED
    hi = int(c)                   # truncation; c < 2^32
    frac = f32(c - f32(hi))       # exact: hi has at most 24 significant bits
    scaled = f32(frac * TWO32)    # exact scaling
    lo = int(np.rint(scaled)) if round_lo else int(scaled)
    assert 0 <= hi < (1 << 32) and 0 <= lo <= (1 << 32)
    return (hi << 32) + lo


def clamp01(v):
    return f32(0) if v < 0 else (f32(1) if v > 1 else v)


def resolve(total, count, clamp):
    """k_resolve: f32(f32(float(total) * 2^-32) / f32(count)); Python's int -> float is correctly rounded, as u64 -> f64 is"""
    assert 0 <= total < WRAP and count > 0
    v = f32(f32(float(total) * 2.0 ** -32) / f32(count))
    return clamp01(v) if clamp else v


def resolve_double_divide(total, count):
    """WRONG variant (a): divide in binary64, round once"""
    return f32(float(total) * 2.0 ** -32 / float(count))


def resolve_reciprocal(total, count):
    """WRONG variant (b): multiply by fl(1 / n)"""
    return f32(f32(float(total) * 2.0 ** -32) * f32(f32(1) / f32(count)))


def contributions(W, wrong_order=False):
    """(ray, sample, pixel, contrib) of every ray of the walk that hits, visited by depth.  A primary ray carries (1, 1, 1); a
    hit goes through kats_scatter.scatter with its incoming throughput, its oracle normal and its object's material, and each
    child receives the weight scatter returned for it.  wrong_order: the WRONG carry fl(thr * fl(colour' * factor))."""
    thr, given = {}, set()
    out = []
    for i in sorted(range(W.n), key=lambda i: int(W.keys[i][2])):
        p, s, depth, branch = (int(v) for v in W.keys[i])
        if depth == 0:
            assert i not in given, "a primary ray is nobody's child"
            t = kats_scatter.ONES
        else:
            t = thr.pop(i)  # (a KeyError: a ray visited before its parent, or never claimed)
        if W.oid[i] < 0:
            assert not W.children[i], "a miss ends the path and contributes nothing"
            continue
        obj = W.scene.objs[int(W.oid[i])]
        draws = kats_scatter.draws(W.seed, p, s, depth, branch)
        args = (W.d[i], W.nrm[i], tuple(obj.color), tuple(obj.emission), obj.reflect_type, depth, branch, draws)
        if wrong_order:
            got = kats_scatter.scatter(*args)
            contrib, weights = t * got["emission"], [t * c[1] for c in got["children"]]
        else:
            got = kats_scatter.scatter(*args, thr=t)
            contrib, weights = got["contrib"], [c[1] for c in got["children"]]
        out.append((i, s, p, contrib))
        kids = W.children[i]
        assert len(weights) == len(kids), (i, got["kind"])
        for w, k in zip(weights, kids):
            assert k not in given, "a ray receives a throughput exactly once"
            given.add(k)
            thr[k] = w
    assert not thr
    assert given == {i for i in range(W.n) if W.keys[i][2] != 0}, "every ray but the primary ones received a throughput"
    return out


def walk_sums(W, wrong_order=False, round_lo=False):
    """sums[sample][pixel][channel] as Python ints: the to_fixed of every contribution of the walk at its (sample, pixel)"""
    sums = [[[0, 0, 0] for _ in range(W.width * W.height)] for _ in range(W.spp)]
    for _, s, p, contrib in contributions(W, wrong_order):
        for c in range(3):
            sums[s][p][c] += to_fixed(contrib[c], round_lo)
    return sums


@functools.lru_cache(maxsize=None)
def frame(sid, width, height, spp, seed):
    """(walk, sums[sample][pixel][channel]) of a frame, computed once per process and left unchanged by its users"""
    W = scatter_walk.walk(sid, width, height, spp, seed)
    return W, walk_sums(W)


def total_over(sums, samples):
    """[pixel][channel]: the sums of the given samples added"""
    return [[sum(sums[s][p][c] for s in samples) for c in range(3)] for p in range(len(sums[0]))]


def planes(total, begin=0, end=None):
    """pixel totals [begin, end) as pt_ctx_accum_save writes them: (3, n) uint64, channel planes in pixel order"""
    part = total[begin:end]
    assert all(v < WRAP for px in part for v in px)
    return np.array([[px[c] for px in part] for c in range(3)], dtype=np.uint64)


def resolved(total, count, clamp):
    """(pixels, 3) float32: every pixel total through resolve"""
    return np.array([[resolve(v, count, clamp) for v in px] for px in total], dtype=f32)


# ---- the probe table: to_fixed and k_resolve at their edges (tests/test_gpu_frame_sums.py, through pt_ctx_radiance) ----------
# every value is finite: the door (pt_ctx_set_scene, pt_ctx_set_object) refuses +inf, whose saturation 4294967040, 2^32 and 3e38 show
EMISSIONS = [f32(v) for v in (2.0 ** -33, 2.0 ** -32, 1.5 * 2.0 ** -32, 0.1, f32(1) / f32(3), 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23,
                              12.0, 2.8125155, 16777217.0, 2097151.875, 2.0 ** 31, 4294967040.0, 2.0 ** 32, 3e38)]
SAMPLE_COUNTS = (1, 2, 3, 5, 7, 63, 64, 65, 255, 257, 1000, 4095)
SUBSET_COUNTS = (1, 3, 65, 1000)  # what every form but the two flagship ones runs


def fits(e, n):
    """does the sum of n contributions of e stay below the wrap (the tests do not pin the wrap)"""
    return n * to_fixed(e) < WRAP


def table_cases(counts=SAMPLE_COUNTS):
    """[(n, (er, eg, eb))]: for every n, every emission that fits n samples once in each channel, beside two OTHER values so
    that a swapped plane shows"""
    out = []
    for n in counts:
        ok = [e for e in EMISSIONS if fits(e, n)]
        assert len(ok) >= 3
        out += [(n, (ok[k], ok[(k + 1) % len(ok)], ok[(k + 2) % len(ok)])) for k in range(len(ok))]
    return out
