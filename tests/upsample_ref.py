"""pt_ctx_upsample restated: the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_upsample) in numpy binary32, one numpy
operation per operation of the contract, over whole frames at once.  Nothing is shared with csrc/pt_upsample.h: the tap position
is written with // and %.  Also the synthetic
inputs the GPU tests and the CPU test of their coverage share."""
import ctypes as C

import numpy as np

from ptlib import PtUpsampleParams

F32 = np.float32
I32 = np.int32
MAX_SIZE = 1 << 14


def defaults(L):
    p = PtUpsampleParams()
    assert L.pt_upsample_defaults(C.byref(p)) == 0
    return dict(depth_tol=p.depth_tol, normal_min=p.normal_min)


# ------------------------------------------------------------------------------------------------------ the arithmetic
def tap(size, lo, coord):
    """step 1 for the coordinates given of one axis: (first, frac), int64 and binary32 arrays"""
    coord = np.asarray(coord, dtype=np.int64)
    a = (2 * coord + 1) * lo + size
    assert a.max() < 2 ** 32
    first = a // (2 * size) - 1
    frac = (a % (2 * size)).astype(F32) / F32(2 * size)
    assert frac.dtype == F32
    return first, frac


def normalized(n):
    """N(.): pt_ctx_denoise's normalised normal; (..., 3)"""
    n = np.asarray(n, dtype=F32)
    l = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = n / l[..., None]
    return np.where((l > 0)[..., None], q, F32(0)).astype(F32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def demod(albedo):
    """m_c(.) per channel"""
    albedo = np.asarray(albedo, dtype=F32)
    return np.where(albedo > F32(2.0 ** -6), albedo, F32(1)).astype(F32)


def upsample(W, H, w, h, lo_color, lo_depth, lo_object_id, depth, object_id, lo_normal=None, lo_albedo=None, normal=None, albedo=None,
             depth_tol=0.125, normal_min=0.9, detail=False):
    """the two outputs of pt_ctx_upsample: (W*H, 3) and (W*H,) binary32.  The parameters are the values in use: no zero stands for
    a default here.  detail=True: also a dict of per-pixel facts - `taken` (W*H, 4) bool, `inside` (W*H, 4) bool."""
    n, nl = W * H, w * h
    lo_color = np.ascontiguousarray(lo_color, dtype=F32).reshape(nl, 3)
    lo_depth = np.ascontiguousarray(lo_depth, dtype=F32).reshape(nl)
    lo_oid = np.ascontiguousarray(lo_object_id, dtype=I32).reshape(nl)
    depth = np.ascontiguousarray(depth, dtype=F32).reshape(n)
    oid = np.ascontiguousarray(object_id, dtype=I32).reshape(n)
    normals = normal is not None and lo_normal is not None
    if normals:
        N = normalized(np.asarray(normal, dtype=F32).reshape(n, 3))
        Nl = normalized(np.asarray(lo_normal, dtype=F32).reshape(nl, 3))
    if albedo is not None and lo_albedo is not None:
        m = demod(np.asarray(albedo, dtype=F32).reshape(n, 3))
        ml = demod(np.asarray(lo_albedo, dtype=F32).reshape(nl, 3))
    else:
        m, ml = np.ones((n, 3), dtype=F32), np.ones((nl, 3), dtype=F32)
    depth_tol, normal_min = F32(depth_tol), F32(normal_min)
    idx = np.arange(n, dtype=np.int64)
    x0, fx = tap(W, w, idx % W)
    r0, fr = tap(H, h, idx // W)
    one = F32(1.0)
    u = lo_color / ml
    hit = oid >= 0
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            qx, qr = x0 + i, r0 + j
            inside = (qx >= 0) & (qx < w) & (qr >= 0) & (qr < h)
            b = (fx if i else one - fx) * (fr if j else one - fr)
            taps.append((np.where(inside, qr * w + qx, 0), b.astype(F32), inside))
    s = np.zeros((n, 3), dtype=F32)
    bsum = np.zeros(n, dtype=F32)
    s2 = np.zeros((n, 3), dtype=F32)
    bsum2 = np.zeros(n, dtype=F32)
    taken = []
    with np.errstate(all="ignore"):
        for q, b, inside in taps:
            lz = lo_depth[q]
            take = inside & (lo_oid[q] == oid)
            take &= ~hit | (np.abs(depth - lz) <= depth_tol * np.where(depth > lz, depth, lz))
            if normals:
                take &= ~hit | (dot(N, Nl[q]) >= normal_min)
            s = np.where(take[:, None], s + u[q] * b[:, None], s)
            bsum = np.where(take, bsum + b, bsum)
            s2 = np.where(inside[:, None], s2 + u[q] * b[:, None], s2)
            bsum2 = np.where(inside, bsum2 + b, bsum2)
            taken.append(take)
        tested = bsum > 0
        weight = np.where(tested, bsum, F32(0)).astype(F32)
        s = np.where(tested[:, None], s, s2)
        bsum = np.where(tested, bsum, bsum2)
        assert (bsum > 0).all()
        v = (s / bsum[:, None]) * m
        out = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
    assert s.dtype == F32 and bsum.dtype == F32 and v.dtype == F32 and u.dtype == F32
    if detail:
        return out, weight, dict(taken=np.stack(taken, axis=1), inside=np.stack([t[2] for t in taps], axis=1))
    return out, weight


# ------------------------------------------------------------------------------- the inputs of the GPU tests (and of one CPU test)
CASES = ((1, 1, 1, 1), (7, 5, 3, 2), (257, 3, 129, 2), (33, 25, 16, 12), (16, 12, 33, 25), (33, 25, 33, 25))  # frame <- low
# The shapes at the limits csrc/pt_upsample.h argues, a tuple of its own so that the parametrisations over CASES keep their cost.
# With S = kUpsampleMaxSize = 2^14, the largest size of an axis:
# - 16384x2 <- 8192x1, 16384x3 <- 5461x2, 2x16384 <- 1x8191: an axis at the limit on either side, an integer ratio and none, a
#   low-resolution axis of one pixel (every tap pair has one tap outside it);
# - 16384x2 <- 16384x3: both widths at the limit, where the numerator (2x + 1) * w + W reaches (2S - 1) * S + S = 2^29 exactly,
#   the bound upsample_div is proved for (n < 2^30), at the divisor 2W = 2^15;
# - 16384x16 <- 16384x16: idx reaches 2^18 - 1 with W at the limit, so idx / W runs the division by the largest W over 16 rows;
# - 1024x768 <- 512x384: the documented preview loop, 3072 workgroups, the shape the four template instances are timed at.
LARGE = ((16384, 2, 8192, 1), (16384, 3, 5461, 2), (2, 16384, 1, 8191), (16384, 2, 16384, 3), (16384, 16, 16384, 16),
         (1024, 768, 512, 384))
PARAMS = dict(depth_tol=0.05, normal_min=0.5)


def synthetic(W, H, w, h):
    """(hi, lo): guides in the style of test_gpu_reproject.synthetic.  The frame's: depths on a few planes, in blocks so that
    neighbours mostly share one, and +inf on the misses; ids in {-1, 0, 1, 2}; normals around one direction, a tenth of them zero;
    albedos on either side of 2^-6.  The low-resolution guides are the frame's, sampled at the nearest pixel, with a part disturbed
    (other depth, other id, flipped normal); the low-resolution colour is random in [0, 1]."""
    rng = np.random.default_rng(((W * 100 + H) * 100 + w) * 100 + h)
    n, nl = W * H, w * h
    planes = np.array([2.0, 6.0, 6.25, 9.0], dtype=F32)
    x, r = np.arange(n) % W, np.arange(n) // W
    block = x // 5 + r // 4
    depth = np.where(rng.random(n) < 0.1, planes[rng.integers(0, 4, n)], planes[block % 4]).astype(F32)
    oid = np.where(rng.random(n) < 0.15, rng.integers(-1, 3, n), block % 3).astype(I32)
    miss = ((x // 6 + r // 5) % 4 == 3) & (n > 1)   # blocks of misses, so that a miss finds missing taps
    oid[miss] = -1
    depth[oid < 0] = np.inf
    normal = (np.array([0.2, 0.3, 1.0], dtype=F32) + (rng.random((n, 3)).astype(F32) - F32(0.5)) * F32(0.6)).astype(F32)
    normal[rng.random(n) < 0.1] = 0
    albedo = rng.random((n, 3)).astype(F32)
    albedo[rng.random((n, 3)) < 0.1] = F32(0.01)
    hi = dict(depth=depth, oid=oid, normal=normal, albedo=albedo)
    lx = np.minimum(((np.arange(nl) % w) * 2 + 1) * W // (2 * w), W - 1)
    lr = np.minimum(((np.arange(nl) // w) * 2 + 1) * H // (2 * h), H - 1)
    src = lr * W + lx
    ldepth = np.where(rng.random(nl) < 0.15, depth[src] * F32(1.2), depth[src]).astype(F32)
    loid = np.where(rng.random(nl) < 0.1, rng.integers(-1, 3, nl), oid[src]).astype(I32)
    ldepth[loid < 0] = np.inf
    ldepth[(loid >= 0) & ~np.isfinite(ldepth)] = F32(6.0)
    lnormal = normal[src].copy()
    flip = rng.random(nl) < 0.1
    lnormal[flip] = -lnormal[flip]
    lalbedo = albedo[src].copy()
    change = rng.random(nl) < 0.3
    lalbedo[change] = rng.random((int(change.sum()), 3)).astype(F32)
    lo = dict(color=rng.random((nl, 3)).astype(F32), depth=ldepth, oid=loid, normal=lnormal, albedo=lalbedo)
    return hi, lo


def want(W, H, w, h, hi, lo, normal=(True, True), albedo=(True, True), params=PARAMS, detail=False):
    """the restatement on synthetic()'s planes; normal / albedo: (the frame's given, the low-resolution one given)"""
    return upsample(W, H, w, h, lo["color"], lo["depth"], lo["oid"], hi["depth"], hi["oid"],
                    lo_normal=lo["normal"] if normal[1] else None, lo_albedo=lo["albedo"] if albedo[1] else None,
                    normal=hi["normal"] if normal[0] else None, albedo=hi["albedo"] if albedo[0] else None, detail=detail, **params)


def kinds(hi, weight, detail):
    """how many pixels of each kind the comparison needs: all four taps taken, one to three, the fallback (weight 0), a miss with
    a tap taken, a tap outside the low-resolution frame"""
    taken, inside = detail["taken"], detail["inside"]
    k = taken.sum(axis=1)
    return dict(all_four=int((k == 4).sum()), some=int(((k >= 1) & (k <= 3)).sum()), fallback=int((weight == 0).sum()),
                miss_taken=int(((hi["oid"] < 0) & (k >= 1)).sum()), outside=int((~inside).any(axis=1).sum()))
