"""pt_ctx_denoise restated in numpy binary32, written from the contract in include/ptrace.h ("THE ARITHMETIC") and from
nothing else: it shares no code with the HIP source and reads no constant out of it.  Vectorised over pixels; the 25 taps of
a level are looped in the stated order (dy outer, dx inner), so every pixel sees its additions in the contract's order.
Every intermediate is an np.float32 array or scalar: numpy's + - * / and sqrt on binary32 are correctly rounded and never
contracted."""
import ctypes as C

import numpy as np

from ptlib import abi, PtDenoiseParams

F32 = np.float32
NO_DEMODULATE = abi.PT_DENOISE_NO_DEMODULATE
B = (F32(0.375), F32(0.25), F32(0.0625))
ZERO, ONE, EIGHTH = F32(0.0), F32(1.0), F32(0.125)


def defaults(L):
    """(levels, sigma_color, sigma_depth) as pt_denoise_defaults reports them"""
    p = PtDenoiseParams()
    assert L.pt_denoise_defaults(C.byref(p)) == 0
    return p.levels, p.sigma_color, p.sigma_depth


def pos(v):
    return np.where(v > ZERO, v, ZERO).astype(F32)


def fall(v):
    t = pos(ONE - v * EIGHTH)
    t = t * t
    t = t * t
    return t * t


def prepare(color, albedo, normal, depth, w, h, flags):
    """(u_0 (h, w, 3), m (h, w, 3), N (h, w, 3) or None, z (h, w) or None, hit (h, w))"""
    col = np.ascontiguousarray(color, dtype=F32).reshape(h, w, 3)
    if albedo is None or (flags & NO_DEMODULATE):
        m = np.ones((h, w, 3), F32)
    else:
        a = np.ascontiguousarray(albedo, dtype=F32).reshape(h, w, 3)
        m = np.where(a > F32(2.0 ** -6), a, ONE).astype(F32)
    u = col / m
    if depth is None:
        z, hit = None, np.ones((h, w), bool)
    else:
        z = np.ascontiguousarray(depth, dtype=F32).reshape(h, w)
        hit = z < F32(np.inf)
    if normal is None:
        N = None
    else:
        n = np.ascontiguousarray(normal, dtype=F32).reshape(h, w, 3)
        l = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            N = np.where((l > ZERO)[..., None], n / l[..., None], ZERO).astype(F32)
    return u, m, N, z, hit


def level(u, N, z, hit, i, sigma_color, sigma_depth):
    h, w, _ = u.shape
    s = 1 << i
    sc = F32(sigma_color) * F32(2.0 ** -i)
    rc = ONE / (sc * sc)
    sds = F32(sigma_depth) * F32(s)
    acc = np.zeros((h, w, 3), F32)
    wsum = np.zeros((h, w), F32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = dx * s, dy * s
            x0, x1 = max(0, -ox), min(w, w - ox)
            y0, y1 = max(0, -oy), min(h, h - oy)
            if x0 >= x1 or y0 >= y1:
                continue  # no pixel has this tap inside the frame
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            hh = B[abs(dy)] * B[abs(dx)]
            uq = u[Q]
            if dx == 0 and dy == 0:
                wt = np.full(wsum[P].shape, hh, F32)
                keep = np.ones(wt.shape, bool)
            else:
                keep = hit[P] == hit[Q]
                both = hit[P] & hit[Q]
                if N is None:
                    wn = np.ones(keep.shape, F32)
                else:
                    a, b = N[P], N[Q]
                    e = pos((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])
                    for _ in range(4):
                        e = e * e
                    wn = np.where(both, e * e, ONE).astype(F32)
                if z is None:
                    xz = np.zeros(keep.shape, F32)
                else:
                    zp, zq = z[P], z[Q]
                    with np.errstate(all="ignore"):
                        xz = np.abs(zp - zq) * (ONE / (sds * np.where(zp > zq, zp, zq)))
                    xz = np.where(both, xz, ZERO).astype(F32)
                d = u[P] - uq
                with np.errstate(all="ignore"):
                    xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * rc
                    wt = ((hh * wn) * fall(xz)) * fall(xc)
            with np.errstate(all="ignore"):
                acc[P] = np.where(keep[..., None], acc[P] + uq * wt[..., None], acc[P])
                wsum[P] = np.where(keep, wsum[P] + wt, wsum[P])
    return acc / wsum[..., None]


def denoise(color, w, h, albedo=None, normal=None, depth=None, levels=5, sigma_color=None, sigma_depth=None, flags=0,
            keep_demodulated=False):
    """out (w*h, 3) float32.  levels / sigmas are the effective values (a caller maps 0 to pt_denoise_defaults' first)."""
    assert levels >= 1 and sigma_color is not None and sigma_depth is not None
    u, m, N, z, hit = prepare(color, albedo, normal, depth, w, h, flags)
    for i in range(levels):
        u = level(u, N, z, hit, i, sigma_color, sigma_depth)
    if keep_demodulated:
        return u.reshape(w * h, 3)
    v = u * m
    out = np.where(v < ZERO, ZERO, np.where(v > ONE, ONE, v)).astype(F32)
    return out.reshape(w * h, 3)
