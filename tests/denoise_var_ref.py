"""pt_ctx_denoise_var restated in numpy binary32, written from the contract in include/ptrace.h (the second "THE ARITHMETIC")
and from nothing else: it shares no code with the HIP source and reads no constant out of it.  What the contract takes over
from pt_ctx_denoise "word for word" is taken over from tests/denoise_ref.py: prepare, pos, fall, B.  Vectorised over pixels;
the taps are looped in the stated order (dy outer, dx inner).  Every intermediate is an np.float32 array or scalar."""
import ctypes as C

import numpy as np

from denoise_ref import B, F32, NO_DEMODULATE, ONE, ZERO, fall, pos, prepare  # noqa: F401
from ptlib import PtDenoiseVarParams

G = (F32(0.5), F32(0.25))
EV_MAX = F32(12.0)
EPS = F32(2.0 ** -20)


def defaults(L):
    """(levels, sigma_var, sigma_depth) as pt_denoise_var_defaults reports them"""
    p = PtDenoiseVarParams()
    assert L.pt_denoise_var_defaults(C.byref(p)) == 0
    return p.levels, p.sigma_var, p.sigma_depth


def raw_variance(color, error, m, w, h):
    """Vraw (h, w): step 1"""
    col = np.ascontiguousarray(color, dtype=F32).reshape(h, w, 3)
    e = np.ascontiguousarray(error, dtype=F32).reshape(h, w)
    with np.errstate(invalid="ignore"):
        ev = np.where(e < EV_MAX, pos(e), EV_MAX).astype(F32)
        d = ev * np.sqrt(F32(2.0 ** -6) + ((col[..., 0] + col[..., 1]) + col[..., 2]))
    t = d[..., None] / m
    return ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]).astype(F32)


def prefilter(v):
    """V_0 (h, w): step 2"""
    h, w = v.shape
    acc = np.zeros((h, w), F32)
    gsum = np.zeros((h, w), F32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            x0, x1 = max(0, -dx), min(w, w - dx)
            y0, y1 = max(0, -dy), min(h, h - dy)
            if x0 >= x1 or y0 >= y1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            g = G[abs(dy)] * G[abs(dx)]
            acc[P] = acc[P] + v[Q] * g
            gsum[P] = gsum[P] + g
    return acc / gsum


def level(u, V, N, z, hit, i, kv, sigma_depth):
    """(u_{i+1}, V_{i+1}): step 3"""
    h, w, _ = u.shape
    s = 1 << i
    sds = F32(sigma_depth) * F32(s)
    r = (ONE / ((F32(kv) * V) + EPS)).astype(F32)
    acc = np.zeros((h, w, 3), F32)
    wsum = np.zeros((h, w), F32)
    vs = np.zeros((h, w), F32)
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
                    xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * r[P]
                    wt = ((hh * wn) * fall(xz)) * fall(xc)
            with np.errstate(all="ignore"):
                acc[P] = np.where(keep[..., None], acc[P] + uq * wt[..., None], acc[P])
                wsum[P] = np.where(keep, wsum[P] + wt, wsum[P])
                vs[P] = np.where(keep, vs[P] + V[Q] * (wt * wt), vs[P])
    with np.errstate(all="ignore"):
        return acc / wsum[..., None], vs / (wsum * wsum)


def denoise_var(color, error, w, h, albedo=None, normal=None, depth=None, levels=5, sigma_var=None, sigma_depth=None, flags=0,
                keep_demodulated=False, return_variance=False):
    """out (w*h, 3) float32.  levels / sigmas are the effective values (a caller maps 0 to pt_denoise_var_defaults' first)."""
    assert levels >= 1 and sigma_var is not None and sigma_depth is not None
    u, m, N, z, hit = prepare(color, albedo, normal, depth, w, h, flags)
    V = prefilter(raw_variance(color, error, m, w, h))
    kv = F32(sigma_var) * F32(sigma_var)
    for i in range(levels):
        u, V = level(u, V, N, z, hit, i, kv, sigma_depth)
    if return_variance:
        return u.reshape(w * h, 3), V.reshape(w * h)
    if keep_demodulated:
        return u.reshape(w * h, 3)
    v = u * m
    out = np.where(v < ZERO, ZERO, np.where(v > ONE, ONE, v)).astype(F32)
    return out.reshape(w * h, 3)
