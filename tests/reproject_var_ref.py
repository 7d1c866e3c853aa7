"""pt_ctx_reproject_var restated: the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_reproject_var) in numpy binary32,
one numpy operation per operation of the contract, over whole frames at once.  It stands on tests/reproject_ref.py: the colour
and the length are its reproject(), and the moments are its reproject() again, applied to the pair (s, s*s) in place of the
colour and to the history moments in place of the history colour - "the colour's blend applied to the pair", with the same taps
and the same b because the guides are the same.  Nothing is shared with csrc/pt_reproject.h."""
import ctypes as C

import numpy as np

from ptlib import PtReprojectVarParams
import reproject_ref as ref
from reproject_ref import F32, I32

E_MAX = F32(12.0)
MAX_RADIUS = 3


def defaults(L):
    p = PtReprojectVarParams()
    assert L.pt_reproject_var_defaults(C.byref(p)) == 0
    return dict(weight=p.weight, max_history=p.max_history, depth_tol=p.depth_tol, normal_min=p.normal_min,
                min_frames=p.min_frames, radius=p.radius)


def pos(v):
    """v > 0 ? v : 0: a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, F32(0)).astype(F32)


def s_of(color):
    """s = (c[0] + c[1]) + c[2]; (n,)"""
    c = np.asarray(color, dtype=F32)
    return ((c[..., 0] + c[..., 1]) + c[..., 2]).astype(F32)


def spatial(W, H, s, oid, depth, radius, depth_tol):
    """(vs, cnt) of every pixel: the window of the contract, dy outside and dx inside, taps outside the frame skipped"""
    s = np.asarray(s, dtype=F32).reshape(H, W)
    oid = np.asarray(oid, dtype=I32).reshape(H, W)
    z = np.asarray(depth, dtype=F32).reshape(H, W)
    depth_tol = F32(depth_tol)
    S1 = np.zeros((H, W), F32)
    S2 = np.zeros((H, W), F32)
    cnt = np.zeros((H, W), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x0, x1 = max(0, -dx), min(W, W - dx)
            y0, y1 = max(0, -dy), min(H, H - dy)
            if x0 >= x1 or y0 >= y1:
                continue  # no pixel has this tap inside the frame
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            if dx == 0 and dy == 0:
                take = np.ones(s[P].shape, bool)
            else:
                zp, zq = z[P], z[Q]
                with np.errstate(all="ignore"):
                    near = np.abs(zp - zq) <= depth_tol * np.where(zp > zq, zp, zq)
                take = (oid[Q] == oid[P]) & ((oid[P] < 0) | near)
            sq = s[Q]
            with np.errstate(all="ignore"):
                S1[P] = np.where(take, S1[P] + sq, S1[P])
                S2[P] = np.where(take, S2[P] + sq * sq, S2[P])
            cnt[P] = cnt[P] + take
    fc = np.maximum(cnt, 1).astype(F32)
    with np.errstate(all="ignore"):
        mean = S1 / fc
        vs = pos(S2 / fc - mean * mean)
    assert mean.dtype == F32 and vs.dtype == F32
    return vs.reshape(W * H), cnt.reshape(W * H)


def error_of(v, k, out):
    """e = sqrt(v*k) / sqrt(2^-6 + ((out[0] + out[1]) + out[2])); if !(e < 12), e = 12"""
    with np.errstate(all="ignore"):
        e = np.sqrt(v * k) / np.sqrt(F32(2.0 ** -6) + s_of(out))
        e = np.where(e < E_MAX, e, E_MAX).astype(F32)
    return e


def reproject_var(W, H, cam, color, depth, object_id, normal=None, hist_cam=None, hist_color=None, hist_len=None, hist_moments=None,
                  hist_depth=None, hist_object_id=None, hist_normal=None, weight=1, max_history=64.0, depth_tol=0.125, normal_min=0.9,
                  min_frames=2, radius=3, parts=False):
    """the four outputs of pt_ctx_reproject_var: colour (W*H, 3), length (W*H,), moments (W*H, 2), error (W*H,), binary32.  The
    parameters are the values in use: no zero stands for a default here except weight 0 = 1.  min_frames 0 is not the entry
    point's (where 0 stands for the default): it makes every pixel long, the temporal-only estimate of the CPU study.
    parts: also a dict of the intermediates (vt, vs, cnt, long)."""
    n = W * H
    assert 0 <= radius <= MAX_RADIUS
    color = np.ascontiguousarray(color, dtype=F32).reshape(n, 3)
    wt = F32(weight if weight else 1)
    kw = dict(weight=weight, max_history=max_history, depth_tol=depth_tol, normal_min=normal_min)
    hist = dict(hist_cam=hist_cam, hist_len=hist_len, hist_depth=hist_depth, hist_object_id=hist_object_id, hist_normal=hist_normal)
    out, out_len = ref.reproject(W, H, cam, color, depth, object_id, normal, hist_color=hist_color, **hist, **kw)
    s = s_of(color)
    pair = np.stack([s, s * s, np.zeros(n, F32)], axis=1).astype(F32)
    if hist_color is None:
        mom = pair[:, :2].copy()
    else:
        hm = np.ascontiguousarray(hist_moments, dtype=F32).reshape(n, 2)
        hpair = np.concatenate([hm, np.zeros((n, 1), F32)], axis=1)
        mom3, len2 = ref.reproject(W, H, cam, pair, depth, object_id, normal, hist_color=hpair, **hist, **kw)
        assert len2.tobytes() == out_len.tobytes()
        mom = np.ascontiguousarray(mom3[:, :2])
    with np.errstate(all="ignore"):
        vt = pos(mom[:, 1] - mom[:, 0] * mom[:, 0])
        k = wt / out_len
        long = out_len >= F32(min_frames) * wt
    vs, cnt = spatial(W, H, s, object_id, depth, radius, depth_tol)
    with np.errstate(invalid="ignore"):
        v = np.where(long, vt, np.where(vs > vt, vs, vt)).astype(F32)
    e = error_of(v, k, out)
    e = np.where(~long & (cnt < 2), F32(np.inf), e).astype(F32)
    assert vt.dtype == F32 and k.dtype == F32 and e.dtype == F32
    if parts:
        return out, out_len, mom, e, dict(vt=vt, vs=vs, cnt=cnt, long=long, s=s)
    return out, out_len, mom, e
