"""pt_ctx_reproject restated: the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_reproject) in numpy binary32, one numpy
operation per operation of the contract, over whole frames at once.  Nothing is shared with csrc/pt_reproject.h.  Cameras are the
dicts of tests/kats_camera.py."""
import ctypes as C

import numpy as np

import ptlib
from ptlib import PtReprojectParams

F32 = np.float32
I32 = np.int32


def defaults(L):
    p = PtReprojectParams()
    assert L.pt_reproject_defaults(C.byref(p)) == 0
    return dict(weight=p.weight, max_history=p.max_history, depth_tol=p.depth_tol, normal_min=p.normal_min)


def pt_camera(cam):
    return ptlib.make_camera(cam["position"], cam["direction"], cam["focal_length"], cam["sensor_width"], cam["aspect_ratio"])


def cam_dict(c):
    """a PtCamera as a dict"""
    return dict(position=tuple(c.position), direction=tuple(c.direction), focal_length=c.focal_length,
                sensor_width=c.sensor_width, aspect_ratio=c.aspect_ratio)


def cam_floats(cam):
    return np.array(list(cam["position"]) + list(cam["direction"]) + [cam["focal_length"], cam["sensor_width"], cam["aspect_ratio"]],
                    dtype=F32)


# ------------------------------------------------------------------------------------------------------ the arithmetic
def v3(x):
    return np.array([F32(x[0]), F32(x[1]), F32(x[2])], dtype=F32)


def dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z over the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], dtype=F32)


def basis(cam):
    """pt_camera_basis (CameraData::lens_center, orthogonals; mod.rs:211-232) in binary32: (C, D, f, L, su, sv)"""
    pos, d = v3(cam["position"]), v3(cam["direction"])
    f, sw, ar = F32(cam["focal_length"]), F32(cam["sensor_width"]), F32(cam["aspect_ratio"])
    sh = sw / ar
    lens = pos + d * f
    up = v3((0, 1, 0)) if abs(d[1]) < F32(0.9) else v3((0, 0, 1))
    c = cross(d, up)
    su = c * (F32(1.0) / np.sqrt(dot(c, c)))
    sv = cross(su, d)
    return pos, d, f, lens, su * sw, sv * sh


def normalized(n):
    """N(.): pt_ctx_denoise's normalised normal; (..., 3)"""
    n = np.asarray(n, dtype=F32)
    l = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = n / l[..., None]
    return np.where((l > 0)[..., None], q, F32(0)).astype(F32)


def project(cam, hist_cam, W, H, idx, depth):
    """step 3 for the pixels idx at the depths given: (ok, px, pr, zexp), arrays; where ok is False the rest is unspecified"""
    idx = np.asarray(idx, dtype=np.int64)
    depth = np.asarray(depth, dtype=F32)
    Cc, _, _, Lc, su, sv = basis(cam)
    _, Dh, fh, Lh, suh, svh = basis(hist_cam)
    x = (idx % W).astype(F32)
    y = (H - 1 - idx // W).astype(F32)
    fw, fhh = F32(W), F32(H)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        sx = (x + half) / fw - half
        sy = (y + half) / fhh - half
        S = (Cc + su * sx[:, None]) + sv * sy[:, None]
        g = Lc - S
        P = Lc + (g * (F32(1.0) / np.sqrt(dot(g, g)))[:, None]) * depth[:, None]
        v = P - Lh
        a = dot(v, Dh)
        ok = a > 0
        t = a / (fh * dot(Dh, Dh))
        w = Dh * fh - v / t[:, None]
        sxh = dot(w, suh) / dot(suh, suh)
        syh = dot(w, svh) / dot(svh, svh)
        px = (sxh + half) * fw - half
        py = (syh + half) * fhh - half
        pr = F32(H - 1) - py
        ok = ok & (px > -1) & (px < fw) & (pr > -1) & (pr < fhh)
        zexp = np.sqrt(dot(v, v))
    assert px.dtype == F32 and pr.dtype == F32 and zexp.dtype == F32
    return ok, px, pr, zexp


def reproject(W, H, cam, color, depth, object_id, normal=None, hist_cam=None, hist_color=None, hist_len=None, hist_depth=None,
              hist_object_id=None, hist_normal=None, weight=1, max_history=64.0, depth_tol=0.125, normal_min=0.9):
    """the two outputs of pt_ctx_reproject: (W*H, 3) and (W*H,) binary32.  The parameters are the values in use: no zero stands
    for a default here except weight 0 = 1."""
    n = W * H
    color = np.ascontiguousarray(color, dtype=F32).reshape(n, 3)
    wt = F32(weight if weight else 1)
    out = color.copy()
    out_len = np.full(n, wt, dtype=F32)
    if hist_color is None:
        return out, out_len
    depth = np.ascontiguousarray(depth, dtype=F32).reshape(n)
    oid = np.ascontiguousarray(object_id, dtype=I32).reshape(n)
    h_color = np.ascontiguousarray(hist_color, dtype=F32).reshape(n, 3)
    h_len = np.ascontiguousarray(hist_len, dtype=F32).reshape(n)
    h_depth = np.ascontiguousarray(hist_depth, dtype=F32).reshape(n)
    h_oid = np.ascontiguousarray(hist_object_id, dtype=I32).reshape(n)
    normals = normal is not None and hist_normal is not None
    if normals:
        N = normalized(np.asarray(normal, dtype=F32).reshape(n, 3))
        Nh = normalized(np.asarray(hist_normal, dtype=F32).reshape(n, 3))
    max_history, depth_tol, normal_min = F32(max_history), F32(depth_tol), F32(normal_min)
    idx = np.arange(n, dtype=np.int64)
    alive = oid >= 0
    if cam_floats(cam).tobytes() == cam_floats(hist_cam).tobytes():
        taps = [(idx, np.ones(n, dtype=F32), np.ones(n, dtype=bool))]
        zexp = depth
    else:
        ok, px, pr, zexp = project(cam, hist_cam, W, H, idx, depth)
        alive = alive & ok
        px, pr = np.where(alive, px, F32(0)), np.where(alive, pr, F32(0))
        flx, flr = np.floor(px), np.floor(pr)
        x0, r0 = flx.astype(np.int64), flr.astype(np.int64)
        fx, fr = px - flx, pr - flr
        one = F32(1.0)
        taps = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qr = x0 + i, r0 + j
                inside = (qx >= 0) & (qx < W) & (qr >= 0) & (qr < H)
                b = (fx if i else one - fx) * (fr if j else one - fr)
                taps.append((np.where(inside, qr * W + qx, 0), b.astype(F32), inside))
    s = np.zeros((n, 3), dtype=F32)
    nsum = np.zeros(n, dtype=F32)
    bsum = np.zeros(n, dtype=F32)
    with np.errstate(all="ignore"):
        for q, b, inside in taps:
            hz = h_depth[q]
            take = alive & inside & (h_len[q] > 0) & (h_oid[q] == oid)
            take &= np.abs(zexp - hz) <= depth_tol * np.where(zexp > hz, zexp, hz)
            if normals:
                take &= dot(N, Nh[q]) >= normal_min
            s = np.where(take[:, None], s + h_color[q] * b[:, None], s)
            nsum = np.where(take, nsum + h_len[q] * b, nsum)
            bsum = np.where(take, bsum + b, bsum)
        blend = bsum > 0
        h = s / bsum[:, None]
        nn = nsum / bsum + wt
        nn = np.where(nn > max_history, max_history, nn)
        nn = np.where(nn < wt, wt, nn)
        mixed = h + (color - h) * (wt / nn)[:, None]
    out = np.where(blend[:, None], mixed, out).astype(F32)
    out_len = np.where(blend, nn, out_len).astype(F32)
    assert s.dtype == F32 and nn.dtype == F32 and mixed.dtype == F32
    return out, out_len


# ---------------------------------------------------------------------------------- the camera move of the quality checks
# Fixed by tools/reproject_cpu_study.py (profiles/reproject_cpu_study.json): an orbit about the vertical axis through the
# origin - cornell's room stands around it - in steps of ORBIT_DEGREES, at ORBIT_SPP samples per frame.  The end-to-end test
# of tests/test_gpu_reproject.py renders frame A with the scene's camera and frame B one step on.
ORBIT_DEGREES = 2.0
ORBIT_SPP = 8
ORBIT_SIZE = (96, 64)


def orbit(cam, degrees):
    """cam turned about the vertical axis through the origin: binary64 arithmetic, rounded to binary32 once"""
    a = np.deg2rad(np.float64(degrees))
    c, s = np.cos(a), np.sin(a)

    def turn(v):
        x, y, z = (np.float64(F32(t)) for t in v)
        return tuple(float(F32(t)) for t in (c * x + s * z, y, -s * x + c * z))

    return dict(cam, position=turn(cam["position"]), direction=turn(cam["direction"]))
