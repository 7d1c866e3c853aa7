"""pt_ctx_overlay restated: the contract of include/ptrace_overlay.h ("THE ARITHMETIC" of pt_ctx_overlay) in numpy binary32, one numpy
operation per operation of the contract, over whole frames at once.  Nothing is shared with csrc/pt_overlay.h; the camera basis
and dot() are tests/reproject_ref.py's, themselves a restatement.  Cameras are the dicts of tests/kats_camera.py, the parameters
a dict with the fields of pt_overlay_params (params() builds one; struct() turns it into the ctypes struct).  The window of step
6 is the definition - every (i, j) of the square tried in turn - not the separable form the kernel uses."""
import ctypes as C
import importlib

import numpy as np

import ptlib
from reproject_ref import basis, dot, pt_camera  # noqa: F401  (pt_camera: for the callers)

F32 = np.float32
I32 = np.int32
SKY, GRID = 1, 2
MAX_SELECTED, MAX_RADIUS = 16, 8
overlay_abi = importlib.import_module("path-tracer-rust_amd.overlay_abi")  # include/ptrace_overlay.h as ctypes
PtOverlayParams = overlay_abi.pt_overlay_params
COLOURS = ("outline_color", "fill_color", "sky_top", "sky_bottom", "grid_color")
SCALARS = ("outline_alpha", "fill_alpha", "grid_alpha", "grid_y", "grid_spacing", "grid_half_width", "grid_extent")


def params(**kw):
    """all zero, but for what is named"""
    p = dict(flags=0, selected=(), radius=0)
    p.update({k: (0.0, 0.0, 0.0) for k in COLOURS})
    p.update({k: 0.0 for k in SCALARS})
    assert set(kw) <= set(p), sorted(set(kw) - set(p))
    p.update(kw)
    return p


def struct(p):
    s = PtOverlayParams()
    s.flags, s.n_selected, s.radius = p["flags"], len(p["selected"]), p["radius"]
    for i, v in enumerate(p["selected"]):
        s.selected[i] = v
    for k in COLOURS:
        setattr(s, k, ptlib.f3(*[float(F32(v)) for v in p[k]]))
    for k in SCALARS:
        setattr(s, k, float(F32(p[k])))
    return s


def from_struct(s):
    p = params(flags=s.flags, selected=tuple(s.selected[i] for i in range(s.n_selected)), radius=s.radius)
    p.update({k: tuple(getattr(s, k)) for k in COLOURS})
    p.update({k: getattr(s, k) for k in SCALARS})
    return p


def defaults(L, cam=None):
    s = PtOverlayParams()
    c = pt_camera(cam) if cam is not None else None
    assert L.pt_overlay_defaults(C.byref(c) if c is not None else None, C.byref(s)) == 0, L.pt_last_error()
    return from_struct(s)


def in_use(p):
    """the values a zero field stands for"""
    q = dict(p)
    q["radius"] = p["radius"] or 2
    q["outline_alpha"] = p["outline_alpha"] or 1.0
    q["grid_alpha"] = p["grid_alpha"] or 1.0
    return q


# ------------------------------------------------------------------------------------------------------ the arithmetic
def mix(a, b, t):
    """a + (b - a) * t"""
    return a + (b - a) * t


def ray(cam, W, H, idx):
    """step 1: d for the pixels idx, (n, 3), and the lens centre"""
    Cc, _, _, Lc, su, sv = basis(cam)
    idx = np.asarray(idx, dtype=np.int64)
    x = (idx % W).astype(F32)
    y = (H - 1 - idx // W).astype(F32)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        sx = (x + half) / F32(W) - half
        sy = (y + half) / F32(H) - half
        S = (Cc + su * sx[:, None]) + sv * sy[:, None]
        g = Lc - S
        d = g * (F32(1.0) / np.sqrt(dot(g, g)))[:, None]
    assert d.dtype == F32
    return d, Lc


def mask(object_id, selected):
    """M: the id is one of the listed ones; an id below 0 never is"""
    oid = np.asarray(object_id, dtype=I32)
    m = np.zeros(oid.shape, dtype=bool)
    for s in selected:
        m |= oid == I32(s)
    return m & (oid >= 0)


def window(M, W, H, R):
    """step 6's test: some q = (x+i, r+j) inside the frame has M(q), |i| <= R, |j| <= R; (W*H,) bool"""
    M = np.asarray(M, dtype=bool).reshape(H, W)
    pad = np.zeros((H + 2 * R, W + 2 * R), dtype=bool)
    pad[R:R + H, R:R + W] = M
    out = np.zeros((H, W), dtype=bool)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            out |= pad[R + j:R + j + H, R + i:R + i + W]
    return out.reshape(W * H)


def shade(cam, W, H, p, idx, object_id, depth, selected, outlined, rgb):
    """steps 1 to 7 for the pixels idx, each with its id, depth, M and window result given: ((n, 3) binary32, (n,) touched).
    This is what pt_overlay_pixel_host computes for one pixel."""
    p = in_use(p)
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx)
    rgb = np.ascontiguousarray(rgb, dtype=F32).reshape(n, 3)
    v = rgb.copy()
    touched = np.zeros(n, dtype=bool)
    selected = np.asarray(selected, dtype=bool)
    outlined = np.asarray(outlined, dtype=bool) & ~selected
    col = {k: np.array([F32(c) for c in p[k]], dtype=F32) for k in COLOURS}
    with np.errstate(all="ignore"):
        if p["flags"] & (SKY | GRID):
            d, Lc = ray(cam, W, H, idx)
        if p["flags"] & SKY:
            sky = np.asarray(object_id, dtype=I32) < 0
            s = d[:, 1] * F32(0.5) + F32(0.5)
            s = np.where(s > 0, np.where(s > 1, F32(1.0), s), F32(0.0)).astype(F32)
            v = np.where(sky[:, None], mix(col["sky_bottom"][None, :], col["sky_top"][None, :], s[:, None]), v)
            touched |= sky
        if p["flags"] & GRID:
            depth = np.asarray(depth, dtype=F32)
            sp, hw, ext = F32(p["grid_spacing"]), F32(p["grid_half_width"]), F32(p["grid_extent"])
            t = (F32(p["grid_y"]) - Lc[1]) / d[:, 1]
            sees = (t > 0) & (t < depth)
            qx = Lc[0] + d[:, 0] * t
            qz = Lc[2] + d[:, 2] * t
            inside = (np.abs(qx) <= ext) & (np.abs(qz) <= ext)
            line = np.zeros(n, dtype=bool)
            for q in (qx, qz):
                k = np.floor(q / sp + F32(0.5))
                line |= np.abs(q - k * sp) <= hw
            on = sees & inside & line
            v = np.where(on[:, None], mix(v, col["grid_color"][None, :], F32(p["grid_alpha"])), v)
            touched |= on
        if F32(p["fill_alpha"]) != 0:
            v = np.where(selected[:, None], mix(v, col["fill_color"][None, :], F32(p["fill_alpha"])), v)
            touched |= selected
        v = np.where(outlined[:, None], mix(v, col["outline_color"][None, :], F32(p["outline_alpha"])), v)
        touched |= outlined
    assert v.dtype == F32
    out = rgb.copy().view(np.uint32)
    out[touched] = v.view(np.uint32)[touched]  # an untouched pixel keeps its input's bits
    return out.view(F32), touched


def overlay(W, H, p, cam, rgb, object_id=None, depth=None):
    """pt_ctx_overlay's output for a whole frame: ((W*H, 3) binary32, (W*H,) touched); p None = all zero"""
    p = params() if p is None else p
    n = W * H
    oid = np.full(n, 0, dtype=I32) if object_id is None else np.ascontiguousarray(object_id, dtype=I32).reshape(n)
    z = np.zeros(n, dtype=F32) if depth is None else np.ascontiguousarray(depth, dtype=F32).reshape(n)
    M = mask(oid, p["selected"]) if object_id is not None else np.zeros(n, dtype=bool)
    near = window(M, W, H, in_use(p)["radius"])
    return shade(cam, W, H, p, np.arange(n), oid, z, M, near & ~M, rgb)


def default_grid(position):
    """pt_overlay_defaults' camera rule in binary64, each value rounded once: (spacing, half width, extent)"""
    x, y, z = (np.float64(F32(c)) for c in position)
    zoom = np.sqrt(x * x + y * y + z * z) / 5.0
    spacing = 10.0 ** np.floor(np.log10(zoom * 1.2 + 1.0))
    return F32(spacing), F32(0.01 * zoom), F32(5.0 * spacing)
