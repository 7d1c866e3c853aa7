"""pt_ctx_reproject_moved and pt_ctx_reproject_var_moved restated: the contract of include/ptrace.h ("reprojecting history through
object edits") in numpy binary32.  It stands on tests/reproject_ref.py and tests/reproject_var_ref.py for everything that is
unchanged - the projection's camera half, the taps, their tests, the blend, the moments, the spatial estimate - and states only
what is new: the record lookup, the map Pm[a] = P[a]*scale + offset[a], the rule that a moved pixel never takes step 2, and,
independently of host/scene_io.cpp, pt_object_motion_between.  Nothing is shared with csrc/pt_reproject.h."""
import contextlib

import numpy as np

import ptlib
from ptlib import PtObjectMotion
import reproject_ref as ref
import reproject_var_ref as vref
from reproject_ref import F32, I32

IDENTITY = (0.0, 0.0, 0.0, 1.0)   # offset, scale
MARKER = (0.0, 0.0, 0.0, 0.0)
MAX_MOTION = 1 << 20
PT_SPHERE, PT_MESH = ptlib.abi.PT_SPHERE, ptlib.abi.PT_MESH


def table(records):
    """a ctypes array of PtObjectMotion from (ox, oy, oz, scale) tuples"""
    arr = (PtObjectMotion * max(len(records), 1))()
    for i, r in enumerate(records):
        arr[i].offset[:] = [float(v) for v in r[:3]]
        arr[i].scale = float(r[3])
    return arr


def words(rec):
    """the four words of a record, as stored"""
    return np.array(rec, dtype=F32).view(np.uint32)


def is_identity(rec):
    return words(rec).tolist() == [0, 0, 0, 0x3F800000]


def is_marker(rec):
    return F32(rec[3]) == 0


# ------------------------------------------------------------------------------------------ pt_object_motion_between
def motion_between(now, before):
    """The record of one edit.  now, before: dicts with kind, position, radius, color, emission, reflect_type, tri_offset,
    tri_count (floats as binary32).  Returns (ox, oy, oz, scale) as binary32."""
    def bits(v):
        return np.array(v, dtype=F32).view(np.uint32).tolist()

    marker = tuple(F32(v) for v in MARKER)
    if any(now[k] != before[k] for k in ("kind", "tri_offset", "tri_count", "reflect_type")):
        return marker
    if bits(now["color"]) != bits(before["color"]) or bits(now["emission"]) != bits(before["emission"]):
        return marker
    pn, pb = np.array(now["position"], dtype=F32), np.array(before["position"], dtype=F32)
    if not (np.isfinite(pn).all() and np.isfinite(pb).all()):
        return marker
    with np.errstate(all="ignore"):
        if now["kind"] == PT_SPHERE:
            rn, rb = F32(now["radius"]), F32(before["radius"])
            if not (np.isfinite(rn) and np.isfinite(rb)) or rn == 0:
                return marker
            scale = np.abs(rb) / np.abs(rn)
            off = pb - pn * scale
        else:
            scale = F32(1.0)
            off = pb - pn
    off = np.where(off == 0, F32(0.0), off).astype(F32)  # -0 is stored as +0
    if not (scale > 0 and np.isfinite(scale) and np.isfinite(off).all()):
        return marker
    assert off.dtype == F32 and scale.dtype == F32
    return (off[0], off[1], off[2], scale)


def object_dict(o):
    """a ptlib.PtObject as motion_between's dict"""
    return dict(kind=o.kind, position=tuple(o.position), radius=o.radius, color=tuple(o.color), emission=tuple(o.emission),
                reflect_type=o.reflect_type, tri_offset=o.tri_offset, tri_count=o.tri_count)


# ---------------------------------------------------------------------------------------------------------- the map
def project_moved(cam, hist_cam, W, H, idx, depth, offset, scale):
    """Step 3 with the mapped point, for the pixels idx: offset (n, 3) and scale (n,) are each pixel's record.  A pixel whose
    record is IDENTITY keeps P's bits.  The camera half (S, g, P) and the history half (a .. zexp) are reproject_ref.project's
    operations; the two lines between them are what is new."""
    idx = np.asarray(idx, dtype=np.int64)
    depth = np.asarray(depth, dtype=F32)
    offset = np.asarray(offset, dtype=F32).reshape(len(idx), 3)
    scale = np.asarray(scale, dtype=F32).reshape(len(idx))
    Cc, _, _, Lc, su, sv = ref.basis(cam)
    _, Dh, fh, Lh, suh, svh = ref.basis(hist_cam)
    x = (idx % W).astype(F32)
    y = (H - 1 - idx // W).astype(F32)
    fw, fhh = F32(W), F32(H)
    half = F32(0.5)
    ident = (offset.view(np.uint32) == 0).all(axis=1) & (scale.view(np.uint32) == 0x3F800000)
    with np.errstate(all="ignore"):
        sx = (x + half) / fw - half
        sy = (y + half) / fhh - half
        S = (Cc + su * sx[:, None]) + sv * sy[:, None]
        g = Lc - S
        P = Lc + (g * (F32(1.0) / np.sqrt(ref.dot(g, g)))[:, None]) * depth[:, None]
        Pm = P * scale[:, None] + offset                                  # the map: two operations per component
        P = np.where(ident[:, None], P, Pm).astype(F32)
        v = P - Lh
        a = ref.dot(v, Dh)
        ok = a > 0
        t = a / (fh * ref.dot(Dh, Dh))
        w = Dh * fh - v / t[:, None]
        sxh = ref.dot(w, suh) / ref.dot(suh, suh)
        syh = ref.dot(w, svh) / ref.dot(svh, svh)
        px = (sxh + half) * fw - half
        py = (syh + half) * fhh - half
        pr = F32(H - 1) - py
        ok = ok & (px > -1) & (px < fw) & (pr > -1) & (pr < fhh)
        zexp = np.sqrt(ref.dot(v, v))
    assert Pm.dtype == F32 and px.dtype == F32 and pr.dtype == F32 and zexp.dtype == F32
    return ok, px, pr, zexp


def lookup(object_id, motion):
    """(offset (n, 3), scale (n,), marker (n,), identity (n,)) of every pixel: rec = (uint32)id < n_motion ? motion[id] : IDENTITY;
    a pixel without a hit (id < 0) has no record and counts as IDENTITY here - the plain steps end it at step 1"""
    oid = np.asarray(object_id, dtype=I32).reshape(-1)
    tab = np.array(list(motion) + [IDENTITY], dtype=F32).reshape(-1, 4)
    n_motion = len(tab) - 1
    slot = np.where((oid >= 0) & (oid < n_motion), oid, n_motion)
    rec = tab[slot]
    scale = rec[:, 3].copy()
    offset = rec[:, :3].copy()
    marker = scale == 0
    ident = (offset.view(np.uint32) == 0).all(axis=1) & (scale.view(np.uint32) == 0x3F800000)
    return offset, scale, marker, ident


@contextlib.contextmanager
def _never_step_2(cam, hist_cam, offset, scale):
    """reproject_ref.reproject run for the moved pixels: its step 3 is project_moved with each pixel's record, and its same-camera
    test is made to fail by the history camera it is HANDED (returned here), which project_moved does not read - it closes over
    the true one.  "Otherwise step 2 is never taken, not even under bitwise-equal cameras."
    This rests on how the two restatements find their step 3: reproject_ref.reproject calls `project` through its module's
    global of that name, and reproject_var_ref goes through ref.reproject.  A `from reproject_ref import project` in either
    would bind the plain function and project with the decoy camera; the assertion below the patch is there to say so."""
    plain = ref.project

    def moved(_cam, _hist, W, H, idx, depth):
        idx = np.asarray(idx, dtype=np.int64)
        return project_moved(cam, hist_cam, W, H, idx, depth, offset[idx], scale[idx])

    decoy = dict(hist_cam, focal_length=float(F32(hist_cam["focal_length"])) * 2.0 + 1.0)
    assert ref.cam_floats(decoy).tobytes() != ref.cam_floats(cam).tobytes()
    ref.project = moved
    try:
        assert ref.reproject.__globals__["project"] is moved and vref.ref is ref, "the restatements no longer find step 3 this way"
        yield decoy
    finally:
        ref.project = plain


def _select(marker, ident, plain, moved, first):
    """per pixel: the marker's result is the first-frame form's (step 1), IDENTITY's the plain call's, any other record's the
    moved run's.  Every output of both calls is a function of the pixel's own taps and of the INPUT frame around it, so the
    choice per pixel is the choice per output word."""
    out = []
    for p, m, f in zip(plain, moved, first):
        mk = marker.reshape((-1,) + (1,) * (p.ndim - 1))
        idn = ident.reshape((-1,) + (1,) * (p.ndim - 1))
        out.append(np.where(mk, f, np.where(idn, p, m)).astype(p.dtype))
    return tuple(out)


def reproject_moved(W, H, cam, color, depth, object_id, normal=None, hist_cam=None, hist_color=None, motion=(), **kw):
    """the two outputs of pt_ctx_reproject_moved; motion: a sequence of (ox, oy, oz, scale); the rest as reproject_ref.reproject"""
    args = (W, H, cam, color, depth, object_id, normal)
    plain = ref.reproject(*args, hist_cam=hist_cam, hist_color=hist_color, **kw)
    if hist_color is None:
        return plain
    offset, scale, marker, ident = lookup(object_id, motion)
    first = ref.reproject(*args, weight=kw.get("weight", 1))
    with _never_step_2(cam, hist_cam, offset, scale) as decoy:
        moved = ref.reproject(*args, hist_cam=decoy, hist_color=hist_color, **kw)
    return _select(marker, ident, plain, moved, first)


def reproject_var_moved(W, H, cam, color, depth, object_id, normal=None, hist_cam=None, hist_color=None, motion=(), **kw):
    """the four outputs of pt_ctx_reproject_var_moved: "colour, length and taps are pt_ctx_reproject_moved's" - the moments ride
    the same taps, the spatial estimate does not read the table"""
    args = (W, H, cam, color, depth, object_id, normal)
    plain = vref.reproject_var(*args, hist_cam=hist_cam, hist_color=hist_color, **kw)
    if hist_color is None:
        return plain
    offset, scale, marker, ident = lookup(object_id, motion)
    own = {k: v for k, v in kw.items() if not k.startswith("hist_")}
    first = vref.reproject_var(*args, **own)
    with _never_step_2(cam, hist_cam, offset, scale) as decoy:
        moved = vref.reproject_var(*args, hist_cam=decoy, hist_color=hist_color, **kw)
    return _select(marker, ident, plain, moved, first)
