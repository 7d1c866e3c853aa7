"""pt_ctx_reproject_var_weighted and pt_ctx_spp_plane restated: the contract of include/ptrace.h ("reprojection with per-pixel
sample counts") in numpy binary32, one numpy operation per operation of the contract, over whole frames at once.  Written from
the header, not from the kernel; nothing is shared with csrc/pt_reproject.h.  What is another restatement's text is imported:
the projection with the record's map (reproject_moved_ref.project_moved), the record lookup, N(.), dot, pos, s_of and the error
(reproject_ref, reproject_var_ref).  What is stated here is what the contract changes: the gather kept apart from the blend - a
pixel without samples needs h, h1, h2 and n themselves, which no blended output gives back -, the per-pixel wt, the two `long`
tests, and the window's one more condition.  tests/test_reproject_weighted_abi.py holds it against the two it stands on: with a
constant plane it is reproject_moved_ref.reproject_var_moved, byte for byte."""
import numpy as np

import reproject_moved_ref as mref
import reproject_ref as ref
import reproject_var_ref as vref
from reproject_ref import F32, I32

U32 = np.uint32
INF = F32(np.inf)


def spp_plane(n, base, mask=None, masked=0):
    """spp[p] = (d_mask && mask[p] != 0) ? masked : base"""
    if mask is None:
        return np.full(n, base, dtype=U32)
    return np.where(np.asarray(mask, dtype=np.uint8).reshape(n) != 0, U32(masked), U32(base)).astype(U32)


def gather(W, H, cam, depth, object_id, normal, hist_cam, hist_color, hist_len, hist_moments, hist_depth, hist_object_id, hist_normal,
           motion, depth_tol, normal_min):
    """Steps 2 to 4 with the record ahead of step 2, and the quotients of step 5: (blend, h (n, 3), h1, h2, n) - blend False
    where step 1 applies, the rest unspecified there."""
    n = W * H
    depth = np.ascontiguousarray(depth, dtype=F32).reshape(n)
    oid = np.ascontiguousarray(object_id, dtype=I32).reshape(n)
    h_color = np.ascontiguousarray(hist_color, dtype=F32).reshape(n, 3)
    h_len = np.ascontiguousarray(hist_len, dtype=F32).reshape(n)
    h_mom = np.ascontiguousarray(hist_moments, dtype=F32).reshape(n, 2)
    h_depth = np.ascontiguousarray(hist_depth, dtype=F32).reshape(n)
    h_oid = np.ascontiguousarray(hist_object_id, dtype=I32).reshape(n)
    normals = normal is not None and hist_normal is not None
    if normals:
        N = ref.normalized(np.asarray(normal, dtype=F32).reshape(n, 3))
        Nh = ref.normalized(np.asarray(hist_normal, dtype=F32).reshape(n, 3))
    depth_tol, normal_min = F32(depth_tol), F32(normal_min)
    idx = np.arange(n, dtype=np.int64)
    offset, scale, marker, ident = mref.lookup(oid, motion)
    same = ref.cam_floats(cam).tobytes() == ref.cam_floats(hist_cam).tobytes()
    one_tap = ident if same else np.zeros(n, bool)  # step 2: an IDENTITY record under bitwise-equal cameras
    ok, px, pr, zexp = mref.project_moved(cam, hist_cam, W, H, idx, depth, offset, scale)
    alive = (oid >= 0) & ~marker & (one_tap | ok)
    four = alive & ~one_tap
    px, pr = np.where(four, px, F32(0)), np.where(four, pr, F32(0))
    flx, flr = np.floor(px), np.floor(pr)
    x0, r0 = flx.astype(np.int64), flr.astype(np.int64)
    fx, fr = px - flx, pr - flr
    one = F32(1.0)
    zexp = np.where(one_tap, depth, zexp).astype(F32)
    s = np.zeros((n, 3), dtype=F32)
    a1 = np.zeros(n, dtype=F32)
    a2 = np.zeros(n, dtype=F32)
    nsum = np.zeros(n, dtype=F32)
    bsum = np.zeros(n, dtype=F32)
    with np.errstate(all="ignore"):
        for j in (0, 1):
            for i in (0, 1):
                qx, qr = x0 + i, r0 + j
                inside = (qx >= 0) & (qx < W) & (qr >= 0) & (qr < H)
                b = ((fx if i else one - fx) * (fr if j else one - fr)).astype(F32)
                q = np.where(inside, qr * W + qx, 0)
                first = i == 0 and j == 0
                q = np.where(one_tap, idx, q)                      # the single tap: q = idx with b = 1
                b = np.where(one_tap, one, b).astype(F32)
                inside = np.where(one_tap, first, inside)
                hz = h_depth[q]
                take = alive & inside & (h_len[q] > 0) & (h_oid[q] == oid)
                take &= np.abs(zexp - hz) <= depth_tol * np.where(zexp > hz, zexp, hz)
                if normals:
                    take &= ref.dot(N, Nh[q]) >= normal_min
                s = np.where(take[:, None], s + h_color[q] * b[:, None], s)
                a1 = np.where(take, a1 + h_mom[q, 0] * b, a1)
                a2 = np.where(take, a2 + h_mom[q, 1] * b, a2)
                nsum = np.where(take, nsum + h_len[q] * b, nsum)
                bsum = np.where(take, bsum + b, bsum)
        blend = bsum > 0
        h = s / bsum[:, None]
        h1, h2 = a1 / bsum, a2 / bsum
        nq = nsum / bsum
    assert h.dtype == F32 and h1.dtype == F32 and nq.dtype == F32
    return blend, h, h1, h2, nq


def spatial(W, H, s, oid, depth, spp, radius, depth_tol):
    """reproject_var_ref.spatial with the one more condition on every q but the centre: spp[q] == spp[idx]"""
    s = np.asarray(s, dtype=F32).reshape(H, W)
    oid = np.asarray(oid, dtype=I32).reshape(H, W)
    z = np.asarray(depth, dtype=F32).reshape(H, W)
    c = np.asarray(spp, dtype=U32).reshape(H, W)
    depth_tol = F32(depth_tol)
    S1 = np.zeros((H, W), F32)
    S2 = np.zeros((H, W), F32)
    cnt = np.zeros((H, W), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x0, x1 = max(0, -dx), min(W, W - dx)
            y0, y1 = max(0, -dy), min(H, H - dy)
            if x0 >= x1 or y0 >= y1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            if dx == 0 and dy == 0:
                take = np.ones(s[P].shape, bool)
            else:
                zp, zq = z[P], z[Q]
                with np.errstate(all="ignore"):
                    near = np.abs(zp - zq) <= depth_tol * np.where(zp > zq, zp, zq)
                take = (oid[Q] == oid[P]) & ((oid[P] < 0) | near) & (c[Q] == c[P])
            sq = s[Q]
            with np.errstate(all="ignore"):
                S1[P] = np.where(take, S1[P] + sq, S1[P])
                S2[P] = np.where(take, S2[P] + sq * sq, S2[P])
            cnt[P] = cnt[P] + take
    fc = np.maximum(cnt, 1).astype(F32)
    with np.errstate(all="ignore"):
        mean = S1 / fc
        vs = vref.pos(S2 / fc - mean * mean)
    return vs.reshape(W * H), cnt.reshape(W * H)


def reproject_var_weighted(W, H, cam, color, depth, object_id, normal=None, spp=None, hist_cam=None, hist_color=None, hist_len=None,
                           hist_moments=None, hist_depth=None, hist_object_id=None, hist_normal=None, motion=(), weight=1,
                           max_history=64.0, depth_tol=0.125, normal_min=0.9, min_frames=2, radius=3):
    """the four outputs of pt_ctx_reproject_var_weighted: colour (W*H, 3), length (W*H,), moments (W*H, 2), error (W*H,).  The
    parameters are the values in use, as in reproject_var_ref.reproject_var.  spp None: the delegation."""
    if spp is None:
        return mref.reproject_var_moved(W, H, cam, color, depth, object_id, normal, hist_cam=hist_cam, hist_color=hist_color,
                                        hist_len=hist_len, hist_moments=hist_moments, hist_depth=hist_depth,
                                        hist_object_id=hist_object_id, hist_normal=hist_normal, motion=motion, weight=weight,
                                        max_history=max_history, depth_tol=depth_tol, normal_min=normal_min, min_frames=min_frames,
                                        radius=radius)
    n = W * H
    color = np.ascontiguousarray(color, dtype=F32).reshape(n, 3)
    count = np.ascontiguousarray(spp, dtype=U32).reshape(n)
    w0 = F32(weight if weight else 1)
    wp = count.astype(F32)                        # round to nearest
    some = count > 0
    max_history, mf = F32(max_history), F32(min_frames)
    with np.errstate(all="ignore"):
        s = vref.s_of(color)
        q2 = s * s
    # step 1, for every pixel
    out = color.copy()
    out_len = wp.copy()
    m1, m2 = s.copy(), q2.copy()
    if hist_color is not None:
        blend, h, h1, h2, nq = gather(W, H, cam, depth, object_id, normal, hist_cam, hist_color, hist_len, hist_moments, hist_depth,
                                      hist_object_id, hist_normal, motion, depth_tol, normal_min)
        with np.errstate(all="ignore"):
            # c > 0: step 5 with wt = wp
            nn = nq + wp
            nn = np.where(nn > max_history, max_history, nn)
            nn = np.where(nn < wp, wp, nn)
            k = wp / nn
            mixed = h + (color - h) * k[:, None]
            b1 = h1 + (s - h1) * k
            b2 = h2 + (q2 - h2) * k
            # c == 0: the history as it is
            ne = np.where(nq > max_history, max_history, nq)
        assert nn.dtype == F32 and mixed.dtype == F32 and b1.dtype == F32 and ne.dtype == F32
        out = np.where((blend & some)[:, None], mixed, np.where((blend & ~some)[:, None], h, out)).astype(F32)
        out_len = np.where(blend, np.where(some, nn, ne), out_len).astype(F32)
        m1 = np.where(blend, np.where(some, b1, h1), m1).astype(F32)
        m2 = np.where(blend, np.where(some, b2, h2), m2).astype(F32)
    mom = np.stack([m1, m2], axis=1).astype(F32)
    with np.errstate(all="ignore"):
        vt = vref.pos(m2 - m1 * m1)
        long = np.where(some, out_len >= mf * wp, out_len >= mf * w0)
        k = np.where(some, wp / out_len, w0 / out_len).astype(F32)
    vs, cnt = spatial(W, H, s, object_id, depth, count, radius, depth_tol)
    with np.errstate(invalid="ignore"):
        v = np.where(long, vt, np.where(vs > vt, vs, vt)).astype(F32)
    e = vref.error_of(v, k, out)
    e = np.where(~long & (~some | (cnt < 2)), INF, e).astype(F32)
    assert vt.dtype == F32 and k.dtype == F32 and e.dtype == F32
    return out, out_len, mom, e
