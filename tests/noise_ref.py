"""numpy restatement of pt_ctx_accum_noise's contract ("THE NOISE ESTIMATE" in include/ptrace.h), written from the header's
text: every operation in binary32, in the header's order, on arrays; plus a parser for checkpoint versions 1 and 2.

H, A: the held and the half-A sums, uint64 arrays of shape (3, n) (32.32 fixed point).  n_a, n_b: samples per pixel in the
halves."""
import struct

import numpy as np

f32 = np.float32
FRAC_BITS = 28   # the fixed-point sum: floor(e * 2^28)
BINS = 64
BIN_BASE = 460   # (127 - 12) << 2: four bins per octave from 2^-12


def clamp01(v):
    v = np.asarray(v, dtype=f32)
    return np.where(v < f32(0), f32(0), np.where(v > f32(1), f32(1), v)).astype(f32)


def mean(S, n):
    """clamp((float)((double)S * 2^-32) / (float)n)"""
    d = np.asarray(S, dtype=np.uint64).astype(np.float64) * (1.0 / 4294967296.0)
    return clamp01(d.astype(f32) / f32(n))


def weight(n_a, n_b):
    """sqrt((float)nA * (float)nB) / ((float)nA + (float)nB)"""
    fa, fb = f32(n_a), f32(n_b)
    return f32(np.sqrt(f32(fa * fb), dtype=f32) / f32(fa + fb))


def error_from_means(a, b, m, w):
    """e(p) from the half means a, b and the whole mean m, arrays of shape (3, n) in binary32"""
    a, b, m = (np.asarray(v, dtype=f32) for v in (a, b, m))
    d = np.abs(a - b).astype(f32)
    num = ((d[0] + d[1]).astype(f32) + d[2]).astype(f32) * f32(w)
    den = np.sqrt((f32(0.015625) + ((m[0] + m[1]).astype(f32) + m[2]).astype(f32)).astype(f32), dtype=f32)
    return (num.astype(f32) / den).astype(f32)


def error(H, A, n_a, n_b):
    H, A = np.asarray(H, dtype=np.uint64), np.asarray(A, dtype=np.uint64)
    return error_from_means(mean(A, n_a), mean(H - A, n_b), mean(H, n_a + n_b), weight(n_a, n_b))


def fixed_sum(e):
    """the sum of floor(e * 2^28) as a Python int"""
    q = np.floor(np.asarray(e, dtype=f32).astype(np.float64) * float(1 << FRAC_BITS)).astype(np.uint64)
    return int(q.sum(dtype=np.uint64))


def mean_error(total, pixels):
    """(double)sum * 2^-28 / (double)pixels"""
    return float(total) * (1.0 / (1 << FRAC_BITS)) / float(pixels)


def bins(e):
    k = (np.asarray(e, dtype=f32).view(np.uint32) >> np.uint32(21)).astype(np.int64)
    return np.where(k <= BIN_BASE, 0, np.where(k >= BIN_BASE + 63, 63, k - BIN_BASE))


def histogram(e):
    return np.bincount(bins(e), minlength=BINS).astype(np.uint32)


def bin_upper(b):
    """the upper edge of bin b: the float with bits (461 + b) << 21; +inf for the last"""
    if b >= BINS - 1:
        return float("inf")
    return float(np.array([(BIN_BASE + 1 + b) << 21], dtype=np.uint32).view(f32)[0])


def quantile_bin(hist, pixels, q):
    """the first bin at which the cumulative count reaches ceil(q * pixels)"""
    need = max(1, int(np.ceil(float(f32(q)) * float(pixels))))
    cum = np.cumsum(np.asarray(hist, dtype=np.uint64))
    return int(np.searchsorted(cum, need, side="left"))


def parse_checkpoint(data):
    """A pt_ctx_accum_save file (version 1 or 2) as a dict: version, key fields, total, part_px, counts, n_a (version 2, else
    None), sums (3, total) uint64, a (version 2, else None).  The trailing hash is not checked here."""
    assert data[:8] == b"PTACCUM1", data[:8]
    version, = struct.unpack_from("<I", data, 8)
    assert version in (1, 2), version
    width, height, idx_begin, idx_end, chunk_pixels, chunk_first, chunk_step = struct.unpack_from("<7I", data, 12)
    seed, fingerprint = struct.unpack_from("<2Q", data, 40)
    total, part_px, n_parts = struct.unpack_from("<3I", data, 56)
    at = 68
    counts = np.frombuffer(data, dtype="<u4", count=n_parts, offset=at).copy()
    at += 4 * n_parts
    n_a = None
    if version == 2:
        n_a = np.frombuffer(data, dtype="<u4", count=n_parts, offset=at).copy()
        at += 4 * n_parts
    sums = np.frombuffer(data, dtype="<u8", count=3 * total, offset=at).reshape(3, total).copy()
    at += 24 * total
    a = None
    if version == 2:
        a = np.frombuffer(data, dtype="<u8", count=3 * total, offset=at).reshape(3, total).copy()
        at += 24 * total
    assert len(data) == at + 8, (len(data), at)
    return dict(version=version, width=width, height=height, idx_begin=idx_begin, idx_end=idx_end, chunk_pixels=chunk_pixels,
                chunk_first=chunk_first, chunk_step=chunk_step, seed=seed, fingerprint=fingerprint, total=total,
                part_px=part_px, counts=counts, n_a=n_a, sums=sums, a=a)
