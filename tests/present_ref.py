"""pt_ctx_present restated: the contract of include/ptrace.h ("THE ARITHMETIC" of pt_ctx_present) with Python integers for S and
numpy.float32 / float64 for the conversions.  The table is an argument (pt_present_thresholds gives the library's)."""
import ctypes as C

import numpy as np

from ptlib import abi

F32 = np.float32
RGBA8, RGB8 = abi.PT_PRESENT_RGBA8, abi.PT_PRESENT_RGB8
FRAMEBUFFER_ORDER = abi.PT_PRESENT_FRAMEBUFFER_ORDER
ONE_BITS = 0x3F800000


def thresholds(L):
    t = (C.c_uint32 * 256)()
    assert L.pt_present_thresholds(t) == 0
    return np.array(t, dtype=np.uint32)


def quantize_host(L, values, exposure=0.0):
    a = np.ascontiguousarray(values, dtype=F32)
    out = np.zeros(a.shape, dtype=np.uint8)
    assert L.pt_present_quantize_host(a.ctypes.data_as(C.c_void_p), a.size, exposure, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def bits_to_f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(F32)


# ------------------------------------------------------------------------------------------------------ the arithmetic
def clamp(v, exposure):
    """step 2: v' = v * exposure in binary32; c(v') = v' > 0 ? (v' > 1 ? 1 : v') : 0 (NaN and -0 give +0, +inf gives 1)"""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.asarray(v, dtype=F32) * F32(exposure if exposure != 0.0 else 1.0)
        return np.where(e > 0, np.where(e > 1, F32(1), e), F32(0)).astype(F32)


def byte(table, m):
    """step 5: the number of k in 1..255 with bits(m) >= T[k]"""
    b = np.ascontiguousarray(m, dtype=F32).view(np.uint32)
    return (b[..., None] >= np.asarray(table, dtype=np.uint32)[1:]).sum(axis=-1).astype(np.uint8)


def weights(n, on):
    """w[X][x]: the integer overlap of output cell X, [X*n, (X+1)*n), with source pixel x, [x*on, (x+1)*on); on rows, n columns"""
    w = [[0] * n for _ in range(on)]
    for X in range(on):
        lo, hi = X * n, (X + 1) * n
        for x in range(lo // on, -(-hi // on)):
            w[X][x] = min(hi, (x + 1) * on) - max(lo, x * on)
    return w


def display(frame, w, h, flags=0):
    """step 1: D[y][x] of a (w*h, 3) frame"""
    f = np.asarray(frame, dtype=F32).reshape(w * h, 3)
    return (f if flags & FRAMEBUFFER_ORDER else f[::-1]).reshape(h, w, 3)


def mean(frame, w, h, ow, oh, exposure=0.0, flags=0):
    """steps 1-4: m per output pixel and channel, (oh, ow, 3) binary32"""
    c = clamp(display(frame, w, h, flags), exposure)
    if (ow, oh) == (w, h):
        return c
    q = np.floor(c.astype(np.float64) * 4294967296.0).astype(np.uint64)  # exact: c has 24 bits, the factor is a power of two
    ql = [[[int(v) for v in px] for px in row] for row in q.tolist()]
    wx, wy = weights(w, ow), weights(h, oh)
    div = np.float64(w * h) * np.float64(4294967296.0)
    out = np.zeros((oh, ow, 3), dtype=F32)
    for Y in range(oh):
        ys = [(y, wy[Y][y]) for y in range(h) if wy[Y][y]]
        for X in range(ow):
            xs = [(x, wx[X][x]) for x in range(w) if wx[X][x]]
            for ch in range(3):
                S = sum(a * b * ql[y][x][ch] for y, a in ys for x, b in xs)
                assert S < 1 << 60
                out[Y, X, ch] = F32(np.float64(S) / div)  # int -> binary64 rounds to nearest even; one division; one rounding
    return out


# ------------------------------------------------------------------------------- the same arithmetic for full-size frames
# mean() above is triple-nested Python over big integers: the independent form, and too slow beyond a few thousand pixels.  The
# forms below are the same integers computed separably - rows, then columns - in uint64, and the same count of thresholds by a
# binary search.  tests/test_present_abi.py holds them equal to the slow forms on every small shape.
def overlaps(n, on):
    """the pairs (X, x) of an output cell and a source pixel that overlap, in order, and the integer length of each overlap: cut the
    axis of n * on units at every multiple of n (a cell's border) and of on (a pixel's border); each piece lies in one cell and one
    pixel.  Three int64 / uint64 arrays."""
    cuts = np.union1d(np.arange(on + 1, dtype=np.int64) * n, np.arange(n + 1, dtype=np.int64) * on)
    lo = cuts[:-1]
    return lo // n, lo // on, (cuts[1:] - lo).astype(np.uint64)


def fold(a, n, on):
    """axis 0 of the uint64 array a (n source pixels) folded into `on` cells: out[X] = sum over x of weight(X, x) * a[x]"""
    assert a.dtype == np.uint64 and a.shape[0] == n
    X, x, wgt = overlaps(n, on)
    first = np.searchsorted(X, np.arange(on))  # every cell has a piece, and X does not decrease
    return np.add.reduceat(a[x] * wgt.reshape((-1,) + (1,) * (a.ndim - 1)), first, axis=0)


def sums_separable(frame, w, h, ow, oh, exposure=0.0, flags=0):
    """step 4's S per output pixel and channel, (oh, ow, 3) uint64: rows first, then columns.  Every partial sum is at most the
    final S, and S < 2^60 by the contract (asserted), so nothing wraps."""
    c = clamp(display(frame, w, h, flags), exposure)
    q = np.floor(c.astype(np.float64) * 4294967296.0).astype(np.uint64)  # (h, w, 3)
    mid = fold(q, h, oh)                                  # (oh, w, 3)
    S = fold(np.ascontiguousarray(mid.transpose(1, 0, 2)), w, ow).transpose(1, 0, 2)  # (oh, ow, 3)
    assert int(S.max()) < 1 << 60
    return np.ascontiguousarray(S)


def mean_separable(frame, w, h, ow, oh, exposure=0.0, flags=0):
    """mean() through sums_separable(): uint64 -> binary64 rounds to nearest even, one division, one rounding to binary32"""
    if (ow, oh) == (w, h):
        return clamp(display(frame, w, h, flags), exposure)
    S = sums_separable(frame, w, h, ow, oh, exposure, flags)
    return (S.astype(np.float64) / (np.float64(w * h) * np.float64(4294967296.0))).astype(F32)


def byte_sorted(table, m):
    """byte() by binary search: T[1..255] increases strictly, so the count of k with T[k] <= bits is where bits would be put in"""
    t = np.asarray(table, dtype=np.uint32)[1:]
    assert (np.diff(t.astype(np.int64)) > 0).all()
    b = np.ascontiguousarray(m, dtype=F32).view(np.uint32)
    return np.searchsorted(t, b, side="right").astype(np.uint8)


def present(table, frame, w, h, ow=0, oh=0, exposure=0.0, fmt=RGBA8, flags=0, separable=False):
    """the bytes pt_ctx_present writes: (oh, ow, 4 or 3) uint8.  separable: through the forms for full-size frames."""
    ow, oh = (ow, oh) if ow or oh else (w, h)
    if separable:
        b = byte_sorted(table, mean_separable(frame, w, h, ow, oh, exposure, flags))
    else:
        b = byte(table, mean(frame, w, h, ow, oh, exposure, flags))
    if fmt == RGBA8:
        b = np.concatenate([b, np.full((oh, ow, 1), 255, dtype=np.uint8)], axis=2)
    return b


def read_p3(path):
    """the numbers of pt_write_ppm's file: (h, w, 3) uint8"""
    lines = [ln for ln in open(path).read().split("\n") if not ln.startswith("#")]
    tok = " ".join(lines).split()
    assert tok[0] == "P3" and tok[3] == "255"
    w, h = int(tok[1]), int(tok[2])
    return np.array(tok[4:], dtype=np.int64).astype(np.uint8).reshape(h, w, 3)


def read_p6(path):
    data = open(path, "rb").read()
    magic, dims, maxval, body = data.split(b"\n", 3)
    assert magic == b"P6" and maxval == b"255"
    w, h = (int(v) for v in dims.split())
    assert len(body) == w * h * 3
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)
