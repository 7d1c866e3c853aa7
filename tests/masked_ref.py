"""pt_ctx_select_pixels' predicate (include/ptrace.h, "THE PREDICATE") in numpy binary32, the ctypes declarations of it and of
pt_ctx_render_masked, and the planes the tests feed it.  Shared by tests/test_masked_abi.py and tests/test_gpu_masked.py."""

import numpy as np


F32 = np.float32
U8 = np.uint8
SIZES = ((1, 1), (7, 5), (257, 3), (64, 1))
PARAMS = dict(weight_max=0.0, len_max=8.0)  # what the loop passes: the fallback's weight, one frame of 8 samples


def select(weight=None, length=None, weight_max=0.0, len_max=0.0):
    """(mask as uint8, the number of ones): mask[p] = ((weight && !(weight[p] > weight_max)) || (len && !(len[p] > len_max)))"""
    assert weight is not None or length is not None
    n = len(weight if weight is not None else length)
    m = np.zeros(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        if weight is not None:
            m |= ~(np.asarray(weight, dtype=F32) > F32(weight_max))
        if length is not None:
            m |= ~(np.asarray(length, dtype=F32) > F32(len_max))
    return m.astype(U8), int(m.sum())


def plane(n, threshold, seed):
    """n values around `threshold`: below it, equal to it, its two neighbours in binary32, NaN, +inf, -inf and -0, in random
    places; every special value at least once when n allows (n >= 8)"""
    rng = np.random.default_rng(seed)
    t = F32(threshold)
    special = np.array([t, np.nan, np.inf, -0.0, -np.inf, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf)), t - F32(1)],
                       dtype=F32)
    v = (rng.random(n) * 4 - 1).astype(F32) + t
    pick = rng.random(n) < 0.5
    v[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    if n >= len(special):
        v[rng.permutation(n)[:len(special)]] = special
    return v
