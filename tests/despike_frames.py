"""The frames tests/test_despike_abi.py (on the host) and tests/test_gpu_despike.py (on the device) walk: a background that cannot
spike (despike_ref.background: uniform in [0.5, 1] per channel, so with threshold >= 2 no background pixel is one) and what is
planted on it.  The sizes are the smallest at which a tile of 32 x 8, its halo or a tail can go wrong."""
import numpy as np

import despike_ref as ref
from despike_ref import F32

SIZES = ((1, 1), (1, 7), (7, 1), (31, 7), (32, 8), (33, 9), (64, 16), (67, 19), (96, 64))
COMBOS = [(radius, rank, flag) for radius in (1, 2) for rank in (1, 2, 3, 4) for flag in (0, 1)]
SPIKE = 64.0


def planted(w, h, seed=0):
    """(rgb (w*h, 3), ids (w*h,), plan): what fits into the frame of
    - isolated spikes of 64 in every corner, on every edge, on both sides of the tile seams (x = 31/32/33, y = 7/8/9), one of
      1e30, one beside a NaN pixel and one beside a +inf pixel;
    - touching pairs across the seam between x = 31 and 32 and the one between y = 7 and 8;
    - a one-pixel bright line along y = 30 from x = 10 to 40;
    - NaN, +inf and -inf channels alone; a pixel of -0 channels; a pixel of negative luminance.
    plan: pixel indices by kind - "isolated", "pairs", "line", "line_ends", "nonfinite"."""
    rgb = ref.background(w, h, seed + 1000 * w + h)
    plan = {"isolated": [], "pairs": [], "line": [], "line_ends": [], "nonfinite": []}

    def fits(x, y):
        return 0 <= x < w and 0 <= y < h

    def put(kind, x, y, value):
        rgb[y, x] = value
        plan[kind].append(y * w + x)

    isolated = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2),
                (31, 12), (32, 15), (33, 18), (40, 7), (44, 8), (48, 9), (33, 5), (71, 20), (70, 41)]
    for x, y in dict.fromkeys(isolated):
        if fits(x, y):
            put("isolated", x, y, SPIKE)
    if fits(20, 20):
        put("isolated", 20, 20, 1e30)
    for a, b in (((31, 3), (32, 3)), ((50, 7), (50, 8))):
        if fits(*a) and fits(*b):
            put("pairs", *a, SPIKE)
            put("pairs", *b, SPIKE)
    if fits(12, 30):
        xs = list(range(10, min(41, w)))
        for x in xs:
            put("line", x, 30, SPIKE)
        plan["line_ends"] = [30 * w + xs[0], 30 * w + xs[-1]]
    for x, y, c, v in ((60, 20, 0, np.nan), (62, 24, 1, np.inf), (64, 28, 2, -np.inf), (70, 20, 1, np.nan), (70, 40, 0, np.inf),
                       (3, 0, 2, np.nan), (0, 4, 0, -np.inf)):
        if fits(x, y) and (y * w + x) not in plan["isolated"]:
            rgb[y, x, c] = v
            plan["nonfinite"].append(y * w + x)
    if fits(80, 50):
        rgb[50, 80] = -0.0
    if fits(84, 54):
        rgb[54, 84] = -3.0
    if fits(5, 3):
        rgb[3, 5, 1] = -0.0  # one -0 channel in a pixel that is copied
    return np.ascontiguousarray(rgb.reshape(-1, 3), dtype=F32), ref.voronoi_ids(w, h, seed + 7), plan


def scattered(w, h, count, seed):
    """a large frame: the background with `count` plants at random places - spikes of 64 and of 1e30, and NaN and inf channels"""
    rng = np.random.default_rng(seed)
    rgb = ref.background(w, h, seed).reshape(-1, 3)
    at = rng.choice(w * h, size=count, replace=False)
    kind = rng.integers(0, 8, size=count)
    for i, k in zip(at.tolist(), kind.tolist()):
        if k < 5:
            rgb[i] = SPIKE * (1 + k)
        elif k == 5:
            rgb[i] = 1e30
        elif k == 6:
            rgb[i, i % 3] = np.nan
        else:
            rgb[i, i % 3] = np.inf if i % 2 else -np.inf
    return np.ascontiguousarray(rgb, dtype=F32), ref.voronoi_ids(w, h, seed + 1), at
