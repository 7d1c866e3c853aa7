"""numpy replay of pt_ctx_render_adaptive's decision rule, written from the header's text (include/ptrace.h, "adaptive sampling")
on top of noise_ref.py: the levels, the split of a level's samples into the halves, the tiles, E and the closing decision.

A call's pixels are `rows` whole image rows of `width` pixels in call order; pixel k lies in tile row (k // width) // tile and
tile column (k % width) // tile; tiles are numbered row by row."""
import numpy as np

import noise_ref

f32 = np.float32


def levels(min_spp, cap):
    """n_0 = min_spp (0 = 16) rounded up to a multiple of 8, n_(j+1) = min(2 n_j, cap); a cap below n_0 is the only level"""
    n = (min_spp or 16)
    n = min((n + 7) // 8 * 8, cap)
    out = [n]
    while out[-1] < cap:
        out.append(min(2 * out[-1], cap))
    return out


def halves(lv):
    """[(nA, nB)] the open tiles hold after each level: [c, m) goes to A, [m, T) to B, m = min(T, c + 4 ceil((T - c) / 8))"""
    out, c, n_a = [], 0, 0
    for t in lv:
        m = min(t, c + 4 * ((t - c + 7) // 8))
        n_a += m - c
        out.append((n_a, t - n_a))
        c = t
    return out


def threshold(tile_error):
    """q = (uint64) floor((double) tile_error * 2^28), tile_error a binary32"""
    return int(np.floor(float(f32(tile_error)) * float(1 << noise_ref.FRAC_BITS)))


def tile_ids(width, rows, tile):
    k = np.arange(width * rows)
    tiles_x = (width + tile - 1) // tile
    return (k // width) // tile * tiles_x + (k % width) // tile, tiles_x * ((rows + tile - 1) // tile)


def replay(maps, width, rows, tile, tile_error, lv, stop_after=None):
    """maps[j]: e(p) of EVERY pixel of the call at level j as a uniform frame would have it (float32, width * rows), or None
    where the level has no estimate (nB = 0).  stop_after: a cancel after that many levels.  Returns a dict: spp and error per
    pixel (+inf without an evaluation), closed_at per tile (-1: open at the end), tiles, tiles_open, tiles_closed per level,
    level_spp, samples, err_sum (the sum of the tiles' last E) and mean_error."""
    tid, n_tiles = tile_ids(width, rows, tile)
    npix = width * rows
    q = threshold(tile_error)
    pixels = np.bincount(tid, minlength=n_tiles)
    is_open = np.ones(n_tiles, dtype=bool)
    closed_at = np.full(n_tiles, -1)
    spp = np.zeros(npix, dtype=np.uint32)
    err = np.full(npix, np.inf, dtype=f32)
    last_e = [None] * n_tiles
    tiles_closed = []
    n_run = len(lv) if stop_after is None else min(stop_after, len(lv))
    for j in range(n_run):
        if not is_open.any():
            break
        live = is_open[tid]
        spp[live] = lv[j]
        closed = 0
        if maps[j] is not None:
            e = np.asarray(maps[j], dtype=f32)
            err[live] = e[live]
            fixed = np.floor(e.astype(np.float64) * float(1 << noise_ref.FRAC_BITS)).astype(np.uint64)
            tile_sum = np.zeros(n_tiles, dtype=np.uint64)
            np.add.at(tile_sum, tid, fixed)  # integers: one pass over the pixels whatever the number of tiles (34 320 at 1056 x 520)
            for t in np.nonzero(is_open)[0]:
                E = int(tile_sum[t])
                last_e[t] = E
                if E <= q * int(pixels[t]):
                    is_open[t] = False
                    closed_at[t] = j
                    closed += 1
        tiles_closed.append(closed)
    err_sum = sum(v for v in last_e if v is not None)
    every = all(v is not None for v in last_e)
    return dict(spp=spp, error=err, closed_at=closed_at, tiles=n_tiles, tiles_open=int(is_open.sum()), tiles_closed=tiles_closed,
                level_spp=list(lv[:len(tiles_closed)]), samples=int(spp.sum(dtype=np.uint64)), err_sum=err_sum,
                mean_error=noise_ref.mean_error(err_sum, npix) if every else float("inf"))


def maps_from_sums(H, A, lv):
    """the per-level error maps from the held / half-A sums a uniform frame holds after each level ((3, n) uint64 each)"""
    out = []
    for (n_a, n_b), h, a in zip(halves(lv), H, A):
        out.append(noise_ref.error(h, a, n_a, n_b) if n_a and n_b else None)
    return out
