#!/usr/bin/env python3
"""(pixel, sample) pairs whose draw of the block (SEED; pixel, sample, (branch << 8) | (depth + 1)) has given 24 high bits: the
edge cases of tests/kats_scatter.py that need one particular rand01() - r1 with k = 0 and on both sides of every eighth of a
turn, r2 = 0 and r2 = 1 - 2^-24, a choice draw equal to P and its two neighbours (kats_scatter.DRAW_TARGETS).  A draw hits one
24-bit value once in 2^24 tries: vectorised Philox4x32-7 over samples 0 .. 2^24 - 1 of pixels 0, 1, 2, ..., in numpy, every
target of a tag in one sweep.
    python tools/find_scatter_draws.py         ->  the entries of DRAWS in tests/kats_scatter.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import kats_scatter as ks  # noqa: E402


def philox7(c0, c1, c2, seed):
    m = np.uint64(0xFFFFFFFF)
    c3 = np.zeros_like(c0)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(7):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0 = (k0 + np.uint64(0x9E3779B9)) & m
        k1 = (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1, c2, c3


def main():
    by_tag = {}
    for name, word, k, depth, branch in ks.DRAW_TARGETS:
        by_tag.setdefault((branch << 8) | (depth + 1), []).append((name, word, k))
    found = {}
    step = 1 << 22
    for tag, targets in by_tag.items():
        left = dict((name, (word, k)) for name, word, k in targets)
        pixel = 0
        while left and pixel < 64:
            for base in range(0, 1 << 24, step):
                sample = np.arange(base, base + step, dtype=np.uint64)
                w = philox7(np.full_like(sample, pixel), sample, np.full_like(sample, tag), ks.SEED)
                for word in (1, 2):
                    ks_left = [(name, k) for name, (wd, k) in left.items() if wd == word]
                    if not ks_left:
                        continue
                    bits = w[word] >> np.uint64(8)
                    hit = np.nonzero(np.isin(bits, np.array([k for _, k in ks_left], dtype=np.uint64)))[0]
                    for i in hit:
                        for name, k in ks_left:
                            if name in left and int(bits[i]) == k:
                                found[name] = (pixel, int(sample[i]))
                                del left[name]
            pixel += 1
        assert not left, left
    for name, _, _, _, _ in ks.DRAW_TARGETS:
        print('    "%s": (%d, %d),' % (name, *found[name]))


if __name__ == "__main__":
    main()
