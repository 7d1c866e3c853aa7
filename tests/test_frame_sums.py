"""tests/frame_sums.py on the CPU: the restated pixel sums against the reference's own order of summation (the oracle's frame),
the conditions on the walked frames that keep tests/test_gpu_frame_sums.py from passing vacuously, to_fixed's known answers, and
proof that the probe table and the walks tell the wrong variants of the arithmetic from the real one."""
import numpy as np
import pytest

import frame_sums as fs
import ptlib

f32 = np.float32
TOL = 1e-4  # the project's frame tolerance (tests/test_gpu_parity.py)


def _totals(frame):
    W, sums = fs.frame(*frame)
    return W, sums, fs.total_over(sums, range(W.spp))


@pytest.mark.parametrize("frame", fs.WALKS, ids=fs.WALK_IDS)
def test_restated_sums_resolve_to_the_oracles_frame(frame):
    """The chain sums top-down in 32.32 fixed point, the oracle bottom-up in binary32 as the reference does: resolved and
    clamped, the two agree within the project's frame tolerance (measured: 1.2e-7 or less)."""
    W, sums, total = _totals(frame)
    want, cnt, _ = ptlib.oracle_render(W.scene, W.width, W.height, W.spp, W.seed)
    assert cnt.ray_bounces == W.n
    got = fs.resolved(total, W.spp, clamp=True)
    worst = float(np.abs(got - want).max())
    print("%s: %d rays, max |restated - oracle| = %.3g" % (frame[0], W.n, worst))
    assert worst <= TOL, (frame, worst)


def test_the_walked_frames_are_not_vacuous():
    """From the oracle's paths alone: pixels the clamp hides, black pixels, contributions small enough that truncating the low
    word differs from rounding it, and a contribution that arrives through a split child (branch 2 or higher)."""
    by_id = dict(zip([f[0] for f in fs.WALKS[:3]], fs.WALKS[:3]))
    W, sums, total = _totals(by_id["cornell"])
    mean = fs.resolved(total, W.spp, clamp=False)
    above, black = int((mean > 1).any(axis=1).sum()), sum(1 for px in total if px == [0, 0, 0])
    print("cornell: %d pixels above 1, %d black" % (above, black))
    assert above >= 40 and black >= 1
    contribs = fs.contributions(W)
    positive = [float(v) for _, _, _, c in contribs for v in c if v > 0]
    print("cornell: smallest contribution %.3g, largest %.17g" % (min(positive), max(positive)))
    assert min(positive) < 2.0 ** -8
    assert max(positive) <= float(f32(2.8125155)), "the probe table's 2.8125155f is the largest contribution cornell makes"
    assert any(W.keys[i][3] >= 2 and any(v > 0 for v in c) for i, _, _, c in contribs), "no contribution from a split child"
    W, sums, total = _totals(by_id["three-spheres"])
    mean = fs.resolved(total, W.spp, clamp=False)
    above, black = int((mean > 1).any(axis=1).sum()), sum(1 for px in total if px == [0, 0, 0])
    print("three-spheres: %d pixels above 1, %d black" % (above, black))
    assert black >= 150 and above >= 1
    # the extra walk's seed does not fit 32 bits: the frame kernels see a non-zero high key word
    assert fs.WALKS[3][4] >> 32 != 0 and all(f[4] >> 32 == 0 for f in fs.WALKS[:3])


TO_FIXED_KATS = [
    (2.0 ** -33, 0), (2.0 ** -32, 1), (1.5 * 2.0 ** -32, 1), (f32(0.1), 0x199999a0), (1.0 - 2.0 ** -24, 0xffffff00), (1.0, 1 << 32),
    (1.0 + 2.0 ** -23, 0x100000200), (12.0, 12 << 32), (2097151.875, 0x1fffffe0000000), (2.0 ** 31, 1 << 63),
    (4294967040.0, 0xffffff0000000000), (2.0 ** 32, 0xffffff0000000000), (3e38, 0xffffff0000000000),
    (float("inf"), 0xffffff0000000000), (0.0, 0), (-0.0, 0),
]


@pytest.mark.parametrize("v,want", TO_FIXED_KATS, ids=[repr(float(v)) for v, _ in TO_FIXED_KATS])
def test_to_fixed_known_answers(v, want):
    """hand-derived: 0.1f = 0x3dcccccd = 13421773 * 2^-27, times 2^32 = 13421773 * 32 = 0x199999a0; 1 - 2^-24 = (2^24 - 1) *
    2^-24, times 2^32 = 0xffffff00; 1 + 2^-23 -> hi 1, lo 2^9; 2097151.875 = 2^21 - 2^-3 -> hi 0x1fffff, lo 0xe0000000"""
    assert fs.to_fixed(v) == want, (v, hex(fs.to_fixed(v)), hex(want))


def test_the_vectorised_to_fixed_of_the_aov_test_is_this_one():
    """tests/test_gpu_aov.py keeps its numpy form; on the values its rebuild feeds it - colours and normal components in [0, 1]
    - and on the known answers, the two agree"""
    import test_gpu_aov
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.random(4096, dtype=f32), np.array([v for v, _ in TO_FIXED_KATS if np.isfinite(v)], f32),
                           np.array([0.75, 0.25, 0.999, 0.7, 1.0, 0.0], f32)])
    got = test_gpu_aov.to_fixed(vals)
    assert got.dtype == np.uint64 and [int(v) for v in got] == [fs.to_fixed(v) for v in vals]


def test_the_probe_table_tells_the_wrong_variants_apart():
    """On the cases tests/test_gpu_frame_sums.py runs (every emission x sample count whose sum fits), each wrong variant of
    k_resolve or to_fixed changes at least one expected value - on the full table and on the subset the other forms run."""
    for counts in (fs.SAMPLE_COUNTS, fs.SUBSET_COUNTS):
        cases = [(e, n) for n in counts for e in fs.EMISSIONS if fs.fits(e, n)]
        assert len({e for e, _ in cases}) == len(fs.EMISSIONS) and len({n for _, n in cases}) == len(counts)
        real = [fs.resolve(n * fs.to_fixed(e), n, clamp=False) for e, n in cases]
        told = {
            "divide in double": [(e, n) for (e, n), r in zip(cases, real) if fs.resolve_double_divide(n * fs.to_fixed(e), n) != r],
            "multiply by fl(1/n)": [(e, n) for (e, n), r in zip(cases, real) if fs.resolve_reciprocal(n * fs.to_fixed(e), n) != r],
            "round lo": [(e, n) for (e, n), r in zip(cases, real) if fs.resolve(n * fs.to_fixed(e, round_lo=True), n, False) != r],
        }
        print("%d cases of %d counts: %s" % (len(cases), len(counts), {k: len(v) for k, v in told.items()}))
        for name, where in told.items():
            assert where, (name, counts)
        assert (f32(1.5 * 2.0 ** -32), 1) in told["round lo"]
    # the walked frames cannot tell the two wrong divisions apart: their sample counts are powers of two
    assert all(f[3] & (f[3] - 1) == 0 for f in fs.WALKS)
    # every triple of the table holds three different values, and every case appears in each channel
    for n, triple in fs.table_cases():
        assert len({float(v) for v in triple}) == 3 and all(fs.fits(e, n) for e in triple)
    want = sorted((n, float(e)) for n in fs.SAMPLE_COUNTS for e in fs.EMISSIONS if fs.fits(e, n))
    for c in range(3):
        assert sorted((n, float(t[c])) for n, t in fs.table_cases()) == want, c


def test_cornell_tells_a_wrong_throughput_order_and_a_rounded_low_word():
    """fl(thr * fl(colour' * factor)) in place of fl(fl(thr * colour') * factor), and a low word rounded instead of truncated,
    each change at least one pixel sum of cornell's walk: the GPU comparison on that frame would catch either."""
    W, sums, total = _totals(fs.WALKS[0])
    assert fs.WALKS[0][0] == "cornell"
    for name, kw in (("throughput order", dict(wrong_order=True)), ("rounded low word", dict(round_lo=True))):
        wrong = fs.total_over(fs.walk_sums(W, **kw), range(W.spp))
        differ = sum(1 for a, b in zip(total, wrong) for x, y in zip(a, b) if x != y)
        print("%s: %d of %d pixel sums differ" % (name, differ, 3 * len(total)))
        assert differ >= 1, name
