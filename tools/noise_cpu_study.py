#!/usr/bin/env python3
"""The CPU study behind the bounds of the noise estimate's behaviour tests (tests/test_gpu_noise.py).

For cornell and mesh at 96x64 and n = 16, 64, 256 samples per pixel, PAIRS pairs of oracle frames of n/2 samples each (seeds
11 + 2k and 12 + 2k) stand for the two halves: a, b = the two frames, m = clamp((a + b) / 2) = the frame of all n samples.
`estimate` is the mean of e(p) by the numpy restatement of the contract (tests/noise_ref.py, w = 1/2); `actual` is the same
expression with |m - truth| in the place of |a - b| * w, truth = the oracle's frame at 4096 samples, seed 5
(tests/golden/denoise_*_96x64_4096.npz).  No GPU is involved.

The bounds (`bounds` in the file; the tests read them from there) are the worst value over the pairs with the margin the
denoiser's tests use, 1.15:
  fall_256_over_16   mean e at 256 samples / mean e at 16 samples is at most (largest estimate at 256 / smallest at 16) * 1.15
  ratio_lo, ratio_hi estimate / actual at n samples lies in [smallest / 1.15, largest * 1.15]
  target             a mean_error target between the rows for 64 and 256 samples: the geometric mean of the smallest estimate
                     at 64 and the largest at 256 (refused if the two rows overlap)

    python tools/noise_cpu_study.py            # writes profiles/noise_cpu_study.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_ref  # noqa: E402
import ptlib  # noqa: E402

W, H, PAIRS, MARGIN = 96, 64, 8, 1.15
SPP = (16, 64, 256)
SCENES = ("cornell", "mesh")
f32 = np.float32


def row(sc, truth, n, k):
    a = ptlib.oracle_render(sc, W, H, n // 2, 11 + 2 * k)[0].T.astype(f32)
    b = ptlib.oracle_render(sc, W, H, n // 2, 12 + 2 * k)[0].T.astype(f32)
    m = noise_ref.clamp01(((a.astype(np.float64) + b.astype(np.float64)) * 0.5).astype(f32))
    est = noise_ref.error_from_means(a, b, m, f32(0.5))
    act = noise_ref.error_from_means(m, truth, m, f32(1.0))
    return float(est.astype(np.float64).mean()), float(act.astype(np.float64).mean())


def main():
    rows, bounds = {}, {}
    for sid in SCENES:
        sc = ptlib.load_scene_py(ptlib.scene_path(sid))
        gold = np.load(os.path.join(ROOT, "tests", "golden", "denoise_%s_%dx%d_4096.npz" % (sid, W, H)))
        assert int(gold["seed"]) == 5 and int(gold["spp"]) == 4096
        truth = gold["frame"].reshape(W * H, 3).T.astype(f32)
        rows[sid] = {}
        for n in SPP:
            pairs = [row(sc, truth, n, k) for k in range(PAIRS)]
            est, act = [p[0] for p in pairs], [p[1] for p in pairs]
            ratio = [e / a for e, a in pairs]
            rows[sid][str(n)] = {"estimate": est, "actual": act, "ratio": ratio}
            print("%-8s n %4d  estimate %.4f..%.4f  actual %.4f..%.4f  ratio %.3f..%.3f" %
                  (sid, n, min(est), max(est), min(act), max(act), min(ratio), max(ratio)), flush=True)
        r = rows[sid]
        lo64, hi256 = min(r["64"]["estimate"]), max(r["256"]["estimate"])
        assert hi256 < lo64, "the rows for 64 and 256 samples overlap"
        bounds[sid] = {
            "fall_256_over_16": max(r["256"]["estimate"]) / min(r["16"]["estimate"]) * MARGIN,
            "ratio_lo": {str(n): min(r[str(n)]["ratio"]) / MARGIN for n in SPP},
            "ratio_hi": {str(n): max(r[str(n)]["ratio"]) * MARGIN for n in SPP},
            "target": float(np.sqrt(lo64 * hi256)),
        }
    doc = {
        "command": "python tools/noise_cpu_study.py",
        "what": "mean e(p) of two oracle half frames (estimate) against the same expression with |m - truth| (actual); 96x64, "
                "%d seed pairs per row (11 + 2k, 12 + 2k), truth = oracle at 4096 spp seed 5, e(p) = tests/noise_ref.py" % PAIRS,
        "margin": MARGIN,
        "rows": rows,
        "bounds": bounds,
    }
    path = os.path.join(ROOT, "profiles", "noise_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("bounds:", json.dumps(bounds), "->", path)


if __name__ == "__main__":
    main()
