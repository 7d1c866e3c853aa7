#!/usr/bin/env python3
"""Writes tests/golden/denoise_{cornell,mesh}_96x64_4096.npz: the CPU oracle's frames (oracle/pt_oracle.c through
ptlib.oracle_render) at 4096 samples per pixel, seed 5 - the converged pictures tests/test_denoise_abi.py and
tools/denoise_cpu_study.py measure a denoised 16-sample frame against.  Deterministic: running it again gives the same
bytes.  About a minute per scene on 16 cores.

    python tools/make_denoise_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptlib  # noqa: E402

W, H, SPP, SEED = 96, 64, 4096, 5


def main():
    for sid in ("cornell", "mesh"):
        sc = ptlib.load_scene_py(ptlib.scene_path(sid))
        frame, _, secs = ptlib.oracle_render(sc, W, H, SPP, SEED)
        path = os.path.join(ROOT, "tests", "golden", "denoise_%s_%dx%d_%d.npz" % (sid, W, H, SPP))
        np.savez(path, frame=frame.astype(np.float32), width=W, height=H, spp=SPP, seed=SEED)
        print("%s: %.1f s, %d bytes" % (path, secs, os.path.getsize(path)))


if __name__ == "__main__":
    main()
