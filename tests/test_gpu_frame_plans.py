"""How the library cuts a wavefront frame, against a RECORDING: tests/golden/frame_plan_frames_parent.json holds pt_stats.passes,
intersect_launches, samples and ray_bounces and the image hash of the frames below, rendered by the library built from the commit
the file names - the last one whose render_wavefront sized its passes itself (host::plan_frame does now, csrc/pt_host.h;
tests/test_frame_plan.py pins its arithmetic on the CPU).  Compared with ==.

The frames are the smallest that reach each branch of the sizing: the default plan (cornell 16x12 @8), the knobs by hand
(PT_STREAMS=4 PT_TAPER_CUT=4 PT_TAPER_PIECES=4: four streams, each cut into four pieces), walks and parking areas (mesh.json
16x12 @4), the memory budget with k_pass_cand's stacks (cornell 128x96 @64 under 8 MiB: plan_pass's retries down to one sample per
pass) and with the level-by-level form (PT_FLAG_SEPARATE_KERNELS: 352 B per primary ray), and an explicit rays_per_pass (cornell
48x32 @8, two samples per pass).

The recorder is this file run as a script, so that the test and the recording render the same frames:
    python tests/test_gpu_frame_plans.py <libptrace_hip.so of the commit> <commit id> [<file to write instead>]"""
import ctypes as C
import json
import os
import sys

import pytest

import gpudev
import ptlib
from gpudev import L  # noqa: F401  (fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_plan_frames_parent.json")
SEED = 4
SEPARATE_KERNELS = ptlib.abi.PT_FLAG_SEPARATE_KERNELS
BY_HAND = {"PT_STREAMS": "4", "PT_TAPER_CUT": "4", "PT_TAPER_PIECES": "4"}
# name: (scene, width, height, spp, tuning environment, memory budget, flags, rays_per_pass)
FRAMES = {
    "cornell-16x12@8": ("cornell", 16, 12, 8, {}, 0, 0, 0),
    "cornell-16x12@8-by-hand": ("cornell", 16, 12, 8, BY_HAND, 0, 0, 0),
    "mesh-16x12@4": ("mesh", 16, 12, 4, {}, 0, 0, 0),
    "cornell-128x96@64-8MiB": ("cornell", 128, 96, 64, {}, 8 << 20, 0, 0),
    "cornell-128x96@64-8MiB-separate": ("cornell", 128, 96, 64, {}, 8 << 20, SEPARATE_KERNELS, 0),
    "cornell-48x32@8-two-per-pass": ("cornell", 48, 32, 8, {}, 0, 0, 2 * 48 * 32),
}


def frame(L, name):
    """-> {passes, intersect_launches, samples, ray_bounces, image_hash} of one frame in a context of its own"""
    sid, w, h, spp, env, budget, flags, rpp = FRAMES[name]
    sc = ptlib.load_scene_py(ptlib.scene_path(sid))
    with gpudev.Device(L, sc, env=env) as dev:
        assert L.pt_ctx_set_memory_budget(dev.ctx, budget) == 0
        cfg = gpudev.config(w, h, spp, backend=ptlib.BACKEND_WAVEFRONT, seed=SEED, rays_per_pass=rpp, flags=flags)
        img, st = dev.render(cfg, dev.alloc(w * h * 12))
    return {"passes": st.passes, "intersect_launches": st.intersect_launches, "samples": st.samples, "ray_bounces": st.ray_bounces,
            "image_hash": "%016x" % L.pt_image_hash(ptlib._np_f(img), img.size)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_are_cut_as_recorded(L, name):
    want = json.load(open(GOLDEN))
    assert len(want["commit"]) == 40 and sorted(want["frames"]) == sorted(FRAMES)
    assert frame(L, name) == want["frames"][name], name


def test_the_recorded_frames_reach_their_branches():
    """from the recording alone: the budget cuts the 64 samples into 64 passes (k_pass_cand) and into ceil(64 / floor(8 MiB / 352 B
    / pixels)) (level by level, twelve launches a pass); the explicit size gives four passes; the others are one launch"""
    rec = json.load(open(GOLDEN))["frames"]
    assert (rec["cornell-128x96@64-8MiB"]["passes"], rec["cornell-128x96@64-8MiB"]["intersect_launches"]) == (64, 64)
    per_pass = (8 << 20) // 352 // (128 * 96)
    assert per_pass == 1 and rec["cornell-128x96@64-8MiB-separate"]["passes"] == 64
    assert rec["cornell-128x96@64-8MiB-separate"]["intersect_launches"] == 64 * 12
    assert rec["cornell-48x32@8-two-per-pass"]["passes"] == 4
    for name in ("cornell-16x12@8", "cornell-16x12@8-by-hand", "mesh-16x12@4"):
        assert rec[name]["passes"] == 1, name
    assert rec["cornell-16x12@8"] == rec["cornell-16x12@8-by-hand"]  # (streams and pieces batch the samples: same image, same rays)
    assert rec["cornell-128x96@64-8MiB"]["image_hash"] == rec["cornell-128x96@64-8MiB-separate"]["image_hash"]
    for name, (_, w, h, spp, *_rest) in FRAMES.items():
        assert rec[name]["samples"] == w * h * spp, name


if __name__ == "__main__":
    lib = ptlib.abi.declare(C.CDLL(os.path.abspath(sys.argv[1])), partial=True)  # an older commit lacks newer entry points
    rec = {"commit": sys.argv[2], "frames": {name: frame(lib, name) for name in FRAMES}}
    with open(sys.argv[3] if len(sys.argv) > 3 else GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("recorded %d frames of %s" % (len(rec["frames"]), sys.argv[1]))
