"""ptrace --orbit N --move I:DX,DY,DZ: the drag loop from the command line, the object moved with pt_ctx_set_object.  A frame in
which the object moved passes no history on, so frame 2 of a run whose camera stands still (--orbit-step 0) is, byte for byte,
the one frame of a plain run on the scene SAVED with the object at frame 2's position."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptlib

pytestmark = pytest.mark.gpu

H, SPP, SEED, FRAMES = 32, 2, 5, 3
CLI = os.path.join(ptlib.PKG, "ptrace")
F32 = np.float32
MOVE = (0.1, 1.0 / 3.0, 0.07)  # (up from the floor: the sphere stays inside the room, the scene's reach)


def run(args, cwd):
    return subprocess.run([CLI, str(SPP), str(H)] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120)


def test_move_frames_equal_a_render_of_the_saved_scene(tmp_path):
    L = ptlib.product()
    root = tmp_path / "root"
    os.makedirs(root / "scenes")
    # cornell.json, and beside it the same scene with its first sphere where frame 2 puts it: position + 2 * d in binary32
    h = C.c_void_p()
    assert L.pt_scene_load(ptlib.scene_path("cornell").encode(), ptlib.ROOT.encode(), C.byref(h)) == 0, L.pt_last_error()
    n = C.c_uint32()
    objs = L.pt_scene_objects(h, C.byref(n))
    index = [i for i in range(n.value) if objs[i].kind == ptlib.PT_SPHERE][0]
    assert L.pt_scene_save(h, str(root / "scenes" / "cornell.json").encode()) == 0, L.pt_last_error()
    d = [float(F32(x)) for x in MOVE]
    for a in range(3):
        objs[index].position[a] = float(F32(objs[index].position[a]) + F32(2.0) * F32(d[a]))
    assert L.pt_scene_save(h, str(root / "scenes" / "moved.json").encode()) == 0, L.pt_last_error()
    L.pt_scene_free(h)
    common = ["--root", str(root), "--seed", str(SEED), "--orbit-step", "0"]
    r = run(["cornell", "--orbit", str(FRAMES), "--preview", str(tmp_path / "drag.ppm"), "--move", "%d:%r,%r,%r" % (index, *d)] + common,
            tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("frame ")]
    assert len(lines) == FRAMES and all("pt_ctx_set_object" in l and "pt_ctx_set_camera" in l for l in lines), r.stderr
    assert all("(rebuilt)" not in l for l in lines), lines  # the sphere stays inside the room: nothing is rebuilt
    r = run(["moved", "--orbit", "1", "--preview", str(tmp_path / "plain.ppm")] + common, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    frames = [open(tmp_path / ("drag-%03d.ppm" % k), "rb").read() for k in range(FRAMES)]
    assert frames[2] == open(tmp_path / "plain-000.ppm", "rb").read()
    assert frames[0] != frames[1] != frames[2]


def test_move_refuses_what_it_cannot_do(tmp_path):
    pv = ["cornell", "--root", ptlib.ROOT, "--preview", str(tmp_path / "m.ppm")]
    for extra, word in ((["--move", "0:1,0,0"], "--move goes with --orbit"), (["--orbit", "2", "--move", "0:1,0"], "--move needs"),
                        (["--orbit", "2", "--move", "x:1,0,0"], "--move needs"), (["--orbit", "2", "--move", "0:1,nan,0"], "--move needs"),
                        (["--orbit", "2", "--move", "99:1,0,0"], "--move: object 99")):
        r = run(pv + extra, tmp_path)
        assert r.returncode == 1 and word in r.stderr, (extra, r.returncode, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".ppm")]
