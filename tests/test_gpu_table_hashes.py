"""The scene's fourteen device tables against a RECORDING: tests/golden/scene_table_hashes_parent.json holds
pt_ctx_table_hashes of the library built from the commit it names, taken at every state below.  The other tests compare a
context's tables with another context of the same build, which a table dropped or mis-sized on both sides would pass; here
every hash must equal the recorded one.

The states are the paths through which tables reach the device: pt_ctx_set_scene; an inexact move of a sphere inside the reach
(sph_pairs, flat_pairs and cand_pairs go up whole) and back; an exact move of a mesh with a BVH (refit by the kernels) and a
material edit of it; pt_ctx_reserve_camera_reach with a larger box and a pt_ctx_set_camera that leaves the reach (both rebuild).
Nothing is rendered.

The recorder is this file run as a script, so that the test and the recording walk the same states:
    python tests/test_gpu_table_hashes.py <libptrace_hip.so of the commit> <commit id> [<file to write instead>]"""
import ctypes as C
import json
import os
import sys

import pytest

import ptlib
import test_gpu_set_object as so
from gpudev import L  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_table_hashes_parent.json")
SCENES = ("cornell-sphere", "bvh19")
# the cornell sphere rests on the floor, which is a face of the scene's box: up and inwards stays in reach
SPHERE_MOVE = (0.1, 1.0 / 3.0, 0.07)
MESH_MOVE = (0.125, -0.5, 1.0)
# lens centres far outside the box pt_ctx_reserve_camera_reach left
FAR_CAMERA = {"cornell-sphere": ((0.0, 0.5, 40.0), (0.0, -0.0625, -1.0)), "bvh19": ((0.5, 7.0, -200.0), (0.0, -0.3125, 1.0))}


def states(L, sid):
    """-> [(state, {table: hash as 16 hex digits})] of one context walked through the states of scene `sid`"""
    sc, index = so.scene(L, sid)
    dev = so.Dev(L, sc)
    out = []
    snap = lambda state: out.append((state, {k: "%016x" % v for k, v in dev.hashes().items()}))
    try:
        snap("set_scene")
        if sid == "cornell-sphere":
            dev.set_object(index, so.edited(sc, index, move=SPHERE_MOVE).objs[index], expect=0)
            snap("sphere moved in reach")
            dev.set_object(index, sc.objs[index], expect=0)
            snap("sphere moved back")
        else:
            cur = so.edited(sc, index, move=MESH_MOVE)
            dev.set_object(index, cur.objs[index], expect=0)
            snap("mesh moved in reach")
            cur = so.edited(cur, index, color=(0.125, 0.5, 1.0), reflect_type=1)
            dev.set_object(index, cur.objs[index], expect=0)
            snap("mesh material")
        lo, hi = dev.reach()
        assert dev.reserve(lo - so.F32(1.0), hi + so.F32(1.0)) == 1
        snap("reach reserved")
        rebuilt = C.c_int(-7)
        cam = ptlib.make_camera(*FAR_CAMERA[sid])
        assert L.pt_ctx_set_camera(dev.ctx, C.byref(cam), C.byref(rebuilt)) == 0, L.pt_last_error()
        assert rebuilt.value == 1
        snap("camera out of reach")
    finally:
        dev.close()
    return out


@pytest.mark.parametrize("sid", SCENES)
def test_tables_are_the_recorded_ones(L, sid):
    want = json.load(open(GOLDEN))
    assert len(want["commit"]) == 40
    got = states(L, sid)
    assert [s for s, _ in got] == list(want["scenes"][sid])
    for state, tables in got:
        rec = want["scenes"][sid][state]
        assert sorted(rec) == sorted(so.TABLES) and sorted(tables) == sorted(so.TABLES)
        assert tables == rec, (sid, state, [k for k in so.TABLES if tables[k] != rec[k]])


if __name__ == "__main__":
    ptlib.PRODUCT_SO = os.path.abspath(sys.argv[1])
    lib = ptlib.product()
    rec = {"commit": sys.argv[2], "scenes": {sid: dict(states(lib, sid)) for sid in SCENES}}
    with open(sys.argv[3] if len(sys.argv) > 3 else GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("recorded %d states of %s" % (sum(len(v) for v in rec["scenes"].values()), sys.argv[1]))
