"""The oracle's paths with their keys (pto_dump_paths) for the frames the scatter tests walk, computed once per process: every
ray of every path, its (pixel, sample, depth, branch), its pto_intersect_batch hit, and its children - the dumped rays with the
same pixel and sample, depth + 1 and branch b (one child) or 2b and 2b + 1 (a split).  tests/test_oracle.py holds the oracle to
tests/kats_scatter.py on them, tests/test_gpu_scatter.py holds the device (pt_ctx_scatter) to the oracle.  A walk is of SEED
unless another is asked for (tests/frame_sums.py walks one frame at a seed above 2^32); W.seed says which."""
import ctypes as C
import functools

import numpy as np

import ptlib
from ptlib import PtScatterItem, PtScatterSurface

SEED = 11
FRAMES = [("cornell", 16, 12, 8), ("three-spheres", 16, 12, 8), ("mesh", 12, 8, 4)]
KINDS = ("diffuse_child", "mirror_child", "split_pair", "chosen_reflection", "chosen_transmission", "roulette_death",
         "roulette_survival", "stop_at_12", "miss")


class Walk:
    pass


def walk(sid, width, height, spp, seed=SEED):
    return walk_scene(_scene(sid), width, height, spp, seed)


@functools.lru_cache(maxsize=None)
def _scene(sid):
    return ptlib.load_scene_py(ptlib.scene_path(sid))


@functools.lru_cache(maxsize=None)
def walk_scene(sc, width, height, spp, seed=SEED):
    L = ptlib.oracle()
    cap = width * height * spp * 64  # a path holds at most 4 branches of 12 rays
    rays = np.zeros((cap, 6), np.float32)
    keys = np.zeros((cap, 4), np.uint32)
    cfg = ptlib.PtoConfig(width, height, spp, 0, seed)
    ps = sc.pto()
    n = L.pto_dump_paths(C.byref(ps), C.byref(cfg), 0, width * height, ptlib._np_f(rays), keys.ctypes.data_as(ptlib.u32p), cap)
    assert 0 < n < cap
    W = Walk()
    W.scene, W.n, W.width, W.height, W.spp, W.seed = sc, int(n), width, height, spp, seed
    W.o, W.d, W.keys = rays[:n, :3].copy(), rays[:n, 3:].copy(), keys[:n].copy()
    W.t, W.oid, W.tid, W.x, W.nrm = ptlib.oracle_intersect(sc, W.o, W.d)
    W.index = {tuple(int(v) for v in k): i for i, k in enumerate(W.keys)}
    assert len(W.index) == W.n, "a key names one ray"
    W.children = []
    for i, (p, s, dep, b) in enumerate(W.keys.tolist()):
        one = W.index.get((p, s, dep + 1, b))
        two = (W.index.get((p, s, dep + 1, 2 * b)), W.index.get((p, s, dep + 1, 2 * b + 1)))
        assert one is None or two == (None, None), "a ray continues or splits"
        assert (two[0] is None) == (two[1] is None), "a split has both rays"
        W.children.append([one] if one is not None else ([two[0], two[1]] if two[0] is not None else []))
    return W


def hit_id(W, i):
    """the device's hit id of ray i from the oracle's (object, triangle of the mesh): -1, the object, or n_objs + flattened triangle"""
    if W.oid[i] < 0:
        return -1
    o = W.scene.objs[int(W.oid[i])]
    return int(W.oid[i]) if o.kind == ptlib.PT_SPHERE else W.scene.n_objs + o.tri_offset + int(W.tid[i])


def kinds(W):
    """what the frame shows of each kind, from the oracle alone (the dump, its hits, the scene's materials)"""
    c = dict.fromkeys(KINDS, 0)
    for i in range(W.n):
        if W.oid[i] < 0:
            c["miss"] += 1
            assert not W.children[i]
            continue
        reflect = W.scene.objs[int(W.oid[i])].reflect_type
        new_depth = int(W.keys[i][2]) + 1
        kids = W.children[i]
        if new_depth == 12:
            c["stop_at_12"] += 1
            assert not kids
        elif new_depth > 5:
            c["roulette_survival" if kids else "roulette_death"] += 1
        if len(kids) == 2:
            c["split_pair"] += 1
        elif len(kids) == 1 and reflect == 0:
            c["diffuse_child"] += 1
        elif len(kids) == 1 and reflect == 1:
            c["mirror_child"] += 1
        elif len(kids) == 1 and new_depth > 2:  # the reflected ray leaves on the side of the normal the ray came from
            came, goes = float(np.dot(W.nrm[i], W.d[i])), float(np.dot(W.nrm[i], W.d[kids[0]]))
            c["chosen_reflection" if (came < 0) != (goes < 0) else "chosen_transmission"] += 1
    return c


# ---- pt_ctx_scatter at the ABI (include/ptrace.h): the structs, the binding, arrays from cases and walks -----------------------
GIVEN, BY_ID, BY_RANK, DEFER_REFRACT, REFRACT_ONLY, NOT_SHADED = ptlib.abi.PT_SCATTER_GIVEN, ptlib.abi.PT_SCATTER_BY_ID, ptlib.abi.PT_SCATTER_BY_RANK, ptlib.abi.PT_SCATTER_DEFER_REFRACT, ptlib.abi.PT_SCATTER_REFRACT_ONLY, ptlib.abi.PT_SCATTER_NOT_SHADED
f3 = C.c_float * 3


def _f3(v):
    return f3(*[float(x) for x in v])


def item(o, d, thr, pixel, sample, depth, branch):
    return PtScatterItem(_f3(o), _f3(d), _f3(thr), int(pixel), int(sample), int(depth), int(branch))


def case_arrays(cases, thrs=None):
    """items and surfaces of kats_scatter cases (thrs: one incoming throughput per case; default (1, 1, 1))"""
    items = (PtScatterItem * len(cases))(*[item(c["o"], c["d"], (1, 1, 1) if thrs is None else thrs[i], c["pixel"], c["sample"],
                                                c["depth"], c["branch"]) for i, c in enumerate(cases)])
    surfs = (PtScatterSurface * len(cases))(*[PtScatterSurface(_f3(c["x"]), _f3(c["n"]), _f3(c["color"]), _f3(c["emission"]),
                                                               int(c["reflect"])) for c in cases])
    return items, surfs


def bits(v):
    """the bytes of a float triple (a ctypes float[3] or a numpy float32[3])"""
    return np.asarray(list(v) if not isinstance(v, np.ndarray) else v, dtype=np.float32).tobytes()


def walk_items(W):
    """every dumped ray of a walk as an item with its key and an incoming throughput of (1, 1, 1)"""
    return (PtScatterItem * W.n)(*[item(W.o[i], W.d[i], (1, 1, 1), *W.keys[i]) for i in range(W.n)])
