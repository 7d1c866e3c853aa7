#!/usr/bin/env python3
"""What an object edit costs a viewport: pt_ctx_set_scene of the edited scene (the only way before pt_ctx_set_object) against
pt_ctx_set_object, in one process: for DESIGN.md section 4 and the README.

Per call.  On mesh.json and mesh.json with its mesh replaced by a generated grid of 20 000 triangles ("mesh-20k"; with --big also
one of 640 000): pt_ctx_set_scene of the scene with the mesh moved (what a host pays today: the number to beat); the FIRST MOVE
edit of the mesh on a fresh context (the refit plan is built and uploaded with the object-local triangles); a LATER MOVE edit
(the refit alone); a MATERIAL edit of the mesh; and on cornell.json (mesh.json has no sphere) a MOVE of a sphere.  Every edit
alternates between two values, so that no call is a no-op, and stays inside the scene's reach (asserted: rebuilt == 0).  After a
warm-up call, the median of 7 single calls (tools/timing.py's wall) - each ends in the call's own device synchronise - but for
the 640 000-triangle pt_ctx_set_scene, measured once.

Per frame.  The "half" chain of tools/upsample_timing.py at 1024x768 and 8 samples - pt_ctx_render and pt_ctx_render_aov at half
size, pt_ctx_render_aov at full size, pt_ctx_upsample - with the edit INSIDE the timed region, both ways: pt_ctx_set_scene per
frame, then pt_ctx_set_object per frame; wall time, the median of 7 frames after a warm-up.

    python tools/set_object_timing.py [--big] [out.json]
"""
import ctypes as C
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import timing  # noqa: E402
from ptlib import PtConfig, PtObject, PtStats  # noqa: E402
from set_camera_timing import Generated  # noqa: E402

N = 7
W, H, SPP = 1024, 768, 8
F32 = np.float32


def alternating(call, first, second):
    """call(first), call(second), call(first), ... one per call of the result"""
    values = itertools.cycle((first, second))
    return lambda: call(next(values))


def main():
    big = "--big" in sys.argv[1:]
    L = ptlib.product()
    timing.need_gpu(L, "set_object_timing")
    mesh = ptlib.load_scene_py(ptlib.scene_path("mesh"))
    scenes = [mesh, Generated(L, mesh, 100)] + ([Generated(L, mesh, 566)] if big else [])
    doc = {"command": "python tools/set_object_timing.py" + (" --big" if big else ""), "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "one process; per call: after a warm-up the median of %d single calls, each alternating between two values of the "
                     "object and ending in its own device synchronise (pt_ctx_set_scene of the 640 000-triangle scene: once); per "
                     "frame: wall time of the half-resolution chain of tools/upsample_timing.py at %dx%d @ %d spp with the edit "
                     "inside, the median of %d frames" % (N, W, H, SPP, N),
           "per_call": {}, "per_frame": {}}

    def variants(sc, index, **how):
        """two copies of object `index`: as the scene has it, and moved / recoloured"""
        a, b = PtObject.from_buffer_copy(sc.objs[index]), PtObject.from_buffer_copy(sc.objs[index])
        if "move" in how:
            b.position = ptlib.f3(*[float(F32(p) + F32(d)) for p, d in zip(a.position, how["move"])])
        if "color" in how:
            b.color = ptlib.f3(*how["color"])
        return a, b

    def with_object(sc, index, obj):
        objs = (PtObject * sc.n_objs)(*[obj if i == index else sc.objs[i] for i in range(sc.n_objs)])
        return objs

    def set_scene(ctx, sc, objs):
        assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), objs, sc.n_objs, sc.tris, sc.n_tris) == 0, L.pt_last_error()

    def set_object(ctx, index, obj):
        rebuilt = C.c_int(-1)
        assert L.pt_ctx_set_object(ctx, index, C.byref(obj), C.byref(rebuilt)) == 0, L.pt_last_error()
        assert rebuilt.value == 0, "the edits of this tool stay inside the scene's reach"

    def edited_scene(sc, index, here, there, frames):
        """pt_ctx_set_scene of the scene with the object there, here, ... on a fresh context; the warm-up call (here) allocates"""
        with gpudev.Device(L) as d:
            return timing.wall(alternating(lambda objs: set_scene(d.ctx, sc, objs), with_object(sc, index, here), with_object(sc, index, there)),
                               frames)

    def the_mesh(sc):
        return max((i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_MESH), key=lambda i: sc.objs[i].tri_count)

    for sc in scenes:
        once = sc.n_tris > 100000
        index = the_mesh(sc)
        here, there = variants(sc, index, move=(0.05, 0.02, -0.03))
        res = {"triangles": sc.n_tris, "mesh_triangles": sc.objs[index].tri_count}
        res["set_scene_of_the_edited_scene"] = edited_scene(sc, index, here, there, 1 if once else N)
        with gpudev.Device(L, sc) as d:

            def edit(obj):
                set_object(d.ctx, index, obj)

            t0 = time.perf_counter()
            edit(there)
            res["first_move_edit_once"] = {"ms": (time.perf_counter() - t0) * 1e3}
            # the warm-up of the later edits moves it back: the kernels' code objects are loaded by now
            res["later_move_edit"] = timing.wall(alternating(edit, here, there), N)
            plain, tinted = variants(sc, index, color=(0.25, 0.875, 0.5))
            res["material_edit"] = timing.wall(alternating(edit, tinted, plain), N)
            res["set_scene_over_later_move_edit"] = res["set_scene_of_the_edited_scene"]["ms_median"] / res["later_move_edit"]["ms_median"]
            doc["per_call"][sc.id] = res
            timing.report(sc.id, res)

    # a sphere: mesh.json has none, so cornell.json's first one that is not the light
    sc = ptlib.load_scene_py(ptlib.scene_path("cornell"))
    index = [i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_SPHERE and not any(sc.objs[i].emission)][0]
    here, there = variants(sc, index, move=(0.01, 0.0, -0.01))
    res = {"triangles": sc.n_tris, "set_scene_of_the_edited_scene": edited_scene(sc, index, here, there, N)}
    with gpudev.Device(L, sc) as d:
        res["sphere_move_edit"] = timing.wall(alternating(lambda obj: set_object(d.ctx, index, obj), there, here), N)
    doc["per_call"][sc.id] = res
    timing.report(sc.id, res)

    # ---- the loop: wall time per frame, the edit inside
    w, h = W // 2, H // 2
    n, nl = W * H, w * h
    for sc in scenes:
        once = sc.n_tris > 100000
        index = the_mesh(sc)
        here, there = variants(sc, index, move=(0.05, 0.02, -0.03))
        scene_objs = (with_object(sc, index, here), with_object(sc, index, there))
        with gpudev.Device(L, sc) as d:
            ctx = d.ctx
            F = {k: d.alloc(n * b) for k, b in (("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4), ("out", 12))}
            Lo = {k: d.alloc(nl * b) for k, b in (("color", 12), ("albedo", 12), ("normal", 12), ("depth", 4), ("oid", 4))}
            st = PtStats()
            seed = [100]

            def chain():
                seed[0] += 1
                lo, full = PtConfig(w, h, SPP, 0, seed[0], 0, 0, 0, 0), PtConfig(W, H, SPP, 0, seed[0], 0, 0, 0, 0)
                assert L.pt_ctx_render(ctx, C.byref(lo), Lo["color"], None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
                assert L.pt_ctx_render_aov(ctx, C.byref(lo), Lo["albedo"], Lo["normal"], Lo["depth"], Lo["oid"], None) == 0, L.pt_last_error()
                assert L.pt_ctx_render_aov(ctx, C.byref(full), F["albedo"], F["normal"], F["depth"], F["oid"], None) == 0, L.pt_last_error()
                rc = L.pt_ctx_upsample(ctx, W, H, w, h, None, Lo["color"], Lo["depth"], Lo["oid"], Lo["normal"], Lo["albedo"], F["depth"],
                                       F["oid"], F["normal"], F["albedo"], F["out"], None, None)
                assert rc == 0, L.pt_last_error()

            res = {"triangles": sc.n_tris}
            for name, update, frames in (("set_scene_per_frame", lambda k: set_scene(ctx, sc, scene_objs[k & 1]), 2 if once else N),
                                         ("set_object_per_frame", lambda k: set_object(ctx, index, (here, there)[k & 1]), N),
                                         ("no_edit", lambda k: None, N)):
                update(0)
                update(1)
                chain()  # warm-up: scratch, code objects, the refit plan, the scene's pass rate
                total, upd = [], []
                for k in range(frames):
                    t0 = time.perf_counter()
                    update(k)
                    t1 = time.perf_counter()
                    chain()
                    t2 = time.perf_counter()
                    total.append((t2 - t0) * 1e3)
                    upd.append((t1 - t0) * 1e3)
                res[name] = {"frame": timing.stats(total), "edit": timing.stats(upd), "frames": frames}
            res["set_object_over_set_scene"] = res["set_object_per_frame"]["frame"]["ms_median"] / res["set_scene_per_frame"]["frame"]["ms_median"]
            doc["per_frame"]["%s %dx%d @ %d spp" % (sc.id, W, H, SPP)] = res
            timing.report(sc.id, res)
    k20 = doc["per_call"]["mesh-20k"]
    doc["condition"] = {"text": "a later MOVE edit of the 20 000-triangle mesh costs less than pt_ctx_set_scene of that scene, same run",
                        "later_move_edit_ms": k20["later_move_edit"]["ms_median"], "set_scene_ms": k20["set_scene_of_the_edited_scene"]["ms_median"],
                        "verdict": "HIT" if k20["later_move_edit"]["ms_median"] < k20["set_scene_of_the_edited_scene"]["ms_median"] else "MISSES"}
    timing.report("condition:", doc["condition"])
    timing.write(doc, "set_object_timing.json")


if __name__ == "__main__":
    main()
