#!/usr/bin/env python3
"""What a camera move costs a viewport: pt_ctx_set_scene per frame (the only way before pt_ctx_set_camera) against
pt_ctx_set_camera per frame, in one process: for DESIGN.md section 4.

Per call.  On cornell, mesh.json and mesh.json with its mesh replaced by a generated grid of 20 000 triangles ("mesh-20k"; with
--big also one of 640 000, measured once): pt_ctx_set_scene, and pt_ctx_set_camera on the fast path, alternating between two
cameras 2 degrees apart so that no call is a no-op; after a warm-up, the median of 7 (a pt_ctx_set_camera sample is the mean of
200 calls: one call is below the clock's step).  And one pt_ctx_set_camera on the slow path (a turn of 90 degrees on a fresh
context), a single call.

Per frame.  The "half" chain of tools/upsample_timing.py at 1024x768 and 8 samples on mesh.json and mesh-20k - pt_ctx_render and
pt_ctx_render_aov at half size, pt_ctx_render_aov at full size, pt_ctx_upsample - with the camera update INSIDE the timed
region: pt_ctx_set_scene per frame, then pt_ctx_set_camera per frame, wall time, the median of 7 frames after a warm-up.

    python tools/set_camera_timing.py [--big] [out.json]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpudev  # noqa: E402
import ptlib  # noqa: E402
import reproject_ref  # noqa: E402
import timing  # noqa: E402
from ptlib import PtConfig, PtObject, PtStats, PtTriangle  # noqa: E402

N = 7
BATCH = 200
W, H, SPP = 1024, 768, 8


class Generated:
    """mesh.json's room around a generated mesh: its largest mesh replaced by a rippled grid of 2 * side^2 triangles"""

    def __init__(self, L, base, side):
        big = max((i for i in range(base.n_objs) if base.objs[i].kind == ptlib.PT_MESH), key=lambda i: base.objs[i].tri_count)
        o = base.objs[big]
        R = np.float32(o.bs_radius * 0.5)
        g = np.arange(side + 1, dtype=np.float32) / np.float32(side) - np.float32(0.5)
        x, z = np.meshgrid(g * 2 * R, g * 2 * R, indexing="ij")
        y = np.float32(0.1) * R * np.sin(9 * x / R) * np.cos(7 * z / R)
        v = np.stack([x + o.bs_center[0], y + o.bs_center[1], z + o.bs_center[2]], axis=-1).astype(np.float32)
        a, b, c, d = v[:-1, :-1], v[1:, :-1], v[1:, 1:], v[:-1, 1:]
        grid = np.stack([np.stack([a, b, c], axis=2), np.stack([a, c, d], axis=2)], axis=2).reshape(-1, 9)
        parts, objs = [grid], []
        n = len(grid)
        for i in range(base.n_objs):
            q = PtObject.from_buffer_copy(base.objs[i])
            if q.kind == ptlib.PT_MESH and i != big:
                t = np.frombuffer(base.tris, dtype=np.float32).reshape(-1, 9)[q.tri_offset:q.tri_offset + q.tri_count]
                parts.append(t)
                q.tri_offset = n
                n += len(t)
            objs.append(q)
        self.host = np.ascontiguousarray(np.vstack(parts), dtype=np.float32)
        self.n_tris = len(self.host)
        self.tris = C.cast(self.host.ctypes.data_as(C.c_void_p), C.POINTER(PtTriangle))
        objs[big].tri_offset, objs[big].tri_count = 0, len(grid)
        ctr, rad = (C.c_float * 3)(), C.c_float()
        assert L.pt_mesh_bounding_sphere(self.tris, len(grid), ctr, C.byref(rad)) == 0
        objs[big].bs_center, objs[big].bs_radius = ctr, rad.value
        self.n_objs = len(objs)
        self.objs = (PtObject * self.n_objs)(*objs)
        self.cam = base.cam
        self.id = "mesh-%dk" % (len(grid) // 1000)


def orbit(cam, deg):
    d = reproject_ref.orbit({"position": tuple(cam.position), "direction": tuple(cam.direction), "focal_length": cam.focal_length,
                             "sensor_width": cam.sensor_width, "aspect_ratio": cam.aspect_ratio}, deg)
    return ptlib.make_camera(d["position"], d["direction"], d["focal_length"], d["sensor_width"], d["aspect_ratio"])


def main():
    L = ptlib.product()
    timing.need_gpu(L, "set_camera_timing")
    mesh = ptlib.load_scene_py(ptlib.scene_path("mesh"))
    scenes = [ptlib.load_scene_py(ptlib.scene_path("cornell")), mesh, Generated(L, mesh, 100)]
    if "--big" in sys.argv[1:]:
        scenes.append(Generated(L, mesh, 566))
    doc = {"command": "python tools/set_camera_timing.py" + (" --big" if "--big" in sys.argv[1:] else ""),
           "isa_hash": L.pt_kernel_isa_hash().decode(),
           "method": "one process; per call: after a warm-up the median of %d, alternating between two cameras 2 degrees apart (a "
                     "pt_ctx_set_camera sample: the mean of %d calls); per frame: wall time of the half-resolution chain of "
                     "tools/upsample_timing.py at %dx%d @ %d spp with the camera update inside, the median of %d frames" % (N, BATCH, W, H, SPP, N),
           "per_call": {}, "per_frame": {}}

    def set_camera(ctx, cam):
        rebuilt = C.c_int()
        assert L.pt_ctx_set_camera(ctx, C.byref(cam), C.byref(rebuilt)) == 0, L.pt_last_error()
        return rebuilt.value

    for sc in scenes:
        once = sc.n_tris > 100000  # the largest scene: seconds per rebuild, measured once
        cams = (sc.cam, orbit(sc.cam, 2.0))
        with gpudev.Device(L, sc, cams[0]) as d:  # warm-up: allocations
            ctx = d.ctx
            ms = []
            for k in range(1 if once else N):
                t0 = time.perf_counter()
                d.set_scene(sc, cams[(k + 1) & 1])
                ms.append((time.perf_counter() - t0) * 1e3)
            res = {"triangles": sc.n_tris, "set_scene": timing.stats(ms)}
            d.set_scene(sc, cams[0])
            assert set_camera(ctx, cams[1]) == 0 and set_camera(ctx, cams[0]) == 0, "2 degrees must stay on the fast path"
            ms = []
            for _ in range(N):
                t0 = time.perf_counter()
                for k in range(BATCH):
                    set_camera(ctx, cams[(k + 1) & 1])
                ms.append((time.perf_counter() - t0) * 1e3 / BATCH)
            res["set_camera_fast"] = timing.stats(ms)
            res["set_scene_over_set_camera_fast"] = res["set_scene"]["ms_median"] / res["set_camera_fast"]["ms_median"]
            t0 = time.perf_counter()
            rebuilt = set_camera(ctx, orbit(sc.cam, 90.0))
            res["set_camera_slow_once"] = {"ms": (time.perf_counter() - t0) * 1e3, "rebuilt": rebuilt}
            doc["per_call"][sc.id] = res
            timing.report(sc.id, res)

    # ---- the loop: wall time per frame, the camera update inside
    w, h = W // 2, H // 2
    n, nl = W * H, w * h
    for sc in scenes[1:3]:
        cams = (sc.cam, orbit(sc.cam, 2.0))
        with gpudev.Device(L, sc, cams[0]) as d:
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
            for name, update in (("set_scene_per_frame", lambda cam: d.set_scene(sc, cam)),
                                 ("set_camera_per_frame", lambda cam: set_camera(ctx, cam)), ("no_update", lambda cam: None)):
                update(cams[0])
                chain()  # warm-up: scratch, code objects, the scene's pass rate
                total, upd = [], []
                for k in range(N):
                    t0 = time.perf_counter()
                    update(cams[(k + 1) & 1])
                    t1 = time.perf_counter()
                    chain()
                    t2 = time.perf_counter()
                    total.append((t2 - t0) * 1e3)
                    upd.append((t1 - t0) * 1e3)
                res[name] = {"frame": timing.stats(total), "update": timing.stats(upd)}
            res["set_camera_over_set_scene"] = res["set_camera_per_frame"]["frame"]["ms_median"] / res["set_scene_per_frame"]["frame"]["ms_median"]
            doc["per_frame"]["%s %dx%d @ %d spp" % (sc.id, W, H, SPP)] = res
            timing.report(sc.id, res)
    timing.write(doc, "set_camera_timing.json")


if __name__ == "__main__":
    main()
