"""Every LDS layout of the kernels that stage scene records, on both sides of its cliff (tests/lds_layouts.py), against the oracle.
-m gpu.

Frames of every ladder scene through the device paths that can reach its layouts - the default wavefront, the separate kernels,
the megakernel, and PT_CAND_SCAN=0 / PT_CAND_BVH=0 / PT_GLASS_DEFER=1 / PT_NODES_LDS=0 where they apply: the oracle's bounce
count exactly, its image within TOL, and every path the same image bit for bit.  Then probe rays through pt_ctx_radiance at the
primitives whose records sit at the edges of the staged regions (the last staged shading rank, the first one outside, the highest
rank, the first and last candidate records), each starting just off its target so that the oracle's first hit is that very sphere
or triangle (checked): with the scene black and a distinct emission per object the radiance is the emission of the object the
kernel found, bit for bit the oracle's, after one bounce; with the colours kept, the path after it depends on the triangle's own
normal.  A frame alone can miss a wrong record whose object few pixels see.

Every context runs with PT_LDS_PAD=0, under which the library says on stderr the layout each launcher of the context runs with
whenever it changes; the test reads those lines and checks that each case ran the layout the CPU ladder expects for it."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import boundary_rays as br
import gpudev
import lds_layouts as ll
import ptlib
from ptlib import PtStats, _np_f

pytestmark = pytest.mark.gpu

SEED = 20261016
TOL = 1e-4
FLAG_SEPARATE_KERNELS = ptlib.abi.PT_FLAG_SEPARATE_KERNELS
M_STREAMS = 4  # the stream-length rungs: PT_STREAMS=4 and a frame of m x 4 pixels
LINE = re.compile(r"^(k_\S+): \d+ bytes of LDS per workgroup \(\+ \d+ of padding\)")
WHICH = {"k_pass_cand": 0, "k_pass_cand<BVH>": 0, "k_pass": 0, "k_intersect_cand": 1, "k_mega_cand": 2, "k_mega": 2}


@pytest.fixture(scope="module")
def ladder():
    return ll.build(SEED)


class _Said:
    """The layout lines each context has said so far (a context says one only when it differs from the last it said for that
    launcher), read after every call on that context."""

    def __init__(self, capfd):
        self.capfd, self.last = capfd, {}

    def now(self, key):
        last = self.last.setdefault(key, [None, None, None])
        for line in self.capfd.readouterr().err.splitlines():
            mt = LINE.match(line)
            if mt:
                last[WHICH[mt.group(1)]] = line
        return list(last)


def _forms(rung):
    """(name, tuning environment, backend, flags, which launcher's line must equal the rung's, or None)."""
    env = rung.env
    if rung.cliff.endswith("_m"):
        env = dict(env, PT_STREAMS=str(M_STREAMS))
    bvh = rung.L["n_bvh_nodes"] != 0
    cand = rung.L["cand_scan"] == 1
    out = [("wavefront", env, 0, 0, 0 if (cand or not bvh) else None),
           ("separate", env, 0, FLAG_SEPARATE_KERNELS, 1 if (cand and not bvh) else None),
           ("mega", env, 1, 0, 2)]
    if rung.sw == 0:
        out.append(("cand_scan0", dict(env, PT_CAND_SCAN="0"), 0, 0, None))
        if bvh:
            out.append(("cand_bvh0", dict(env, PT_CAND_BVH="0"), 0, 0, None))
            out.append(("nodes_lds0", dict(env, PT_NODES_LDS="0"), 0, 0, None))
        if any(rung.scene.objs[i].reflect_type == ptlib.REFLECT["Refract"] for i in range(rung.scene.n_objs)):
            out.append(("glass_defer", dict(env, PT_GLASS_DEFER="1"), 0, 0, None))
    return out


def _frame(rung):
    if rung.cliff.endswith("_m"):
        return rung.m, M_STREAMS, 2
    return 24, 16, 2


def test_ladder_frames_and_table_edge_rays(ladder, capfd):
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "no HIP device visible: the product has no CPU fallback"
    said = _Said(capfd)
    ctxs = {}
    ran = []  # (rung, form, launcher, the line said for it)
    t_start = time.perf_counter()
    n_frames = n_rays = 0

    def ctx_for(env):
        key = tuple(sorted(env.items()))
        if key not in ctxs:
            said.now(None)  # (whatever was said before belongs to no context of this test)
            ctxs[key] = gpudev.Device(L, env=dict(env, PT_LDS_PAD="0"))
        return key, ctxs[key]

    try:
        for k, (name, a, b) in enumerate(ladder):
            for rung in (a, b):
                sc = br.first_hit_variant(rung.scene, keep_color=True)
                w, h, spp = _frame(rung)
                seed = 100 + k
                want, cnt, _ = ptlib.oracle_render(sc, w, h, spp, seed)
                ref = None
                for form, env, backend, flags, which in _forms(rung):
                    key, dev = ctx_for(env)
                    dev.set_scene(sc)
                    out = dev.alloc(w * h * 12)
                    img, st = dev.render(gpudev.config(w, h, spp, backend=backend, seed=seed, flags=flags), out)
                    dev.free(out)
                    n_frames += 1
                    lines = said.now(key)
                    if which is not None:
                        ran.append((rung, form, which, lines[which]))
                    assert st.ray_bounces == cnt.ray_bounces, (rung.cliff, rung.side, form, st.ray_bounces, cnt.ray_bounces)
                    assert float(np.abs(img - want).max()) <= TOL, (rung.cliff, rung.side, form)
                    if ref is None:
                        ref = img
                    else:
                        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (rung.cliff, rung.side, form)
                if rung.cliff.endswith("_m"):
                    continue  # (pt_ctx_radiance runs one pixel per stream: the scene rungs below are its layouts)
                # probe rays at the edges of the staged tables, each hitting the sphere or triangle of its rank first (by the oracle)
                tabs = br.scene_tables(rung.scene)
                probes = ll.probe_rays(rung, tabs)
                rays = [(t[3], t[4]) for t in probes]
                _, oid, tid, _, _ = ptlib.oracle_intersect(rung.scene, np.array([r[0] for r in rays]), np.array([r[1] for r in rays]))
                assert [(int(x), int(y)) for x, y in zip(oid, tid)] == [t[1:3] for t in probes], (rung.cliff, rung.side)
                for tag, scp, depth, pseed in (("first", br.first_hit_variant(rung.scene), 5, 3), ("shaded", sc, 0, 5)):
                    refs = [ptlib.oracle_radiance(scp, o, d, depth, 1, pseed, j) for j, (o, d) in enumerate(rays)]
                    if tag == "first":
                        assert all(c.ray_bounces == 1 for _, c in refs), rung.cliff
                    for form, env, backend, flags, which in _forms(rung)[:3]:
                        key, dev = ctx_for(env)
                        dev.set_scene(scp)
                        for j, ((o, d), (want_rgb, want_cnt)) in enumerate(zip(rays, refs)):
                            out = np.zeros(3, np.float32)
                            st = PtStats()
                            rc = L.pt_ctx_radiance(dev.ctx, _np_f(np.ascontiguousarray(o)), _np_f(np.ascontiguousarray(d)), depth, 1,
                                                   pseed, j, backend, flags, _np_f(out), C.byref(st))
                            assert rc == 0, L.pt_last_error()
                            n_rays += 1
                            what = (rung.cliff, rung.side, form, tag, probes[j][:3])
                            assert st.ray_bounces == want_cnt.ray_bounces, what
                            if tag == "first":
                                assert np.array_equal(out.view(np.uint32), np.asarray(want_rgb, np.float32).view(np.uint32)), what
                            else:
                                assert np.allclose(out, want_rgb, rtol=2e-6, atol=0), what
                        lines = said.now(key)
                        if which is not None:
                            ran.append((rung, form + " probe " + tag, which, lines[which]))
    finally:
        for dev in ctxs.values():
            dev.close()
    # every case ran with the layout the CPU ladder expects for it
    for rung, form, which, line in ran:
        assert line == rung.lines[which], (rung.cliff, rung.side, form, line, rung.lines[which])
    with capfd.disabled():
        print("\n%d ladder frames, %d probe rays, %d layouts checked, %.1f s" % (n_frames, n_rays, len(ran),
                                                                               time.perf_counter() - t_start))
