"""How well a launch of k_pass_cand fills the chip's workgroup slots, from a -DPT_TAIL_STATS build of the library (`make -C
path-tracer-rust_amd tail`, never the shipped one) on one GPU:
  PT_LIB=scratch/libptrace_tail.so python tools/tail_probe.py <scene> <spp> [NAME=value ...]
Every workgroup of the build writes its begin and end stamp (s_memrealtime, 100 MHz) into a table indexed by blockIdx.x.  One pass
of <spp> samples per pixel of the bench frame's size is rendered (warm-up frame first; an explicit pass size of 512 Mi primaries,
as tools/pmc_run.sh gives, so that the frame is ONE launch: 683 is the bench frame's pass) under the given tuning variables, and
the table of that launch gives
  slot-time efficiency   sum of the workgroups' lifetimes / (slots x the launch's span), slots = the most workgroups alive at once;
  ... of the tail        the same over the time after the last workgroup began: what the launch's end costs;
  the spread             of the lifetimes (of the whole-stream workgroups and of the taper's pieces apart), which is what
                         makes a launch end ragged."""
import ctypes as C
import os
import sys

import numpy as np

scene, spp, sets = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
for kv in sets:
    k, v = kv.split("=")
    os.environ[k] = v
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import ptlib
from ptlib import PtConfig, PtStats

L = ptlib.abi.load(os.environ.get("PT_LIB") or ptlib.PRODUCT_SO)
assert hasattr(L, "pt_debug_tail_stats"), "not a -DPT_TAIL_STATS build: make -C path-tracer-rust_amd tail, PT_LIB=scratch/libptrace_tail.so"
W, H, CAP = 1024, 768, 1 << 18

sc = ptlib.load_scene_py(ptlib.scene_path(scene))
ctx = C.c_void_p()
assert L.pt_ctx_create(0, C.byref(ctx)) == 0
assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0
cfg = PtConfig(W, H, spp, 0, 1, 0, 0, 536870912, 0, 0, 0, 0, 0)
d = C.c_void_p()
assert L.pt_device_malloc(0, W * H * 12, C.byref(d)) == 0
st = PtStats()
table = np.zeros((CAP, 2), np.uint64)
for rep in range(2):  # (the first frame warms up; reading the table clears it)
    assert L.pt_ctx_render(ctx, C.byref(cfg), d, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
    assert st.passes == 1, st.passes
    assert L.pt_debug_tail_stats(ctx, table.ctypes.data_as(C.c_void_p), CAP) == CAP
L.pt_device_free(0, d)
L.pt_ctx_destroy(ctx)

ran = np.nonzero(table[:, 1])[0]
n = int(ran[-1]) + 1
t0, t1 = table[ran, 0].astype(np.int64), table[ran, 1].astype(np.int64)
begin, end = int(t0.min()), int(t1.max())
span = end - begin
life = t1 - t0
# the most workgroups alive at once: +1 at every begin, -1 at every end (ends first at equal stamps)
ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
slots = int(np.cumsum(ev[:, 1]).max())
last = int(t0.max())
tail = np.clip(t1, last, None) - np.clip(t0, last, None)
name = " ".join(sets) or "defaults"
print("%s @%d [%s]: %d workgroups (%d ran), %.2f ms launch, %.3f G bounces/s with the stamps in" % (
    scene, spp, name, n, len(ran), span / 1e5, st.ray_bounces / (st.ms_device * 1e-3) / 1e9 if st.ms_device else 0.0))
print("  slots (most workgroups alive at once) %d; rounds %.2f" % (slots, len(ran) / slots))
print("  slot-time efficiency          %.4f" % (life.sum() / (slots * span)))
print("  ... before the last dispatch  %.4f  (%.1f %% of the launch)" % (
    (life.sum() - tail.sum()) / (slots * (last - begin)), 100.0 * (last - begin) / span))
print("  ... after the last dispatch   %.4f  (%.1f %% of the launch, %.2f ms)" % (
    tail.sum() / (slots * (end - last)) if end > last else 0.0, 100.0 * (end - last) / span, (end - last) / 1e5))


def spread(what, v):
    if len(v) == 0:
        return
    q = np.percentile(v, [0, 5, 50, 95, 100]) / 1e2
    print("  %-22s n %6d  mean %8.1f us  sd/mean %.3f  min %.1f  p5 %.1f  median %.1f  p95 %.1f  max %.1f" % (
        what, len(v), v.mean() / 1e2, v.std() / v.mean(), q[0], q[1], q[2], q[3], q[4]))


cut, pieces = int(os.environ.get("PT_TAPER_CUT", "0") or 0), int(os.environ.get("PT_TAPER_PIECES", "0") or 0)
n_whole = n - cut * pieces if cut > 0 and pieces > 1 and n >= cut * pieces else n
spread("lifetimes, whole streams", life[ran < n_whole])
spread("lifetimes, pieces", life[ran >= n_whole])
